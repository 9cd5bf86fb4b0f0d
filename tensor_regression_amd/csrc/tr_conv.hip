// tr_conv.hip — convolutional spectral CP regression on the untiled (T, D) series
// (convolutional_spectral_tensor_regression.py: conv 259-290, complex_magnitude 292-303,
// slmm_helper 426-430, conv_linear 650-678, L2_penalty 700-718).
//
//   z[t,d,k]  = sum_w X[t+w,d] * Kp[w,k]            k over the K = Rn + Rs*C kernel columns
//   u[t,d,r]  = z (signed) for a one-component rank, ||z[t,d,s,:]||_2 for a spectral rank
//   q[t,r]    = sum_d u[t,d,r] * Bd[d,r]
//   y_hat     = q . Bo^T + bias,  loss = mean (y_hat - y)^2
//
// k_conv<1>: one workgroup of 256 threads owns tiles of TT = 256 consecutive output times over
// all of D.  The (TT + W - 1) x DC slab of X is staged in LDS transposed (column-major, odd
// pitch: the strided writes and the time-contiguous reads are both conflict free), D in chunks
// of DC columns when the slab does not fit.
//   phase A   thread = one output time, its columns serial: z for one group of 16 kernel columns
//             at a time (16 accumulators; the kernel row Kp[g][w][0..15] is wave-uniform), then
//             u and q.  q stays thread-private (LDS row of the thread): no cross-lane reduction.
//   epilogue  y_hat, squared error (double), e = 2 (y_hat - y) / (T' N) (+ eadd[t, n] when a penalty on
//             y_hat brings its own gradient: tr_conv_spectrum.hip) to a global scratch,
//             dBo / dbias by one thread per entry over the tile's times, dq = e . Bo in place of q.
//   phase B   wave = every fourth column of the chunk, its lanes the times of one 64-time
//             subtile after another: z recomputed from the slab still in LDS, dBd by one wave
//             butterfly per (column, group), dz to a wave-private LDS tile, then the same wave
//             with lanes = kernel taps w (and, for W < 64, 64 / W' time sub-ranges) accumulates
//             dKp[w, k] += X[t + w, d] dz[t, d, k] in registers.  Per group the four waves'
//             accumulators are summed in a fixed order.
// Every workgroup adds into its own gradient slab (same thread, same order every time);
// k_conv_finish sums the slabs in index order and applies the softplus chain.  No float atomics:
// two runs on the same inputs are bitwise equal.
// k_conv<0> is phase A + y_hat only (predict); k_conv<2> is k_conv<1> with eadd.
//
// Form: fp32 fmaf on the VALU throughout ("conv-1pass-fmaf").  Bounds: every LDS index is
// < DC*XP + 256*QP + 4*64*16 (conv_geom_init sizes the allocation from the same terms); slab rows
// beyond T are zero-filled and times >= T' contribute e = 0.
#include <cstring>

#include "tr_adam.h"
#include "tr_conv.h"

namespace tr {

namespace {
constexpr int QP = CONV_MAXR + 1;          // LDS pitch of a q / dq row
constexpr int DZ_FLOATS = 4 * 64 * CONV_KC;  // four wave-private dz tiles
constexpr int LDS_BUDGET_FLOATS = 38912;     // 152 KiB of the CU's 160 KiB

// z[0..15] of one (time, column): the slab column at xp, the group's kernel rows at kp
__device__ __forceinline__ void conv_z(const float* __restrict__ xp, const float* __restrict__ kp, int W,
                                       float (&z)[CONV_KC]) {
#pragma unroll
  for (int j = 0; j < CONV_KC; ++j) z[j] = 0.f;
#pragma unroll 2
  for (int w = 0; w < W; ++w) {
    const float x = xp[w];
#pragma unroll
    for (int j = 0; j < CONV_KC; ++j) z[j] = fmaf(x, kp[w * CONV_KC + j], z[j]);
  }
}

template <int CC>
__device__ __forceinline__ float conv_mag(const float (&z)[CONV_KC], int j) {
  if (CC == 1) return z[j];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CC; ++c) s = fmaf(z[j * CC + c], z[j * CC + c], s);
  return sqrtf(s);
}

// phase A of one column group: q[t, rbase + j] += sum_d u[t, d, j] Bd[d, rbase + j]
template <int CC>
__device__ __forceinline__ void conv_a_group(const float* sX, float* sQrow, const float* __restrict__ kp,
                                             const float* __restrict__ bd, int R, int nr, int W, int XP, int dc,
                                             int tid) {
  constexpr int RPG = CONV_KC / CC;
  float qa[RPG];
#pragma unroll
  for (int j = 0; j < RPG; ++j) qa[j] = 0.f;
  for (int dl = 0; dl < dc; ++dl) {
    float z[CONV_KC];
    conv_z(sX + dl * XP + tid, kp, W, z);
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      const float b = j < nr ? bd[(int64_t)dl * R + j] : 0.f;
      qa[j] = fmaf(conv_mag<CC>(z, j), b, qa[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < RPG; ++j)
    if (j < nr) sQrow[j] += qa[j];
}

// phase B of one column group (see the header comment); contains workgroup barriers: every wave
// of the workgroup calls it with the same (dc, W, group)
template <int CC>
__device__ __forceinline__ void conv_b_group(const float* sX, const float* sDQ, float* sDZ,
                                             const float* __restrict__ kp, const float* __restrict__ bdp,
                                             float* slabBd, float* slabK, int R, int nr, int W, int XP, int dc,
                                             int tid) {
  constexpr int RPG = CONV_KC / CC;
  constexpr int NPMAX = (CONV_MAXW + 63) / 64;
  const int lane = tid & 63, wv = tid >> 6;
  const int npass = (W + 63) / 64;
  int WL = 64;
  if (W < 64) {
    WL = 1;
    while (WL < W) WL <<= 1;
  }
  const int NTS = 64 / WL;  // time sub-ranges of a subtile; each WL times long
  const int wl = lane & (WL - 1), ts = lane / WL;
  float acc[NPMAX][CONV_KC];
#pragma unroll
  for (int p = 0; p < NPMAX; ++p)
#pragma unroll
    for (int k = 0; k < CONV_KC; ++k) acc[p][k] = 0.f;
  float* myDZ = sDZ + wv * 64 * CONV_KC;
  for (int dl = wv; dl < dc; dl += 4) {
    float bd[RPG], bdv[RPG];
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      bd[j] = 0.f;
      bdv[j] = j < nr ? bdp[(int64_t)dl * R + j] : 0.f;
    }
    for (int tsb = 0; tsb < CONV_TT / 64; ++tsb) {
      const int tl = tsb * 64 + lane;
      float z[CONV_KC], dz[CONV_KC];
      conv_z(sX + dl * XP + tl, kp, W, z);
#pragma unroll
      for (int k = 0; k < CONV_KC; ++k) dz[k] = 0.f;
#pragma unroll
      for (int j = 0; j < RPG; ++j) {
        const float dqv = j < nr ? sDQ[tl * QP + j] : 0.f;
        const float m = conv_mag<CC>(z, j);
        bd[j] = fmaf(m, dqv, bd[j]);
        if (CC == 1) {
          dz[j] = dqv * bdv[j];
        } else {
          // d||z|| / dz = z / ||z||, 0 where ||z|| = 0 (torch.norm's backward)
          const float cf = m > 0.f ? dqv * bdv[j] / m : 0.f;
#pragma unroll
          for (int c = 0; c < CC; ++c) dz[j * CC + c] = cf * z[j * CC + c];
        }
      }
      float4* wr = reinterpret_cast<float4*>(myDZ + lane * CONV_KC);
#pragma unroll
      for (int k4 = 0; k4 < CONV_KC / 4; ++k4)
        wr[k4] = make_float4(dz[4 * k4], dz[4 * k4 + 1], dz[4 * k4 + 2], dz[4 * k4 + 3]);
      wv_lds_sync();
      for (int tt = ts * WL; tt < ts * WL + WL; ++tt) {
        float dzv[CONV_KC];
        const float4* rd = reinterpret_cast<const float4*>(myDZ + tt * CONV_KC);
#pragma unroll
        for (int k4 = 0; k4 < CONV_KC / 4; ++k4) {
          const float4 v = rd[k4];
          dzv[4 * k4] = v.x;
          dzv[4 * k4 + 1] = v.y;
          dzv[4 * k4 + 2] = v.z;
          dzv[4 * k4 + 3] = v.w;
        }
        const float* xb = sX + dl * XP + tsb * 64 + tt;
#pragma unroll
        for (int p = 0; p < NPMAX; ++p) {
          if (p < npass) {
            const int w = p * 64 + wl;
            const float x = w < W ? xb[w] : 0.f;
#pragma unroll
            for (int k = 0; k < CONV_KC; ++k) acc[p][k] = fmaf(x, dzv[k], acc[p][k]);
          }
        }
      }
      wv_lds_sync();
    }
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      const float s = wv_allreduce(bd[j]);
      if (lane == j && j < nr) slabBd[(int64_t)dl * R + j] += s;
    }
  }
  // the four waves' (and the time sub-ranges') dKp partials, summed in a fixed order
#pragma unroll
  for (int p = 0; p < NPMAX; ++p) {
    if (p < npass) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < CONV_KC; ++k) myDZ[lane * CONV_KC + k] = acc[p][k];
      __syncthreads();
      for (int o = tid; o < WL * CONV_KC; o += CONV_TT) {
        const int wlo = o / CONV_KC, k = o - wlo * CONV_KC;
        const int w = p * 64 + wlo;
        if (w < W) {
          float s = 0.f;
          for (int v = 0; v < 4; ++v)
            for (int u = 0; u < NTS; ++u) s += sDZ[(v * 64 + u * WL + wlo) * CONV_KC + k];
          slabK[w * CONV_KC + k] += s;
        }
      }
    }
  }
  __syncthreads();
}
}  // namespace

template <int TRAIN>
__global__ __launch_bounds__(CONV_TT) void k_conv(ConvGeom g, const float* __restrict__ X, int64_t T, int64_t xld,
                                                  const float* __restrict__ phi, const float* __restrict__ params,
                                                  const float* __restrict__ Kp, const float* __restrict__ y,
                                                  float scale, float* gpart, double* __restrict__ dpart,
                                                  float* ebuf, float* __restrict__ yhat,
                                                  const int32_t* __restrict__ stop,
                                                  const float* __restrict__ eadd) {
  if (stop != nullptr && *stop != 0) return;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int XP = g.XP, W = g.W, R = g.R, N = g.N, D = g.D, DC = g.DC;
  float* sDZ = lds;  // first: 16-byte aligned for the float4 accesses
  float* sQ = sDZ + DZ_FLOATS;
  float* sX = sQ + CONV_TT * QP;
  const int tid = threadIdx.x;
  const int64_t Tp = T - W + 1;
  const int64_t ntiles = (Tp + CONV_TT - 1) / CONV_TT;
  const int nchunks = (D + DC - 1) / DC;
  const int rows = CONV_TT + W - 1;
  const float* pBd = phi + g.offBd;
  const float* pBo = phi + g.offBo;
  const float* bias = params + g.offB;
  float* slab = TRAIN ? gpart + (int64_t)blockIdx.x * g.slab : nullptr;
  double lossacc = 0.0;

  auto stage = [&](int64_t t0, int d0, int dc) {
    const int n = rows * dc;
    for (int idx = tid; idx < n; idx += CONV_TT) {
      const int row = idx / dc, dl = idx - row * dc;
      const int64_t t = t0 + row;
      sX[dl * XP + row] = t < T ? X[t * xld + d0 + dl] : 0.f;
    }
  };

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t t0 = tile * CONV_TT;
    const int64_t t = t0 + tid;
    const bool valid = t < Tp;
    for (int r = 0; r < R; ++r) sQ[tid * QP + r] = 0.f;
    for (int c = 0; c < nchunks; ++c) {
      const int d0 = c * DC, dc = D - d0 < DC ? D - d0 : DC;
      __syncthreads();  // the slab's previous readers are done
      stage(t0, d0, dc);
      __syncthreads();
      for (int gi = 0; gi < g.G; ++gi) {
        const ConvGroup gr = g.grp[gi];
        const float* kp = Kp + (int64_t)gi * W * CONV_KC;
        const float* bd = pBd + (int64_t)d0 * R + gr.rbase;
        float* qrow = sQ + tid * QP + gr.rbase;
        switch (gr.cc) {
          case 1: conv_a_group<1>(sX, qrow, kp, bd, R, gr.nr, W, XP, dc, tid); break;
          case 2: conv_a_group<2>(sX, qrow, kp, bd, R, gr.nr, W, XP, dc, tid); break;
          case 3: conv_a_group<3>(sX, qrow, kp, bd, R, gr.nr, W, XP, dc, tid); break;
          default: conv_a_group<4>(sX, qrow, kp, bd, R, gr.nr, W, XP, dc, tid); break;
        }
      }
    }
    // epilogue: y_hat, squared error, residual
    for (int n = 0; n < N; ++n) {
      float yh = 0.f;
      for (int r = 0; r < R; ++r) yh = fmaf(sQ[tid * QP + r], pBo[n * R + r], yh);
      yh += bias[n];
      if (valid) {
        if (yhat != nullptr) yhat[t * N + n] = yh;
        if (TRAIN) {
          const float diff = yh - y[t * N + n];
          lossacc += (double)diff * (double)diff;
          // TRAIN == 2: eadd, the gradient of a penalty on y_hat (the spectrum penalty), joins the
          // residual's; an instantiation of its own and the last kernel argument, so that k_conv<1>
          // and k_conv<0> stay the code they were
          ebuf[t * N + n] = TRAIN == 2 ? scale * diff + eadd[t * N + n] : scale * diff;
        }
      }
    }
    if (!TRAIN) continue;
    __syncthreads();  // e (global scratch) and q (LDS) of every time of the tile
    const int nvalid = Tp - t0 < CONV_TT ? (int)(Tp - t0) : CONV_TT;
    for (int p = tid; p < N * R; p += CONV_TT) {
      const int n = p / R, r = p - n * R;
      float s = 0.f;
      for (int tl = 0; tl < nvalid; ++tl) s = fmaf(ebuf[(t0 + tl) * N + n], sQ[tl * QP + r], s);
      slab[g.sOffBo + p] += s;
    }
    for (int n = tid; n < N; n += CONV_TT) {
      float s = 0.f;
      for (int tl = 0; tl < nvalid; ++tl) s += ebuf[(t0 + tl) * N + n];
      slab[g.sOffB + n] += s;
    }
    __syncthreads();  // q has been read: dq = e . Bo takes its place
    for (int r = 0; r < R; ++r) {
      float s = 0.f;
      if (valid)
        for (int n = 0; n < N; ++n) s = fmaf(ebuf[t * N + n], pBo[n * R + r], s);
      sQ[tid * QP + r] = s;
    }
    __syncthreads();
    for (int c = nchunks - 1; c >= 0; --c) {  // the last chunk is still in LDS
      const int d0 = c * DC, dc = D - d0 < DC ? D - d0 : DC;
      if (c != nchunks - 1) {
        __syncthreads();
        stage(t0, d0, dc);
        __syncthreads();
      }
      for (int gi = 0; gi < g.G; ++gi) {
        const ConvGroup gr = g.grp[gi];
        const float* kp = Kp + (int64_t)gi * W * CONV_KC;
        const float* bd = pBd + (int64_t)d0 * R + gr.rbase;
        float* sBd = slab + g.sOffBd + (int64_t)d0 * R + gr.rbase;
        float* sK = slab + g.sOffK + (int64_t)gi * W * CONV_KC;
        const float* dq = sQ + gr.rbase;
        switch (gr.cc) {
          case 1: conv_b_group<1>(sX, dq, sDZ, kp, bd, sBd, sK, R, gr.nr, W, XP, dc, tid); break;
          case 2: conv_b_group<2>(sX, dq, sDZ, kp, bd, sBd, sK, R, gr.nr, W, XP, dc, tid); break;
          case 3: conv_b_group<3>(sX, dq, sDZ, kp, bd, sBd, sK, R, gr.nr, W, XP, dc, tid); break;
          default: conv_b_group<4>(sX, dq, sDZ, kp, bd, sBd, sK, R, gr.nr, W, XP, dc, tid); break;
        }
      }
    }
  }
  if (TRAIN) {
    __shared__ double wl[CONV_TT / 64];
    const double s = wv_allreduce_d(lossacc);
    if ((tid & 63) == 0) wl[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) dpart[blockIdx.x] = (wl[0] + wl[1]) + (wl[2] + wl[3]);
  }
}

__global__ __launch_bounds__(256) void k_conv_kp(int n, const float* __restrict__ phi,
                                                 const int32_t* __restrict__ kmap, float* __restrict__ Kp,
                                                 const int32_t* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t src = kmap[i];
  Kp[i] = src >= 0 ? phi[src] : 0.f;
}

__global__ __launch_bounds__(256) void k_conv_finish(int64_t nparams, int64_t nfelem, int nslabs, int64_t slab,
                                                     const float* __restrict__ gpart,
                                                     const double* __restrict__ dpart,
                                                     const int32_t* __restrict__ gmap,
                                                     const float* __restrict__ dphi, double loss_scale,
                                                     float* __restrict__ grad_out,
                                                     const int32_t* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < nparams) {
    const int64_t src = gmap[e];
    float s = 0.f;
    for (int b = 0; b < nslabs; ++b) s += gpart[(int64_t)b * slab + src];
    grad_out[e] = e < nfelem ? s * dphi[e] : s;
  } else if (e == nparams) {
    double l = 0.0;
    for (int b = 0; b < nslabs; ++b) l += dpart[b];
    grad_out[nparams] = (float)(l * loss_scale);
    grad_out[nparams + 1] = 0.f;
  }
}

// The update of the three convolutional models (conv spectral, phase-constrained, Fourier): k_update's
// norms, prologue and Adam step (tr_adam.h) with one lambda per factor, a fixed nf = 4, one element per
// trip, and the reference's order of the penalty sum,
//   loss + L2_penalty(Bcp_w, [l0, l0]) + L2_penalty(Bcp_n, l[1:])                    (conv …py:1046)
//   ... + loss_spectral + loss_smoothness                                 (phase …py:1412, Fourier …py:1281)
// A kernel of its own: k_update as compiled for the other models is untouched.
//   SMOOTH = false   the conv spectral model: no smoothness term, no dynamic LDS.
//   SMOOTH = true    plus lambda_s mean((Delta^q F)^2) over the raw Kn (W, Rn) and Ks seen as (W, RsK)
//                    (RsK = Rs for the phase model, Rs C for the Fourier model):
//                    Delta^q F = F convolved (full) with the stencil (-1)^j C(q, j), W + q rows, kept in
//                    dynamic LDS ((W + q) (Rn + RsK) floats); gradient (2 lambda_s / ((W + q) R_F))
//                    (Delta^q)^T Delta^q F.  spec_val (nullable) is the spectrum penalty's value.
// nan_armed: the host's decision that a NaN total stops the fit at this iteration (the two stop-rule
// families differ in it, launch_update_conv).
struct ConvLam {
  float v[4];  // by arena factor: Bd, Bo, Kn, Ks
};

template <bool SMOOTH>
__global__ __launch_bounds__(1024) void k_update_conv(FactorSet fs, int n_bias, ConvLam lam, ConvSmooth sm, int W,
                                                      int Rn, int RsK, const float* __restrict__ spec_val,
                                                      int nan_armed, float* __restrict__ params,
                                                      const float* __restrict__ grad, UpdateArgs ua,
                                                      float* __restrict__ m, float* __restrict__ v,
                                                      float* __restrict__ vmax, float* __restrict__ grad_total_out,
                                                      float* __restrict__ loss_out, double* __restrict__ loss_hist,
                                                      int32_t* __restrict__ stop) {
#pragma clang fp contract(off)
  __shared__ float wsum[4 * 16];
  __shared__ float norms[4];
  __shared__ float coef[4];
  __shared__ float ssum[2 * 16];  // SMOOTH only (as sval and sd)
  __shared__ float sval[2];
  extern __shared__ float sd[];  // Delta^q of [Kn | Ks], (W + q) x (Rn + RsK)
  const int t = threadIdx.x, lane = t & 63, q = t >> 6;
  const int64_t nfe = fs.nfelem, np = nfe + n_bias;
  const StopState ss = stop_load(stop, ua.mode == 0, grad, np);
  float accn[TR_MAXF] = {};
  for (int64_t k = t; k < nfe; k += 1024) norm_add(fs, 4, k, params[k], accn);
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const float r = wv_allreduce(accn[f]);
    if (lane == 0) wsum[f * 16 + q] = r;
  }
  const int ord = sm.order, Wq = W + ord, Rk = Rn + RsK;
  if constexpr (SMOOTH) {
    // Delta^q of the raw kernels and the two sums of its squares
    float accs[2] = {0.f, 0.f};
    for (int idx = t; idx < Wq * Rk; idx += 1024) {
      const int i = idx / Rk, c = idx - i * Rk;
      const float* col = c < Rn ? params + fs.off[2] + c : params + fs.off[3] + (c - Rn);
      const int ld = c < Rn ? Rn : RsK;
      float d = 0.f;
      for (int j = 0; j <= ord; ++j) {
        const int w = i - j;
        if (w >= 0 && w < W) d = d + sm.c[j] * col[(int64_t)w * ld];
      }
      sd[idx] = d;
      if (c < Rn)
        accs[0] = fmaf(d, d, accs[0]);
      else
        accs[1] = fmaf(d, d, accs[1]);
    }
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float r = wv_allreduce(accs[f]);
      if (lane == 0) ssum[f * 16 + q] = r;
    }
  }
  __syncthreads();
  if (t < 4) {
    norm_finish<16>(wsum, t, lam.v[t], norms, coef);
  } else if (SMOOTH && t >= 64 && t < 66) {
    const int f = t - 64;
    float tot = 0.f;
    for (int w = 0; w < 16; ++w) tot += ssum[f * 16 + w];
    const int rf = f == 0 ? Rn : RsK;
    sval[f] = rf > 0 ? (tot / (float)(Wq * rf)) * sm.lam : 0.f;  // torch.mean(...) * lambda_smooth
  }
  __syncthreads();
  if (stop_taken(ss, stop, ua.iter, t)) return;
  const bool adam = ua.mode != 1;
  const bool ams = adam && ua.amsgrad;
  for (int64_t e = t; e < np; e += 1024) {
    float g = grad[e], p = params[e];
    if (e < nfe) {
      const int f = factor_of(fs, 4, e);
      g = g + coef[f] * (2.0f * p);
      if (SMOOTH && f >= 2) {
        const int rf = f == 2 ? Rn : RsK;
        const int le = (int)(e - fs.off[f]);
        const int w = le / rf, c = (f == 2 ? 0 : Rn) + (le - w * rf);
        float gs = 0.f;
        for (int j = 0; j <= ord; ++j) gs = gs + sm.c[j] * sd[(w + j) * Rk + c];
        g = g + (2.0f * sm.lam / (float)(Wq * rf)) * gs;
      }
    }
    if (!adam) {
      grad_total_out[e] = g;
      continue;
    }
    float mm = m[e], vv = v[e], vm = ams ? vmax[e] : 0.f;
    adam_moments(p, g, mm, vv, ua.weight_decay, ua.one_minus_b1, ua.beta2, ua.one_minus_b2);
    vm = fmaxf(vm, vv);
    if (ams) vmax[e] = vm;
    p = adam_param(p, mm, ams ? vm : vv, ua.bc2_sqrt, ua.eps, ua.step_size);
    m[e] = mm;
    v[e] = vv;
    params[e] = p;
  }
  if (t == 0) {
    const float pw = (0.f + norms[2] * lam.v[2]) + norms[3] * lam.v[3];
    const float pn = (0.f + norms[0] * lam.v[0]) + norms[1] * lam.v[1];
    float total = (grad[np] + pw) + pn;
    if (SMOOTH) {
      if (spec_val != nullptr) total = total + *spec_val;
      float ps = 0.f;  // an empty factor is skipped (comp.numel() > 0, phase …py:954, Fourier …py:875)
      if (Rn > 0) ps = ps + sval[0];
      if (RsK > 0) ps = ps + sval[1];
      total = total + ps;
    }
    if (loss_out != nullptr) *loss_out = total;
    if (ua.mode == 0 && loss_hist != nullptr) loss_hist[ua.hist_base + ua.iter] = (double)total;
    if (nan_armed && __builtin_isnan(total)) *stop = -(int32_t)(ua.iter + 1);
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
bool conv_geom_init(ConvGeom* g, int64_t n_w, int64_t n_d, int64_t n_out, int rank_normal, int rank_spectral,
                    int n_complex, const int32_t* non_negative, std::string* why) {
  std::memset(g, 0, sizeof(*g));
  auto no = [&](const char* m) {
    *why = m;
    return false;
  };
  if (n_w > CONV_MAXW) return no("temporal window beyond the conv kernel's envelope (W <= 257)");
  if (n_d > 65536) return no("n_d beyond the conv kernel's envelope (D <= 65536)");
  if (n_out > CONV_MAXN) return no("n_out beyond the conv kernel's envelope (N <= 64)");
  if (rank_normal + rank_spectral > CONV_MAXR)
    return no("rank_normal + rank_spectral beyond the conv kernel's envelope (R <= 32)");
  if (n_complex > CONV_MAXC) return no("n_complex beyond the conv kernel's envelope (C <= 4)");
  if (rank_normal + rank_spectral * n_complex > CONV_MAXK)
    return no("rank_normal + rank_spectral * n_complex beyond the conv kernel's envelope (K <= 64)");
  g->W = (int)n_w;
  g->D = (int)n_d;
  g->N = (int)n_out;
  g->Rn = rank_normal;
  g->Rs = rank_spectral;
  g->C = n_complex;
  g->R = rank_normal + rank_spectral;
  g->K = rank_normal + rank_spectral * n_complex;
  for (int i = 0; i < 3; ++i) g->nonneg[i] = non_negative != nullptr && non_negative[i] ? 1 : 0;
  g->offBd = 0;
  g->offBo = g->offBd + (int64_t)g->D * g->R;
  g->offKn = g->offBo + (int64_t)g->N * g->R;
  g->offKs = g->offKn + (int64_t)g->W * g->Rn;
  g->offB = g->offKs + (int64_t)g->W * g->Rs * g->C;
  g->nparams = g->offB + g->N;
  // column groups: one-component ranks (normal, and spectral when C == 1) 16 to a group, then
  // spectral ranks 16 / C to a group
  const int n1 = g->C == 1 ? g->R : g->Rn;
  int G = 0;
  for (int r = 0; r < n1; r += CONV_KC) {
    g->grp[G].cc = 1;
    g->grp[G].rbase = r;
    g->grp[G].nr = n1 - r < CONV_KC ? n1 - r : CONV_KC;
    ++G;
  }
  if (g->C > 1) {
    const int rpg = CONV_KC / g->C;
    for (int s = 0; s < g->Rs; s += rpg) {
      if (G >= CONV_MAXG) return no("too many kernel column groups");
      g->grp[G].cc = g->C;
      g->grp[G].rbase = g->Rn + s;
      g->grp[G].nr = g->Rs - s < rpg ? g->Rs - s : rpg;
      ++G;
    }
  }
  g->G = G;
  g->sOffBd = 0;
  g->sOffBo = g->sOffBd + (int64_t)g->D * g->R;
  g->sOffK = g->sOffBo + (int64_t)g->N * g->R;
  g->sOffB = g->sOffK + (int64_t)G * g->W * CONV_KC;
  g->slab = (g->sOffB + g->N + 3) & ~(int64_t)3;
  g->XP = (CONV_TT + g->W - 1) | 1;
  const int fixed = DZ_FLOATS + CONV_TT * QP;
  int dc = (LDS_BUDGET_FLOATS - fixed) / g->XP;
  if (dc > g->D) dc = g->D;
  if (dc >= 4) dc &= ~3;  // phase B deals columns to four waves
  g->DC = dc;
  g->lds_bytes = (size_t)(fixed + dc * g->XP) * 4;
  return true;
}

void conv_build_maps(const ConvGeom& g, int32_t* kmap, int32_t* gmap) {
  for (int64_t i = 0; i < (int64_t)g.G * g.W * CONV_KC; ++i) kmap[i] = -1;
  for (int64_t e = 0; e < g.offKn; ++e) gmap[e] = (int32_t)e;  // Bd, Bo: same place in arena and slab
  for (int n = 0; n < g.N; ++n) gmap[g.offB + n] = (int32_t)(g.sOffB + n);
  for (int gi = 0; gi < g.G; ++gi) {
    const ConvGroup& gr = g.grp[gi];
    for (int j = 0; j < gr.nr; ++j) {
      const int r = gr.rbase + j;
      for (int c = 0; c < gr.cc; ++c)
        for (int w = 0; w < g.W; ++w) {
          const int64_t arena = r < g.Rn ? g.offKn + (int64_t)w * g.Rn + r
                                         : g.offKs + ((int64_t)w * g.Rs + (r - g.Rn)) * g.C + c;
          const int64_t pos = ((int64_t)gi * g.W + w) * CONV_KC + j * gr.cc + c;
          kmap[pos] = (int32_t)arena;
          gmap[arena] = (int32_t)(g.sOffK + pos);
        }
    }
  }
}

hipError_t conv_prepare(const ConvGeom& g) {
  // the attribute is per kernel, not per plan: always the whole budget (every plan's lds_bytes is within it)
  if (g.lds_bytes > (size_t)LDS_BUDGET_FLOATS * 4) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv<1>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BUDGET_FLOATS * 4);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv<2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          LDS_BUDGET_FLOATS * 4);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv<0>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             LDS_BUDGET_FLOATS * 4);
}

hipError_t launch_conv_kp(const ConvGeom& g, const float* phi, const int32_t* kmap, float* Kp, const int32_t* stop,
                          hipStream_t st) {
  const int n = g.G * g.W * CONV_KC;
  hipLaunchKernelGGL(k_conv_kp, dim3((n + 255) / 256), dim3(256), 0, st, n, phi, kmap, Kp, stop);
  return hipGetLastError();
}

hipError_t launch_conv(int train, const ConvGeom& g, int grid, const float* X, int64_t T, int64_t xld,
                       const float* phi, const float* params, const float* Kp, const float* y, float scale,
                       float* gpart, double* dpart, float* ebuf, const float* eadd, float* yhat, const int32_t* stop,
                       hipStream_t st) {
  if (T < g.W || grid < 1) return hipErrorInvalidValue;
  if (train && eadd != nullptr)
    hipLaunchKernelGGL(k_conv<2>, dim3(grid), dim3(CONV_TT), g.lds_bytes, st, g, X, T, xld, phi, params, Kp, y, scale,
                       gpart, dpart, ebuf, yhat, stop, eadd);
  else if (train)
    hipLaunchKernelGGL(k_conv<1>, dim3(grid), dim3(CONV_TT), g.lds_bytes, st, g, X, T, xld, phi, params, Kp, y, scale,
                       gpart, dpart, ebuf, yhat, stop, eadd);
  else
    hipLaunchKernelGGL(k_conv<0>, dim3(grid), dim3(CONV_TT), g.lds_bytes, st, g, X, T, xld, phi, params, Kp, y, scale,
                       gpart, dpart, ebuf, yhat, stop, eadd);
  return hipGetLastError();
}

hipError_t launch_conv_finish(const ConvGeom& g, int nslabs, const float* gpart, const double* dpart,
                              const int32_t* gmap, const float* dphi, double loss_scale, float* grad_out,
                              const int32_t* stop, hipStream_t st) {
  const int64_t n = g.nparams + 1;
  hipLaunchKernelGGL(k_conv_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g.nparams, g.offB, nslabs,
                     g.slab, gpart, dpart, gmap, dphi, loss_scale, grad_out, stop);
  return hipGetLastError();
}

void conv_smooth_init(ConvSmooth* s, float lambda_smooth, int order) {
  std::memset(s, 0, sizeof(*s));
  s->lam = lambda_smooth;
  s->order = order;
  double c = 1.0;  // (-1)^j C(q, j)
  for (int j = 0; j <= order; ++j) {
    s->c[j] = (float)c;
    c = -c * (double)(order - j) / (double)(j + 1);
  }
}

hipError_t conv_update_prepare() {
  // Delta^q of the widest plan, (257 + 8) x 64 floats, is past the 64 KiB a kernel gets unasked
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_update_conv<true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (CONV_MAXW + CONV_MAXQ) * CONV_MAXK * 4);
}

hipError_t launch_update_conv(const FactorSet& fs, int n_bias, const float lam[4], const ConvSmooth* sm, int W, int Rn,
                              int RsK, const float* spec_val, bool tail_rule, float* params, const float* grad,
                              const UpdateArgs& ua, float* m, float* v, float* vmax, float* grad_total_out,
                              float* loss_out, double* loss_hist, int32_t* stop, hipStream_t st) {
  if (fs.nf != 4) return hipErrorInvalidValue;
  if (sm != nullptr && (sm->order < 0 || sm->order > CONV_MAXQ || W > CONV_MAXW || Rn + RsK > CONV_MAXK))
    return hipErrorInvalidValue;
  ConvLam l;
  for (int i = 0; i < 4; ++i) l.v[i] = lam[i];
  // The two stop-rule families.  Conv spectral (…py:1057-1064) counts this fit's iterations: the NaN stop
  // is armed while iter <= patience, then k_converge tests the plateau.  Phase and Fourier (tail_rule; phase
  // …py:1445-1452, Fourier …py:1313-1320) count len(loss_running): the NaN stop is armed while it is
  // <= patience, then k_converge_tail tests the slice loss_running[-patience+1:].
  const int64_t n_losses = ua.hist_base + ua.iter + 1;
  const bool can_stop = ua.mode == 0 && stop != nullptr;
  const bool early = tail_rule ? n_losses <= ua.patience : ua.iter <= ua.patience;
  const int nan_armed = can_stop && ua.nan_stop && early;
  if (sm != nullptr) {
    const size_t lds = (size_t)(W + sm->order) * (Rn + RsK) * 4;
    hipLaunchKernelGGL(k_update_conv<true>, dim3(1), dim3(1024), lds, st, fs, n_bias, l, *sm, W, Rn, RsK, spec_val,
                       nan_armed, params, grad, ua, m, v, vmax, grad_total_out, loss_out, loss_hist, stop);
  } else {
    hipLaunchKernelGGL(k_update_conv<false>, dim3(1), dim3(1024), 0, st, fs, n_bias, l, ConvSmooth{}, 0, 0, 0,
                       nullptr, nan_armed, params, grad, ua, m, v, vmax, grad_total_out, loss_out, loss_hist, stop);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !can_stop || loss_hist == nullptr || !(ua.tol > 0.0)) return e;
  if (tail_rule) {
    if (ua.patience >= 0 && n_losses > ua.patience)
      e = launch_converge_tail(loss_hist, n_losses, ua.iter, ua.patience, ua.tol, stop, st);
  } else if (ua.iter > ua.patience) {
    e = launch_converge(loss_hist, ua.hist_base, ua.iter, ua.patience, ua.tol, stop, st);
  }
  return e;
}

}  // namespace tr
