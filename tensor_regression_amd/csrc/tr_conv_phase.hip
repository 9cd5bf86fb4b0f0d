// tr_conv_phase.hip — phase-constrained spectral convolutional CP regression
// (phase_constrained_spectral_convolutional_tensor_regression.py: forward_model 696-744,
// phase_shifter 959-1027, smoothness_penalty / diff_highOrder 933-956, loss 1400-1413).
//
// The model is tr_conv.hip's with C = 2 spectral components, the second one derived: a spectral
// rank carries one kernel k (W taps) and its pair is k with every frequency shifted by 90 degrees.
// The reference writes that as fft -> (abs, angle) -> angle + mask * pi/2 -> ifft -> real; it is the
// fixed real linear map "circular convolution with h",
//   h[d] = (2 / W) sum_{j=1..(W-1)/2} sin(2 pi j d / W),   (H k)[n] = sum_m h[(n - m) mod W] k[m],
// h odd (h[-d] = -h[d]), so H^T = -H.  h is computed on the host in fp64 (exact pi/2; the
// reference's fp32 mask shifts by fp32(pi/2), whose cosine is -4.4e-8) and uploaded once, laid out
// twice (h2[i] = h[i mod W], i < 2W) so that the circular index is the plain h2[a - b + W].
//
//   k_phase_kp      one workgroup per rank: kernel column(s) of the rank into Kp (G, W, 16) as k_conv
//                   reads them; a spectral rank writes phi(Ks)[:, s] and H phi(Ks)[:, s], each
//                   entry one fmaf chain over m ascending.
//   k_conv          tr_conv.hip, unchanged: the X pass over the pair columns.
//   k_phase_finish  slab sum in index order (as k_conv_finish); a spectral rank's two column
//                   gradients fold back as dK0[w] + sum_n h[(n - w) mod W] dK1[n] (H^T, one fmaf chain
//                   over n ascending, then one add); softplus chain, loss slot, status slot.
//   k_update_conv_phase  k_update_conv plus lambda_s mean((Delta^q F)^2) over the raw Kn and Ks
//                   (and this reference's plateau slice loss_running[-patience+1:], k_converge_tail):
//                   Delta^q F = F convolved (full) with the stencil (-1)^j C(q, j), W + q rows;
//                   gradient (2 lambda_s / ((W + q) R_F)) (Delta^q)^T Delta^q F.
// No float atomics anywhere; every sum has one fixed order: two runs are bitwise equal.
// Bounds: Kp and the slab's dKp are (G, W, 16) and a rank's group / column come from the same
// rule as conv_geom_init's groups; LDS arrays are sized by CONV_MAXW, PHASE_MAXQ and CONV_MAXR.
#include <cmath>
#include <cstring>
#include <vector>

#include "tr_conv_phase.h"

namespace tr {

namespace {
constexpr int PH_T = 256;
constexpr int RPG2 = CONV_KC / 2;  // spectral ranks per column group

// group and first column of rank r in Kp / dKp
__device__ __forceinline__ void phase_rank_pos(const ConvGeom& g, int r, int* gi, int* col) {
  const int gn = (g.Rn + CONV_KC - 1) / CONV_KC;
  if (r < g.Rn) {
    *gi = r / CONV_KC;
    *col = r % CONV_KC;
  } else {
    const int s = r - g.Rn;
    *gi = gn + s / RPG2;
    *col = 2 * (s % RPG2);
  }
}
}  // namespace

__global__ __launch_bounds__(PH_T) void k_phase_kp(ConvGeom g, const float* __restrict__ phi,
                                                   const float* __restrict__ h2, float* __restrict__ Kp,
                                                   const int32_t* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  __shared__ float sk[CONV_MAXW];
  __shared__ float sh[2 * CONV_MAXW];
  const int r = blockIdx.x, tid = threadIdx.x, W = g.W;
  int gi, col;
  phase_rank_pos(g, r, &gi, &col);
  float* kp = Kp + (int64_t)gi * W * CONV_KC + col;
  if (r < g.Rn) {
    for (int w = tid; w < W; w += PH_T) kp[w * CONV_KC] = phi[g.offKn + (int64_t)w * g.Rn + r];
    return;
  }
  const int s = r - g.Rn;
  for (int w = tid; w < W; w += PH_T) sk[w] = phi[g.offKs + (int64_t)w * g.Rs + s];
  for (int i = tid; i < 2 * W; i += PH_T) sh[i] = h2[i];
  __syncthreads();
  for (int n = tid; n < W; n += PH_T) {
    const float* hp = sh + n + W;  // hp[-m] = h[(n - m) mod W]
    float acc = 0.f;
    for (int m = 0; m < W; ++m) acc = fmaf(hp[-m], sk[m], acc);
    kp[n * CONV_KC] = sk[n];
    kp[n * CONV_KC + 1] = acc;
  }
}

__global__ __launch_bounds__(PH_T) void k_phase_finish(ConvGeom g, int nslabs, const float* __restrict__ gpart,
                                                       const double* __restrict__ dpart,
                                                       const int32_t* __restrict__ gmap,
                                                       const float* __restrict__ dphi, const float* __restrict__ h2,
                                                       double loss_scale, float* __restrict__ grad_out,
                                                       const int32_t* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  const int tid = threadIdx.x, W = g.W;
  if ((int)blockIdx.x < g.Rs) {
    __shared__ float d0[CONV_MAXW];
    __shared__ float d1[CONV_MAXW];
    __shared__ float sh[2 * CONV_MAXW];
    const int s = blockIdx.x;
    for (int w = tid; w < W; w += PH_T) {
      const int64_t src = gmap[g.offKs + (int64_t)w * g.Rs + s];
      float a = 0.f, b = 0.f;
      for (int sl = 0; sl < nslabs; ++sl) {
        a += gpart[(int64_t)sl * g.slab + src];
        b += gpart[(int64_t)sl * g.slab + src + 1];
      }
      d0[w] = a;
      d1[w] = b;
    }
    for (int i = tid; i < 2 * W; i += PH_T) sh[i] = h2[i];
    __syncthreads();
    for (int w = tid; w < W; w += PH_T) {
      const float* hp = sh + W - w;  // hp[n] = h[(n - w) mod W]
      float acc = 0.f;
      for (int n = 0; n < W; ++n) acc = fmaf(hp[n], d1[n], acc);
      const int64_t e = g.offKs + (int64_t)w * g.Rs + s;
      grad_out[e] = (d0[w] + acc) * dphi[e];
    }
    return;
  }
  const int64_t e = (int64_t)(blockIdx.x - g.Rs) * PH_T + tid;
  if (e < g.nparams) {
    if (e >= g.offKs && e < g.offB) return;  // the spectral ranks' blocks write these
    const int64_t src = gmap[e];
    float s = 0.f;
    for (int b = 0; b < nslabs; ++b) s += gpart[(int64_t)b * g.slab + src];
    grad_out[e] = e < g.offB ? s * dphi[e] : s;
  } else if (e == g.nparams) {
    double l = 0.0;
    for (int b = 0; b < nslabs; ++b) l += dpart[b];
    grad_out[g.nparams] = (float)(l * loss_scale);
    grad_out[g.nparams + 1] = 0.f;
  }
}

// k_update_conv (tr_conv.hip) restated with the smoothness term; the reference's sum is
//   loss_rec + L2(Bcp_w) + L2(Bcp_n) + loss_spectral (0: not offered) + loss_smoothness   (…py:1412)
struct PhaseLam {
  float v[4];  // by arena factor: Bd, Bo, Kn, Ks
};

__global__ __launch_bounds__(1024) void k_update_conv_phase(FactorSet fs, int n_bias, PhaseLam lam, PhaseSmooth sm,
                                                            int W, int Rn, int Rs, float* __restrict__ params,
                                                            const float* __restrict__ grad, UpdateArgs ua,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            float* __restrict__ vmax,
                                                            float* __restrict__ grad_total_out,
                                                            float* __restrict__ loss_out,
                                                            double* __restrict__ loss_hist,
                                                            int32_t* __restrict__ stop) {
#pragma clang fp contract(off)
  __shared__ float wsum[4 * 16];
  __shared__ float norms[4];
  __shared__ float coef[4];
  __shared__ float ssum[2 * 16];
  __shared__ float sval[2];
  __shared__ float sd[(CONV_MAXW + PHASE_MAXQ) * CONV_MAXR];  // Delta^q of [Kn | Ks], (W + q) x (Rn + Rs)
  const int t = threadIdx.x, lane = t & 63, q = t >> 6;
  const int64_t nfe = fs.nfelem, np = nfe + n_bias;
  const bool checked = ua.mode == 0 && stop != nullptr;
  const int32_t stop0 = stop != nullptr ? *stop : 0;
  const float status = checked ? grad[np + 1] : 0.f;
  auto factor_of = [&](int64_t e) {
    int f = 0;
#pragma unroll
    for (int g = 1; g < 4; ++g)
      if (e >= fs.off[g]) f = g;
    return f;
  };
  float accn[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t k = t; k < nfe; k += 1024) {
    const float a = params[k];
    const int f = factor_of(k);
#pragma unroll
    for (int g = 0; g < 4; ++g) accn[g] = g == f ? fmaf(a, a, accn[g]) : accn[g];
  }
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const float r = tr_wave_allreduce(accn[f]);
    if (lane == 0) wsum[f * 16 + q] = r;
  }
  // Delta^q of the raw kernels and the two sums of its squares
  const int ord = sm.order, Wq = W + ord, Rk = Rn + Rs;
  float accs[2] = {0.f, 0.f};
  for (int idx = t; idx < Wq * Rk; idx += 1024) {
    const int i = idx / Rk, c = idx - i * Rk;
    const float* col = c < Rn ? params + fs.off[2] + c : params + fs.off[3] + (c - Rn);
    const int ld = c < Rn ? Rn : Rs;
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
    const float r = tr_wave_allreduce(accs[f]);
    if (lane == 0) ssum[f * 16 + q] = r;
  }
  __syncthreads();
  if (t < 4) {
    float tot = 0.f;
    for (int w = 0; w < 16; ++w) tot += wsum[t * 16 + w];
    norms[t] = sqrtf(tot);
    coef[t] = lam.v[t] / (2.0f * norms[t]);
  } else if (t >= 64 && t < 66) {
    const int f = t - 64;
    float tot = 0.f;
    for (int w = 0; w < 16; ++w) tot += ssum[f * 16 + w];
    const int rf = f == 0 ? Rn : Rs;
    sval[f] = rf > 0 ? (tot / (float)(Wq * rf)) * sm.lam : 0.f;  // torch.mean(...) * lambda_smooth
  }
  __syncthreads();
  if (stop0 != 0) return;
  if (checked && status != 0.0f) {
    if (t == 0) *stop = TR_STOP_DEVICE_ERROR - (int32_t)ua.iter;
    return;
  }
  const bool adam = ua.mode != 1;
  const bool ams = adam && ua.amsgrad;
  for (int64_t e = t; e < np; e += 1024) {
    float g = grad[e], p = params[e];
    if (e < nfe) {
      const int f = factor_of(e);
      g = g + coef[f] * (2.0f * p);
      if (f >= 2) {
        const int rf = f == 2 ? Rn : Rs;
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
    g = ua.weight_decay != 0.0f ? fmaf(p, ua.weight_decay, g) : g;
    mm = fmaf(ua.one_minus_b1, g - mm, mm);
    vv = vv * ua.beta2;
    vv = vv + ua.one_minus_b2 * g * g;
    vm = fmaxf(vm, vv);
    if (ams) vmax[e] = vm;
    const float denom = sqrtf(ams ? vm : vv) / ua.bc2_sqrt + ua.eps;
    p = p + (-ua.step_size) * (mm / denom);
    m[e] = mm;
    v[e] = vv;
    params[e] = p;
  }
  if (t == 0) {
    const float pw = (0.f + norms[2] * lam.v[2]) + norms[3] * lam.v[3];
    const float pn = (0.f + norms[0] * lam.v[0]) + norms[1] * lam.v[1];
    float ps = 0.f;  // an empty factor is skipped (comp.numel() > 0, …py:954)
    if (Rn > 0) ps = ps + sval[0];
    if (Rs > 0) ps = ps + sval[1];
    const float total = ((grad[np] + pw) + pn) + ps;
    if (loss_out != nullptr) *loss_out = total;
    if (ua.mode == 0 && loss_hist != nullptr) loss_hist[ua.hist_base + ua.iter] = (double)total;
    // the reference tests the plateau once len(loss_running) > patience, else the NaN stop (…py:1445-1452)
    if (ua.mode == 0 && ua.nan_stop && stop != nullptr && ua.hist_base + ua.iter + 1 <= ua.patience &&
        __builtin_isnan(total))
      *stop = -(int32_t)(ua.iter + 1);
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
bool phase_geom_init(ConvGeom* g, int64_t n_w, int64_t n_d, int64_t n_out, int rank_normal, int rank_spectral,
                     const int32_t* non_negative, std::string* why) {
  if (!conv_geom_init(g, n_w, n_d, n_out, rank_normal, rank_spectral, 2, non_negative, why)) return false;
  // the arena holds one kernel per spectral rank; the slab and the groups keep the pair
  g->offB = g->offKs + (int64_t)g->W * g->Rs;
  g->nparams = g->offB + g->N;
  return true;
}

void phase_build_filter(int W, float* h2) {
  const double pi = 3.14159265358979323846;
  std::vector<double> h((size_t)W, 0.0);
  for (int d = 0; d < W; ++d) {
    double s = 0.0;
    for (int j = 1; j <= (W - 1) / 2; ++j) s += std::sin(2.0 * pi * (double)j * (double)d / (double)W);
    h[d] = 2.0 * s / (double)W;
  }
  for (int i = 0; i < 2 * W; ++i) h2[i] = (float)h[i % W];
}

void phase_build_gmap(const ConvGeom& g, int32_t* gmap) {
  for (int64_t e = 0; e < g.offKn; ++e) gmap[e] = (int32_t)e;  // Bd, Bo: same place in arena and slab
  for (int n = 0; n < g.N; ++n) gmap[g.offB + n] = (int32_t)(g.sOffB + n);
  for (int gi = 0; gi < g.G; ++gi) {
    const ConvGroup& gr = g.grp[gi];
    for (int j = 0; j < gr.nr; ++j) {
      const int r = gr.rbase + j;
      for (int w = 0; w < g.W; ++w) {
        const int64_t arena =
            r < g.Rn ? g.offKn + (int64_t)w * g.Rn + r : g.offKs + (int64_t)w * g.Rs + (r - g.Rn);
        gmap[arena] = (int32_t)(g.sOffK + ((int64_t)gi * g.W + w) * CONV_KC + j * gr.cc);
      }
    }
  }
}

void phase_smooth_init(PhaseSmooth* s, float lambda_smooth, int order) {
  std::memset(s, 0, sizeof(*s));
  s->lam = lambda_smooth;
  s->order = order;
  double c = 1.0;  // (-1)^j C(q, j)
  for (int j = 0; j <= order; ++j) {
    s->c[j] = (float)c;
    c = -c * (double)(order - j) / (double)(j + 1);
  }
}

hipError_t launch_phase_kp(const ConvGeom& g, const float* phi, const float* h2, float* Kp, const int32_t* stop,
                           hipStream_t st) {
  hipLaunchKernelGGL(k_phase_kp, dim3(g.R), dim3(PH_T), 0, st, g, phi, h2, Kp, stop);
  return hipGetLastError();
}

hipError_t launch_phase_finish(const ConvGeom& g, int nslabs, const float* gpart, const double* dpart,
                               const int32_t* gmap, const float* dphi, const float* h2, double loss_scale,
                               float* grad_out, const int32_t* stop, hipStream_t st) {
  const int64_t n = g.nparams + 1;
  hipLaunchKernelGGL(k_phase_finish, dim3((unsigned)(g.Rs + (n + PH_T - 1) / PH_T)), dim3(PH_T), 0, st, g, nslabs,
                     gpart, dpart, gmap, dphi, h2, loss_scale, grad_out, stop);
  return hipGetLastError();
}

hipError_t launch_update_conv_phase(const FactorSet& fs, int n_bias, const float lam[4], const PhaseSmooth& sm, int W,
                                    int Rn, int Rs, float* params, const float* grad, const UpdateArgs& ua, float* m,
                                    float* v, float* vmax, float* grad_total_out, float* loss_out, double* loss_hist,
                                    int32_t* stop, hipStream_t st) {
  if (fs.nf != 4 || sm.order < 0 || sm.order > PHASE_MAXQ || W > CONV_MAXW || Rn + Rs > CONV_MAXR)
    return hipErrorInvalidValue;
  PhaseLam l;
  for (int i = 0; i < 4; ++i) l.v[i] = lam[i];
  hipLaunchKernelGGL(k_update_conv_phase, dim3(1), dim3(1024), 0, st, fs, n_bias, l, sm, W, Rn, Rs, params, grad, ua,
                     m, v, vmax, grad_total_out, loss_out, loss_hist, stop);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t n_losses = ua.hist_base + ua.iter + 1;
  if (ua.mode == 0 && loss_hist != nullptr && stop != nullptr && ua.patience >= 0 && n_losses > ua.patience &&
      ua.tol > 0.0)
    e = launch_converge_tail(loss_hist, n_losses, ua.iter, ua.patience, ua.tol, stop, st);
  return e;
}

}  // namespace tr
