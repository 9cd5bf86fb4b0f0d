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
//   k_update_conv   tr_conv.hip, SMOOTH = true with Ks seen as (W, Rs): the smoothness term over the
//                   raw Kn and Ks, and this reference's plateau slice loss_running[-patience+1:].
// No float atomics anywhere; every sum has one fixed order: two runs are bitwise equal.
// Bounds: Kp and the slab's dKp are (G, W, 16) and a rank's group / column come from the same
// rule as conv_geom_init's groups; LDS arrays are sized by CONV_MAXW.
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

}  // namespace tr
