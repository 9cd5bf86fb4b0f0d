// tr_conv.h — host-side interface of the convolutional spectral kernels (tr_conv.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "tr_common.h"
#include "tr_kernels.h"

namespace tr {

constexpr int CONV_TT = 256;     // output times per tile (= threads of the workgroup)
constexpr int CONV_KC = 16;      // kernel columns per column group
constexpr int CONV_MAXG = 8;     // column groups at most (K <= 64 gives <= 7)
constexpr int CONV_MAXW = 257;
constexpr int CONV_MAXR = 32;
constexpr int CONV_MAXN = 64;
constexpr int CONV_MAXK = 64;
constexpr int CONV_MAXC = 4;
constexpr int CONV_MAXQ = 8;     // highest difference order of the smoothness term

// Column group: a run of `nr` ranks starting at rank `rbase` whose temporal kernels have `cc`
// components each (normal ranks and spectral ranks with one component: cc = 1, signed; spectral
// ranks with C components: cc = C, magnitude).  Rank j of the group owns columns j*cc .. j*cc+cc-1
// of the group's 16; the rest are zero.
struct ConvGroup {
  int cc, rbase, nr;
};

struct ConvGeom {
  int W, D, N, Rn, Rs, C, R, K;
  int nonneg[3];  // (w, d, out)
  // parameter arena: Bd (D, R) | Bo (N, R) | Kn (W, Rn) | Ks (W, Rs, C) | bias (N)
  int64_t offBd, offBo, offKn, offKs, offB, nparams;
  int G;
  ConvGroup grp[CONV_MAXG];
  // gradient slab of one workgroup: dBd (D, R) | dBo (N, R) | dKp (G, W, 16) | dbias (N)
  int64_t sOffBd, sOffBo, sOffK, sOffB, slab;
  int XP;   // LDS pitch of one column of the X slab (TT + W - 1 rows, odd)
  int DC;   // columns of X per LDS chunk
  size_t lds_bytes;
};

// false + *why outside the envelope (W odd, 1 <= W <= 257, D <= 2^16, N <= 64, 1 <= R <= 32, C <= 4, K <= 64)
bool conv_geom_init(ConvGeom* g, int64_t n_w, int64_t n_d, int64_t n_out, int rank_normal, int rank_spectral,
                    int n_complex, const int32_t* non_negative, std::string* why);
// host maps: kmap[(g*W + w)*16 + col] = arena index of that kernel entry (or -1: padding);
// gmap[e] = slab index of arena element e
void conv_build_maps(const ConvGeom& g, int32_t* kmap, int32_t* gmap);
hipError_t conv_prepare(const ConvGeom& g);
// softplus'd factors -> padded kernel columns Kp (G, W, 16)
hipError_t launch_conv_kp(const ConvGeom& g, const float* phi, const int32_t* kmap, float* Kp, const int32_t* stop,
                          hipStream_t st);
// train = 1: forward + loss + all gradients into the workgroups' slabs; train = 0: y_hat only.
// eadd (T', N), nullable: added to the residual scale * (y_hat - y) before the backward phases
hipError_t launch_conv(int train, const ConvGeom& g, int grid, const float* X, int64_t T, int64_t xld,
                       const float* phi, const float* params, const float* Kp, const float* y, float scale,
                       float* gpart, double* dpart, float* ebuf, const float* eadd, float* yhat, const int32_t* stop,
                       hipStream_t st);
// fixed-order slab sum + softplus chain + loss slot + status slot
hipError_t launch_conv_finish(const ConvGeom& g, int nslabs, const float* gpart, const double* dpart,
                              const int32_t* gmap, const float* dphi, double loss_scale, float* grad_out,
                              const int32_t* stop, hipStream_t st);
// Smoothness term lambda * mean((Delta^q F)^2) of the raw temporal kernels (Kn, Ks) of the phase and
// Fourier models.
struct ConvSmooth {
  float lam;
  int order;                // q, 0..CONV_MAXQ
  float c[CONV_MAXQ + 1];   // (-1)^j C(q, j): the stencil of Delta^q
};
void conv_smooth_init(ConvSmooth* s, float lambda_smooth, int order);
// once per process before a launch_update_conv with a smoothness term: its Delta^q scratch is dynamic
// LDS of up to (257 + 8) x 64 floats
hipError_t conv_update_prepare();
// The update step of the three conv models (one kernel, k_update_conv): L2 term with one lambda per
// factor (lam: Bd, Bo, Kn, Ks) + Adam / AMSGrad step + loss record + stops.
//   sm         nullptr: no smoothness term (conv spectral; W, Rn, RsK are not read).  Else its value and
//              gradient over Kn (W, Rn) and Ks seen as (W, RsK) join the total and the gradient.
//   spec_val   nullable device scalar added to the total between the L2 terms and the smoothness term
//   tail_rule  false: conv spectral's stops (NaN while iter <= patience, then k_converge);
//              true: phase / Fourier's (NaN while hist_base + iter + 1 <= patience, then k_converge_tail)
hipError_t launch_update_conv(const FactorSet& fs, int n_bias, const float lam[4], const ConvSmooth* sm, int W, int Rn,
                              int RsK, const float* spec_val, bool tail_rule, float* params, const float* grad,
                              const UpdateArgs& ua, float* m, float* v, float* vmax, float* grad_total_out,
                              float* loss_out, double* loss_hist, int32_t* stop, hipStream_t st);

}  // namespace tr
