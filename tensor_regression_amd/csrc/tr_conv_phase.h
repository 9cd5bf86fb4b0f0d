// tr_conv_phase.h — host-side interface of the phase-constrained convolutional kernels
// (tr_conv_phase.hip).  The X pass is k_conv (tr_conv.h) with C = 2; these kernels build its
// quadrature pair and fold the pair's gradient back.  The update step is tr_conv.h's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "tr_conv.h"

namespace tr {

// ConvGeom of the phase model: conv_geom_init with C = 2 (the column groups, the slab and the LDS
// carve of k_conv), then the arena re-laid as Bd (D, R) | Bo (N, R) | Kn (W, Rn) | Ks (W, Rs) | bias (N).
bool phase_geom_init(ConvGeom* g, int64_t n_w, int64_t n_d, int64_t n_out, int rank_normal, int rank_spectral,
                     const int32_t* non_negative, std::string* why);
// h2[i] = h[i mod W], i in [0, 2W): the quadrature filter, computed in fp64 and rounded once, laid
// out twice so that h[(a - b) mod W] = h2[a - b + W] for a, b in [0, W)
void phase_build_filter(int W, float* h2);
// gmap[e] = slab index of arena element e; for Ks[w, s] the slab index of column 2j (its pair
// column 2j + 1 follows)
void phase_build_gmap(const ConvGeom& g, int32_t* gmap);
// softplus'd factors -> padded kernel columns Kp (G, W, 16); a spectral rank's two columns are
// phi(Ks)[:, s] and H phi(Ks)[:, s]
hipError_t launch_phase_kp(const ConvGeom& g, const float* phi, const float* h2, float* Kp, const int32_t* stop,
                           hipStream_t st);
// fixed-order slab sum + H^T fold of the pair + softplus chain + loss slot + status slot
hipError_t launch_phase_finish(const ConvGeom& g, int nslabs, const float* gpart, const double* dpart,
                               const int32_t* gmap, const float* dphi, const float* h2, double loss_scale,
                               float* grad_out, const int32_t* stop, hipStream_t st);
}  // namespace tr
