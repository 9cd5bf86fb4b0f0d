// tr_mnl_resident.h — the resident multinomial fit (tr_mnl_resident.hip): one workgroup on one CU
// holds X, the factors and the Adam state in LDS and runs whole fit_Adam iterations per launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tr {

constexpr int RES_T = 1024;           // threads of the one workgroup
constexpr int RES_MAX_ITERS = 64;     // iterations per launch (the host-sync interval of the fit loop)
constexpr int RES_MAX_C = 16;         // classes (a sample's logits live in registers)
constexpr int RES_MAX_R = 16;
constexpr int64_t RES_LDS_BYTES = 160 * 1024;

// Shape and LDS image of one problem.  Offsets are in 4-byte words from the start of dynamic LDS.
struct ResGeom {
  int N, I0, I1, P, C, R;
  int XP;    // row pitch of the X image: odd, so lanes over samples (Z pass) hit 32 distinct banks;
             // lanes over features (G pass) read consecutive words either way
  int CP;    // row pitch of Z / dZ: odd, same reason
  int S;     // sample splits of the G pass (S * P * C <= RES_T work items, 1 <= S <= 8)
  int np;    // (I0 + I1 + C) * R parameters
  int off1, off2;  // parameter offsets of factors 1 and 2
  int oX, oB, oG, oGp, oZ, oY, oW, oPar, oM, oV, oVm, oPhi, oDphi, oGrad, oNorm;
  int words;  // total, including the leading 16 fp64 loss partials and the control words
};

// False outside the envelope: two feature modes are the caller's to check; here C <= 16, R <= 16 and
// the carve within 160 KiB.
bool resident_geom(int64_t N, int64_t I0, int64_t I1, int C, int R, ResGeom* g);

struct ResArgs {
  ResGeom g;
  int nonneg[3];
  float beta, thr;
  float lambda_l2;
  float one_minus_b1, beta2, one_minus_b2, eps, weight_decay;
  int amsgrad;
  int n_iters;             // 1 .. RES_MAX_ITERS
  int64_t hist_base, iter0, patience;
  double tol;
  float inv_n;             // 1 / N (unweighted CrossEntropyLoss mean)
  float step_size[3][RES_MAX_ITERS];  // lr_f / (1 - b1^t) of iteration iter0 + k
  float bc2_sqrt[RES_MAX_ITERS];      // sqrt(1 - b2^t)
};

hipError_t prepare_resident();
hipError_t launch_resident(const ResArgs& a, const float* X, int64_t xld, const int64_t* target, float* params,
                           const float* w, float* m, float* v, float* vmax, double* loss_hist, int32_t* stop,
                           hipStream_t st);
hipError_t touch_code_object_mnl_resident();

}  // namespace tr
