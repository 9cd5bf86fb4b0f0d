// tr_mnl_resident_table.h — the host side of the resident multinomial fit's arguments: the LDS carve
// (resident_geom), the argument block of one fit (ResArgs, filled by fill_res_args for the single
// launch and for every member of a batch alike) and the member table of k_mnl_resident_many
// (ResMember, built from the public tr_resident_member).  No HIP dependency: tests/cpp/
// resident_many_check.cpp compiles this header with the host compiler alone.
#pragma once

#include <stdint.h>

#include <cstdio>
#include <cstring>

#include "../../include/tensor_regression_hip.h"
#include "tr_member_table.h"

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
inline bool resident_geom(int64_t N, int64_t I0, int64_t I1, int C, int R, ResGeom* g) {
  if (N < 1 || I0 < 1 || I1 < 1 || C < 1 || C > RES_MAX_C || R < 1 || R > RES_MAX_R) return false;
  const int64_t P = I0 * I1;
  if (N > 65536 || P > 65536) return false;  // far past what 160 KiB holds; keeps the words in int
  const int64_t XP = P | 1, CP = C | 1, PC = P * C;
  int64_t S = RES_T / PC;
  if (S > 8) S = 8;
  if (S > N) S = N;
  if (S < 1) S = 1;
  const int64_t np = (I0 + I1 + C) * R;
  int64_t o = 32 + 8;  // 16 fp64 loss partials, then the control words
  auto take = [&](int64_t n) {
    const int64_t at = o;
    o += (n + 3) & ~(int64_t)3;
    return at;
  };
  const int64_t oX = take(N * XP), oB = take(PC), oG = take(PC), oGp = take(S > 1 ? S * PC : 0), oZ = take(N * CP),
                oY = take(N), oW = take(R), oPar = take(np), oM = take(np), oV = take(np), oVm = take(np),
                oPhi = take(np), oDphi = take(np), oGrad = take(np), oNorm = take(8);
  if (o * 4 > RES_LDS_BYTES) return false;
  if (g != nullptr) {
    *g = ResGeom{(int)N, (int)I0, (int)I1, (int)P, C, R, (int)XP, (int)CP, (int)S, (int)np, (int)(I0 * R),
                 (int)((I0 + I1) * R), (int)oX, (int)oB, (int)oG, (int)oGp, (int)oZ, (int)oY, (int)oW, (int)oPar,
                 (int)oM, (int)oV, (int)oVm, (int)oPhi, (int)oDphi, (int)oGrad, (int)oNorm, (int)o};
  }
  return true;
}

struct ResArgs {
  ResGeom g;
  int nonneg[3];
  float beta, thr;
  float lambda_l2;
  float one_minus_b1, beta2, one_minus_b2, eps, weight_decay;
  int amsgrad;
  int n_iters;             // 1 .. RES_MAX_ITERS (0 in a member table: the member does nothing)
  int64_t hist_base, iter0, patience;
  double tol;
  float inv_n;             // 1 / N (unweighted CrossEntropyLoss mean)
  float step_size[3][RES_MAX_ITERS];  // lr_f / (1 - b1^t) of iteration iter0 + k
  float bc2_sqrt[RES_MAX_ITERS];      // sqrt(1 - b2^t)
};

// One row of k_mnl_resident_many's table: workgroup j fits member j from its own arguments and buffers.
struct ResMember {
  ResArgs a;
  const float* X;
  int64_t xld;
  const int64_t* target;
  float* params;
  const float* w;
  float *m, *v, *vmax;
  double* loss_hist;
  int32_t* stop;
};

// The argument block of n_iters iterations from loop index `iter` (Adam step count `step`, step + 1, ...)
// on the carve `g`: tr_fit_adam_resident's and every table member's.  `memo` may be NULL.
inline void fill_res_args(ResArgs* a, const ResGeom& g, const int* nonneg, float sp_beta, float sp_thr,
                          float lambda_l2, const double* lr, double beta1, double beta2, double eps,
                          double weight_decay, int amsgrad, int64_t step, int n_iters, int64_t hist_base,
                          int64_t iter, int64_t patience, double tol, AdamMemo* memo) {
  std::memset(a, 0, sizeof(*a));
  a->g = g;
  for (int f = 0; f < 3; ++f) a->nonneg[f] = nonneg[f] != 0 ? 1 : 0;
  a->beta = sp_beta;
  a->thr = sp_thr;
  a->lambda_l2 = lambda_l2;
  fill_adam_scalars(a, beta1, beta2, eps, weight_decay, amsgrad);
  a->n_iters = n_iters;
  a->hist_base = hist_base;
  a->iter0 = iter;
  a->patience = patience;
  a->tol = tol;
  a->inv_n = (float)(1.0 / (double)g.N);
  fill_adam_rows(memo, beta1, beta2, step, n_iters, lr, 3, a->step_size, a->bc2_sqrt);
}

// The argument checks of one member of tr_fit_adam_resident_many; no device is touched.  Returns 0
// with the member's carve in *g, or TR_E_ARG / TR_E_UNSUPPORTED with the reason in `why`.
inline int check_resident_member(const tr_resident_member& m, ResGeom* g, const char** why) {
  *why = "";
  if (m.X == nullptr || m.target == nullptr || m.params == nullptr || m.weights == nullptr) {
    *why = "NULL buffer";
    return TR_E_ARG;
  }
  if (int rc = check_adam_member(m, RES_MAX_ITERS, why)) return rc;
  if (m.n_rows < 1) {
    *why = "n_rows must be >= 1";
    return TR_E_ARG;
  }
  if (m.x_row_stride < 0) {
    *why = "x_row_stride must be >= 0";
    return TR_E_ARG;
  }
  for (int f = 0; f < 3; ++f)
    if (!(m.lr[f] >= 0.0)) {
      *why = "learning rates must be >= 0";
      return TR_E_ARG;
    }
  if (!resident_geom(m.n_rows, m.I0, m.I1, m.n_classes, m.rank, g)) {
    *why = "outside the resident envelope";
    return TR_E_UNSUPPORTED;
  }
  return 0;
}

// Checks every member, then writes the table: nothing is written unless all members pass.  On failure
// `*bad` is the first offending member's index.  `*lds_bytes` is the launch's dynamic LDS size (the
// largest carve among the members), `*n_active` the number of members with n_iters > 0.
inline int build_resident_table(const tr_resident_member* members, int n_members, ResMember* table,
                                int64_t* lds_bytes, int* n_active, int* bad, const char** why, AdamMemo* memo) {
  *lds_bytes = 0;
  *n_active = 0;
  *bad = -1;
  ResGeom g;
  for (int j = 0; j < n_members; ++j)
    if (int rc = check_resident_member(members[j], &g, why)) {
      *bad = j;
      return rc;
    }
  for (int j = 0; j < n_members; ++j) {
    const tr_resident_member& m = members[j];
    ResMember& t = table[j];
    resident_geom(m.n_rows, m.I0, m.I1, m.n_classes, m.rank, &g);
    fill_res_args(&t.a, g, m.nonneg, m.softplus_beta, m.softplus_threshold, m.lambda_l2, m.lr, m.beta1, m.beta2,
                  m.eps, m.weight_decay, m.amsgrad, m.step, m.n_iters, m.hist_base, m.iter, m.patience, m.tol, memo);
    t.X = m.X;
    t.xld = m.x_row_stride == 0 ? (int64_t)g.P : m.x_row_stride;
    t.target = static_cast<const int64_t*>(m.target);
    t.params = m.params;
    t.w = m.weights;
    t.m = m.exp_avg;
    t.v = m.exp_avg_sq;
    t.vmax = m.max_exp_avg_sq;
    t.loss_hist = m.loss_hist;
    t.stop = m.stop_flag;
    const int64_t b = (int64_t)g.words * 4;
    if (b > *lds_bytes) *lds_bytes = b;
    if (m.n_iters > 0) ++*n_active;
  }
  return 0;
}

}  // namespace tr
