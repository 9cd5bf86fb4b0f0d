// tr_linear_many.h — the shared-X linear sweep (tr_linear_many.hip): up to 16 CP linear models with two
// feature modes fitted over ONE X, so that an iteration reads X twice whatever the number of models.
// This header holds the host side: the geometry of a pass (LmGeom: feature slices, row chunks and the
// carve of the caller's workspace), the device member table (LmMember, built from the public
// tr_linear_member) and the per-member argument checks; and the same for the scoring pass, the forward
// half alone for two or three feature modes (LsGeom, LsWork, LsMember).  No HIP dependency: tests/cpp/
// linear_many_check.cpp compiles it with the host compiler alone.  The launchers at the end take the
// stream as void* for the same reason.
#pragma once

#include <stdint.h>

#include <cstring>

#include "../../include/tensor_regression_hip.h"
#include "tr_member_table.h"
#include "tr_workspace.h"

namespace tr {

constexpr int LM_MAX_M = 16;          // members of one call: the columns of one 16x16x4 MFMA tile
constexpr int LM_MAX_R = 32;
constexpr int LM_MAX_ITERS = 64;      // iterations per call of tr_linear_many_fit (the host-sync interval)
constexpr int LM_FWD_ROWS = 128;      // rows of one forward workgroup: 4 waves x 2 tiles of 16 rows
constexpr int LM_FOLD = 512;          // features between two folds of the forward's 8 accumulator chains
constexpr int LM_MIN_SLICE = 1024;    // features of a forward slice at least (a multiple of LM_FOLD)
constexpr int LM_EPI_ROWS = 256;      // rows of one epilogue workgroup (one pair of fp64 partials per column)
constexpr int LM_GRAD_FEATS = 256;    // features of one gradient wave (4 column tiles of 64)
constexpr int LM_GRAD_MIN_ROWS = 128; // rows of a gradient chunk at least (slab traffic <= 1/4 of X's)
constexpr int LM_MAX_CHUNKS = 64;
constexpr int64_t LM_MAX_DIM = int64_t(1) << 20;
constexpr int64_t LM_MAX_P = int64_t(1) << 30;
constexpr int64_t LM_MAX_ROWS = int64_t(1) << 30;

// The envelope of a shape: two feature modes of I0 x I1, P = I0 * I1 and the row stride (in floats,
// 0 = P) multiples of 4 (16-byte loads of X rows), rank 1..32.  A stride below P is a windowed view.
inline bool linear_many_envelope(int64_t I0, int64_t I1, int64_t xld, int rank) {
  if (I0 < 1 || I1 < 1 || I0 > LM_MAX_DIM || I1 > LM_MAX_DIM) return false;
  const int64_t P = I0 * I1;
  if (P > LM_MAX_P || (P & 3) != 0) return false;
  if (xld < 0 || (xld & 3) != 0) return false;
  return rank >= 1 && rank <= LM_MAX_R;
}

// One pass over (N, I0, I1): how the forward splits the features, how the gradient splits the rows,
// and where the pieces of the workspace lie (byte offsets, each a multiple of 256).  Depends on the
// shape alone, never on the members: a member's bits do not depend on its neighbours.
struct LmGeom {
  int64_t N, I0, I1, P;
  int64_t npmax;     // (I0 + I1) * LM_MAX_R: a member's phi / dphi slot, in floats
  int64_t nrw;       // forward workgroups over the rows
  int64_t slice;     // features per forward slice (a multiple of LM_FOLD)
  int64_t ns;        // forward slices
  int64_t nepi;      // epilogue workgroups
  int64_t nfw;       // gradient waves over the features
  int64_t nch, rpc;  // gradient row chunks and rows per chunk (a multiple of 8)
  int64_t oBt, oG, oPhi, oDphi, oR, oZ, oD, oGp, bytes;
};

// The forward's split of (N, P), shared with the scoring pass (LsGeom): about 1024 workgroups (4 per
// CU) over rows x slices; a slice is at least LM_MIN_SLICE features, so the Z partials stay below 1/32
// of X's bytes.
inline void lm_forward_split(int64_t N, int64_t P, int64_t* nrw, int64_t* slice, int64_t* n_slices) {
  *nrw = (N + LM_FWD_ROWS - 1) / LM_FWD_ROWS;
  int64_t ns = (1024 + *nrw - 1) / *nrw;
  const int64_t ns_max = (P + LM_MIN_SLICE - 1) / LM_MIN_SLICE;
  if (ns > ns_max) ns = ns_max;
  if (ns < 1) ns = 1;
  *slice = ((P + ns - 1) / ns + LM_FOLD - 1) / LM_FOLD * LM_FOLD;
  *n_slices = (P + *slice - 1) / *slice;
}

inline bool linear_many_geom(int64_t N, int64_t I0, int64_t I1, LmGeom* g) {
  if (N < 1 || N > LM_MAX_ROWS || !linear_many_envelope(I0, I1, 0, 1)) return false;
  LmGeom q;
  std::memset(&q, 0, sizeof(q));
  q.N = N;
  q.I0 = I0;
  q.I1 = I1;
  q.P = I0 * I1;
  q.npmax = (I0 + I1) * LM_MAX_R;
  lm_forward_split(N, q.P, &q.nrw, &q.slice, &q.ns);
  q.nepi = (N + LM_EPI_ROWS - 1) / LM_EPI_ROWS;
  // gradient: about 4096 waves over feature blocks x row chunks
  q.nfw = (q.P + LM_GRAD_FEATS - 1) / LM_GRAD_FEATS;
  int64_t nch = (4096 + q.nfw - 1) / q.nfw;
  const int64_t by_rows = (N + LM_GRAD_MIN_ROWS - 1) / LM_GRAD_MIN_ROWS;
  if (nch > by_rows) nch = by_rows;
  if (nch > LM_MAX_CHUNKS) nch = LM_MAX_CHUNKS;
  if (nch < 1) nch = 1;
  q.rpc = ((N + nch - 1) / nch + 7) / 8 * 8;
  q.nch = (N + q.rpc - 1) / q.rpc;
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += (bytes + 255) / 256 * 256;
    return at;
  };
  const int64_t npad = q.nepi * LM_EPI_ROWS;
  q.oBt = take(LM_MAX_M * q.P * 4);
  q.oG = take(LM_MAX_M * q.P * 4);
  q.oPhi = take(LM_MAX_M * q.npmax * 4);
  q.oDphi = take(LM_MAX_M * q.npmax * 4);
  q.oR = take(npad * LM_MAX_M * 4);
  q.oZ = take(q.ns * npad * LM_MAX_M * 4);
  q.oD = take(q.nepi * LM_MAX_M * 2 * 8);
  q.oGp = take(q.nch * LM_MAX_M * q.P * 4);
  q.bytes = o;
  if (g != nullptr) *g = q;
  return true;
}

// One row of the device table: kernels select their member by blockIdx.y (or the column of a tile).
struct LmMember {
  float* params;        // factors 0, 1 (I0 x R, I1 x R), then the bias
  const float* w;
  const float* y;
  float *m, *v, *vmax;
  float* grad;          // num_params + 2: factor gradients, bias gradient, data loss, status
  double* loss_hist;
  int32_t* stop;
  int rank, nonneg[2], amsgrad;
  float beta, thr, lambda_l2;
  float one_minus_b1, beta2, one_minus_b2, eps, weight_decay;
  int n_iters;
  int64_t hist_base, iter0, patience;
  double tol;
  float step_size[LM_MAX_ITERS];  // lr / (1 - b1^t) of iteration iter0 + k
  float bc2_sqrt[LM_MAX_ITERS];   // sqrt(1 - b2^t)
};

// want_step: the call updates (tr_linear_many_step / _fit) and needs the Adam buffers; want_grad: it
// evaluates (tr_linear_many_loss_grad / _fit) and needs y and the weights.
inline int check_linear_member(const tr_linear_member& m, bool want_grad, bool want_step, int max_iters,
                               const char** why) {
  *why = "";
  if (m.params == nullptr || m.grad == nullptr) {
    *why = "NULL buffer";
    return TR_E_ARG;
  }
  if (want_grad && (m.weights == nullptr || m.y == nullptr)) {
    *why = "NULL buffer";
    return TR_E_ARG;
  }
  if (want_step) {
    if (int rc = check_adam_member(m, max_iters, why)) return rc;
    if (!(m.lr >= 0.0)) {
      *why = "the learning rate must be >= 0";
      return TR_E_ARG;
    }
  }
  if (m.rank < 1 || m.rank > LM_MAX_R) {
    *why = "rank outside 1..32";
    return TR_E_UNSUPPORTED;
  }
  return 0;
}

// Checks the call's shape and every member, then writes the table: nothing is written unless all
// pass.  *bad is the first offending member's index (-1: the call's own arguments).
inline int build_linear_table(const tr_linear_member* members, int n_members, bool want_grad, bool want_step,
                              int max_iters, LmMember* table, int* n_active, int* bad, const char** why,
                              AdamMemo* memo) {
  *bad = -1;
  *n_active = 0;
  *why = "";
  if (n_members < 0 || n_members > LM_MAX_M) {
    *why = "n_members outside 0..16";
    return TR_E_ARG;
  }
  for (int j = 0; j < n_members; ++j)
    if (int rc = check_linear_member(members[j], want_grad, want_step, max_iters, why)) {
      *bad = j;
      return rc;
    }
  for (int j = 0; j < n_members; ++j) {
    const tr_linear_member& m = members[j];
    LmMember& t = table[j];
    std::memset(&t, 0, sizeof(t));
    t.params = m.params;
    t.w = m.weights;
    t.y = m.y;
    t.m = m.exp_avg;
    t.v = m.exp_avg_sq;
    t.vmax = m.max_exp_avg_sq;
    t.grad = m.grad;
    t.loss_hist = m.loss_hist;
    t.stop = m.stop_flag;
    t.rank = m.rank;
    t.nonneg[0] = m.nonneg[0] != 0 ? 1 : 0;
    t.nonneg[1] = m.nonneg[1] != 0 ? 1 : 0;
    t.beta = m.softplus_beta;
    t.thr = m.softplus_threshold;
    t.lambda_l2 = m.lambda_l2;
    fill_adam_scalars(&t, m.beta1, m.beta2, m.eps, m.weight_decay, m.amsgrad);
    t.n_iters = want_step ? m.n_iters : 0;
    t.hist_base = m.hist_base;
    t.iter0 = m.iter;
    t.patience = m.patience;
    t.tol = m.tol;
    fill_adam_rows(memo, m.beta1, m.beta2, m.step, t.n_iters, &m.lr, 1, &t.step_size, t.bc2_sqrt);
    if (t.n_iters > 0) ++*n_active;
  }
  return 0;
}

// ---- scoring: the forward half alone (tr_linear_many_score) ----
constexpr int LS_SUMS = 5;  // sum e^2, sum (yhat - k), sum (yhat - k)^2, sum (y - k), sum (y - k)^2; k = y[0]

// Two or three feature modes; P, the stride and the rank as linear_many_envelope.
inline bool linear_score_envelope(int n_modes, const int64_t* dims, int64_t xld, int rank) {
  if ((n_modes != 2 && n_modes != 3) || dims == nullptr) return false;
  int64_t P = 1;
  for (int f = 0; f < n_modes; ++f) {
    if (dims[f] < 1 || dims[f] > LM_MAX_DIM) return false;
    if (P > LM_MAX_P / dims[f]) return false;
    P *= dims[f];
  }
  if ((P & 3) != 0) return false;
  if (xld < 0 || (xld & 3) != 0) return false;
  return rank >= 1 && rank <= LM_MAX_R;
}

// A scoring pass over (N, dims): the forward's split is lm_forward_split's, so Z is the fit's bit for
// bit; nothing of the gradient half (LmGeom's R, G and slabs) is there.
struct LsGeom {
  int64_t N, P;
  int n_modes;
  int64_t I[3];
  int64_t isum;      // I0 + I1 (+ I2): the bias sits at params[isum * rank]
  int64_t npmax;     // isum * LM_MAX_R: a member's phi slot, in floats
  int64_t nrw, slice, ns, nepi;
};

inline bool linear_score_geom(int64_t N, int n_modes, const int64_t* dims, LsGeom* g) {
  if (N < 1 || N > LM_MAX_ROWS || !linear_score_envelope(n_modes, dims, 0, 1)) return false;
  LsGeom q;
  std::memset(&q, 0, sizeof(q));
  q.N = N;
  q.n_modes = n_modes;
  q.P = 1;
  for (int f = 0; f < n_modes; ++f) {
    q.I[f] = dims[f];
    q.P *= dims[f];
    q.isum += dims[f];
  }
  q.npmax = q.isum * LM_MAX_R;
  lm_forward_split(N, q.P, &q.nrw, &q.slice, &q.ns);
  q.nepi = (N + LM_EPI_ROWS - 1) / LM_EPI_ROWS;
  if (g != nullptr) *g = q;
  return true;
}

// The pieces of the scoring workspace.  dphi is k_lm_prep's second output, which the two-mode pass
// shares with the fit; the three-mode prepare writes phi alone and the piece is absent.
struct LsWork {
  float *Bt, *phi, *dphi, *Z;
  double* D;
};

inline void linear_score_carve(const LsGeom& g, LsWork* w, Carver* c) {
  const size_t npad = (size_t)(g.nepi * LM_EPI_ROWS);
  c->add(&w->Bt, (size_t)LM_MAX_M * (size_t)g.P * 4);
  c->add(&w->phi, (size_t)LM_MAX_M * (size_t)g.npmax * 4);
  c->add_optional(&w->dphi, g.n_modes == 2 ? (size_t)LM_MAX_M * (size_t)g.npmax * 4 : 0);
  c->add(&w->Z, (size_t)g.ns * npad * LM_MAX_M * 4);
  c->add(&w->D, (size_t)g.nepi * LM_MAX_M * LS_SUMS * 8);
}

// What the kernels read of a scoring member beside its LmMember row (params, w, y, rank, nonneg[0..1],
// beta, thr: the fields k_lm_prep and k_lm_dense read).  The device table is n LmMember rows followed
// by n LsMember rows.
struct LsMember {
  float* yhat;   // NULL: not wanted
  double* sums;  // LS_SUMS doubles (y != NULL)
  int nonneg2;   // the third factor's flag
  int pad;
};

inline int64_t linear_score_table_bytes(int n_members) {
  return n_members < 0 ? 0 : (int64_t)n_members * (int64_t)(sizeof(LmMember) + sizeof(LsMember));
}

inline int check_linear_score_member(const tr_linear_score_member& m, const char** why) {
  *why = "";
  if (m.params == nullptr || m.weights == nullptr) {
    *why = "NULL buffer";
    return TR_E_ARG;
  }
  if (m.y != nullptr && m.sums == nullptr) {
    *why = "y without sums";
    return TR_E_ARG;
  }
  if (m.y == nullptr && m.yhat == nullptr) {
    *why = "neither yhat nor y";
    return TR_E_ARG;
  }
  if (m.rank < 1 || m.rank > LM_MAX_R) {
    *why = "rank outside 1..32";
    return TR_E_UNSUPPORTED;
  }
  return 0;
}

// build_linear_table's contract: every member is checked, then the two tables are written; nothing is
// written unless all pass.
inline int build_linear_score_table(const tr_linear_score_member* members, int n_members, LmMember* table,
                                    LsMember* ext, int* bad, const char** why) {
  *bad = -1;
  *why = "";
  if (n_members < 0 || n_members > LM_MAX_M) {
    *why = "n_members outside 0..16";
    return TR_E_ARG;
  }
  for (int j = 0; j < n_members; ++j)
    if (int rc = check_linear_score_member(members[j], why)) {
      *bad = j;
      return rc;
    }
  for (int j = 0; j < n_members; ++j) {
    const tr_linear_score_member& m = members[j];
    LmMember& t = table[j];
    std::memset(&t, 0, sizeof(t));
    t.params = const_cast<float*>(m.params);  // (the scoring kernels only read it)
    t.w = m.weights;
    t.y = m.y;
    t.rank = m.rank;
    t.nonneg[0] = m.nonneg[0] != 0 ? 1 : 0;
    t.nonneg[1] = m.nonneg[1] != 0 ? 1 : 0;
    t.beta = m.softplus_beta;
    t.thr = m.softplus_threshold;
    LsMember& e = ext[j];
    std::memset(&e, 0, sizeof(e));
    e.yhat = m.yhat;
    e.sums = m.y != nullptr ? m.sums : nullptr;
    e.nonneg2 = m.nonneg[2] != 0 ? 1 : 0;
  }
  return 0;
}

// ---- launchers (tr_linear_many.hip); `stream` is a hipStream_t, the return value a hipError_t ----
// The scoring pass: prepare, dense build, forward, score, sum.  5 launches whatever n_members is.
int launch_linear_many_score(const LsGeom& g, const float* X, int64_t xld, const LmMember* table, const LsMember* ext,
                             int n_members, const LsWork& w, void* stream);
// One evaluation: prepare, forward, epilogue, gradient slabs, slab reduction, fold.  Fills every
// member's grad arena.  8 launches with the update, whatever n_members is.
int launch_linear_many_loss_grad(const LmGeom& g, const float* X, int64_t xld, const LmMember* table, int n_members,
                                 void* workspace, void* stream);
// The update of every member whose stop word is clear and whose n_iters exceeds k.
int launch_linear_many_update(const LmGeom& g, LmMember* table, int n_members, int k, void* stream);

}  // namespace tr
