// tr_mnl_many.h — the shared-X multinomial sweep (tr_mnl_many.hip): CP multinomial models with two
// feature modes and a class factor fitted over ONE X.  A model with C classes is C columns of a dense
// coefficient matrix; a group holds up to 64 columns (four 16-column MFMA tiles), so that an iteration
// reads X twice whatever the number of models.  This header holds the host side: the geometry of a
// pass (MmGeom: feature slices, row chunks, the carve of the caller's workspace), the device table
// (MmMember rows and the MmCols column map that follows them, built from the public
// tr_mnl_many_member) and the per-member checks.  No HIP dependency: tests/cpp/mnl_many_check.cpp
// compiles it with the host compiler alone.  The launchers at the end take the stream as void*.
#pragma once

#include <stdint.h>

#include <cstring>

#include "../../include/tensor_regression_hip.h"
#include "tr_member_table.h"

namespace tr {

constexpr int MM_MAX_COLS = 64;       // columns of one call: four 16x16x4 MFMA tiles
constexpr int MM_TILE = 16;
constexpr int MM_MAX_C = 16;          // classes of a member (2..16)
constexpr int MM_MAX_MEMBERS = 32;    // 64 columns / 2 classes
constexpr int MM_MAX_R = 32;
constexpr int MM_MAX_ITERS = 64;      // iterations per call of tr_mnl_many_fit (the host-sync interval)
constexpr int MM_FWD_ROWS = 128;      // rows of one forward workgroup: 4 waves x 2 tiles of 16 rows
constexpr int MM_FOLD = 512;          // features between two folds of the forward's 2 accumulator chains
constexpr int MM_MIN_SLICE = 1024;    // features of a forward slice at least (a multiple of MM_FOLD)
constexpr int MM_EPI_ROWS = 256;      // rows of one epilogue workgroup (one fp64 partial per member)
constexpr int MM_GRAD_FEATS = 128;    // features of one gradient wave (2 column tiles of 64)
constexpr int MM_GRAD_MIN_ROWS = 128; // rows of a gradient chunk at least
constexpr int MM_MAX_CHUNKS = 64;
constexpr int64_t MM_MAX_DIM = int64_t(1) << 20;
constexpr int64_t MM_MAX_P = int64_t(1) << 28;  // 64 * P * 4 bytes of Bt stay below 2^36
constexpr int64_t MM_MAX_ROWS = int64_t(1) << 30;

// The envelope of a shape: two feature modes of I0 x I1, P = I0 * I1 and the row stride (in floats,
// 0 = P) multiples of 4 (16-byte loads of X rows), 2..16 classes, rank 1..32.
inline bool mnl_many_envelope(int64_t I0, int64_t I1, int64_t xld, int n_classes, int rank) {
  if (I0 < 1 || I1 < 1 || I0 > MM_MAX_DIM || I1 > MM_MAX_DIM) return false;
  const int64_t P = I0 * I1;
  if (P > MM_MAX_P || (P & 3) != 0) return false;
  if (xld < 0 || (xld & 3) != 0) return false;
  if (n_classes < 2 || n_classes > MM_MAX_C) return false;
  return rank >= 1 && rank <= MM_MAX_R;
}

// One pass over (N, I0, I1).  Depends on the shape alone, never on the members, their columns or the
// number of column tiles in use: a member's bits depend neither on its neighbours nor on its position.
struct MmGeom {
  int64_t N, I0, I1, P;
  int64_t npmax;     // (I0 + I1 + MM_MAX_C) * MM_MAX_R: a member's phi / dphi slot, in floats
  int64_t nh;        // (I0 + I1) * MM_MAX_R: a column's slot of the fold's first stage, in floats
  int64_t nrw;       // forward workgroups over the rows
  int64_t slice;     // features per forward slice (a multiple of MM_FOLD)
  int64_t ns;        // forward slices
  int64_t nepi;      // epilogue workgroups
  int64_t nfw;       // gradient waves over the features
  int64_t nch, rpc;  // gradient row chunks and rows per chunk (a multiple of 8)
  int64_t oBt, oG, oPhi, oDphi, oR, oZ, oD, oH, oGp, bytes;
};

inline bool mnl_many_geom(int64_t N, int64_t I0, int64_t I1, MmGeom* g) {
  if (N < 1 || N > MM_MAX_ROWS || !mnl_many_envelope(I0, I1, 0, 2, 1)) return false;
  MmGeom q;
  std::memset(&q, 0, sizeof(q));
  q.N = N;
  q.I0 = I0;
  q.I1 = I1;
  q.P = I0 * I1;
  q.npmax = (I0 + I1 + MM_MAX_C) * MM_MAX_R;
  q.nh = (I0 + I1) * MM_MAX_R;
  q.nrw = (N + MM_FWD_ROWS - 1) / MM_FWD_ROWS;
  // forward: about 1024 workgroups over rows x slices; a slice is at least MM_MIN_SLICE features
  int64_t ns = (1024 + q.nrw - 1) / q.nrw;
  const int64_t ns_max = (q.P + MM_MIN_SLICE - 1) / MM_MIN_SLICE;
  if (ns > ns_max) ns = ns_max;
  if (ns < 1) ns = 1;
  q.slice = ((q.P + ns - 1) / ns + MM_FOLD - 1) / MM_FOLD * MM_FOLD;
  q.ns = (q.P + q.slice - 1) / q.slice;
  q.nepi = (N + MM_EPI_ROWS - 1) / MM_EPI_ROWS;
  // gradient: about 2048 waves over feature blocks x row chunks (a 64-column slab is four times the
  // linear sweep's, so fewer, longer chunks)
  q.nfw = (q.P + MM_GRAD_FEATS - 1) / MM_GRAD_FEATS;
  int64_t nch = (2048 + q.nfw - 1) / q.nfw;
  const int64_t by_rows = (N + MM_GRAD_MIN_ROWS - 1) / MM_GRAD_MIN_ROWS;
  if (nch > by_rows) nch = by_rows;
  if (nch > MM_MAX_CHUNKS) nch = MM_MAX_CHUNKS;
  if (nch < 1) nch = 1;
  q.rpc = ((N + nch - 1) / nch + 7) / 8 * 8;
  q.nch = (N + q.rpc - 1) / q.rpc;
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += (bytes + 255) / 256 * 256;
    return at;
  };
  const int64_t npad = q.nepi * MM_EPI_ROWS;
  q.oBt = take(MM_MAX_COLS * q.P * 4);
  q.oG = take(MM_MAX_COLS * q.P * 4);
  q.oPhi = take(MM_MAX_MEMBERS * q.npmax * 4);
  q.oDphi = take(MM_MAX_MEMBERS * q.npmax * 4);
  q.oR = take(npad * MM_MAX_COLS * 4);
  q.oZ = take(q.ns * npad * MM_MAX_COLS * 4);
  q.oD = take(q.nepi * MM_MAX_MEMBERS * 8);
  q.oH = take(MM_MAX_COLS * q.nh * 4);
  q.oGp = take(q.nch * MM_MAX_COLS * q.P * 4);
  q.bytes = o;
  if (g != nullptr) *g = q;
  return true;
}

// One row of the device table: kernels select their member by blockIdx.y.
struct MmMember {
  float* params;        // factors 0, 1 and the class factor (I0 x R, I1 x R, C x R)
  const float* w;
  const int64_t* y;
  const float* cw;
  float *m, *v, *vmax;
  float* grad;          // num_params + 2: factor gradients, data loss, status
  double* loss_hist;
  int32_t* stop;
  double cw_norm;       // W = sum_n cw[y_n]
  float inv_w;          // (float)(1 / W)
  int rank, n_classes, col0, nonneg[3], amsgrad;
  float beta, thr, lambda_l2;
  float one_minus_b1, beta2, one_minus_b2, eps, weight_decay;
  int n_iters;
  int64_t hist_base, iter0, patience;
  double tol;
  float step_size[MM_MAX_ITERS];  // lr / (1 - b1^t) of iteration iter0 + k
  float bc2_sqrt[MM_MAX_ITERS];   // sqrt(1 - b2^t)
};

// The column map, which follows the n_members rows of the table: column -> (member, class), -1 past
// the group's total (those columns of Bt and R are zero).
struct MmCols {
  int32_t total, tiles, pad[2];
  int32_t member[MM_MAX_COLS];
  int32_t cls[MM_MAX_COLS];
};

inline int64_t mnl_many_table_bytes(int n_members) {
  return n_members < 0 ? 0 : (int64_t)n_members * (int64_t)sizeof(MmMember) + (int64_t)sizeof(MmCols);
}

// want_step: the call updates (tr_mnl_many_step / _fit) and needs the Adam buffers; want_grad: it
// evaluates (tr_mnl_many_loss_grad / _fit) and needs the labels and the weights.
inline int check_mnl_many_member(const tr_mnl_many_member& m, bool want_grad, bool want_step, int max_iters,
                                 const char** why) {
  *why = "";
  if (m.params == nullptr || m.grad == nullptr) {
    *why = "NULL buffer";
    return TR_E_ARG;
  }
  if (want_grad) {
    if (m.weights == nullptr || m.y == nullptr || m.class_weights == nullptr) {
      *why = "NULL buffer";
      return TR_E_ARG;
    }
    if (!(m.cw_norm > 0.0)) {
      *why = "cw_norm must be > 0";
      return TR_E_ARG;
    }
  }
  if (want_step) {
    if (int rc = check_adam_member(m, max_iters, why)) return rc;
    if (!(m.lr >= 0.0)) {
      *why = "the learning rate must be >= 0";
      return TR_E_ARG;
    }
  }
  if (m.n_classes < 2 || m.n_classes > MM_MAX_C) {
    *why = "n_classes outside 2..16";
    return TR_E_UNSUPPORTED;
  }
  if (m.rank < 1 || m.rank > MM_MAX_R) {
    *why = "rank outside 1..32";
    return TR_E_UNSUPPORTED;
  }
  return 0;
}

// Checks the call's shape and every member, then writes the table (`table`: mnl_many_table_bytes(n)
// bytes, the rows and then the column map): nothing is written unless all pass.  *bad is the first
// offending member's index (-1: the call's own arguments).  Member j owns the columns col0_j ..
// col0_j + C_j - 1, col0 the running sum of the class counts; a member may straddle a tile boundary.
inline int build_mnl_many_table(const tr_mnl_many_member* members, int n_members, bool want_grad, bool want_step,
                                int max_iters, void* table, int* n_active, int* n_cols, int* bad, const char** why,
                                AdamMemo* memo) {
  *bad = -1;
  *n_active = 0;
  *n_cols = 0;
  *why = "";
  if (n_members < 0 || n_members > MM_MAX_MEMBERS) {
    *why = "n_members outside 0..32";
    return TR_E_ARG;
  }
  int total = 0;
  for (int j = 0; j < n_members; ++j) {
    if (int rc = check_mnl_many_member(members[j], want_grad, want_step, max_iters, why)) {
      *bad = j;
      return rc;
    }
    total += members[j].n_classes;
  }
  if (total > MM_MAX_COLS) {
    *why = "the members' class counts sum to more than 64 columns";
    return TR_E_ARG;
  }
  if (n_members == 0) return 0;
  MmMember* rows = static_cast<MmMember*>(table);
  MmCols cols;
  std::memset(&cols, 0, sizeof(cols));
  for (int c = 0; c < MM_MAX_COLS; ++c) cols.member[c] = cols.cls[c] = -1;
  int col0 = 0;
  for (int j = 0; j < n_members; ++j) {
    const tr_mnl_many_member& m = members[j];
    MmMember& t = rows[j];
    std::memset(&t, 0, sizeof(t));
    t.params = m.params;
    t.w = m.weights;
    t.y = m.y;
    t.cw = m.class_weights;
    t.m = m.exp_avg;
    t.v = m.exp_avg_sq;
    t.vmax = m.max_exp_avg_sq;
    t.grad = m.grad;
    t.loss_hist = m.loss_hist;
    t.stop = m.stop_flag;
    t.cw_norm = want_grad ? m.cw_norm : 1.0;
    t.inv_w = (float)(1.0 / t.cw_norm);
    t.rank = m.rank;
    t.n_classes = m.n_classes;
    t.col0 = col0;
    for (int f = 0; f < 3; ++f) t.nonneg[f] = m.nonneg[f] != 0 ? 1 : 0;
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
    for (int c = 0; c < m.n_classes; ++c) {
      cols.member[col0 + c] = j;
      cols.cls[col0 + c] = c;
    }
    col0 += m.n_classes;
  }
  cols.total = total;
  cols.tiles = (total + MM_TILE - 1) / MM_TILE;
  std::memcpy(static_cast<char*>(table) + (size_t)n_members * sizeof(MmMember), &cols, sizeof(cols));
  *n_cols = total;
  return 0;
}

// ---- launchers (tr_mnl_many.hip); `stream` is a hipStream_t, the return value a hipError_t ----
// One evaluation: prepare, dense, forward, epilogue, gradient slabs, slab reduction, two fold stages.
// Fills every member's grad arena.  9 launches with the update, whatever the members are.
int launch_mnl_many_loss_grad(const MmGeom& g, const float* X, int64_t xld, const void* table, int n_members,
                              int n_cols, void* workspace, void* stream);
// The update of every member whose stop word is clear and whose n_iters exceeds k.
int launch_mnl_many_update(const MmGeom& g, void* table, int n_members, int k, void* stream);

}  // namespace tr
