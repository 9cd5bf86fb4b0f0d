// tr_mnl_score_table.h — the host side of the multinomial scoring sweep (tr_mnl_score.hip): the LDS
// image of one member (score_geom), the argument checks of a public tr_score_member and the table of
// k_mnl_score_many (ScoreMember), whose first_block column is the prefix table that maps a workgroup
// to its (member, row block).  No HIP dependency: tests/cpp/score_many_check.cpp compiles this header
// with the host compiler alone.
#pragma once

#include <stdint.h>

#include <cstring>

#include "../../include/tensor_regression_hip.h"

#ifdef __HIPCC__
#define TR_SCORE_HD __host__ __device__
#else
#define TR_SCORE_HD
#endif

namespace tr {

constexpr int SCORE_T = 1024;                  // threads of a workgroup (16 waves)
constexpr int SCORE_ROWS = TR_SCORE_ROW_BLOCK; // rows of one workgroup: a wave takes every 16th of them
constexpr int SCORE_MAX_C = 16;                // classes (a row's logits live in registers)
constexpr int SCORE_MAX_R = 16;
constexpr int64_t SCORE_LDS_BYTES = 160 * 1024;
// workgroups of one launch: HIP takes a grid of at most 2^32 - 1 threads in x (about 1.07e9 rows a call)
constexpr int64_t SCORE_MAX_BLOCKS = 0xFFFFFFFFll / SCORE_T;

// Shape and LDS image of one member.  Offsets are in 4-byte words from the start of dynamic LDS.  X is
// not part of the image (it streams from global memory), so the image does not depend on n_rows.
struct ScoreGeom {
  int I0, I1, P, C, R;
  int np;          // (I0 + I1 + C) * R parameters
  int off1, off2;  // parameter offsets of factors 1 and 2
  int oRed;        // [SCORE_T / 64][2] fp64: a wave's sum of w[y] l and of w[y]
  int oCnt;        // [C * C] int32: the workgroup's part of counts[pred, true]
  int oW;          // [R] component weights
  int oPhi;        // [np] softplus(A) or A
  int oB;          // [C][P] the dense coefficient tensor, class-major: lanes over p read consecutive words
  int words;
};

// False outside the envelope: two feature modes are the caller's to check; here C <= 16, R <= 16 and
// the image within 160 KiB.  The image is smaller than the resident fit's carve of the same shape at
// one row (which holds B twice, X and seven copies of the parameters), so every shape the resident
// route admits at any n_rows is inside.
inline bool score_geom(int64_t I0, int64_t I1, int C, int R, ScoreGeom* g) {
  if (I0 < 1 || I1 < 1 || C < 1 || C > SCORE_MAX_C || R < 1 || R > SCORE_MAX_R) return false;
  if (I0 > 65536 || I1 > 65536) return false;  // far past what 160 KiB holds; keeps the products in int64
  const int64_t P = I0 * I1, PC = P * C, np = (I0 + I1 + C) * R;
  int64_t o = 0;
  auto take = [&](int64_t n) {
    const int64_t at = o;
    o += (n + 3) & ~(int64_t)3;
    return at;
  };
  const int64_t oRed = take(2 * 2 * (SCORE_T / 64)), oCnt = take(SCORE_MAX_C * SCORE_MAX_C), oW = take(SCORE_MAX_R),
                oPhi = take(np), oB = take(PC);
  if (o * 4 > SCORE_LDS_BYTES) return false;
  if (g != nullptr)
    *g = ScoreGeom{(int)I0, (int)I1, (int)P, C, R, (int)np, (int)(I0 * R), (int)((I0 + I1) * R),
                   (int)oRed, (int)oCnt, (int)oW, (int)oPhi, (int)oB, (int)o};
  return true;
}

inline int64_t score_blocks(int64_t n_rows) { return (n_rows + SCORE_ROWS - 1) / SCORE_ROWS; }

// One row of k_mnl_score_many's table.  Workgroups first_block .. first_block + n_blocks - 1 of the
// launch score rows [k * SCORE_ROWS, (k + 1) * SCORE_ROWS) of this member; the last block may be partial.
struct ScoreMember {
  ScoreGeom g;
  int nonneg[3];
  float beta, thr;
  int first_block, n_blocks;
  int64_t n_rows, xld;
  const float* X;
  const int64_t* target;
  const float* params;
  const float* w;
  const float* cw;
  float* prob;
  int64_t* pred;
  int32_t* counts;
  double* loss;
  double* loss_parts;
};

// The argument checks of one member of tr_mnl_score_many; no device is touched.  Returns 0 with the
// member's image in *g, or TR_E_ARG / TR_E_UNSUPPORTED with the reason in `why`.
inline int check_score_member(const tr_score_member& m, ScoreGeom* g, const char** why) {
  *why = "";
  if (m.X == nullptr || m.params == nullptr || m.weights == nullptr) {
    *why = "NULL buffer (X, params, weights)";
    return TR_E_ARG;
  }
  if (m.n_rows < 1) {
    *why = "n_rows must be >= 1";
    return TR_E_ARG;
  }
  if (m.x_row_stride < 0) {
    *why = "x_row_stride must be >= 0";
    return TR_E_ARG;
  }
  if ((m.counts != nullptr || m.loss != nullptr) && m.target == nullptr) {
    *why = "counts and loss need target";
    return TR_E_ARG;
  }
  if (m.loss != nullptr && m.loss_parts == nullptr) {
    *why = "loss needs loss_parts";
    return TR_E_ARG;
  }
  if (!score_geom(m.I0, m.I1, m.n_classes, m.rank, g)) {
    *why = "outside the scoring envelope";
    return TR_E_UNSUPPORTED;
  }
  return 0;
}

// Checks every member, then writes the table: nothing is written unless all members pass.  On failure
// `*bad` is the first offending member's index.  `*lds_bytes` is the launch's dynamic LDS size (the
// largest image among the members), `*total_blocks` the launch's workgroup count, `*any_counts` /
// `*any_loss` whether some member asks for them.
inline int build_score_table(const tr_score_member* members, int n_members, ScoreMember* table, int64_t* lds_bytes,
                             int64_t* total_blocks, int* any_counts, int* any_loss, int* bad, const char** why) {
  *lds_bytes = 0;
  *total_blocks = 0;
  *any_counts = 0;
  *any_loss = 0;
  *bad = -1;
  ScoreGeom g;
  int64_t blocks = 0;
  for (int j = 0; j < n_members; ++j) {
    if (int rc = check_score_member(members[j], &g, why)) {
      *bad = j;
      return rc;
    }
    blocks += score_blocks(members[j].n_rows);
    if (blocks > SCORE_MAX_BLOCKS) {
      *bad = j;
      *why = "more row blocks than one launch's grid holds";
      return TR_E_UNSUPPORTED;
    }
  }
  blocks = 0;
  for (int j = 0; j < n_members; ++j) {
    const tr_score_member& m = members[j];
    ScoreMember& t = table[j];
    std::memset(&t, 0, sizeof(t));
    score_geom(m.I0, m.I1, m.n_classes, m.rank, &t.g);
    for (int f = 0; f < 3; ++f) t.nonneg[f] = m.nonneg[f] != 0 ? 1 : 0;
    t.beta = m.softplus_beta;
    t.thr = m.softplus_threshold;
    t.first_block = (int)blocks;
    t.n_blocks = (int)score_blocks(m.n_rows);
    blocks += t.n_blocks;
    t.n_rows = m.n_rows;
    t.xld = m.x_row_stride == 0 ? (int64_t)t.g.P : m.x_row_stride;
    t.X = m.X;
    t.target = static_cast<const int64_t*>(m.target);
    t.params = m.params;
    t.w = m.weights;
    t.cw = m.class_weights;
    t.prob = m.prob;
    t.pred = m.pred;
    t.counts = m.counts;
    t.loss = m.loss;
    t.loss_parts = m.loss_parts;
    const int64_t b = (int64_t)t.g.words * 4;
    if (b > *lds_bytes) *lds_bytes = b;
    if (m.counts != nullptr) *any_counts = 1;
    if (m.loss != nullptr) *any_loss = 1;
  }
  *total_blocks = blocks;
  return 0;
}

// The member that owns workgroup b of the launch: the last one whose first_block is <= b (every member
// has at least one block, so first_block increases strictly).  The kernel runs this very function.
TR_SCORE_HD inline int score_member_of_block(const ScoreMember* table, int n_members, int total_blocks, int b) {
  int j = (int)(((int64_t)b * n_members) / total_blocks);  // exact when the members have equal block counts
  if (table[j].first_block <= b && b < table[j].first_block + table[j].n_blocks) return j;
  int lo = 0, hi = n_members - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (table[mid].first_block <= b)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

}  // namespace tr
