// Stand-alone check of the shared-X multinomial sweep's host side (tensor_regression_amd/csrc/
// tr_mnl_many.h), built with -fsanitize=address,undefined by tests/test_mnl_many_host.py.  Member tables
// are built into heap blocks of exactly mnl_many_table_bytes(n); every workspace carve is walked piece
// by piece against its byte count for the GPU test shapes and the envelope's edges; the column packing
// (prefix sums, a member straddling tiles, exactly 64 and 65 columns) and the per-member checks, which
// name the bad member and leave the table untouched.  Exit status 0 and "mnl many ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "check.h"
#include "tr_mnl_many.h"

namespace {

// never dereferenced by the host code: distinct non-NULL addresses inside static blocks
float g_f[16];
int64_t g_y[1];
double g_h[1];
int32_t g_stop[64];

tr_mnl_many_member member(int j, int n_classes) {
  tr_mnl_many_member m;
  std::memset(&m, 0, sizeof(m));
  m.params = g_f;
  m.weights = g_f + 1;
  m.y = g_y;
  m.class_weights = g_f + 2;
  m.exp_avg = g_f + 3;
  m.exp_avg_sq = g_f + 4;
  m.max_exp_avg_sq = (j % 3 == 0) ? g_f + 5 : nullptr;
  m.grad = g_f + 6;
  m.loss_hist = g_h;
  m.stop_flag = g_stop + j;
  m.cw_norm = 100.0 + j;
  m.n_classes = n_classes;
  static const int ranks[4] = {1, 3, 8, 32};
  m.rank = ranks[j % 4];
  m.nonneg[0] = j & 1;
  m.nonneg[1] = (j >> 1) & 1;
  m.nonneg[2] = (j >> 2) & 1;
  m.amsgrad = (j % 3 == 0) ? 1 : 0;
  m.softplus_beta = 50.f;
  m.softplus_threshold = 1.f;
  m.lambda_l2 = 0.01f + 0.001f * (float)j;
  m.n_iters = (j == 2) ? 0 : (j == 4 ? 7 : 64);
  m.lr = 0.01 + 0.002 * j;
  m.beta1 = (j == 3) ? 0.8 : 0.9;  // two distinct beta pairs among the members
  m.beta2 = (j == 3) ? 0.99 : 0.999;
  m.eps = 1e-8;
  m.weight_decay = (j == 3) ? 0.01 : 0.0;
  m.step = 65;
  m.hist_base = 5;
  m.iter = 64;
  m.patience = 10;
  m.tol = 1e-5;
  return m;
}

void check_geom(int64_t N, int64_t I0, int64_t I1) {
  using namespace tr;
  MmGeom g;
  CHECK(mnl_many_geom(N, I0, I1, &g));
  const int64_t P = I0 * I1;
  CHECK(g.P == P && g.N == N);
  // the forward's slices cover the features, each a multiple of the fold length
  CHECK(g.slice % MM_FOLD == 0 && g.slice >= MM_FOLD && g.ns >= 1);
  CHECK(g.ns * g.slice >= P && (g.ns - 1) * g.slice < P);
  CHECK(g.nrw * MM_FWD_ROWS >= N && (g.nrw - 1) * MM_FWD_ROWS < N);
  CHECK(g.nepi * MM_EPI_ROWS >= N && (g.nepi - 1) * MM_EPI_ROWS < N);
  // the gradient's chunks cover the rows, none empty
  CHECK(g.rpc % 8 == 0 && g.nch >= 1 && g.nch <= MM_MAX_CHUNKS);
  CHECK(g.nch * g.rpc >= N && (g.nch - 1) * g.rpc < N);
  CHECK(g.nfw * MM_GRAD_FEATS >= P && (g.nfw - 1) * MM_GRAD_FEATS < P);
  CHECK(g.npmax == (I0 + I1 + MM_MAX_C) * MM_MAX_R && g.nh == (I0 + I1) * MM_MAX_R);
  // the carve: in order, 256-byte aligned, nothing overlapping, the total as reported
  const int64_t npad = g.nepi * MM_EPI_ROWS;
  const struct {
    int64_t at, bytes;
  } piece[] = {{g.oBt, MM_MAX_COLS * P * 4},
               {g.oG, MM_MAX_COLS * P * 4},
               {g.oPhi, MM_MAX_MEMBERS * g.npmax * 4},
               {g.oDphi, MM_MAX_MEMBERS * g.npmax * 4},
               {g.oR, npad * MM_MAX_COLS * 4},
               {g.oZ, g.ns * npad * MM_MAX_COLS * 4},
               {g.oD, g.nepi * MM_MAX_MEMBERS * 8},
               {g.oH, MM_MAX_COLS * g.nh * 4},
               {g.oGp, g.nch * MM_MAX_COLS * P * 4}};
  int64_t end = 0;
  for (const auto& p : piece) {
    CHECK(p.at >= end && p.at % 256 == 0 && p.bytes > 0);
    CHECK(p.at + p.bytes <= g.bytes);
    end = p.at + p.bytes;
  }
  if (g.bytes < (int64_t(1) << 25)) {  // small carves are laid into a heap block of exactly that size
    unsigned char* ws = static_cast<unsigned char*>(std::malloc((size_t)g.bytes));
    CHECK(ws != nullptr);
    if (ws != nullptr) {
      for (const auto& p : piece) {
        ws[p.at] = 1;
        ws[p.at + p.bytes - 1] = 2;
      }
      std::free(ws);
    }
  }
}

// builds the table of the given class counts into a heap block of exact size and checks the packing
void check_packing(const std::vector<int>& classes, int want_rc) {
  using namespace tr;
  const int M = (int)classes.size();
  std::vector<tr_mnl_many_member> ms;
  for (int j = 0; j < M; ++j) ms.push_back(member(j, classes[j]));
  const size_t bytes = (size_t)mnl_many_table_bytes(M);
  CHECK(bytes == (size_t)M * sizeof(MmMember) + sizeof(MmCols));
  unsigned char* table = static_cast<unsigned char*>(std::malloc(bytes));
  CHECK(table != nullptr);
  if (table == nullptr) return;
  std::memset(table, 0x5a, bytes);
  int n_active = 0, n_cols = -1, bad = 0;
  const char* why = nullptr;
  const int rc = build_mnl_many_table(ms.data(), M, true, true, MM_MAX_ITERS, table, &n_active, &n_cols, &bad, &why,
                                      nullptr);
  CHECK(rc == want_rc);
  if (rc != 0) {
    CHECK(bad == -1 && why != nullptr && why[0] != '\0' && n_cols == 0);
    for (size_t k = 0; k < bytes; ++k) CHECK(table[k] == 0x5a);  // untouched
  } else {
    const MmMember* rows = reinterpret_cast<const MmMember*>(table);
    MmCols cols;
    std::memcpy(&cols, table + (size_t)M * sizeof(MmMember), sizeof(cols));
    int col0 = 0;
    for (int j = 0; j < M; ++j) {
      CHECK(rows[j].col0 == col0 && rows[j].n_classes == classes[j]);
      for (int c = 0; c < classes[j]; ++c) CHECK(cols.member[col0 + c] == j && cols.cls[col0 + c] == c);
      col0 += classes[j];
    }
    CHECK(cols.total == col0 && n_cols == col0 && cols.tiles == (col0 + MM_TILE - 1) / MM_TILE);
    for (int c = col0; c < MM_MAX_COLS; ++c) CHECK(cols.member[c] == -1 && cols.cls[c] == -1);
  }
  std::free(table);
}

}  // namespace

int main() {
  using namespace tr;
  // the envelope's edges
  CHECK(mnl_many_envelope(8, 12, 0, 5, 32) && !mnl_many_envelope(8, 12, 0, 5, 33) && !mnl_many_envelope(8, 12, 0, 5, 0));
  CHECK(mnl_many_envelope(8, 12, 0, 2, 4) && !mnl_many_envelope(8, 12, 0, 1, 4));         // classes 2..16
  CHECK(mnl_many_envelope(8, 12, 0, 16, 4) && !mnl_many_envelope(8, 12, 0, 17, 4));
  CHECK(!mnl_many_envelope(3, 3, 0, 5, 2) && mnl_many_envelope(3, 4, 0, 5, 2));           // P % 4
  CHECK(!mnl_many_envelope(6, 5, 0, 3, 2));                                               // (160, 6, 5): P = 30
  CHECK(!mnl_many_envelope(8, 12, 98, 5, 2) && mnl_many_envelope(8, 12, 100, 5, 2));      // stride % 4
  CHECK(mnl_many_envelope(9, 12, 12, 4, 2));                                              // stride < P: a windowed view
  CHECK(!mnl_many_envelope(8, 12, -4, 5, 2) && !mnl_many_envelope(0, 12, 0, 5, 2));
  CHECK(!mnl_many_envelope(MM_MAX_DIM, MM_MAX_DIM, 0, 5, 2));
  CHECK(mnl_many_envelope(1 << 14, 1 << 14, 0, 5, 2) && !mnl_many_envelope(1 << 15, 1 << 14, 0, 5, 2));  // P <= 2^28
  CHECK(!mnl_many_geom(0, 8, 12, nullptr) && !mnl_many_geom(5, 3, 3, nullptr));

  const int64_t shapes[][3] = {{1, 2, 2},      {3, 8, 4},     {37, 8, 12},      {130, 16, 16},      {257, 24, 20},
                               {64, 16, 8},    {48, 256, 128}, {292, 9, 12},    {96, 128, 64},      {2000, 500, 500},
                               {65536, 128, 64}, {1000000, 4, 4}, {1, 1 << 14, 1 << 14}};
  for (const auto& s : shapes) check_geom(s[0], s[1], s[2]);
  {  // the shape of a pass does not depend on anything but (N, I0, I1): two builds agree byte for byte
    MmGeom a, b;
    CHECK(mnl_many_geom(257, 24, 20, &a) && mnl_many_geom(257, 24, 20, &b) && std::memcmp(&a, &b, sizeof(a)) == 0);
    CHECK(a.nepi == 2 && a.nch >= 2);  // the GPU test's shape: two epilogue workgroups, several gradient chunks
  }

  // column packing: prefix sums, straddling members, exactly 64 columns, 65 columns, 32 members of 2, 33 members
  check_packing({5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5}, 0);  // member 3 owns 15..19: straddles tiles 0 and 1
  check_packing({3, 3, 3, 3, 3}, 0);                       // 15 columns: one tile
  check_packing({3, 3, 3, 3, 3, 3}, 0);                    // 18: two
  check_packing({16, 16, 16, 16}, 0);                      // exactly 64
  check_packing({2, 5, 16, 3, 7}, 0);
  check_packing({16, 16, 16, 16, 2}, TR_E_ARG);            // 66
  check_packing({13, 13, 13, 13, 13}, TR_E_ARG);           // 65
  check_packing(std::vector<int>(32, 2), 0);
  check_packing(std::vector<int>(33, 2), TR_E_ARG);

  const int M = 8;
  std::vector<tr_mnl_many_member> ms;
  for (int j = 0; j < M; ++j) ms.push_back(member(j, 2 + j));
  const size_t bytes = (size_t)mnl_many_table_bytes(M);
  unsigned char* table = static_cast<unsigned char*>(std::malloc(bytes));
  CHECK(table != nullptr);
  if (table == nullptr) return 1;
  int n_active = 0, n_cols = 0, bad = 0;
  const char* why = nullptr;
  AdamMemo memo;
  CHECK(build_mnl_many_table(ms.data(), M, true, true, MM_MAX_ITERS, table, &n_active, &n_cols, &bad, &why, &memo) == 0);
  CHECK(bad == -1 && n_active == M - 1 && n_cols == 2 + 3 + 4 + 5 + 6 + 7 + 8 + 9);
  CHECK(memo.computed == 2 * MM_MAX_ITERS);  // two beta pairs x 64 steps, not one set per member
  const MmMember* rows = reinterpret_cast<const MmMember*>(table);
  for (int j = 0; j < M; ++j) {
    const tr_mnl_many_member& m = ms[j];
    const MmMember& t = rows[j];
    for (int k = 0; k < MM_MAX_ITERS; ++k) {
      if (k < m.n_iters) {
        const AdamScalars as = adam_scalars(m.beta1, m.beta2, m.step + k);
        CHECK(t.step_size[k] == (float)(m.lr / as.bc1) && t.bc2_sqrt[k] == (float)as.bc2_sqrt);
      } else {
        CHECK(t.step_size[k] == 0.f && t.bc2_sqrt[k] == 0.f);
      }
    }
    CHECK(t.n_iters == m.n_iters && t.iter0 == m.iter && t.hist_base == m.hist_base && t.patience == m.patience);
    CHECK(t.params == m.params && t.w == m.weights && t.y == m.y && t.cw == m.class_weights && t.m == m.exp_avg &&
          t.v == m.exp_avg_sq && t.vmax == m.max_exp_avg_sq && t.grad == m.grad && t.loss_hist == m.loss_hist &&
          t.stop == m.stop_flag);
    CHECK(t.rank == m.rank && t.nonneg[0] == m.nonneg[0] && t.nonneg[1] == m.nonneg[1] && t.nonneg[2] == m.nonneg[2] &&
          t.amsgrad == m.amsgrad);
    CHECK(t.cw_norm == m.cw_norm && t.inv_w == (float)(1.0 / m.cw_norm));
    CHECK(t.one_minus_b1 == (float)(1.0 - m.beta1) && t.beta2 == (float)m.beta2 && t.eps == (float)m.eps);
  }
  // an evaluation alone needs no Adam buffers and leaves every n_iters at 0; a step alone needs no labels
  {
    std::vector<tr_mnl_many_member> v = ms;
    for (auto& m : v) m.exp_avg = nullptr, m.stop_flag = nullptr, m.n_iters = 99;
    std::vector<unsigned char> t2(bytes);
    CHECK(build_mnl_many_table(v.data(), M, true, false, 0, t2.data(), &n_active, &n_cols, &bad, &why, nullptr) == 0);
    CHECK(n_active == 0 && reinterpret_cast<const MmMember*>(t2.data())[3].n_iters == 0);
    v = ms;
    for (auto& m : v) m.y = nullptr, m.class_weights = nullptr, m.cw_norm = 0.0, m.n_iters = 1;
    CHECK(build_mnl_many_table(v.data(), M, false, true, 1, t2.data(), &n_active, &n_cols, &bad, &why, nullptr) == 0);
    CHECK(n_active == M);
  }

  // a failing member: its code, its index, and the table left as it was
  struct Bad {
    int at, code;
    void (*spoil)(tr_mnl_many_member&);
  };
  const Bad bads[] = {
      {3, TR_E_ARG, [](tr_mnl_many_member& m) { m.n_iters = 65; }},
      {0, TR_E_ARG, [](tr_mnl_many_member& m) { m.n_iters = -1; }},
      {5, TR_E_ARG, [](tr_mnl_many_member& m) { m.params = nullptr; }},
      {6, TR_E_ARG, [](tr_mnl_many_member& m) { m.stop_flag = nullptr; }},
      {7, TR_E_ARG, [](tr_mnl_many_member& m) { m.grad = nullptr; }},
      {2, TR_E_ARG, [](tr_mnl_many_member& m) { m.y = nullptr; }},
      {4, TR_E_ARG, [](tr_mnl_many_member& m) { m.class_weights = nullptr; }},
      {1, TR_E_ARG, [](tr_mnl_many_member& m) { m.amsgrad = 1; }},  // (member 1 has no max_exp_avg_sq)
      {4, TR_E_ARG, [](tr_mnl_many_member& m) { m.step = 0; }},
      {4, TR_E_ARG, [](tr_mnl_many_member& m) { m.lr = -1.0; }},
      {2, TR_E_ARG, [](tr_mnl_many_member& m) { m.hist_base = -1; }},
      {6, TR_E_ARG, [](tr_mnl_many_member& m) { m.cw_norm = 0.0; }},
      {5, TR_E_ARG, [](tr_mnl_many_member& m) { m.cw_norm = -3.0; }},
      {7, TR_E_UNSUPPORTED, [](tr_mnl_many_member& m) { m.rank = 33; }},
      {2, TR_E_UNSUPPORTED, [](tr_mnl_many_member& m) { m.rank = 0; }},
      {0, TR_E_UNSUPPORTED, [](tr_mnl_many_member& m) { m.n_classes = 1; }},
      {3, TR_E_UNSUPPORTED, [](tr_mnl_many_member& m) { m.n_classes = 17; }},
  };
  std::vector<unsigned char> before(bytes);
  std::memcpy(before.data(), table, bytes);
  for (const Bad& b : bads) {
    std::vector<tr_mnl_many_member> v = ms;
    b.spoil(v[b.at]);
    CHECK(build_mnl_many_table(v.data(), M, true, true, MM_MAX_ITERS, table, &n_active, &n_cols, &bad, &why, &memo) ==
          b.code);
    CHECK(bad == b.at && why != nullptr && why[0] != '\0');
    CHECK(std::memcmp(before.data(), table, bytes) == 0);
  }
  std::free(table);
  CHECK(build_mnl_many_table(ms.data(), 0, true, true, MM_MAX_ITERS, nullptr, &n_active, &n_cols, &bad, &why, nullptr) == 0);
  CHECK(n_active == 0 && n_cols == 0);
  if (g_failed) return 1;
  std::puts("mnl many ok");
  return 0;
}
