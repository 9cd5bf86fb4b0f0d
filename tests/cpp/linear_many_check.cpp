// Stand-alone check of the shared-X linear sweep's host side (tensor_regression_amd/csrc/tr_linear_many.h),
// built with -fsanitize=address,undefined by tests/test_linear_many_host.py.  Member tables are built
// into heap blocks of exactly n * sizeof(LmMember); every workspace carve is walked piece by piece
// against its byte count; the per-member checks name the bad member.  Exit status 0 and
// "linear many ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "adam_rows_check.h"  // with check.h
#include "tr_linear_many.h"

namespace {

// never dereferenced by the host code: distinct non-NULL addresses inside static blocks
float g_f[16];
double g_h[1];
int32_t g_stop[32];

tr_linear_member member(int j) {
  tr_linear_member m;
  std::memset(&m, 0, sizeof(m));
  m.params = g_f;
  m.weights = g_f + 1;
  m.y = g_f + 2;
  m.exp_avg = g_f + 3;
  m.exp_avg_sq = g_f + 4;
  m.max_exp_avg_sq = (j % 3 == 0) ? g_f + 5 : nullptr;
  m.grad = g_f + 6;
  m.loss_hist = g_h;
  m.stop_flag = g_stop + j;
  static const int ranks[4] = {1, 3, 8, 32};
  m.rank = ranks[j % 4];
  m.nonneg[0] = j & 1;
  m.nonneg[1] = (j >> 1) & 1;
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
  LmGeom g;
  CHECK(linear_many_geom(N, I0, I1, &g));
  const int64_t P = I0 * I1;
  CHECK(g.P == P && g.N == N);
  // the forward's slices cover the features, each a multiple of the fold length
  CHECK(g.slice % LM_FOLD == 0 && g.slice >= LM_FOLD && g.ns >= 1);
  CHECK(g.ns * g.slice >= P && (g.ns - 1) * g.slice < P);
  CHECK(g.nrw * LM_FWD_ROWS >= N && (g.nrw - 1) * LM_FWD_ROWS < N);
  CHECK(g.nepi * LM_EPI_ROWS >= N && (g.nepi - 1) * LM_EPI_ROWS < N);
  // the gradient's chunks cover the rows, none empty
  CHECK(g.rpc % 8 == 0 && g.nch >= 1 && g.nch <= LM_MAX_CHUNKS);
  CHECK(g.nch * g.rpc >= N && (g.nch - 1) * g.rpc < N);
  CHECK(g.nfw * LM_GRAD_FEATS >= P && (g.nfw - 1) * LM_GRAD_FEATS < P);
  // the carve: in order, 256-byte aligned, nothing overlapping, the total as reported
  const int64_t npad = g.nepi * LM_EPI_ROWS;
  const struct {
    int64_t at, bytes;
  } piece[] = {{g.oBt, LM_MAX_M * P * 4},           {g.oG, LM_MAX_M * P * 4},
               {g.oPhi, LM_MAX_M * g.npmax * 4},    {g.oDphi, LM_MAX_M * g.npmax * 4},
               {g.oR, npad * LM_MAX_M * 4},         {g.oZ, g.ns * npad * LM_MAX_M * 4},
               {g.oD, g.nepi * LM_MAX_M * 16},      {g.oGp, g.nch * LM_MAX_M * P * 4}};
  int64_t end = 0;
  for (const auto& p : piece) {
    CHECK(p.at >= end && p.at % 256 == 0 && p.bytes > 0);
    CHECK(p.at + p.bytes <= g.bytes);
    end = p.at + p.bytes;
  }
  if (g.bytes < (int64_t(1) << 24)) {  // small carves are laid into a heap block of exactly that size
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

}  // namespace

int main() {
  using namespace tr;
  check_adam_rows();
  // the envelope's edges
  CHECK(linear_many_envelope(8, 12, 0, 32) && !linear_many_envelope(8, 12, 0, 33) && !linear_many_envelope(8, 12, 0, 0));
  CHECK(!linear_many_envelope(3, 3, 0, 2) && linear_many_envelope(3, 4, 0, 2));        // P % 4
  CHECK(!linear_many_envelope(8, 12, 98, 2) && linear_many_envelope(8, 12, 100, 2));   // stride % 4
  CHECK(linear_many_envelope(9, 12, 12, 2));                                           // stride < P: a windowed view
  CHECK(!linear_many_envelope(8, 12, -4, 2) && !linear_many_envelope(0, 12, 0, 2));
  CHECK(!linear_many_envelope(LM_MAX_DIM, LM_MAX_DIM, 0, 2));
  CHECK(!linear_many_geom(0, 8, 12, nullptr) && !linear_many_geom(5, 3, 3, nullptr));

  const int64_t shapes[][3] = {{1, 2, 2},     {3, 8, 4},       {37, 8, 12},        {130, 16, 16},    {257, 24, 20},
                               {48, 256, 128}, {292, 9, 12},    {2000, 500, 500},   {65536, 256, 128}, {1000000, 4, 4}};
  for (const auto& s : shapes) check_geom(s[0], s[1], s[2]);

  const int M = 8;
  std::vector<tr_linear_member> ms;
  for (int j = 0; j < M; ++j) ms.push_back(member(j));
  LmMember* table = static_cast<LmMember*>(std::malloc((size_t)M * sizeof(LmMember)));
  CHECK(table != nullptr);
  if (table == nullptr) return 1;
  int n_active = 0, bad = 0;
  const char* why = nullptr;
  AdamMemo memo;
  CHECK(build_linear_table(ms.data(), M, true, true, LM_MAX_ITERS, table, &n_active, &bad, &why, &memo) == 0);
  CHECK(bad == -1 && n_active == M - 1);
  CHECK(memo.computed == 2 * LM_MAX_ITERS);  // two beta pairs x 64 steps, not one set per member
  for (int j = 0; j < M; ++j) {
    const tr_linear_member& m = ms[j];
    const LmMember& t = table[j];
    for (int k = 0; k < LM_MAX_ITERS; ++k) {
      if (k < m.n_iters) {
        const AdamScalars as = adam_scalars(m.beta1, m.beta2, m.step + k);
        CHECK(t.step_size[k] == (float)(m.lr / as.bc1) && t.bc2_sqrt[k] == (float)as.bc2_sqrt);
      } else {
        CHECK(t.step_size[k] == 0.f && t.bc2_sqrt[k] == 0.f);
      }
    }
    CHECK(t.n_iters == m.n_iters && t.iter0 == m.iter && t.hist_base == m.hist_base && t.patience == m.patience);
    CHECK(t.params == m.params && t.w == m.weights && t.y == m.y && t.m == m.exp_avg && t.v == m.exp_avg_sq &&
          t.vmax == m.max_exp_avg_sq && t.grad == m.grad && t.loss_hist == m.loss_hist && t.stop == m.stop_flag);
    CHECK(t.rank == m.rank && t.nonneg[0] == m.nonneg[0] && t.nonneg[1] == m.nonneg[1] && t.amsgrad == m.amsgrad);
    CHECK(t.one_minus_b1 == (float)(1.0 - m.beta1) && t.beta2 == (float)m.beta2 && t.eps == (float)m.eps);
  }
  // an evaluation alone needs no Adam buffers and leaves every n_iters at 0
  {
    std::vector<tr_linear_member> v = ms;
    for (auto& m : v) m.exp_avg = nullptr, m.stop_flag = nullptr, m.n_iters = 99;
    std::vector<LmMember> t2(M);
    CHECK(build_linear_table(v.data(), M, true, false, 0, t2.data(), &n_active, &bad, &why, nullptr) == 0);
    CHECK(n_active == 0 && t2[3].n_iters == 0 && t2[3].step_size[0] == 0.f);
  }

  // a failing member: its code, its index, and the table left as it was
  struct Bad {
    int at, code;
    void (*spoil)(tr_linear_member&);
  };
  const Bad bads[] = {
      {3, TR_E_ARG, [](tr_linear_member& m) { m.n_iters = 65; }},
      {0, TR_E_ARG, [](tr_linear_member& m) { m.n_iters = -1; }},
      {5, TR_E_ARG, [](tr_linear_member& m) { m.params = nullptr; }},
      {6, TR_E_ARG, [](tr_linear_member& m) { m.stop_flag = nullptr; }},
      {7, TR_E_ARG, [](tr_linear_member& m) { m.grad = nullptr; }},
      {2, TR_E_ARG, [](tr_linear_member& m) { m.y = nullptr; }},
      {1, TR_E_ARG, [](tr_linear_member& m) { m.amsgrad = 1; }},  // (member 1 has no max_exp_avg_sq)
      {4, TR_E_ARG, [](tr_linear_member& m) { m.step = 0; }},
      {4, TR_E_ARG, [](tr_linear_member& m) { m.lr = -1.0; }},
      {2, TR_E_ARG, [](tr_linear_member& m) { m.hist_base = -1; }},
      {7, TR_E_UNSUPPORTED, [](tr_linear_member& m) { m.rank = 33; }},
      {2, TR_E_UNSUPPORTED, [](tr_linear_member& m) { m.rank = 0; }},
  };
  std::vector<unsigned char> before((size_t)M * sizeof(LmMember));
  std::memcpy(before.data(), table, before.size());
  for (const Bad& b : bads) {
    std::vector<tr_linear_member> v = ms;
    b.spoil(v[b.at]);
    CHECK(build_linear_table(v.data(), M, true, true, LM_MAX_ITERS, table, &n_active, &bad, &why, &memo) == b.code);
    CHECK(bad == b.at && why != nullptr && why[0] != '\0');
    CHECK(std::memcmp(before.data(), table, before.size()) == 0);
  }
  std::free(table);

  // 16 members accepted, 17 refused before the table is touched, 0 accepted
  {
    std::vector<tr_linear_member> v;
    for (int j = 0; j < 17; ++j) v.push_back(member(j));
    LmMember* t16 = static_cast<LmMember*>(std::malloc(16 * sizeof(LmMember)));
    CHECK(t16 != nullptr);
    if (t16 != nullptr) {
      CHECK(build_linear_table(v.data(), 16, true, true, LM_MAX_ITERS, t16, &n_active, &bad, &why, nullptr) == 0);
      CHECK(build_linear_table(v.data(), 17, true, true, LM_MAX_ITERS, t16, &n_active, &bad, &why, nullptr) == TR_E_ARG);
      CHECK(bad == -1 && why[0] != '\0');
      CHECK(build_linear_table(v.data(), 0, true, true, LM_MAX_ITERS, nullptr, &n_active, &bad, &why, nullptr) == 0);
      CHECK(n_active == 0);
      std::free(t16);
    }
  }
  if (g_failed) return 1;
  std::puts("linear many ok");
  return 0;
}
