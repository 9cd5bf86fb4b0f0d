// Stand-alone check of the resident sweep's host side (tensor_regression_amd/csrc/tr_mnl_resident_table.h),
// built with -fsanitize=address,undefined by tests/test_hier_many_host.py.  Member tables are built
// into heap blocks of exactly n * sizeof(ResMember) for the shapes of the heterogeneous GPU test plus
// the envelope's edge; every carve is laid into a heap block of exactly words * 4 bytes and both ends
// of every piece are written, so an overrun is an ASan report.  Exit status 0 and "resident many ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "adam_rows_check.h"  // with check.h
#include "tr_mnl_resident_table.h"

namespace {

struct Shape {
  int64_t N, I0, I1;
  int C, R;
};

int64_t max_rows(int64_t I0, int64_t I1, int C, int R) {  // tr_mnl_resident_max_rows' bisection
  if (!tr::resident_geom(1, I0, I1, C, R, nullptr)) return 0;
  int64_t lo = 1, hi = 65536;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (tr::resident_geom(mid, I0, I1, C, R, nullptr))
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// never dereferenced by the host code: distinct non-NULL addresses inside one static block
float g_f[16];
int64_t g_y[1];
double g_h[1];
int32_t g_stop[64];

tr_resident_member member(const Shape& s, int j) {
  tr_resident_member m;
  std::memset(&m, 0, sizeof(m));
  m.X = g_f;
  m.target = g_y;
  m.params = g_f + 1;
  m.weights = g_f + 2;
  m.exp_avg = g_f + 3;
  m.exp_avg_sq = g_f + 4;
  m.max_exp_avg_sq = (j % 3 == 0) ? g_f + 5 : nullptr;
  m.loss_hist = g_h;
  m.stop_flag = g_stop + j;
  m.n_rows = s.N;
  m.x_row_stride = (j % 2) ? s.I0 * s.I1 + 4 : 0;
  m.I0 = s.I0;
  m.I1 = s.I1;
  m.n_classes = s.C;
  m.rank = s.R;
  m.nonneg[0] = j & 1;
  m.nonneg[1] = (j >> 1) & 1;
  m.nonneg[2] = (j >> 2) & 1;
  m.amsgrad = (j % 3 == 0) ? 1 : 0;
  m.softplus_beta = 50.f;
  m.softplus_threshold = 1.f;
  m.lambda_l2 = 0.01f + 0.001f * (float)j;
  m.n_iters = (j == 2) ? 0 : (j == 4 ? 7 : 64);
  m.lr[0] = 0.01 + 0.002 * j;
  m.lr[1] = 0.02;
  m.lr[2] = 0.0;
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

void check_carve(const tr::ResGeom& g) {
  const int64_t PC = (int64_t)g.P * g.C;
  const struct {
    int at;
    int64_t n;
  } piece[] = {{32, 8},          {g.oX, (int64_t)g.N * g.XP}, {g.oB, PC},     {g.oG, PC},      {g.oGp, g.S > 1 ? g.S * PC : 0},
               {g.oZ, (int64_t)g.N * g.CP}, {g.oY, g.N},       {g.oW, g.R},    {g.oPar, g.np},  {g.oM, g.np},
               {g.oV, g.np},     {g.oVm, g.np},               {g.oPhi, g.np}, {g.oDphi, g.np}, {g.oGrad, g.np},
               {g.oNorm, 8}};
  CHECK((int64_t)g.words * 4 <= tr::RES_LDS_BYTES);
  CHECK(g.XP >= g.P && (g.XP & 1) && g.CP >= g.C && (g.CP & 1));
  CHECK(g.S >= 1 && g.S <= 8 && g.S <= g.N && (g.S == 1 || g.S * PC <= tr::RES_T));
  CHECK(g.np == (g.I0 + g.I1 + g.C) * g.R && g.off1 == g.I0 * g.R && g.off2 == (g.I0 + g.I1) * g.R);
  float* lds = static_cast<float*>(std::malloc((size_t)g.words * 4));  // exactly the launch's dynamic LDS
  CHECK(lds != nullptr);
  if (lds == nullptr) return;
  int64_t end = 32;  // the 16 fp64 loss partials come first
  for (const auto& p : piece) {
    CHECK(p.at >= end && p.at % 4 == 0);  // in order, nothing overlapping, 16-byte aligned
    CHECK(p.at + p.n <= g.words);
    if (p.n > 0 && p.at + p.n <= g.words) {
      lds[p.at] = 1.f;
      lds[p.at + p.n - 1] = 2.f;
    }
    end = p.at + p.n;
  }
  std::free(lds);
}

}  // namespace

int main() {
  using namespace tr;
  check_adam_rows();
  const int64_t nmax = max_rows(8, 12, 4, 6);
  CHECK(nmax >= 227 && nmax < 65536);
  const std::vector<Shape> shapes = {{1, 2, 3, 2, 1},   {5, 3, 4, 3, 2},   {37, 2, 5, 2, 3}, {40, 8, 12, 4, 6},
                                     {65, 4, 4, 16, 2}, {20, 3, 3, 3, 16}, {30, 33, 8, 4, 2}, {nmax, 8, 12, 4, 6}};
  const int M = (int)shapes.size();
  std::vector<tr_resident_member> ms;
  for (int j = 0; j < M; ++j) ms.push_back(member(shapes[j], j));

  ResMember* table = static_cast<ResMember*>(std::malloc((size_t)M * sizeof(ResMember)));
  CHECK(table != nullptr);
  if (table == nullptr) return 1;
  int64_t lds = 0;
  int n_active = 0, bad = 0;
  const char* why = nullptr;
  AdamMemo memo;
  CHECK(build_resident_table(ms.data(), M, table, &lds, &n_active, &bad, &why, &memo) == 0);
  CHECK(bad == -1 && n_active == M - 1);
  CHECK(memo.computed == 2 * RES_MAX_ITERS);  // two beta pairs x 64 steps, not one set per member

  int64_t want_lds = 0;
  for (int j = 0; j < M; ++j) {
    const tr_resident_member& m = ms[j];
    const ResMember& t = table[j];
    ResGeom g;
    CHECK(resident_geom(m.n_rows, m.I0, m.I1, m.n_classes, m.rank, &g));
    CHECK(std::memcmp(&g, &t.a.g, sizeof(g)) == 0);
    check_carve(t.a.g);
    if ((int64_t)g.words * 4 > want_lds) want_lds = (int64_t)g.words * 4;
    // the single route's argument block (no memo) for the same inputs, byte for byte
    ResArgs one;
    fill_res_args(&one, g, m.nonneg, m.softplus_beta, m.softplus_threshold, m.lambda_l2, m.lr, m.beta1, m.beta2, m.eps,
                  m.weight_decay, m.amsgrad, m.step, m.n_iters, m.hist_base, m.iter, m.patience, m.tol, nullptr);
    CHECK(std::memcmp(&one, &t.a, sizeof(one)) == 0);
    // and the step tables against the formula itself
    for (int k = 0; k < RES_MAX_ITERS; ++k) {
      if (k < m.n_iters) {
        const AdamScalars as = adam_scalars(m.beta1, m.beta2, m.step + k);
        for (int f = 0; f < 3; ++f) CHECK(t.a.step_size[f][k] == (float)(m.lr[f] / as.bc1));
        CHECK(t.a.bc2_sqrt[k] == (float)as.bc2_sqrt);
      } else {
        for (int f = 0; f < 3; ++f) CHECK(t.a.step_size[f][k] == 0.f);
        CHECK(t.a.bc2_sqrt[k] == 0.f);
      }
    }
    CHECK(t.a.n_iters == m.n_iters && t.a.iter0 == m.iter && t.a.hist_base == m.hist_base);
    CHECK(t.a.inv_n == (float)(1.0 / (double)m.n_rows));
    CHECK(t.X == m.X && t.target == m.target && t.params == m.params && t.w == m.weights && t.m == m.exp_avg &&
          t.v == m.exp_avg_sq && t.vmax == m.max_exp_avg_sq && t.loss_hist == m.loss_hist && t.stop == m.stop_flag);
    CHECK(t.xld == (m.x_row_stride == 0 ? m.I0 * m.I1 : m.x_row_stride));
  }
  CHECK(lds == want_lds);
  CHECK(lds == (int64_t)table[M - 1].a.g.words * 4);  // the envelope's edge is the largest
  CHECK(lds <= RES_LDS_BYTES && !resident_geom(nmax + 1, 8, 12, 4, 6, nullptr));  // one more row would not fit

  // a failing member: its code, its index, and the table left as it was
  struct Bad {
    int at, code;
    void (*spoil)(tr_resident_member&);
  };
  const Bad bads[] = {
      {3, TR_E_ARG, [](tr_resident_member& m) { m.n_iters = 65; }},
      {0, TR_E_ARG, [](tr_resident_member& m) { m.n_iters = -1; }},
      {5, TR_E_ARG, [](tr_resident_member& m) { m.params = nullptr; }},
      {6, TR_E_ARG, [](tr_resident_member& m) { m.stop_flag = nullptr; }},
      {1, TR_E_ARG, [](tr_resident_member& m) { m.amsgrad = 1; }},  // (member 1 has no max_exp_avg_sq)
      {2, TR_E_ARG, [](tr_resident_member& m) { m.n_rows = 0; }},
      {4, TR_E_ARG, [](tr_resident_member& m) { m.step = 0; }},
      {4, TR_E_ARG, [](tr_resident_member& m) { m.lr[1] = -1.0; }},
      {7, TR_E_UNSUPPORTED, [](tr_resident_member& m) { m.n_rows += 1; }},  // one row past the envelope
      {2, TR_E_UNSUPPORTED, [](tr_resident_member& m) { m.rank = 17; }},
  };
  std::vector<unsigned char> before((size_t)M * sizeof(ResMember));
  std::memcpy(before.data(), table, before.size());
  for (const Bad& b : bads) {
    std::vector<tr_resident_member> v = ms;
    b.spoil(v[b.at]);
    CHECK(build_resident_table(v.data(), M, table, &lds, &n_active, &bad, &why, &memo) == b.code);
    CHECK(bad == b.at && why != nullptr && why[0] != '\0');
    CHECK(std::memcmp(before.data(), table, before.size()) == 0);
  }
  std::free(table);
  if (g_failed) return 1;
  std::puts("resident many ok");
  return 0;
}
