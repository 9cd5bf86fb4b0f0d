// Stand-alone check of the linear score's host side (tensor_regression_amd/csrc/tr_linear_many.h), built with
// -fsanitize=address,undefined by tests/test_linear_score_host.py: the forward split against
// linear_many_geom's over a sweep of (N, P), every carve piece disjoint, 256-aligned and inside the
// carver's byte count, and the table builder, which leaves the table unwritten when a member is bad.
// Tables are built into heap blocks of exactly linear_score_table_bytes(n).  Exit status 0 and
// "linear score ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "check.h"
#include "tr_linear_many.h"

namespace {

using namespace tr;

// never dereferenced by the host code: distinct non-NULL addresses inside static blocks
float g_f[16];
double g_s[16 * LS_SUMS];

tr_linear_score_member member(int j) {
  tr_linear_score_member m;
  std::memset(&m, 0, sizeof(m));
  m.params = g_f;
  m.weights = g_f + 1;
  m.y = (j % 3 == 1) ? nullptr : g_f + 2;
  m.yhat = (j % 3 == 0) ? nullptr : g_f + 3;
  m.sums = m.y != nullptr ? g_s + LS_SUMS * j : nullptr;
  static const int ranks[4] = {1, 3, 8, 32};
  m.rank = ranks[j % 4];
  m.nonneg[0] = j & 1;
  m.nonneg[1] = (j >> 1) & 1;
  m.nonneg[2] = (j >> 2) & 1;
  m.softplus_beta = 50.f;
  m.softplus_threshold = 1.f;
  return m;
}

void check_split(int64_t N, int64_t I0, int64_t I1) {
  LmGeom f;
  LsGeom s;
  const int64_t d2[2] = {I0, I1};
  CHECK(linear_many_geom(N, I0, I1, &f));
  CHECK(linear_score_geom(N, 2, d2, &s));
  CHECK(s.P == f.P && s.nrw == f.nrw && s.slice == f.slice && s.ns == f.ns && s.nepi == f.nepi);
  CHECK(s.npmax == f.npmax && s.isum == I0 + I1);
  // the same (N, P) spelled with three modes splits alike
  if (I1 % 2 == 0) {
    const int64_t d3[3] = {I0, I1 / 2, 2};
    LsGeom t;
    CHECK(linear_score_geom(N, 3, d3, &t));
    CHECK(t.P == f.P && t.nrw == f.nrw && t.slice == f.slice && t.ns == f.ns && t.nepi == f.nepi);
    CHECK(t.isum == I0 + I1 / 2 + 2 && t.npmax == t.isum * LM_MAX_R);
  }
  CHECK(s.slice % LM_FOLD == 0 && s.ns * s.slice >= s.P && (s.ns - 1) * s.slice < s.P);
}

void check_carve(int64_t N, int n_modes, const int64_t* dims) {
  LsGeom g;
  CHECK(linear_score_geom(N, n_modes, dims, &g));
  LsWork w;
  std::memset(&w, 0, sizeof(w));
  Carver c;
  linear_score_carve(g, &w, &c);
  const size_t bytes = c.bytes();
  CHECK(bytes % 256 == 0 && bytes > 0);
  // a small carve is bound to a real block and every piece written end to end (ASan watches the edges)
  const bool real = bytes <= (size_t(1) << 24);
  char* base = real ? static_cast<char*>(std::aligned_alloc(256, bytes)) : reinterpret_cast<char*>(uintptr_t(1) << 40);
  c.bind(base);
  const size_t npad = (size_t)(g.nepi * LM_EPI_ROWS);
  std::vector<std::pair<size_t, size_t>> pieces;  // (offset, bytes)
  auto piece = [&](const void* p, size_t n) {
    const size_t off = (size_t)(static_cast<const char*>(p) - base);
    CHECK(off % 256 == 0 && off + n <= bytes);
    pieces.push_back({off, n});
    if (real) std::memset(base + off, 0x5a, n);
  };
  piece(w.Bt, (size_t)LM_MAX_M * g.P * 4);
  piece(w.phi, (size_t)LM_MAX_M * g.npmax * 4);
  if (n_modes == 2) {
    CHECK(w.dphi != nullptr);
    piece(w.dphi, (size_t)LM_MAX_M * g.npmax * 4);
  } else {
    CHECK(w.dphi == nullptr);
  }
  piece(w.Z, (size_t)g.ns * npad * LM_MAX_M * 4);
  piece(w.D, (size_t)g.nepi * LM_MAX_M * LS_SUMS * 8);
  std::sort(pieces.begin(), pieces.end());
  for (size_t k = 1; k < pieces.size(); ++k) CHECK(pieces[k - 1].first + pieces[k - 1].second <= pieces[k].first);
  if (real) std::free(base);
}

int build(const std::vector<tr_linear_score_member>& v, int n, std::vector<char>* blk, int* bad, const char** why) {
  blk->assign((size_t)linear_score_table_bytes(n > 0 && n <= LM_MAX_M ? n : 0) + 1, (char)0x77);
  LmMember* table = reinterpret_cast<LmMember*>(blk->data());
  LsMember* ext = reinterpret_cast<LsMember*>(table + (n > 0 && n <= LM_MAX_M ? n : 0));
  return build_linear_score_table(v.data(), n, table, ext, bad, why);
}

void check_tables() {
  std::vector<tr_linear_score_member> ms;
  for (int j = 0; j < LM_MAX_M; ++j) ms.push_back(member(j));
  std::vector<char> blk;
  int bad = 0;
  const char* why = nullptr;
  for (int n : {1, 5, 16}) {
    CHECK(build(ms, n, &blk, &bad, &why) == 0 && bad == -1);
    CHECK(blk.back() == (char)0x77);  // nothing past the table's bytes
    const LmMember* table = reinterpret_cast<const LmMember*>(blk.data());
    const LsMember* ext = reinterpret_cast<const LsMember*>(table + n);
    for (int j = 0; j < n; ++j) {
      const tr_linear_score_member& m = ms[j];
      CHECK(table[j].params == m.params && table[j].w == m.weights && table[j].y == m.y);
      CHECK(table[j].rank == m.rank && table[j].nonneg[0] == m.nonneg[0] && table[j].nonneg[1] == m.nonneg[1]);
      CHECK(table[j].beta == 50.f && table[j].thr == 1.f && table[j].grad == nullptr && table[j].n_iters == 0);
      CHECK(ext[j].yhat == m.yhat && ext[j].sums == m.sums && ext[j].nonneg2 == m.nonneg[2]);
    }
  }
  CHECK(sizeof(LsMember) % 8 == 0 && sizeof(LmMember) % 8 == 0);
  CHECK(linear_score_table_bytes(3) == 3 * (int64_t)(sizeof(LmMember) + sizeof(LsMember)));
  CHECK(linear_score_table_bytes(0) == 0 && linear_score_table_bytes(-1) == 0);
  struct Case {
    int at, rc;
    void (*spoil)(tr_linear_score_member&);
  };
  const Case cases[] = {
      {2, TR_E_ARG, [](tr_linear_score_member& m) { m.params = nullptr; }},
      {0, TR_E_ARG, [](tr_linear_score_member& m) { m.weights = nullptr; }},
      {3, TR_E_ARG, [](tr_linear_score_member& m) { m.y = g_f + 2; m.sums = nullptr; }},
      {4, TR_E_ARG, [](tr_linear_score_member& m) { m.y = nullptr; m.yhat = nullptr; }},
      {1, TR_E_UNSUPPORTED, [](tr_linear_score_member& m) { m.rank = 33; }},
      {4, TR_E_UNSUPPORTED, [](tr_linear_score_member& m) { m.rank = 0; }},
  };
  for (const Case& cs : cases) {
    std::vector<tr_linear_score_member> v(ms.begin(), ms.begin() + 5);
    cs.spoil(v[cs.at]);
    CHECK(build(v, 5, &blk, &bad, &why) == cs.rc && bad == cs.at && why[0] != '\0');
    CHECK(std::all_of(blk.begin(), blk.end(), [](char ch) { return ch == (char)0x77; }));  // unwritten
  }
  {  // the first bad member is the one named
    std::vector<tr_linear_score_member> v(ms.begin(), ms.begin() + 5);
    v[3].rank = 40;
    v[1].params = nullptr;
    CHECK(build(v, 5, &blk, &bad, &why) == TR_E_ARG && bad == 1);
  }
  std::vector<tr_linear_score_member> big(17, member(0));
  CHECK(build(big, 17, &blk, &bad, &why) == TR_E_ARG && bad == -1);
  CHECK(build(ms, -1, &blk, &bad, &why) == TR_E_ARG);
  CHECK(build(ms, 0, &blk, &bad, &why) == 0);
}

}  // namespace

int main() {
  const int64_t ns[] = {1, 3, 37, 128, 129, 257, 2000, 4097, 70000, 1 << 20};
  const int64_t shapes[][2] = {{8, 4}, {8, 12}, {16, 16}, {24, 20}, {33, 36}, {256, 128}, {500, 500}, {9, 12}, {1, 4},
                               {1000, 1000}};
  for (int64_t N : ns)
    for (const auto& s : shapes) check_split(N, s[0], s[1]);
  for (int64_t N : ns) {
    for (const auto& s : shapes) check_carve(N, 2, s);
    const int64_t d3[][3] = {{4, 3, 8}, {8, 4, 8}, {20, 25, 36}, {1, 1, 4}};
    for (const auto& d : d3) check_carve(N, 3, d);
  }
  {  // the score's carve holds no gradient slabs: far below the fit's workspace at the notebook's shape
    LmGeom f;
    LsGeom g;
    const int64_t d[2] = {500, 500};
    CHECK(linear_many_geom(2000, 500, 500, &f) && linear_score_geom(2000, 2, d, &g));
    LsWork w;
    Carver c;
    linear_score_carve(g, &w, &c);
    CHECK((int64_t)c.bytes() * 4 < f.bytes);
  }
  // the envelope
  const int64_t a[2] = {8, 12}, b[2] = {3, 3}, z[2] = {0, 12}, h[2] = {LM_MAX_DIM, LM_MAX_DIM};
  const int64_t t[3] = {4, 3, 8}, u[3] = {3, 3, 3}, huge[3] = {LM_MAX_DIM, LM_MAX_DIM, 4};
  CHECK(linear_score_envelope(2, a, 0, 32) && !linear_score_envelope(2, a, 0, 33) && !linear_score_envelope(2, a, 0, 0));
  CHECK(!linear_score_envelope(2, b, 0, 2) && !linear_score_envelope(2, z, 0, 2) && !linear_score_envelope(2, h, 0, 2));
  CHECK(!linear_score_envelope(2, a, 98, 2) && linear_score_envelope(2, a, 100, 2) && linear_score_envelope(2, a, 12, 2));
  CHECK(!linear_score_envelope(2, a, -4, 2));
  CHECK(linear_score_envelope(3, t, 0, 8) && !linear_score_envelope(3, u, 0, 8) && !linear_score_envelope(3, huge, 0, 8));
  CHECK(!linear_score_envelope(1, a, 0, 2) && !linear_score_envelope(4, a, 0, 2) && !linear_score_envelope(2, nullptr, 0, 2));
  CHECK(!linear_score_geom(0, 2, a, nullptr) && !linear_score_geom(5, 2, b, nullptr));
  for (int64_t I0 : {1, 3, 8, 500})
    for (int64_t I1 : {4, 12, 500})
      for (int64_t xld : {0, 4, 98, 100})
        for (int r : {0, 1, 32, 33}) {
          const int64_t d[2] = {I0, I1};
          CHECK(linear_score_envelope(2, d, xld, r) == linear_many_envelope(I0, I1, xld, r));
        }
  check_tables();
  if (g_failed != 0) return 1;
  std::puts("linear score ok");
  return 0;
}
