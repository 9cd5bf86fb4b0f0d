// Stand-alone check of the scoring sweep's host side (tensor_regression_amd/csrc/tr_mnl_score_table.h),
// built with -fsanitize=address,undefined by tests/test_score_many_host.py.  Every image is laid into
// a heap block of exactly words * 4 bytes and both ends of every piece are written; member tables are
// built into heap blocks of exactly n * sizeof(ScoreMember); every workgroup of every table is mapped
// back to its (member, row block) and the rows it would touch are marked in a heap block of exactly
// n_rows bytes, so an overrun is an ASan report.  Exit status 0 and "score many ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "adam_rows_check.h"  // with check.h
#include "tr_mnl_resident_table.h"
#include "tr_mnl_score_table.h"

namespace {

struct Shape {
  int64_t N, I0, I1;
  int C, R;
};

// never dereferenced by the host code: distinct non-NULL addresses inside static blocks
float g_f[16];
int64_t g_y[2];
int32_t g_cnt[1];
double g_d[4];

tr_score_member member(const Shape& s, int j) {
  tr_score_member m;
  std::memset(&m, 0, sizeof(m));
  m.X = g_f;
  m.target = g_y;
  m.params = g_f + 1;
  m.weights = g_f + 2;
  m.class_weights = (j % 2) ? g_f + 3 : nullptr;
  m.prob = (j % 3 == 0) ? g_f + 4 : nullptr;
  m.pred = (j % 3 == 1) ? g_y + 1 : nullptr;
  m.counts = g_cnt;
  m.loss = g_d;
  m.loss_parts = g_d + 2;
  m.n_rows = s.N;
  m.x_row_stride = (j % 2) ? s.I0 * s.I1 + 3 : 0;
  m.I0 = s.I0;
  m.I1 = s.I1;
  m.n_classes = s.C;
  m.rank = s.R;
  m.nonneg[0] = j & 1;
  m.nonneg[1] = (j >> 1) & 1;
  m.nonneg[2] = (j >> 2) & 1;
  m.softplus_beta = 50.f;
  m.softplus_threshold = 1.f;
  return m;
}

void check_image(const tr::ScoreGeom& g) {
  const int64_t PC = (int64_t)g.P * g.C;
  const struct {
    int at;
    int64_t n;
  } piece[] = {{g.oRed, 4 * (tr::SCORE_T / 64)}, {g.oCnt, (int64_t)g.C * g.C}, {g.oW, g.R}, {g.oPhi, g.np}, {g.oB, PC}};
  CHECK((int64_t)g.words * 4 <= tr::SCORE_LDS_BYTES);
  CHECK(g.P == g.I0 * g.I1 && g.np == (g.I0 + g.I1 + g.C) * g.R && g.off1 == g.I0 * g.R &&
        g.off2 == (g.I0 + g.I1) * g.R);
  CHECK(g.oRed % 2 == 0);  // fp64 partials
  float* lds = static_cast<float*>(std::malloc((size_t)g.words * 4));  // exactly the launch's dynamic LDS
  CHECK(lds != nullptr);
  if (lds == nullptr) return;
  int64_t end = 0;
  for (const auto& p : piece) {
    CHECK(p.at >= end && p.at % 4 == 0);  // in order, nothing overlapping, 16-byte aligned
    CHECK(p.at + p.n <= g.words);
    if (p.n > 0 && p.at + p.n <= g.words) {
      lds[p.at] = 1.f;
      lds[p.at + p.n - 1] = 2.f;
    }
    end = p.at + p.n;
  }
  // the kernel's largest indices: B[c][p] at c * P + p, phi of the last parameter
  CHECK((int64_t)(g.C - 1) * g.P + (g.P - 1) == PC - 1 && g.off2 + g.C * g.R == g.np);
  std::free(lds);
}

// Walks every workgroup of a built table as the kernel does and marks the rows it takes.
void check_blocks(const std::vector<tr_score_member>& ms, const tr::ScoreMember* table, int64_t total_blocks) {
  const int M = (int)ms.size();
  std::vector<unsigned char*> seen;
  for (int j = 0; j < M; ++j) seen.push_back(static_cast<unsigned char*>(std::calloc((size_t)ms[j].n_rows, 1)));
  int64_t first = 0;
  for (int j = 0; j < M; ++j) {
    CHECK(table[j].first_block == first && table[j].n_blocks == (ms[j].n_rows + tr::SCORE_ROWS - 1) / tr::SCORE_ROWS);
    CHECK(table[j].n_blocks >= 1);
    first += table[j].n_blocks;
  }
  CHECK(first == total_blocks);
  for (int64_t b = 0; b < total_blocks; ++b) {
    const int j = tr::score_member_of_block(table, M, (int)total_blocks, (int)b);
    CHECK(j >= 0 && j < M);
    if (j < 0 || j >= M) continue;
    const tr::ScoreMember& t = table[j];
    CHECK(t.first_block <= b && b < t.first_block + t.n_blocks);
    const int64_t row0 = (b - t.first_block) * tr::SCORE_ROWS;
    const int64_t nrows = t.n_rows - row0 < tr::SCORE_ROWS ? t.n_rows - row0 : tr::SCORE_ROWS;
    CHECK(nrows >= 1 && nrows <= tr::SCORE_ROWS);
    for (int64_t i = 0; i < nrows; ++i) seen[j][row0 + i] += 1;  // (past n_rows: an ASan report)
  }
  for (int j = 0; j < M; ++j) {
    bool once = true;
    for (int64_t n = 0; n < ms[j].n_rows; ++n) once = once && seen[j][n] == 1;
    CHECK(once);  // every row by exactly one workgroup
    std::free(seen[j]);
  }
}

int build(const std::vector<tr_score_member>& ms, tr::ScoreMember* table, int64_t* lds, int64_t* blocks, int* bad,
          const char** why) {
  int any_counts = 0, any_loss = 0;
  return tr::build_score_table(ms.data(), (int)ms.size(), table, lds, blocks, &any_counts, &any_loss, bad, why);
}

}  // namespace

int main() {
  using namespace tr;
  check_adam_rows();  // (this route writes no Adam rows; the resident header it includes for the envelope does)
  CHECK(SCORE_ROWS == TR_SCORE_ROW_BLOCK && SCORE_ROWS % (SCORE_T / 64) == 0);

  // ---- the envelope: a superset of the resident fit's, at every rank and class count ----
  int inside_both = 0, largest_pc = 0;
  for (int64_t I0 : {1, 2, 3, 8, 33, 64, 128, 257, 1024})
    for (int64_t I1 : {1, 2, 5, 12, 40, 64, 100, 513})
      for (int C : {1, 2, 4, 15, 16})
        for (int R : {1, 6, 16}) {
          const bool res = resident_geom(1, I0, I1, C, R, nullptr);
          ScoreGeom g;
          const bool sc = score_geom(I0, I1, C, R, &g);
          CHECK(!res || sc);
          if (sc) check_image(g);
          if (res) {
            ++inside_both;
            if ((int)(I0 * I1 * C) > largest_pc) largest_pc = (int)(I0 * I1 * C);
          }
        }
  CHECK(inside_both > 100 && largest_pc > 1024);
  // the resident route's largest P * C for C = R = 16, found by bisection on I1, and one past it
  {
    int64_t lo = 1, hi = 65536;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) / 2;
      if (resident_geom(1, 1, mid, 16, 16, nullptr))
        lo = mid;
      else
        hi = mid - 1;
    }
    CHECK(score_geom(1, lo, 16, 16, nullptr) && score_geom(1, lo + 1, 16, 16, nullptr));
  }
  CHECK(!score_geom(8, 12, 17, 6, nullptr) && !score_geom(8, 12, 4, 17, nullptr) && !score_geom(8, 12, 0, 6, nullptr));
  CHECK(!score_geom(0, 12, 4, 6, nullptr) && !score_geom(8, 12, 4, 0, nullptr));
  CHECK(!score_geom(1024, 1024, 4, 6, nullptr) && !score_geom(65537, 1, 1, 1, nullptr));
  {  // the edge of the image: the largest I1 for (I0 = 2, C = 16, R = 1) fits exactly, one more does not
    int64_t lo = 1, hi = 65536;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) / 2;
      if (score_geom(2, mid, 16, 1, nullptr))
        lo = mid;
      else
        hi = mid - 1;
    }
    ScoreGeom g;
    CHECK(score_geom(2, lo, 16, 1, &g) && !score_geom(2, lo + 1, 16, 1, nullptr));
    CHECK((int64_t)g.words * 4 <= SCORE_LDS_BYTES && (int64_t)(g.words + 36) * 4 > SCORE_LDS_BYTES);
    check_image(g);
  }

  // ---- member tables and the prefix table of row blocks ----
  const int64_t B = SCORE_ROWS;
  const std::vector<Shape> shapes = {{1, 1, 1, 2, 1},      {B - 1, 3, 5, 3, 2},  {B, 2, 5, 2, 3},     {B + 1, 8, 12, 4, 6},
                                     {3 * B + 1, 4, 4, 16, 16}, {7, 3, 3, 3, 16},     {227, 8, 12, 4, 6},  {5 * B + 17, 33, 8, 4, 2}};
  for (int M = 1; M <= (int)shapes.size(); ++M) {  // every prefix: the last member's last block is partial for most M
    std::vector<tr_score_member> ms;
    for (int j = 0; j < M; ++j) ms.push_back(member(shapes[j], j));
    ScoreMember* table = static_cast<ScoreMember*>(std::malloc((size_t)M * sizeof(ScoreMember)));
    CHECK(table != nullptr);
    if (table == nullptr) return 1;
    int64_t lds = 0, blocks = 0;
    int bad = 0;
    const char* why = nullptr;
    CHECK(build(ms, table, &lds, &blocks, &bad, &why) == 0 && bad == -1);
    int64_t want_lds = 0;
    for (int j = 0; j < M; ++j) {
      const tr_score_member& m = ms[j];
      const ScoreMember& t = table[j];
      ScoreGeom g;
      CHECK(score_geom(m.I0, m.I1, m.n_classes, m.rank, &g));
      CHECK(std::memcmp(&g, &t.g, sizeof(g)) == 0);
      if ((int64_t)g.words * 4 > want_lds) want_lds = (int64_t)g.words * 4;
      CHECK(t.X == m.X && t.target == m.target && t.params == m.params && t.w == m.weights && t.cw == m.class_weights &&
            t.prob == m.prob && t.pred == m.pred && t.counts == m.counts && t.loss == m.loss &&
            t.loss_parts == m.loss_parts);
      CHECK(t.n_rows == m.n_rows && t.xld == (m.x_row_stride == 0 ? m.I0 * m.I1 : m.x_row_stride));
      CHECK(t.beta == 50.f && t.thr == 1.f);
      for (int f = 0; f < 3; ++f) CHECK(t.nonneg[f] == m.nonneg[f]);
    }
    CHECK(lds == want_lds && lds <= SCORE_LDS_BYTES);
    check_blocks(ms, table, blocks);
    std::free(table);
  }
  {  // equal members (the interpolated first guess is exact) and 300 of them
    std::vector<tr_score_member> ms;
    for (int j = 0; j < 300; ++j) ms.push_back(member({2 * B + 5, 2, 3, 2, 1}, j));
    ScoreMember* table = static_cast<ScoreMember*>(std::malloc(ms.size() * sizeof(ScoreMember)));
    CHECK(table != nullptr);
    if (table == nullptr) return 1;
    int64_t lds = 0, blocks = 0;
    int bad = 0;
    const char* why = nullptr;
    CHECK(build(ms, table, &lds, &blocks, &bad, &why) == 0 && blocks == 900);
    check_blocks(ms, table, blocks);
    std::free(table);
  }

  // ---- a failing member: its code, its index, and the table left as it was ----
  {
    const int M = (int)shapes.size();
    std::vector<tr_score_member> ms;
    for (int j = 0; j < M; ++j) ms.push_back(member(shapes[j], j));
    ScoreMember* table = static_cast<ScoreMember*>(std::malloc((size_t)M * sizeof(ScoreMember)));
    CHECK(table != nullptr);
    if (table == nullptr) return 1;
    int64_t lds = 0, blocks = 0;
    int bad = 0;
    const char* why = nullptr;
    CHECK(build(ms, table, &lds, &blocks, &bad, &why) == 0);
    struct Bad {
      int at, code;
      void (*spoil)(tr_score_member&);
    };
    const Bad bads[] = {
        {3, TR_E_ARG, [](tr_score_member& m) { m.X = nullptr; }},
        {0, TR_E_ARG, [](tr_score_member& m) { m.params = nullptr; }},
        {5, TR_E_ARG, [](tr_score_member& m) { m.weights = nullptr; }},
        {2, TR_E_ARG, [](tr_score_member& m) { m.n_rows = 0; }},
        {6, TR_E_ARG, [](tr_score_member& m) { m.x_row_stride = -1; }},
        {1, TR_E_ARG, [](tr_score_member& m) { m.target = nullptr; m.loss = nullptr; }},    // counts without target
        {4, TR_E_ARG, [](tr_score_member& m) { m.target = nullptr; m.counts = nullptr; }},  // loss without target
        {7, TR_E_ARG, [](tr_score_member& m) { m.loss_parts = nullptr; }},
        {7, TR_E_UNSUPPORTED, [](tr_score_member& m) { m.n_classes = 17; }},
        {2, TR_E_UNSUPPORTED, [](tr_score_member& m) { m.rank = 17; }},
        {0, TR_E_UNSUPPORTED, [](tr_score_member& m) { m.I0 = 1024; m.I1 = 1024; }},
    };
    std::vector<unsigned char> before((size_t)M * sizeof(ScoreMember));
    std::memcpy(before.data(), table, before.size());
    for (const Bad& b : bads) {
      std::vector<tr_score_member> v = ms;
      b.spoil(v[b.at]);
      CHECK(build(v, table, &lds, &blocks, &bad, &why) == b.code);
      CHECK(bad == b.at && why != nullptr && why[0] != '\0');
      CHECK(std::memcmp(before.data(), table, before.size()) == 0);
    }
    // prob, pred, counts and loss are each optional; without target only prob and pred remain
    std::vector<tr_score_member> v = ms;
    v[1].target = nullptr;
    v[1].counts = nullptr;
    v[1].loss = nullptr;
    v[1].loss_parts = nullptr;
    CHECK(build(v, table, &lds, &blocks, &bad, &why) == 0);
    // more row blocks than a grid holds
    v = ms;
    v[0].n_rows = SCORE_MAX_BLOCKS * SCORE_ROWS;  // exactly the grid's limit: the next member is one too many
    CHECK(build(v, table, &lds, &blocks, &bad, &why) == TR_E_UNSUPPORTED && bad == 1);
    CHECK(SCORE_MAX_BLOCKS * SCORE_T <= 0xFFFFFFFFll && (SCORE_MAX_BLOCKS + 1) * SCORE_T > 0xFFFFFFFFll);
    v.resize(1);
    CHECK(build(v, table, &lds, &blocks, &bad, &why) == 0 && blocks == SCORE_MAX_BLOCKS);
    std::free(table);
  }
  if (g_failed) return 1;
  std::puts("score many ok");
  return 0;
}
