// Stand-alone check of tr::Carver (tensor_regression_amd/csrc/tr_workspace.h), built with
// -fsanitize=address,undefined by tests/test_workspace_carver.py: every layout is bound into a heap block
// of exactly bytes() and the first and last byte of every non-empty piece is written, so an overrun
// of the block is an ASan report.  Exit status 0 and "carver ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "check.h"
#include "tr_workspace.h"

namespace {

size_t al(size_t b) { return (b + 255) / 256 * 256; }

// Declares pieces of the given sizes (optional[i]: declared with add_optional), binds them into a block
// of exactly bytes() and checks alignment, order, disjointness and the total.
void check_layout(const std::vector<size_t>& sizes, const std::vector<bool>& optional) {
  const size_t n = sizes.size();
  std::vector<char*> slot(n, reinterpret_cast<char*>(0x1));  // bind must overwrite every slot
  tr::Carver c;
  size_t want = 0;
  for (size_t i = 0; i < n; ++i) {
    if (optional[i])
      c.add_optional(&slot[i], sizes[i]);
    else
      c.add(&slot[i], sizes[i]);
    want += al(sizes[i]);
  }
  CHECK(c.bytes() == want);
  char* base = static_cast<char*>(std::malloc(c.bytes() > 0 ? c.bytes() : 1));
  CHECK(base != nullptr);
  if (base == nullptr) return;
  c.bind(base);
  size_t at = 0;  // where the next piece must start: declaration order, nothing between the pieces
  for (size_t i = 0; i < n; ++i) {
    if (optional[i] && sizes[i] == 0) {
      CHECK(slot[i] == nullptr);
      continue;
    }
    CHECK(slot[i] == base + at);
    CHECK((size_t)(slot[i] - base) % 256 == 0);
    if (sizes[i] > 0) {
      CHECK(at + sizes[i] <= c.bytes());
      slot[i][0] = (char)i;
      slot[i][sizes[i] - 1] = (char)i;
    }
    at += al(sizes[i]);  // the next piece starts at or after this one's end: no overlap
  }
  CHECK(at == c.bytes());
  for (size_t i = 0; i < n; ++i)  // no later piece's write landed in an earlier piece
    if (sizes[i] > 0) CHECK(slot[i][0] == (char)i && slot[i][sizes[i] - 1] == (char)i);
  std::free(base);
}

// Typed slots as a plan declares them: the pointer types differ, one piece is shared by two views.
void check_typed() {
  float* phi = nullptr;
  double* dpart = nullptr;
  int32_t* map = nullptr;
  unsigned long long* gran = nullptr;
  float* absent = reinterpret_cast<float*>(0x1);
  tr::Carver c;
  c.add(&phi, 10 * sizeof(float));
  c.add(&dpart, 33 * sizeof(double));
  c.add(&map, 7 * sizeof(int32_t));
  c.add(&gran, 4 * 8 + 16);
  c.add_optional(&absent, 0);
  CHECK(c.bytes() == 256 + 512 + 256 + 256);
  char* base = static_cast<char*>(std::malloc(c.bytes()));
  CHECK(base != nullptr);
  if (base == nullptr) return;
  c.bind(base);
  CHECK((char*)phi == base && (char*)dpart == base + 256 && (char*)map == base + 768 && (char*)gran == base + 1024);
  CHECK(absent == nullptr);
  phi[9] = 1.f;
  dpart[32] = 2.0;
  map[6] = 3;
  uint32_t* err_word = (uint32_t*)(gran + 4);  // a second view of the same piece
  gran[3] = 4;
  err_word[3] = 5;
  CHECK(phi[9] == 1.f && dpart[32] == 2.0 && map[6] == 3 && gran[3] == 4 && err_word[3] == 5);
  std::free(base);
}

}  // namespace

int main() {
  check_layout({0, 1, 255, 256, 257}, {false, false, false, false, false});
  check_layout({257, 0, 256, 1, 255, 0}, {false, false, false, false, false, false});
  check_layout({1024, 0, 100}, {false, true, false});   // an absent optional piece in the middle
  check_layout({1024, 100, 0}, {false, false, true});   // ... and as the last piece (specT, phaseH)
  check_layout({1024, 100, 40}, {false, false, true});  // a present optional piece
  check_layout({4, 8, 12, 300, 5000, 1, 256, 512, 513, 7, 64, 100000}, std::vector<bool>(12, false));  // a dozen
  check_layout({}, {});
  check_typed();
  if (g_failed) return 1;
  std::puts("carver ok");
  return 0;
}
