// The per-iteration rows that tr::fill_adam_rows (csrc/tr_member_table.h) writes for every fit member's
// table entry, against the formula itself: step_size[f][k] == (float)(lr[f] / bc1) and bc2_sqrt[k] ==
// (float)bc2_sqrt of adam_scalars(b1, b2, step + k), bit for bit, for k in 0..63, with three learning
// rates and with one, two beta pairs, with and without the memo.
#pragma once

#include <cstdint>

#include "check.h"
#include "tr_member_table.h"

inline void check_adam_rows() {
  using namespace tr;
  const double betas[2][2] = {{0.9, 0.999}, {0.8, 0.99}};
  const double lr[3] = {0.012, 0.02, 0.0};
  const int64_t step = 65;
  AdamMemo memo;
  for (int b = 0; b < 2; ++b)
    for (int pass = 0; pass < 3; ++pass) {  // no memo, a memo that computes, the same memo again
      float three[3][64], one[1][64], bc2_three[64], bc2_one[64];
      AdamMemo* mp = pass == 0 ? nullptr : &memo;
      fill_adam_rows(mp, betas[b][0], betas[b][1], step, 64, lr, 3, three, bc2_three);
      fill_adam_rows(mp, betas[b][0], betas[b][1], step, 64, lr, 1, one, bc2_one);
      for (int k = 0; k < 64; ++k) {
        const AdamScalars as = adam_scalars(betas[b][0], betas[b][1], step + k);
        for (int f = 0; f < 3; ++f) CHECK(three[f][k] == (float)(lr[f] / as.bc1));
        CHECK(one[0][k] == (float)(lr[0] / as.bc1));
        CHECK(bc2_three[k] == (float)as.bc2_sqrt && bc2_one[k] == (float)as.bc2_sqrt);
      }
      CHECK(memo.computed == (pass == 0 ? b : b + 1) * 64);  // one set per beta pair, however often it is read
    }
}
