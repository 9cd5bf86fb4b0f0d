// tr_np_sum.h — np.sum(np.abs(np.diff(h))) in numpy's summation order, for the plateau test of the
// fit loops (k_converge, k_converge_tail: tr_update.hip; the resident fit: tr_mnl_resident.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tr {

// sum_{j<n} |h[j+1] - h[j]| in the order of numpy's DOUBLE_pairwise_sum (PW_BLOCKSIZE 128, 8
// accumulators), iterative over the recursion tree (left-first), n <= NP_BUFSIZE.
static __device__ double np_pairwise_block_absdiff(const double* h, int64_t n) {
  double total = 0.0;
  // explicit stack of (start, len, depth-combine) — emulate recursion with partial sums
  struct Frame { int64_t s, n; int state; double left; };
  Frame st[48];
  int sp = 0;
  st[sp++] = {0, n, 0, 0.0};
  double ret = 0.0;
  while (sp > 0) {
    Frame& fr = st[sp - 1];
    if (fr.n <= 128 && fr.state == 0) {
      const int64_t s = fr.s, m = fr.n;
      double res;
      if (m < 8) {
        res = -0.0;
        for (int64_t i = 0; i < m; ++i) res += fabs(h[s + i + 1] - h[s + i]);
      } else {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = fabs(h[s + j + 1] - h[s + j]);
        int64_t i = 8;
        for (; i < m - (m % 8); i += 8)
          for (int j = 0; j < 8; ++j) r[j] += fabs(h[s + i + j + 1] - h[s + i + j]);
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < m; ++i) res += fabs(h[s + i + 1] - h[s + i]);
      }
      ret = res;
      --sp;
      continue;
    }
    int64_t n2 = fr.n / 2;
    n2 -= n2 % 8;
    if (fr.state == 0) {
      fr.state = 1;
      st[sp++] = {fr.s, n2, 0, 0.0};
    } else if (fr.state == 1) {
      fr.left = ret;
      fr.state = 2;
      const int64_t s = fr.s + n2, m = fr.n - n2;
      st[sp++] = {s, m, 0, 0.0};
    } else {
      ret = fr.left + ret;
      --sp;
    }
  }
  total = ret;
  return total;
}
constexpr int64_t NP_BUFSIZE = 8192;  // numpy's ufunc buffer, in elements (np.getbufsize() default)

// np.sum(np.abs(np.diff(h[0 : n + 1]))) as numpy adds it up: the reduction takes its operand in
// chunks of NP_BUFSIZE elements, sums each chunk pairwise and adds the chunk sums to the running
// result one after another (up to 8192 terms: one pairwise sum).
static __device__ double np_pairwise_sum_absdiff(const double* h, int64_t n) {
  double total = -0.0;  // the identity numpy's add reduction starts from
  for (int64_t c = 0; c < n; c += NP_BUFSIZE)
    total += np_pairwise_block_absdiff(h + c, n - c < NP_BUFSIZE ? n - c : NP_BUFSIZE);
  return total;
}

}  // namespace tr
