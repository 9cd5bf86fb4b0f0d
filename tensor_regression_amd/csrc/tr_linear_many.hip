// tr_linear_many.hip — the shared-X linear sweep: up to 16 CP linear models (two feature modes) over
// one X.  With dense coefficient tensors B_m the 16 forward passes are one skinny GEMM Z = X . Bt^T
// and the 16 gradient passes another, G = R^T . X, both on v_mfma_f32_16x16x4_f32 (exact fp32
// products, a k-ordered fmaf chain per output), so an iteration reads X twice whatever M is.
//
//   k_lm_prep      phi = softplus?(A), dphi                          grid (elements, M)
//   k_lm_dense     Bt[m][p] = sum_r (phi0[i, r] w_r) phi1[j, r]      grid (P / 256, 16); rows >= M zero
//   k_lm_forward   Zpart[s][n][m] over feature slice s              grid (row blocks, slices)
//   k_lm_epilogue  z = sum_s Zpart (slice order); e = z + bias - y;  grid (row blocks of 256)
//                  R[n][m] = e 2/N; fp64 partials of sum e^2, sum r
//   k_lm_grad      slab[c][m][p] = sum_{n in chunk c} R[n, m] X[n, p] grid (feature blocks, chunks), last chunk first
//   k_lm_reduce    G[m][p] = sum_c slab[c][m][p] (chunk order)        grid (P / 1024, M)
//   k_lm_fold      two-factor MTTKRP + softplus chain into the member's grad arena; the data loss and
//                  the bias gradient from the fp64 partials          grid (I0 + I1 + 1, M)
//   k_lm_update    k_update<false>'s step (tr_adam.h) + k_converge's plateau test, a workgroup per member
//
// Eight launches per iteration for any M.  No floating-point atomics; every sum has one fixed order
// that depends on the shape alone (LmGeom), and a member's column of an MFMA tile is computed from its
// own operands only: its bits depend neither on the other members nor on its position.
//
// Scoring (tr_linear_many_score) runs the forward half alone, for two or three feature modes:
//   k_lm_prep | k_lm_prep3, k_lm_dense | k_lm_dense3, k_lm_forward, then
//   k_lm_score      yhat = sum_s Zpart + bias (the epilogue's expression), stored when wanted; fp64
//                   partials of the five shifted sums per (row block, column)   grid (row blocks of 256)
//   k_lm_score_sum  a member's partials in k_lm_fold's order into its 5 doubles  grid (M)
// Five launches for any M, X read once.
#include "tr_linear_many.h"

#include "tr_adam.h"
#include "tr_common.h"
#include "tr_np_sum.h"

namespace tr {

namespace {
constexpr int LM_UPD_T = 1024;
}

__global__ __launch_bounds__(256) void k_lm_prep(const LmMember* __restrict__ tab, int64_t I0, int64_t I1,
                                                 int64_t npmax, float* __restrict__ phi,
                                                 float* __restrict__ dphi) {
  const LmMember& tm = tab[blockIdx.y];
  const int R = tm.rank;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (I0 + I1) * R) return;
  const int f = e >= I0 * R ? 1 : 0;
  const float a = tm.params[e];
  const int64_t o = (int64_t)blockIdx.y * npmax + e;
  if (tm.nonneg[f]) {
    phi[o] = tr_softplus(a, tm.beta, tm.thr);
    dphi[o] = tr_softplus_grad(a, tm.beta, tm.thr);
  } else {
    phi[o] = a;
    dphi[o] = 1.0f;
  }
}

// cp_to_tensor in k_build_dense's association: (Phi_0 * w) @ Phi_1^T, one fmaf chain over the rank
__global__ __launch_bounds__(256) void k_lm_dense(const LmMember* __restrict__ tab, int M, int64_t I0, int64_t I1,
                                                  int64_t npmax, const float* __restrict__ phi,
                                                  float* __restrict__ Bt) {
  const int64_t P = I0 * I1;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int m = blockIdx.y;
  float s = 0.f;
  if (m < M) {
    const LmMember& tm = tab[m];
    const int R = tm.rank;
    const int64_t i = p / I1, j = p - i * I1;
    const float* __restrict__ F0 = phi + (int64_t)m * npmax + i * R;
    const float* __restrict__ F1 = phi + (int64_t)m * npmax + I0 * R + j * R;
    for (int r = 0; r < R; ++r) s = fmaf(F0[r] * tm.w[r], F1[r], s);
  }
  Bt[(int64_t)m * P + p] = s;
}

// Forward on the matrix cores, k_rows_mfma's scheme: lane (i, g) loads 8 consecutive features of row
// i and of Bt row i per 32-feature step; MFMA c of a step feeds accumulator chain c; the 8 chains are
// folded by a fixed tree every LM_FOLD features.  A workgroup's 4 waves take 4 x RT tiles of 16 rows
// over the same feature slice (Bt lines shared in L1 / L2).  The tail of the last slice (P a multiple
// of 4, not of 32) is zero-filled on both operands.
template <int RT>
__global__ __launch_bounds__(256) void k_lm_forward(const float* __restrict__ X, int64_t N, int64_t P, int64_t xld,
                                                    const float* __restrict__ Bt, int64_t slice,
                                                    float* __restrict__ Zpart, int64_t npad) {
  const int lane = threadIdx.x & (TR_WAVE - 1);
  const int wave = threadIdx.x / TR_WAVE;
  const int i = lane & 15, g = lane >> 4;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * RT);
  if (row0 >= N) return;
  const int64_t pb = (int64_t)blockIdx.y * slice;
  const int64_t pe = pb + slice < P ? pb + slice : P;
  const float* xr[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    int64_t r = row0 + rt * 16 + i;
    r = r < N ? r : N - 1;
    xr[rt] = X + r * xld + pb;
  }
  const float* br = Bt + (int64_t)i * P + pb;
  wv_f4 ac[RT][8], acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    acc[rt] = wv_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 8; ++c) ac[rt][c] = wv_f4{0.f, 0.f, 0.f, 0.f};
  }
  auto fold = [&]() {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      acc[rt] += ((ac[rt][0] + ac[rt][1]) + (ac[rt][2] + ac[rt][3])) + ((ac[rt][4] + ac[rt][5]) + (ac[rt][6] + ac[rt][7]));
#pragma unroll
      for (int c = 0; c < 8; ++c) ac[rt][c] = wv_f4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto step = [&](const float4(&xa)[RT], const float4(&xb)[RT], const float4 ba, const float4 bb) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      ac[rt][0] = wv_mfma_16x16x4(xa[rt].x, ba.x, ac[rt][0]);
      ac[rt][1] = wv_mfma_16x16x4(xa[rt].y, ba.y, ac[rt][1]);
      ac[rt][2] = wv_mfma_16x16x4(xa[rt].z, ba.z, ac[rt][2]);
      ac[rt][3] = wv_mfma_16x16x4(xa[rt].w, ba.w, ac[rt][3]);
      ac[rt][4] = wv_mfma_16x16x4(xb[rt].x, bb.x, ac[rt][4]);
      ac[rt][5] = wv_mfma_16x16x4(xb[rt].y, bb.y, ac[rt][5]);
      ac[rt][6] = wv_mfma_16x16x4(xb[rt].z, bb.z, ac[rt][6]);
      ac[rt][7] = wv_mfma_16x16x4(xb[rt].w, bb.w, ac[rt][7]);
    }
  };
  auto ld = [](const float* p) { return *reinterpret_cast<const float4*>(p); };
  const int64_t len = pe - pb;
  const int nfull = (int)(len / 32);
  const int o = 8 * g;  // this lane's features of a step: o .. o + 7
  int st = 0;
  for (; st + 1 < nfull; st += 2) {  // two steps of loads in flight before the MFMAs
    float4 xa0[RT], xb0[RT], xa1[RT], xb1[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      xa0[rt] = ld(xr[rt] + 32 * st + o);
      xb0[rt] = ld(xr[rt] + 32 * st + o + 4);
      xa1[rt] = ld(xr[rt] + 32 * st + 32 + o);
      xb1[rt] = ld(xr[rt] + 32 * st + 36 + o);
    }
    const float4 ba0 = ld(br + 32 * st + o), bb0 = ld(br + 32 * st + o + 4);
    const float4 ba1 = ld(br + 32 * st + 32 + o), bb1 = ld(br + 32 * st + 36 + o);
    __builtin_amdgcn_sched_barrier(0);
    step(xa0, xb0, ba0, bb0);
    step(xa1, xb1, ba1, bb1);
    if (((st + 2) & 15) == 0) fold();
  }
  if (st < nfull) {
    float4 xa0[RT], xb0[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      xa0[rt] = ld(xr[rt] + 32 * st + o);
      xb0[rt] = ld(xr[rt] + 32 * st + o + 4);
    }
    const float4 ba0 = ld(br + 32 * st + o), bb0 = ld(br + 32 * st + o + 4);
    step(xa0, xb0, ba0, bb0);
    ++st;
  }
  const int rem = (int)(len - 32 * (int64_t)nfull);  // 0, 4, .., 28 features past the last full step
  if (rem > 0) {
    const bool va = o < rem, vb = o + 4 < rem;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 xa0[RT], xb0[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      xa0[rt] = va ? ld(xr[rt] + 32 * st + o) : zero;
      xb0[rt] = vb ? ld(xr[rt] + 32 * st + o + 4) : zero;
    }
    const float4 ba0 = va ? ld(br + 32 * st + o) : zero;
    const float4 bb0 = vb ? ld(br + 32 * st + o + 4) : zero;
    step(xa0, xb0, ba0, bb0);
  }
  fold();
  // accumulator layout: column (member) = lane & 15, row = 4 * (lane >> 4) + reg
  float* __restrict__ zp = Zpart + (int64_t)blockIdx.y * npad * LM_MAX_M;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t row = row0 + rt * 16 + 4 * g + reg;
      if (row < N) zp[row * LM_MAX_M + i] = acc[rt][reg];
    }
}

// Thread (rl, col) walks rows rl, rl + 16, .. of the workgroup's 256; a column's fp64 partials are the
// 16 threads' sums added in rl order.
__global__ __launch_bounds__(256) void k_lm_epilogue(const LmMember* __restrict__ tab, int M, int64_t N,
                                                     int64_t I01, const float* __restrict__ Zpart, int64_t ns,
                                                     int64_t npad, float scale, float* __restrict__ Rr,
                                                     double* __restrict__ dpart) {
  __shared__ double se[16][16], sr[16][16];
  const int col = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const bool has = col < M;
  const float* __restrict__ y = has ? tab[col].y : nullptr;
  const float bias = has ? tab[col].params[I01 * tab[col].rank] : 0.f;
  double e2 = 0.0, rs = 0.0;
  for (int k = 0; k < LM_EPI_ROWS / 16; ++k) {
    const int64_t row = (int64_t)blockIdx.x * LM_EPI_ROWS + k * 16 + rl;
    if (row >= N) break;
    float z = 0.f;
    for (int64_t s = 0; s < ns; ++s) z += Zpart[(s * npad + row) * LM_MAX_M + col];
    float r = 0.f;
    if (has) {
      const float e = (z + bias) - y[row];
      r = e * scale;
      e2 += (double)e * (double)e;
      rs += (double)r;
    }
    Rr[row * LM_MAX_M + col] = r;
  }
  se[rl][col] = e2;
  sr[rl][col] = rs;
  __syncthreads();
  if (threadIdx.x < 16) {
    double a = 0.0, b = 0.0;
    for (int q = 0; q < 16; ++q) {
      a += se[q][col];
      b += sr[q][col];
    }
    dpart[((int64_t)blockIdx.x * LM_MAX_M + col) * 2] = a;
    dpart[((int64_t)blockIdx.x * LM_MAX_M + col) * 2 + 1] = b;
  }
}

// Gradient slabs on the matrix cores: D[m][p] += sum_k R[n0 + k][m] X[n0 + k][p], 4 rows per MFMA.
// Lane (i, g) supplies A = R[n0 + g][i] and loads the float4 X[n0 + g][p0 + 64 u + 4 i ..]; MFMA j of
// tile u takes component j, so the lane's four results of a member row are 4 consecutive features.
// A wave owns 256 features (4 tiles) and walks its chunk's rows 8 at a time: 8 X loads in flight.
__global__ __launch_bounds__(256) void k_lm_grad(const float* __restrict__ X, int64_t N, int64_t P, int64_t xld,
                                                 const float* __restrict__ Rr, int64_t rpc, int64_t nch,
                                                 float* __restrict__ gpart) {
  const int lane = threadIdx.x & (TR_WAVE - 1);
  const int wave = threadIdx.x / TR_WAVE;
  const int i = lane & 15, g = lane >> 4;
  const int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * LM_GRAD_FEATS;
  if (p0 >= P) return;
  const int64_t c = nch - 1 - (int64_t)blockIdx.y;  // the rows the forward read last come first
  const int64_t nb = c * rpc;
  const int64_t ne = nb + rpc < N ? nb + rpc : N;
  bool pv[4];
  int64_t po[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t p = p0 + 64 * u + 4 * i;
    pv[u] = p < P;
    po[u] = pv[u] ? p : p0;
  }
  wv_f4 acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[u][j] = wv_f4{0.f, 0.f, 0.f, 0.f};
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t n = nb; n < ne; n += 8) {
    const int64_t ra = n + g, rb = n + 4 + g;
    const bool oka = ra < ne, okb = rb < ne;
    const float* __restrict__ xa = X + (oka ? ra : nb) * xld;
    const float* __restrict__ xb = X + (okb ? rb : nb) * xld;
    float4 va[4], vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      va[u] = *reinterpret_cast<const float4*>(xa + po[u]);
      vb[u] = *reinterpret_cast<const float4*>(xb + po[u]);
    }
    const float wa = oka ? Rr[ra * LM_MAX_M + i] : 0.f;
    const float wb = okb ? Rr[rb * LM_MAX_M + i] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float4 a = oka && pv[u] ? va[u] : zero;
      acc[u][0] = wv_mfma_16x16x4(wa, a.x, acc[u][0]);
      acc[u][1] = wv_mfma_16x16x4(wa, a.y, acc[u][1]);
      acc[u][2] = wv_mfma_16x16x4(wa, a.z, acc[u][2]);
      acc[u][3] = wv_mfma_16x16x4(wa, a.w, acc[u][3]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float4 b = okb && pv[u] ? vb[u] : zero;
      acc[u][0] = wv_mfma_16x16x4(wb, b.x, acc[u][0]);
      acc[u][1] = wv_mfma_16x16x4(wb, b.y, acc[u][1]);
      acc[u][2] = wv_mfma_16x16x4(wb, b.z, acc[u][2]);
      acc[u][3] = wv_mfma_16x16x4(wb, b.w, acc[u][3]);
    }
  }
  // result layout: member = 4 * (lane >> 4) + reg, tile column = lane & 15
  float* __restrict__ slab = gpart + c * LM_MAX_M * P;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (pv[u])
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        *reinterpret_cast<float4*>(slab + (int64_t)(4 * g + reg) * P + po[u]) =
            make_float4(acc[u][0][reg], acc[u][1][reg], acc[u][2][reg], acc[u][3][reg]);
}

__global__ __launch_bounds__(256) void k_lm_reduce(const float* __restrict__ gpart, int64_t P, int64_t nch,
                                                   float* __restrict__ G) {
  const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p >= P) return;
  const int64_t m = blockIdx.y;
  float4 s = *reinterpret_cast<const float4*>(gpart + m * P + p);
  for (int64_t c = 1; c < nch; ++c) {
    const float4 v = *reinterpret_cast<const float4*>(gpart + (c * LM_MAX_M + m) * P + p);
    s.x += v.x;
    s.y += v.y;
    s.z += v.z;
    s.w += v.w;
  }
  *reinterpret_cast<float4*>(G + m * P + p) = s;
}

// One wave per (factor row, member), k_mttkrp2's arithmetic with the rank up to 32:
//   grad[A_f][i, r] = dphi * sum_j G[i_f = i, i_g = j] * (w_r * Phi_g[j, r])
// and one more wave per member for the data loss and the bias gradient.
__global__ __launch_bounds__(64) void k_lm_fold(const LmMember* __restrict__ tab, int64_t N, int64_t I0, int64_t I1,
                                                int64_t npmax, const float* __restrict__ phi,
                                                const float* __restrict__ dphi, const float* __restrict__ G,
                                                const double* __restrict__ dpart, int64_t nepi) {
  const int m = blockIdx.y;
  const LmMember& tm = tab[m];
  const int R = tm.rank;
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t nfe = (I0 + I1) * R;
  if (b == I0 + I1) {
    double a = 0.0, s = 0.0;
    for (int64_t k = lane; k < nepi; k += TR_WAVE) {
      a += dpart[(k * LM_MAX_M + m) * 2];
      s += dpart[(k * LM_MAX_M + m) * 2 + 1];
    }
    a = wv_allreduce_d(a);
    s = wv_allreduce_d(s);
    if (lane == 0) {
      tm.grad[nfe] = (float)s;                          // d loss / d bias = sum_n r_n
      tm.grad[nfe + 1] = (float)(a * (1.0 / (double)N));  // the data loss (MSE)
      tm.grad[nfe + 2] = 0.f;                           // status slot
    }
    return;
  }
  const bool f1 = b >= I0;
  const int64_t i = f1 ? b - I0 : b;
  const int64_t dg = f1 ? I0 : I1;
  const int64_t sg = f1 ? I1 : 1;
  const float* __restrict__ Fg = phi + (int64_t)m * npmax + (f1 ? 0 : I0 * R);
  const float* __restrict__ Gi = G + (int64_t)m * I0 * I1 + (f1 ? i : i * I1);
  float wr[LM_MAX_R], acc[LM_MAX_R];
#pragma unroll
  for (int r = 0; r < LM_MAX_R; ++r) {
    wr[r] = r < R ? tm.w[r] : 0.f;
    acc[r] = 0.f;
  }
  for (int64_t j = lane; j < dg; j += TR_WAVE) {
    const float gv = Gi[j * sg];
#pragma unroll
    for (int r = 0; r < LM_MAX_R; ++r)
      if (r < R) acc[r] = fmaf(gv, wr[r] * Fg[j * R + r], acc[r]);
  }
  float res = 0.f;
#pragma unroll
  for (int r = 0; r < LM_MAX_R; ++r) {
    if (r < R) {
      const float s = wv_allreduce(acc[r]);
      if (lane == r) res = s;
    }
  }
  if (lane < R) {
    const int64_t e = (f1 ? I0 * R : 0) + i * R + lane;
    tm.grad[e] = res * dphi[(int64_t)m * npmax + e];
  }
}

// k_update<false> for a two-factor model with one bias entry, then k_converge's test, per member.
// The arithmetic is tr_adam.h's and the orders are k_update's (thread t sums the factor elements
// k = t mod 1024 in increasing k, wave butterfly, wave-order sum): given the same gradient bits the
// parameters, the Adam state and the loss record are k_update's bits.
__global__ __launch_bounds__(LM_UPD_T) void k_lm_update(const LmMember* __restrict__ tab, int64_t I0, int64_t I1,
                                                        int k) {
#pragma clang fp contract(off)
  __shared__ float wsum[2 * 16];
  __shared__ float norms[2];
  __shared__ float coef[2];
  const LmMember& tm = tab[blockIdx.x];
  if (k >= tm.n_iters) return;
  if (*tm.stop != 0) return;
  const int t = threadIdx.x;
  const int lane = t & (TR_WAVE - 1);
  const int q = t / TR_WAVE;
  const int R = tm.rank;
  const int64_t off1 = I0 * R;
  const int64_t nfe = (I0 + I1) * R;
  const int64_t np = nfe + 1;
  float* __restrict__ params = tm.params;
  const float* __restrict__ grad = tm.grad;
  float accn[2] = {0.f, 0.f};
  for (int64_t e = t; e < nfe; e += LM_UPD_T) {
    const float a = params[e];
    const int f = e >= off1 ? 1 : 0;
#pragma unroll
    for (int g = 0; g < 2; ++g) accn[g] = g == f ? fmaf(a, a, accn[g]) : accn[g];
  }
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const float r = wv_allreduce(accn[f]);
    if (lane == 0) wsum[f * 16 + q] = r;
  }
  __syncthreads();
  if (t < 2) norm_finish<LM_UPD_T / TR_WAVE>(wsum, t, tm.lambda_l2, norms, coef);
  __syncthreads();
  const bool ams = tm.amsgrad != 0;
  const float step_size = tm.step_size[k], bc2_sqrt = tm.bc2_sqrt[k];
  for (int64_t e = t; e < np; e += LM_UPD_T) {
    float g = grad[e], p = params[e], mm = tm.m[e], vv = tm.v[e], vm = ams ? tm.vmax[e] : 0.f;
    const int f = e >= off1 ? 1 : 0;
    g = e < nfe ? g + coef[f] * (2.0f * p) : g;
    adam_moments(p, g, mm, vv, tm.weight_decay, tm.one_minus_b1, tm.beta2, tm.one_minus_b2);
    vm = fmaxf(vm, vv);
    if (ams) tm.vmax[e] = vm;
    p = adam_param(p, mm, ams ? vm : vv, bc2_sqrt, tm.eps, step_size);
    tm.m[e] = mm;
    tm.v[e] = vv;
    params[e] = p;
  }
  if (t == 0) {
    float l2 = 0.f;
    for (int f = 0; f < 2; ++f) l2 = l2 + norms[f];
    const float total = grad[np] + tm.lambda_l2 * l2;
    const int64_t iter = tm.iter0 + k;
    tm.loss_hist[tm.hist_base + iter] = (double)total;
    if (iter > tm.patience && tm.tol > 0.0) {  // loss_running[ii - patience:], standard…py:467-470
      const int64_t s = iter - tm.patience;
      const int64_t cnt = tm.hist_base + iter - s;
      const double d = np_pairwise_sum_absdiff(tm.loss_hist + s, cnt);
      if (d < tm.tol) *tm.stop = (int32_t)(iter + 1);
    }
  }
}

// ---- scoring (tr_linear_many_score): the forward half, then the metrics' sums ----

// k_lm_prep for three feature modes: phi alone (no gradient follows), the third flag from the LsMember row.
__global__ __launch_bounds__(256) void k_lm_prep3(const LmMember* __restrict__ tab, const LsMember* __restrict__ ext,
                                                  int64_t I0, int64_t I1, int64_t I2, int64_t npmax,
                                                  float* __restrict__ phi) {
  const LmMember& tm = tab[blockIdx.y];
  const int R = tm.rank;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (I0 + I1 + I2) * R) return;
  const int f = e >= (I0 + I1) * R ? 2 : (e >= I0 * R ? 1 : 0);
  const float a = tm.params[e];
  const bool nn = f == 2 ? ext[blockIdx.y].nonneg2 != 0 : tm.nonneg[f] != 0;
  phi[(int64_t)blockIdx.y * npmax + e] = nn ? tr_softplus(a, tm.beta, tm.thr) : a;
}

// k_lm_dense for three feature modes: ((Phi_0 * w) Phi_1) Phi_2, one fmaf chain over the rank
__global__ __launch_bounds__(256) void k_lm_dense3(const LmMember* __restrict__ tab, int M, int64_t I0, int64_t I1,
                                                   int64_t I2, int64_t npmax, const float* __restrict__ phi,
                                                   float* __restrict__ Bt) {
  const int64_t P = I0 * I1 * I2;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int m = blockIdx.y;
  float s = 0.f;
  if (m < M) {
    const LmMember& tm = tab[m];
    const int R = tm.rank;
    const int64_t i = p / (I1 * I2), q = p - i * (I1 * I2);
    const int64_t j = q / I2, k = q - j * I2;
    const float* __restrict__ F0 = phi + (int64_t)m * npmax + i * R;
    const float* __restrict__ F1 = phi + (int64_t)m * npmax + (I0 + j) * R;
    const float* __restrict__ F2 = phi + (int64_t)m * npmax + (I0 + I1 + k) * R;
    for (int r = 0; r < R; ++r) s = fmaf((F0[r] * tm.w[r]) * F1[r], F2[r], s);
  }
  Bt[(int64_t)m * P + p] = s;
}

// k_lm_epilogue's thread layout and its yhat expression; per (row block, column) LS_SUMS fp64
// partials, the 16 threads' sums added in rl order.  The sums are shifted by k = y[0] of the member.
__global__ __launch_bounds__(256) void k_lm_score(const LmMember* __restrict__ tab, const LsMember* __restrict__ ext,
                                                  int M, int64_t N, int64_t isum, const float* __restrict__ Zpart,
                                                  int64_t ns, int64_t npad, double* __restrict__ dpart) {
  __shared__ double sp[LS_SUMS][16][16];
  const int col = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const bool has = col < M;
  const float* __restrict__ y = has ? tab[col].y : nullptr;
  float* __restrict__ yhat = has ? ext[col].yhat : nullptr;
  const float bias = has ? tab[col].params[isum * tab[col].rank] : 0.f;
  const double k0 = y != nullptr ? (double)y[0] : 0.0;
  double acc[LS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < LM_EPI_ROWS / 16; ++k) {
    const int64_t row = (int64_t)blockIdx.x * LM_EPI_ROWS + k * 16 + rl;
    if (row >= N) break;
    float z = 0.f;
    for (int64_t s = 0; s < ns; ++s) z += Zpart[(s * npad + row) * LM_MAX_M + col];
    const float yh = z + bias;
    if (yhat != nullptr) yhat[row] = yh;
    if (y != nullptr) {
      const float yr = y[row];
      const float e = yh - yr;
      const double a = (double)yh - k0, b = (double)yr - k0;
      acc[0] += (double)e * (double)e;
      acc[1] += a;
      acc[2] += a * a;
      acc[3] += b;
      acc[4] += b * b;
    }
  }
#pragma unroll
  for (int q = 0; q < LS_SUMS; ++q) sp[q][rl][col] = acc[q];
  __syncthreads();
  if (threadIdx.x < 16 * LS_SUMS) {
    const int q = threadIdx.x >> 4;  // (col = threadIdx.x & 15 as above)
    double a = 0.0;
    for (int r = 0; r < 16; ++r) a += sp[q][r][col];
    dpart[((int64_t)blockIdx.x * LM_MAX_M + col) * LS_SUMS + q] = a;
  }
}

// One wave per member: the row blocks' partials in k_lm_fold's order (lane l takes the blocks l,
// l + 64, .. in increasing order, then the wave butterfly), so that sums[0] carries the bits of the
// sum the fit's data loss is formed from.
__global__ __launch_bounds__(64) void k_lm_score_sum(const LsMember* __restrict__ ext,
                                                     const double* __restrict__ dpart, int64_t nepi) {
  const int m = blockIdx.x;
  double* __restrict__ out = ext[m].sums;
  if (out == nullptr) return;
  const int lane = threadIdx.x;
  double a[LS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t k = lane; k < nepi; k += TR_WAVE)
#pragma unroll
    for (int q = 0; q < LS_SUMS; ++q) a[q] += dpart[(k * LM_MAX_M + m) * LS_SUMS + q];
#pragma unroll
  for (int q = 0; q < LS_SUMS; ++q) a[q] = wv_allreduce_d(a[q]);
  if (lane < LS_SUMS) {
    double v = a[0];
#pragma unroll
    for (int q = 1; q < LS_SUMS; ++q) v = lane == q ? a[q] : v;
    out[lane] = v;
  }
}

static inline unsigned lm_cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

// The first three launches of a two-mode pass, the fit's and the score's alike.
static void launch_lm_forward2(hipStream_t st, const float* X, int64_t N, int64_t I0, int64_t I1, int64_t xld,
                               const LmMember* table, int M, int64_t npmax, int64_t nrw, int64_t slice, int64_t ns,
                               int64_t npad, float* phi, float* dphi, float* Bt, float* Zp) {
  const int64_t P = I0 * I1;
  hipLaunchKernelGGL(k_lm_prep, dim3(lm_cdiv(npmax, 256), M), dim3(256), 0, st, table, I0, I1, npmax, phi, dphi);
  hipLaunchKernelGGL(k_lm_dense, dim3(lm_cdiv(P, 256), LM_MAX_M), dim3(256), 0, st, table, M, I0, I1, npmax, phi, Bt);
  hipLaunchKernelGGL(k_lm_forward<2>, dim3((unsigned)nrw, (unsigned)ns), dim3(256), 0, st, X, N, P, xld, Bt, slice, Zp,
                     npad);
}

int launch_linear_many_score(const LsGeom& g, const float* X, int64_t xld, const LmMember* table, const LsMember* ext,
                             int n_members, const LsWork& w, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int M = n_members;
  const int64_t npad = g.nepi * LM_EPI_ROWS;
  if (xld == 0) xld = g.P;
  if (g.n_modes == 2) {
    launch_lm_forward2(st, X, g.N, g.I[0], g.I[1], xld, table, M, g.npmax, g.nrw, g.slice, g.ns, npad, w.phi, w.dphi,
                       w.Bt, w.Z);
  } else {
    hipLaunchKernelGGL(k_lm_prep3, dim3(lm_cdiv(g.npmax, 256), M), dim3(256), 0, st, table, ext, g.I[0], g.I[1],
                       g.I[2], g.npmax, w.phi);
    hipLaunchKernelGGL(k_lm_dense3, dim3(lm_cdiv(g.P, 256), LM_MAX_M), dim3(256), 0, st, table, M, g.I[0], g.I[1],
                       g.I[2], g.npmax, w.phi, w.Bt);
    hipLaunchKernelGGL(k_lm_forward<2>, dim3((unsigned)g.nrw, (unsigned)g.ns), dim3(256), 0, st, X, g.N, g.P, xld, w.Bt,
                       g.slice, w.Z, npad);
  }
  hipLaunchKernelGGL(k_lm_score, dim3((unsigned)g.nepi), dim3(256), 0, st, table, ext, M, g.N, g.isum, w.Z, g.ns, npad,
                     w.D);
  hipLaunchKernelGGL(k_lm_score_sum, dim3(M), dim3(TR_WAVE), 0, st, ext, w.D, g.nepi);
  return (int)hipGetLastError();
}

int launch_linear_many_loss_grad(const LmGeom& g, const float* X, int64_t xld, const LmMember* table, int n_members,
                                 void* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  float* Bt = reinterpret_cast<float*>(ws + g.oBt);
  float* G = reinterpret_cast<float*>(ws + g.oG);
  float* phi = reinterpret_cast<float*>(ws + g.oPhi);
  float* dphi = reinterpret_cast<float*>(ws + g.oDphi);
  float* Rr = reinterpret_cast<float*>(ws + g.oR);
  float* Zp = reinterpret_cast<float*>(ws + g.oZ);
  double* dpart = reinterpret_cast<double*>(ws + g.oD);
  float* gpart = reinterpret_cast<float*>(ws + g.oGp);
  const int M = n_members;
  const int64_t npad = g.nepi * LM_EPI_ROWS;
  if (xld == 0) xld = g.P;
  launch_lm_forward2(st, X, g.N, g.I0, g.I1, xld, table, M, g.npmax, g.nrw, g.slice, g.ns, npad, phi, dphi, Bt, Zp);
  hipLaunchKernelGGL(k_lm_epilogue, dim3((unsigned)g.nepi), dim3(256), 0, st, table, M, g.N, g.I0 + g.I1, Zp,
                     g.ns, npad, (float)(2.0 / (double)g.N), Rr, dpart);
  hipLaunchKernelGGL(k_lm_grad, dim3(lm_cdiv(g.nfw, 4), (unsigned)g.nch), dim3(256), 0, st, X, g.N, g.P, xld, Rr, g.rpc,
                     g.nch, gpart);
  hipLaunchKernelGGL(k_lm_reduce, dim3(lm_cdiv(g.P, 1024), M), dim3(256), 0, st, gpart, g.P, g.nch, G);
  hipLaunchKernelGGL(k_lm_fold, dim3((unsigned)(g.I0 + g.I1 + 1), M), dim3(TR_WAVE), 0, st, table, g.N, g.I0, g.I1,
                     g.npmax, phi, dphi, G, dpart, g.nepi);
  return (int)hipGetLastError();
}

int launch_linear_many_update(const LmGeom& g, LmMember* table, int n_members, int k, void* stream) {
  hipLaunchKernelGGL(k_lm_update, dim3(n_members), dim3(LM_UPD_T), 0, (hipStream_t)stream, table, g.I0, g.I1, k);
  return (int)hipGetLastError();
}

}  // namespace tr
