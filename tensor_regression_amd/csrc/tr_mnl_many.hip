// tr_mnl_many.hip — the shared-X multinomial sweep: CP multinomial models (two feature modes and a
// class factor) over one X.  A model with C classes is C columns of a dense coefficient matrix; a
// group holds up to 64 columns, four 16-column tiles of v_mfma_f32_16x16x4_f32 (exact fp32 products,
// a k-ordered fmaf chain per output).  The forward passes are one skinny GEMM Z = X . Bt^T and the
// gradient passes another, G = R^T . X, so an iteration reads X twice whatever the members are.
//
//   k_mm_prep      phi = softplus?(A), dphi for three factors        grid (elements, M)
//   k_mm_dense     Bt[col][p] = sum_r (phi0[i, r] w_r phi2[c, r]) phi1[j, r]; columns past the total zero
//                                                                    grid (P / 256, 16 tiles)
//   k_mm_forward   Zpart[s][n][col] over feature slice s, templated  grid (row blocks, slices)
//                  on the column tiles in use; an X fragment feeds every tile, Bt is staged in LDS
//   k_mm_epilogue  one thread per (row, member): z = sum_s Zpart (slice order), S = softmax(z), the
//                  CrossEntropyLoss of S (the module's double softmax), R[n][col] = dL/dz; an fp64
//                  partial of sum cw[y] l per (row block, member)    grid (row blocks of 256, M + 1)
//   k_mm_grad      slab[c][col][p] = sum_{n in chunk c} R[n, col] X[n, p], last chunk first
//                                                                    grid (feature blocks, chunks)
//   k_mm_reduce    G[col][p] = sum_c slab[c][col][p] (chunk order)    grid (P / 1024, columns)
//   k_mm_fold1     H[col][i][r] = sum_j G[col][i, j] phi1[j, r] and  grid (I0 + I1, M, 16)
//                  K[col][j][r] = sum_i G[col][i, j] phi0[i, r]
//   k_mm_fold2     the three factor gradients from H, K, the class factor and the softplus chain, into
//                  the member's grad arena; the data loss            grid (I0 + I1 + 17, M)
//   k_mm_update    k_update<false>'s step (tr_adam.h) + k_converge's plateau test, a workgroup per member
//
// Nine launches per iteration whatever the members are.  Invariants:
//   * no floating-point atomics;
//   * slices, chunks and every summation order depend on (N, I0, I1) alone (MmGeom), not on the number
//     of members, columns or tiles: a column of an MFMA tile is computed from its own operands only,
//     in the same order in every instantiation;
//   * so a member's bits depend neither on the other members, nor on its column position, nor on the
//     group size;
//   * given the same gradient bits the update is tr_adam_step's, bit for bit;
//   * the forward and gradient kernels use no scratch (DESIGN.md records their registers).
#include "tr_mnl_many.h"

#include "tr_adam.h"
#include "tr_common.h"
#include "tr_np_sum.h"

namespace tr {

namespace {
constexpr int MM_UPD_T = 1024;
}

__device__ __forceinline__ const MmCols* mm_cols(const MmMember* tab, int M) {
  return reinterpret_cast<const MmCols*>(tab + M);
}

__global__ __launch_bounds__(256) void k_mm_prep(const MmMember* __restrict__ tab, int64_t I0, int64_t I1,
                                                 int64_t npmax, float* __restrict__ phi,
                                                 float* __restrict__ dphi) {
  const MmMember& tm = tab[blockIdx.y];
  const int R = tm.rank;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (I0 + I1 + tm.n_classes) * R) return;
  const int f = e >= (I0 + I1) * R ? 2 : (e >= I0 * R ? 1 : 0);
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

// cp_to_tensor for one class column: ((Phi_0 * w) * Phi_2[c]) @ Phi_1^T, one fmaf chain over the rank
__global__ __launch_bounds__(256) void k_mm_dense(const MmMember* __restrict__ tab, int M, int64_t I0, int64_t I1,
                                                  int64_t npmax, const float* __restrict__ phi,
                                                  float* __restrict__ Bt) {
  const int64_t P = I0 * I1;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int col = blockIdx.y;
  const MmCols* __restrict__ cols = mm_cols(tab, M);
  const int m = cols->member[col];
  float s = 0.f;
  if (m >= 0) {
    const MmMember& tm = tab[m];
    const int R = tm.rank;
    const int64_t i = p / I1, j = p - i * I1;
    const float* __restrict__ F0 = phi + (int64_t)m * npmax + i * R;
    const float* __restrict__ F1 = phi + (int64_t)m * npmax + I0 * R + j * R;
    const float* __restrict__ F2 = phi + (int64_t)m * npmax + (I0 + I1) * R + (int64_t)cols->cls[col] * R;
    for (int r = 0; r < R; ++r) s = fmaf((F0[r] * tm.w[r]) * F2[r], F1[r], s);
  }
  Bt[(int64_t)col * P + p] = s;
}

// Forward on the matrix cores.  Lane (i, g) loads 8 consecutive features of its two rows per 32-feature
// step and reads Bt row i of every tile from LDS; the first float4 feeds accumulator chain 0 and the
// second chain 1, a component at a time; the 2 chains are added every MM_FOLD features.  A wave takes 2
// tiles of 16 rows, a workgroup's 4 waves 128 rows over the same feature slice; the X fragments of a
// step are reused for each of the NT column tiles.  A column's chain sees the same operands in the
// same order for every NT.  The tail of the last slice (P a multiple of 4, not of 32) is zero-filled.
// The workgroup's Bt slice is staged in LDS in chunks of MM_STAGE_K features of every tile's 16
// columns, double-buffered (the next chunk's global loads are in flight during the MFMAs of this one,
// one barrier per chunk), rows padded by 4 floats so that the 16 columns of a 16-byte read fall into
// distinct banks.  Features past the slice's end are zero in LDS.  No wave leaves before the last
// barrier: a wave past the last row computes on row N - 1 and stores nothing.
constexpr int MM_STAGE_K = 64;
constexpr int MM_STAGE_LD = MM_STAGE_K + 4;

template <int NT>
__global__ __launch_bounds__(256) void k_mm_forward(const float* __restrict__ X, int64_t N, int64_t P, int64_t xld,
                                                    const float* __restrict__ Bt, int64_t slice,
                                                    float* __restrict__ Zpart, int64_t npad) {
  constexpr int RT = 2;
  constexpr int NQ = NT * 16 * (MM_STAGE_K / 4) / 256;  // float4 of a chunk per thread
  __shared__ float sB[2][NT * 16][MM_STAGE_LD];
  const int lane = threadIdx.x & (TR_WAVE - 1);
  const int wave = threadIdx.x / TR_WAVE;
  const int i = lane & 15, g = lane >> 4;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * RT);
  const int64_t pb = (int64_t)blockIdx.y * slice;
  const int64_t pe = pb + slice < P ? pb + slice : P;
  const float* xr[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    int64_t r = row0 + rt * 16 + i;
    r = r < N ? r : N - 1;
    xr[rt] = X + r * xld + pb;
  }
  wv_f4 ac[RT][NT][2], acc[RT][NT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc[rt][t] = wv_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 2; ++c) ac[rt][t][c] = wv_f4{0.f, 0.f, 0.f, 0.f};
    }
  auto fold = [&]() {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        acc[rt][t] += ac[rt][t][0] + ac[rt][t][1];
#pragma unroll
        for (int c = 0; c < 2; ++c) ac[rt][t][c] = wv_f4{0.f, 0.f, 0.f, 0.f};
      }
  };
  auto mfmas = [&](const float4(&xa)[RT], const float4(&xb)[RT], const float4(&ba)[NT], const float4(&bb)[NT]) {
    auto comp = [](const float4& v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w)); };
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          ac[rt][t][0] = wv_mfma_16x16x4(comp(xa[rt], k), comp(ba[t], k), ac[rt][t][0]);
          ac[rt][t][1] = wv_mfma_16x16x4(comp(xb[rt], k), comp(bb[t], k), ac[rt][t][1]);
        }
  };
  auto ld = [](const float* p) { return *reinterpret_cast<const float4*>(p); };
  const int64_t len = pe - pb;
  const int nfull = (int)(len / 32);
  const int rem = (int)(len - 32 * (int64_t)nfull);  // 0, 4, .., 28 features past the last full step
  const int nsteps = nfull + (rem > 0 ? 1 : 0);
  const int nchunks = (nsteps + MM_STAGE_K / 32 - 1) / (MM_STAGE_K / 32);
  const int o = 8 * g;  // this lane's features of a step: o .. o + 7
  // thread's share of a chunk: float4 q covers column (q * 256 + tid) / 32, features 4 * ((q * 256 + tid) % 32) ..
  float4 stage[NQ];
  auto fetch = [&](int c) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int idx = q * 256 + (int)threadIdx.x;
      const int col = idx / (MM_STAGE_K / 4), f = 4 * (idx % (MM_STAGE_K / 4));
      const int64_t p = pb + (int64_t)c * MM_STAGE_K + f;
      stage[q] = p < pe ? ld(Bt + (int64_t)col * P + p) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int idx = q * 256 + (int)threadIdx.x;
      const int col = idx / (MM_STAGE_K / 4), f = 4 * (idx % (MM_STAGE_K / 4));
      *reinterpret_cast<float4*>(&sB[buf][col][f]) = stage[q];
    }
  };
  fetch(0);
  put(0);
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunks) fetch(c + 1);
#pragma unroll
    for (int s = 0; s < MM_STAGE_K / 32; ++s) {
      const int st = c * (MM_STAGE_K / 32) + s;
      if (st < nfull) {
        float4 xa[RT], xb[RT], ba[NT], bb[NT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          xa[rt] = ld(xr[rt] + 32 * st + o);
          xb[rt] = ld(xr[rt] + 32 * st + o + 4);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          ba[t] = *reinterpret_cast<const float4*>(&sB[buf][16 * t + i][32 * s + o]);
          bb[t] = *reinterpret_cast<const float4*>(&sB[buf][16 * t + i][32 * s + o + 4]);
        }
        mfmas(xa, xb, ba, bb);
        if (((st + 1) & 15) == 0) fold();
      }
    }
    if (rem > 0 && c == nchunks - 1) {  // the tail step, zero-filled
      const int s = nfull - c * (MM_STAGE_K / 32);
      const bool va = o < rem, vb = o + 4 < rem;
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      float4 xa[RT], xb[RT], ba[NT], bb[NT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        xa[rt] = va ? ld(xr[rt] + 32 * nfull + o) : zero;
        xb[rt] = vb ? ld(xr[rt] + 32 * nfull + o + 4) : zero;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        ba[t] = *reinterpret_cast<const float4*>(&sB[buf][16 * t + i][32 * s + o]);
        bb[t] = *reinterpret_cast<const float4*>(&sB[buf][16 * t + i][32 * s + o + 4]);
      }
      mfmas(xa, xb, ba, bb);
    }
    if (c + 1 < nchunks) put(buf ^ 1);
    __syncthreads();
  }
  fold();
  float* __restrict__ zp = Zpart + (int64_t)blockIdx.y * npad * MM_MAX_COLS;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t row = row0 + rt * 16 + 4 * g + reg;
      if (row < N) {
#pragma unroll
        for (int t = 0; t < NT; ++t) zp[row * MM_MAX_COLS + 16 * t + i] = acc[rt][t][reg];
      }
    }
}

// One thread per (row, member); blockIdx.y == M zero-fills the columns between the group's total and
// the end of its last tile.  k_softmax_rows' arithmetic with the classes walked in order by one thread.
// A member's fp64 partial of a row block: wave butterfly, then the 4 waves in order.
__global__ __launch_bounds__(256) void k_mm_epilogue(const MmMember* __restrict__ tab, int M, int64_t N,
                                                     const float* __restrict__ Zpart, int64_t ns, int64_t npad,
                                                     float* __restrict__ Rr, double* __restrict__ dpart) {
  __shared__ double wsum[4];
  const int64_t row = (int64_t)blockIdx.x * MM_EPI_ROWS + threadIdx.x;
  if ((int)blockIdx.y == M) {
    const MmCols* __restrict__ cols = mm_cols(tab, M);
    if (row < N)
      for (int c = cols->total; c < cols->tiles * MM_TILE; ++c) Rr[row * MM_MAX_COLS + c] = 0.f;
    return;
  }
  const MmMember& tm = tab[blockIdx.y];
  const int C = tm.n_classes;
  const int col0 = tm.col0;
  double lw = 0.0;
  if (row < N) {
    float z[MM_MAX_C];
#pragma unroll
    for (int c = 0; c < MM_MAX_C; ++c) z[c] = 0.f;
    for (int64_t s = 0; s < ns; ++s) {
      const float* __restrict__ zr = Zpart + (s * npad + row) * MM_MAX_COLS + col0;
#pragma unroll
      for (int c = 0; c < MM_MAX_C; ++c)
        if (c < C) z[c] += zr[c];
    }
    const float NEG = -__builtin_huge_valf();
    float mx = NEG;
#pragma unroll
    for (int c = 0; c < MM_MAX_C; ++c)
      if (c < C) mx = fmaxf(mx, z[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < MM_MAX_C; ++c)
      if (c < C) {
        z[c] = expf(z[c] - mx);
        sum += z[c];
      }
    const float inv = 1.0f / sum;
    float m2 = NEG;
#pragma unroll
    for (int c = 0; c < MM_MAX_C; ++c)
      if (c < C) {
        z[c] = z[c] * inv;  // S = softmax(z), the model's output
        m2 = fmaxf(m2, z[c]);
      }
    float s2 = 0.f;
#pragma unroll
    for (int c = 0; c < MM_MAX_C; ++c)
      if (c < C) s2 += expf(z[c] - m2);
    const float lse = logf(s2), inv2 = 1.0f / s2;
    const int yl = (int)tm.y[row];
    const float cw = tm.cw[yl];
    const float gsc = cw * tm.inv_w;
    float dS[MM_MAX_C];
    float dot = 0.f, sy = 0.f;
#pragma unroll
    for (int c = 0; c < MM_MAX_C; ++c)
      if (c < C) {
        dS[c] = (expf(z[c] - m2) * inv2 - (c == yl ? 1.0f : 0.0f)) * gsc;
        dot = fmaf(dS[c], z[c], dot);
        sy = c == yl ? z[c] : sy;
      }
    lw = (double)cw * (double)(-((sy - m2) - lse));
    float* __restrict__ rr = Rr + row * MM_MAX_COLS + col0;
#pragma unroll
    for (int c = 0; c < MM_MAX_C; ++c)
      if (c < C) rr[c] = z[c] * (dS[c] - dot);
  }
  lw = wv_allreduce_d(lw);
  if ((threadIdx.x & (TR_WAVE - 1)) == 0) wsum[threadIdx.x / TR_WAVE] = lw;
  __syncthreads();
  if (threadIdx.x == 0)
    dpart[(int64_t)blockIdx.x * MM_MAX_MEMBERS + blockIdx.y] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// Gradient slabs on the matrix cores: D[col][p] += sum_k R[n0 + k][col] X[n0 + k][p], 4 rows per MFMA.
// Lane (i, g) supplies A = R[n0 + g][16 t + i] for tile t and loads the float4 X[n0 + g][p0 + 64 u + 4 i ..];
// MFMA j of feature tile u takes component j, so the lane's four results of a column are 4 consecutive
// features.  A wave owns 128 features (2 tiles of 64; 8 accumulators of 4 per column tile, 32 for four
// tiles) and walks its chunk's rows 8 at a time; an X load feeds every column tile.
template <int NT>
__global__ __launch_bounds__(256) void k_mm_grad(const float* __restrict__ X, int64_t N, int64_t P, int64_t xld,
                                                 const float* __restrict__ Rr, int64_t rpc, int64_t nch,
                                                 float* __restrict__ gpart) {
  constexpr int NU = MM_GRAD_FEATS / 64;
  const int lane = threadIdx.x & (TR_WAVE - 1);
  const int wave = threadIdx.x / TR_WAVE;
  const int i = lane & 15, g = lane >> 4;
  const int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * MM_GRAD_FEATS;
  if (p0 >= P) return;
  const int64_t c = nch - 1 - (int64_t)blockIdx.y;  // the rows the forward read last come first
  const int64_t nb = c * rpc;
  const int64_t ne = nb + rpc < N ? nb + rpc : N;
  bool pv[NU];
  int64_t po[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int64_t p = p0 + 64 * u + 4 * i;
    pv[u] = p < P;
    po[u] = pv[u] ? p : p0;
  }
  wv_f4 acc[NT][NU][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t][u][j] = wv_f4{0.f, 0.f, 0.f, 0.f};
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t n = nb; n < ne; n += 8) {
    const int64_t ra = n + g, rb = n + 4 + g;
    const bool oka = ra < ne, okb = rb < ne;
    const float* __restrict__ xa = X + (oka ? ra : nb) * xld;
    const float* __restrict__ xb = X + (okb ? rb : nb) * xld;
    float4 va[NU], vb[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      va[u] = *reinterpret_cast<const float4*>(xa + po[u]);
      vb[u] = *reinterpret_cast<const float4*>(xb + po[u]);
    }
    float wa[NT], wb[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      wa[t] = oka ? Rr[ra * MM_MAX_COLS + 16 * t + i] : 0.f;
      wb[t] = okb ? Rr[rb * MM_MAX_COLS + 16 * t + i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const float4 a = oka && pv[u] ? va[u] : zero;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        acc[t][u][0] = wv_mfma_16x16x4(wa[t], a.x, acc[t][u][0]);
        acc[t][u][1] = wv_mfma_16x16x4(wa[t], a.y, acc[t][u][1]);
        acc[t][u][2] = wv_mfma_16x16x4(wa[t], a.z, acc[t][u][2]);
        acc[t][u][3] = wv_mfma_16x16x4(wa[t], a.w, acc[t][u][3]);
      }
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const float4 b = okb && pv[u] ? vb[u] : zero;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        acc[t][u][0] = wv_mfma_16x16x4(wb[t], b.x, acc[t][u][0]);
        acc[t][u][1] = wv_mfma_16x16x4(wb[t], b.y, acc[t][u][1]);
        acc[t][u][2] = wv_mfma_16x16x4(wb[t], b.z, acc[t][u][2]);
        acc[t][u][3] = wv_mfma_16x16x4(wb[t], b.w, acc[t][u][3]);
      }
    }
  }
  // result layout: column of the tile = 4 * (lane >> 4) + reg, feature = lane & 15
  float* __restrict__ slab = gpart + c * MM_MAX_COLS * P;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (pv[u])
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          *reinterpret_cast<float4*>(slab + (int64_t)(16 * t + 4 * g + reg) * P + po[u]) =
              make_float4(acc[t][u][0][reg], acc[t][u][1][reg], acc[t][u][2][reg], acc[t][u][3][reg]);
}

__global__ __launch_bounds__(256) void k_mm_reduce(const float* __restrict__ gpart, int64_t P, int64_t nch,
                                                   float* __restrict__ G) {
  const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p >= P) return;
  const int64_t col = blockIdx.y;
  float4 s = *reinterpret_cast<const float4*>(gpart + col * P + p);
  for (int64_t c = 1; c < nch; ++c) {
    const float4 v = *reinterpret_cast<const float4*>(gpart + (c * MM_MAX_COLS + col) * P + p);
    s.x += v.x;
    s.y += v.y;
    s.z += v.z;
    s.w += v.w;
  }
  *reinterpret_cast<float4*>(G + col * P + p) = s;
}

// The wave's sum over k of gv(k) * F[k, r] for every r < R, lane k mod 64 first, then the butterfly;
// lane r keeps the result of rank r.
__device__ __forceinline__ float mm_wave_rows(const float* __restrict__ Gv, int64_t gs, const float* __restrict__ F,
                                              int64_t fs, int64_t n, int R, int lane) {
  float acc[MM_MAX_R];
#pragma unroll
  for (int r = 0; r < MM_MAX_R; ++r) acc[r] = 0.f;
  for (int64_t k = lane; k < n; k += TR_WAVE) {
    const float gv = Gv[k * gs];
#pragma unroll
    for (int r = 0; r < MM_MAX_R; ++r)
      if (r < R) acc[r] = fmaf(gv, F[k * fs + r], acc[r]);
  }
  float res = 0.f;
#pragma unroll
  for (int r = 0; r < MM_MAX_R; ++r) {
    if (r < R) {
      const float s = wv_allreduce(acc[r]);
      if (lane == r) res = s;
    }
  }
  return res;
}

// The wave's sum over i < n of F[i, r] * Hc[i][r] for every r < R, in mm_wave_rows' order.
__device__ __forceinline__ float mm_wave_dot(const float* __restrict__ F, const float* __restrict__ Hc, int64_t n,
                                             int R, int lane) {
  float acc[MM_MAX_R];
#pragma unroll
  for (int r = 0; r < MM_MAX_R; ++r) acc[r] = 0.f;
  for (int64_t k = lane; k < n; k += TR_WAVE) {
#pragma unroll
    for (int r = 0; r < MM_MAX_R; ++r)
      if (r < R) acc[r] = fmaf(F[k * R + r], Hc[k * MM_MAX_R + r], acc[r]);
  }
  float res = 0.f;
#pragma unroll
  for (int r = 0; r < MM_MAX_R; ++r) {
    if (r < R) {
      const float s = wv_allreduce(acc[r]);
      if (lane == r) res = s;
    }
  }
  return res;
}

// First fold stage, one wave per (factor row, member, class): the contraction of the class's gradient
// plane G[col] with the other feature factor.  Rows b < I0 give H[col][b][r], rows b >= I0 K[col][b][r].
__global__ __launch_bounds__(64) void k_mm_fold1(const MmMember* __restrict__ tab, int64_t I0, int64_t I1,
                                                 int64_t npmax, int64_t nh, const float* __restrict__ phi,
                                                 const float* __restrict__ G, float* __restrict__ H) {
  const int m = blockIdx.y;
  const MmMember& tm = tab[m];
  const int c = blockIdx.z;
  if (c >= tm.n_classes) return;
  const int R = tm.rank;
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t col = tm.col0 + c;
  const bool f1 = b >= I0;
  const int64_t i = f1 ? b - I0 : b;
  const float* __restrict__ Fg = phi + (int64_t)m * npmax + (f1 ? 0 : I0 * R);
  const float* __restrict__ Gi = G + col * I0 * I1 + (f1 ? i : i * I1);
  const float res = mm_wave_rows(Gi, f1 ? I1 : 1, Fg, R, f1 ? I0 : I1, R, lane);
  if (lane < R) H[col * nh + b * MM_MAX_R + lane] = res;
}

// Second fold stage, one wave per (row, member).  Feature factor rows: grad = dphi w_r sum_c phi2[c, r]
// H[col0 + c][b][r], classes in order.  Class rows: grad = dphi w_r sum_i phi0[i, r] H[col0 + c][i][r].
// The last wave: the data loss from the fp64 partials, sum cw[y] l / W.
__global__ __launch_bounds__(64) void k_mm_fold2(const MmMember* __restrict__ tab, int64_t I0, int64_t I1,
                                                 int64_t npmax, int64_t nh, const float* __restrict__ phi,
                                                 const float* __restrict__ dphi, const float* __restrict__ H,
                                                 const double* __restrict__ dpart, int64_t nepi) {
  const int m = blockIdx.y;
  const MmMember& tm = tab[m];
  const int R = tm.rank, C = tm.n_classes;
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t nfe = (I0 + I1 + C) * R;
  const float* __restrict__ ph = phi + (int64_t)m * npmax;
  const float* __restrict__ dp = dphi + (int64_t)m * npmax;
  if (b == I0 + I1 + MM_MAX_C) {
    double a = 0.0;
    for (int64_t k = lane; k < nepi; k += TR_WAVE) a += dpart[k * MM_MAX_MEMBERS + m];
    a = wv_allreduce_d(a);
    if (lane == 0) {
      tm.grad[nfe] = (float)(a / tm.cw_norm);  // the data loss
      tm.grad[nfe + 1] = 0.f;                  // status slot
    }
    return;
  }
  if (b < I0 + I1) {
    if (lane >= R) return;
    const float* __restrict__ F2 = ph + (I0 + I1) * R;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s = fmaf(F2[c * R + lane], H[(int64_t)(tm.col0 + c) * nh + b * MM_MAX_R + lane], s);
    const int64_t e = b * R + lane;
    tm.grad[e] = (tm.w[lane] * s) * dp[e];
    return;
  }
  const int c = (int)(b - (I0 + I1));
  if (c >= C) return;
  const float res = mm_wave_dot(ph, H + (int64_t)(tm.col0 + c) * nh, I0, R, lane);
  if (lane < R) {
    const int64_t e = (I0 + I1) * R + (int64_t)c * R + lane;
    tm.grad[e] = (tm.w[lane] * res) * dp[e];
  }
}

// k_update<false> for a three-factor model without bias entries, then k_converge's test, per member.
// The arithmetic is tr_adam.h's and the orders are k_update's (thread t sums the factor elements
// k = t mod 1024 in increasing k, wave butterfly, wave-order sum): given the same gradient bits the
// parameters, the Adam state and the loss record are k_update's bits.
__global__ __launch_bounds__(MM_UPD_T) void k_mm_update(const MmMember* __restrict__ tab, int64_t I0, int64_t I1,
                                                        int k) {
#pragma clang fp contract(off)
  __shared__ float wsum[3 * 16];
  __shared__ float norms[3];
  __shared__ float coef[3];
  const MmMember& tm = tab[blockIdx.x];
  if (k >= tm.n_iters) return;
  if (*tm.stop != 0) return;
  const int t = threadIdx.x;
  const int lane = t & (TR_WAVE - 1);
  const int q = t / TR_WAVE;
  const int R = tm.rank;
  const int64_t off1 = I0 * R, off2 = (I0 + I1) * R;
  const int64_t np = (I0 + I1 + tm.n_classes) * R;
  float* __restrict__ params = tm.params;
  const float* __restrict__ grad = tm.grad;
  float accn[3] = {0.f, 0.f, 0.f};
  for (int64_t e = t; e < np; e += MM_UPD_T) {
    const float a = params[e];
    const int f = e >= off2 ? 2 : (e >= off1 ? 1 : 0);
#pragma unroll
    for (int g = 0; g < 3; ++g) accn[g] = g == f ? fmaf(a, a, accn[g]) : accn[g];
  }
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const float r = wv_allreduce(accn[f]);
    if (lane == 0) wsum[f * 16 + q] = r;
  }
  __syncthreads();
  if (t < 3) norm_finish<MM_UPD_T / TR_WAVE>(wsum, t, tm.lambda_l2, norms, coef);
  __syncthreads();
  const bool ams = tm.amsgrad != 0;
  const float step_size = tm.step_size[k], bc2_sqrt = tm.bc2_sqrt[k];
  for (int64_t e = t; e < np; e += MM_UPD_T) {
    float g = grad[e], p = params[e], mm = tm.m[e], vv = tm.v[e], vm = ams ? tm.vmax[e] : 0.f;
    const int f = e >= off2 ? 2 : (e >= off1 ? 1 : 0);
    g = g + coef[f] * (2.0f * p);
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
    for (int f = 0; f < 3; ++f) l2 = l2 + norms[f];
    const float total = grad[np] + tm.lambda_l2 * l2;
    const int64_t iter = tm.iter0 + k;
    tm.loss_hist[tm.hist_base + iter] = (double)total;
    if (iter > tm.patience && tm.tol > 0.0) {  // loss_running[ii - patience:], multinomial…py:462-465
      const int64_t s = iter - tm.patience;
      const int64_t cnt = tm.hist_base + iter - s;
      const double d = np_pairwise_sum_absdiff(tm.loss_hist + s, cnt);
      if (d < tm.tol) *tm.stop = (int32_t)(iter + 1);
    }
  }
}

static inline unsigned mm_cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

template <int NT>
static void mm_gemms_forward(const MmGeom& g, const float* X, int64_t xld, const float* Bt, float* Zp, int64_t npad,
                             hipStream_t st) {
  hipLaunchKernelGGL(k_mm_forward<NT>, dim3((unsigned)g.nrw, (unsigned)g.ns), dim3(256), 0, st, X, g.N, g.P, xld, Bt,
                     g.slice, Zp, npad);
}

template <int NT>
static void mm_gemms_grad(const MmGeom& g, const float* X, int64_t xld, const float* Rr, float* gpart, hipStream_t st) {
  hipLaunchKernelGGL(k_mm_grad<NT>, dim3(mm_cdiv(g.nfw, 4), (unsigned)g.nch), dim3(256), 0, st, X, g.N, g.P, xld, Rr,
                     g.rpc, g.nch, gpart);
}

int launch_mnl_many_loss_grad(const MmGeom& g, const float* X, int64_t xld, const void* table, int n_members,
                              int n_cols, void* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const MmMember* tab = static_cast<const MmMember*>(table);
  char* ws = static_cast<char*>(workspace);
  float* Bt = reinterpret_cast<float*>(ws + g.oBt);
  float* G = reinterpret_cast<float*>(ws + g.oG);
  float* phi = reinterpret_cast<float*>(ws + g.oPhi);
  float* dphi = reinterpret_cast<float*>(ws + g.oDphi);
  float* Rr = reinterpret_cast<float*>(ws + g.oR);
  float* Zp = reinterpret_cast<float*>(ws + g.oZ);
  double* dpart = reinterpret_cast<double*>(ws + g.oD);
  float* H = reinterpret_cast<float*>(ws + g.oH);
  float* gpart = reinterpret_cast<float*>(ws + g.oGp);
  const int M = n_members;
  const int tiles = (n_cols + MM_TILE - 1) / MM_TILE;
  if (M < 1 || tiles < 1 || tiles > MM_MAX_COLS / MM_TILE) return (int)hipErrorInvalidValue;
  const int64_t npad = g.nepi * MM_EPI_ROWS;
  if (xld == 0) xld = g.P;
  hipLaunchKernelGGL(k_mm_prep, dim3(mm_cdiv(g.npmax, 256), M), dim3(256), 0, st, tab, g.I0, g.I1, g.npmax, phi, dphi);
  hipLaunchKernelGGL(k_mm_dense, dim3(mm_cdiv(g.P, 256), tiles * MM_TILE), dim3(256), 0, st, tab, M, g.I0, g.I1,
                     g.npmax, phi, Bt);
  switch (tiles) {
    case 1: mm_gemms_forward<1>(g, X, xld, Bt, Zp, npad, st); break;
    case 2: mm_gemms_forward<2>(g, X, xld, Bt, Zp, npad, st); break;
    case 3: mm_gemms_forward<3>(g, X, xld, Bt, Zp, npad, st); break;
    default: mm_gemms_forward<4>(g, X, xld, Bt, Zp, npad, st); break;
  }
  hipLaunchKernelGGL(k_mm_epilogue, dim3((unsigned)g.nepi, M + 1), dim3(256), 0, st, tab, M, g.N, Zp, g.ns, npad, Rr,
                     dpart);
  switch (tiles) {
    case 1: mm_gemms_grad<1>(g, X, xld, Rr, gpart, st); break;
    case 2: mm_gemms_grad<2>(g, X, xld, Rr, gpart, st); break;
    case 3: mm_gemms_grad<3>(g, X, xld, Rr, gpart, st); break;
    default: mm_gemms_grad<4>(g, X, xld, Rr, gpart, st); break;
  }
  hipLaunchKernelGGL(k_mm_reduce, dim3(mm_cdiv(g.P, 1024), n_cols), dim3(256), 0, st, gpart, g.P, g.nch, G);
  hipLaunchKernelGGL(k_mm_fold1, dim3((unsigned)(g.I0 + g.I1), M, MM_MAX_C), dim3(TR_WAVE), 0, st, tab, g.I0, g.I1,
                     g.npmax, g.nh, phi, G, H);
  hipLaunchKernelGGL(k_mm_fold2, dim3((unsigned)(g.I0 + g.I1 + MM_MAX_C + 1), M), dim3(TR_WAVE), 0, st, tab, g.I0,
                     g.I1, g.npmax, g.nh, phi, dphi, H, dpart, g.nepi);
  return (int)hipGetLastError();
}

int launch_mnl_many_update(const MmGeom& g, void* table, int n_members, int k, void* stream) {
  hipLaunchKernelGGL(k_mm_update, dim3(n_members), dim3(MM_UPD_T), 0, (hipStream_t)stream,
                     static_cast<const MmMember*>(table), g.I0, g.I1, k);
  return (int)hipGetLastError();
}

}  // namespace tr
