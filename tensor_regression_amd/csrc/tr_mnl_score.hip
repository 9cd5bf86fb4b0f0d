// tr_mnl_score.hip — the scoring sweep of the multinomial modules: the forward pass, the argmax, the
// confusion counts and the data loss of many (model, data set) pairs in one launch (what a
// hyperparameter grid keeps of every grid point after its fit: demo_tensorRegression_forKim.ipynb calls
// predict + confusion_matrix four times per fitted model).
//
// k_mnl_score_many is table driven like k_mnl_resident_many: a member of the table is one pair, cut
// into row blocks of SCORE_ROWS rows, one 1024-thread workgroup per (member, row block); workgroup b
// finds its member through the table's first_block column (a prefix table).  The workgroups share
// nothing but the integer counts, wait on nothing, and may exceed the CUs.  One workgroup:
//   1  phi = softplus(A) or A                                          (thread per parameter)
//   2  B[c][p] = sum_r (phi0[i0, r] w_r) (phi1[i1, r] phi2[c, r])       (thread per (c, p); the resident
//                                                                       fit's association, r ascending)
//   3  per row, one wave: lanes over the features p (X rows are contiguous in global memory, so the
//      reads coalesce; B is class-major in LDS, so lanes read consecutive words), each lane's p
//      ascending, then the xor butterfly per class: Z[n, c]
//      S = softmax(Z) with the row maximum subtracted; pred = first index of max S; the
//      CrossEntropyLoss of S (the reference's double softmax) times w[y] into the wave's fp64 sums;
//      counts[pred, y] into the workgroup's LDS table
//   4  the 16 waves' fp64 sums added in wave order into loss_parts[block]; the LDS counts added to the
//      member's with integer atomics
// k_mnl_score_reduce then adds a member's loss_parts in block order (thread per member), and
// k_mnl_score_zero, ahead of both, zeroes the members' counts.  Every floating-point sum has one fixed
// order that depends on the member alone: a member's bits do not depend on the rest of the table.
#include "tr_mnl_score.h"

#include "tr_common.h"

namespace tr {

__global__ __launch_bounds__(SCORE_T) void k_mnl_score_many(const ScoreMember* __restrict__ members, int n_members,
                                                            int total_blocks) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.x;
  if (b >= total_blocks) return;
  const ScoreMember& mb = members[score_member_of_block(members, n_members, total_blocks, b)];  // (wave-uniform)
  const ScoreGeom& g = mb.g;
  const int t = threadIdx.x, lane = t & (TR_WAVE - 1), q = t / TR_WAVE;
  constexpr int T = SCORE_T, NW = SCORE_T / TR_WAVE;
  const int I1 = g.I1, P = g.P, C = g.C, R = g.R, np = g.np, PC = g.P * g.C;
  double* dred = reinterpret_cast<double*>(lds + g.oRed);
  int* sCnt = reinterpret_cast<int*>(lds + g.oCnt);
  float* sW = lds + g.oW;
  float* sPhi = lds + g.oPhi;
  float* sB = lds + g.oB;
  const int64_t* __restrict__ target = mb.target;
  const float* __restrict__ cw = mb.cw;
  const bool scored = target != nullptr && (mb.counts != nullptr || mb.loss != nullptr);

  // ---- 1: phi ----
  for (int e = t; e < np; e += T) {
    const int f = e < g.off1 ? 0 : (e < g.off2 ? 1 : 2);
    const float p = mb.params[e];
    sPhi[e] = mb.nonneg[f] != 0 ? tr_softplus(p, mb.beta, mb.thr) : p;
  }
  if (t < R) sW[t] = mb.w[t];
  if (t < C * C) sCnt[t] = 0;
  __syncthreads();
  // ---- 2: dense B[c][p] ----
  {
    const float* phi0 = sPhi;
    const float* phi1 = sPhi + g.off1;
    const float* phi2 = sPhi + g.off2;
    for (int e = t; e < PC; e += T) {
      const int c = e / P, p = e - c * P;
      const int i0 = p / I1, i1 = p - i0 * I1;
      float acc = 0.f;
      for (int r = 0; r < R; ++r) acc = fmaf(phi0[i0 * R + r] * sW[r], phi1[i1 * R + r] * phi2[c * R + r], acc);
      sB[e] = acc;
    }
  }
  __syncthreads();
  // ---- 3: the rows of this block, a wave per row ----
  const int64_t row0 = (int64_t)(b - mb.first_block) * SCORE_ROWS;
  const int nrows = (int)(mb.n_rows - row0 < SCORE_ROWS ? mb.n_rows - row0 : SCORE_ROWS);
  double lsum = 0.0, wsum = 0.0;
  for (int i = q; i < nrows; i += NW) {
    const int64_t n = row0 + i;
    const float* __restrict__ row = mb.X + n * mb.xld;
    float z[SCORE_MAX_C];
#pragma unroll
    for (int c = 0; c < SCORE_MAX_C; ++c) z[c] = 0.f;
    for (int p0 = 0; p0 < P; p0 += 4 * TR_WAVE) {  // four loads in flight per lane, then their fmas, p ascending
      float x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = p0 + u * TR_WAVE + lane;
        x[u] = p < P ? row[p] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = p0 + u * TR_WAVE + lane;
        if (p < P) {
#pragma unroll
          for (int c = 0; c < SCORE_MAX_C; ++c)
            if (c < C) z[c] = fmaf(x[u], sB[c * P + p], z[c]);
        }
      }
    }
    const float NEG = -__builtin_huge_valf();
    float mx = NEG;
#pragma unroll
    for (int c = 0; c < SCORE_MAX_C; ++c) {
      z[c] = c < C ? wv_allreduce(z[c]) : NEG;  // (C is uniform: every lane takes part in the butterfly)
      mx = fmaxf(mx, z[c]);
    }
    // from here every lane holds the same values
    float s[SCORE_MAX_C];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < SCORE_MAX_C; ++c)
      if (c < C) {
        s[c] = expf(z[c] - mx);
        sum += s[c];
      }
    const float inv = 1.0f / sum;
    float m2 = NEG, mine = 0.f;
    int best = 0;
#pragma unroll
    for (int c = 0; c < SCORE_MAX_C; ++c)
      if (c < C) {
        s[c] = s[c] * inv;  // S = softmax(Z)
        if (s[c] > m2) {    // strictly greater: the first index of the maximum
          m2 = s[c];
          best = c;
        }
        if (lane == c) mine = s[c];
      }
    if (mb.prob != nullptr && lane < C) mb.prob[n * C + lane] = mine;
    if (mb.pred != nullptr && lane == 0) mb.pred[n] = (int64_t)best;
    if (scored) {
      const int64_t yl = target[n];
      if (yl >= 0 && yl < C) {
        float s2 = 0.f, sy = 0.f;
#pragma unroll
        for (int c = 0; c < SCORE_MAX_C; ++c)
          if (c < C) {
            s2 += expf(s[c] - m2);
            if (c == (int)yl) sy = s[c];
          }
        const float l = -((sy - m2) - logf(s2));
        const double wy = cw != nullptr ? (double)cw[yl] : 1.0;
        lsum += wy * (double)l;
        wsum += wy;
        if (lane == 0) atomicAdd(&sCnt[best * C + (int)yl], 1);
      }
    }
  }
  // ---- 4: this block's partial sums, the waves in order; its counts ----
  if (lane == 0) {
    dred[2 * q] = lsum;
    dred[2 * q + 1] = wsum;
  }
  __syncthreads();
  if (t == 0 && mb.loss != nullptr && target != nullptr) {
    double a = 0.0, w = 0.0;
    for (int k = 0; k < NW; ++k) {
      a += dred[2 * k];
      w += dred[2 * k + 1];
    }
    double* part = mb.loss_parts + 2 * (int64_t)(b - mb.first_block);
    part[0] = a;
    part[1] = w;
  }
  if (mb.counts != nullptr && target != nullptr && t < C * C) {
    const int v = sCnt[t];
    if (v != 0) atomicAdd(&mb.counts[t], v);
  }
}

// counts of every member to zero, ahead of k_mnl_score_many on the same stream (workgroup per member)
__global__ __launch_bounds__(SCORE_MAX_C * SCORE_MAX_C) void k_mnl_score_zero(const ScoreMember* __restrict__ members,
                                                                               int n_members) {
  const int j = blockIdx.x;
  if (j >= n_members) return;
  const ScoreMember& mb = members[j];
  const int t = threadIdx.x;
  if (mb.counts != nullptr && t < mb.g.C * mb.g.C) mb.counts[t] = 0;
}

// loss[0..1] of a member: its blocks' partial sums in block order (thread per member)
__global__ __launch_bounds__(256) void k_mnl_score_reduce(const ScoreMember* __restrict__ members, int n_members) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_members) return;
  const ScoreMember& mb = members[j];
  if (mb.loss == nullptr || mb.target == nullptr) return;
  double a = 0.0, w = 0.0;
  for (int k = 0; k < mb.n_blocks; ++k) {
    a += mb.loss_parts[2 * (int64_t)k];
    w += mb.loss_parts[2 * (int64_t)k + 1];
  }
  mb.loss[0] = a;
  mb.loss[1] = w;
}

hipError_t prepare_score() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mnl_score_many),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)SCORE_LDS_BYTES);
}

hipError_t launch_score_many(const ScoreMember* members, int n_members, int64_t total_blocks, int64_t lds_bytes,
                             bool any_counts, bool any_loss, hipStream_t st) {
  if (members == nullptr || n_members < 1 || total_blocks < n_members || total_blocks > SCORE_MAX_BLOCKS || lds_bytes < 1 ||
      lds_bytes > SCORE_LDS_BYTES)
    return hipErrorInvalidValue;
  if (any_counts) {
    hipLaunchKernelGGL(k_mnl_score_zero, dim3(n_members), dim3(SCORE_MAX_C * SCORE_MAX_C), 0, st, members, n_members);
    if (hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(k_mnl_score_many, dim3((unsigned)total_blocks), dim3(SCORE_T), (size_t)lds_bytes, st, members,
                     n_members, (int)total_blocks);
  if (hipError_t e = hipGetLastError()) return e;
  if (any_loss) {
    hipLaunchKernelGGL(k_mnl_score_reduce, dim3((n_members + 255) / 256), dim3(256), 0, st, members, n_members);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

}  // namespace tr
