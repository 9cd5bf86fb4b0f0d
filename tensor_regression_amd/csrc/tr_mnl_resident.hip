// tr_mnl_resident.hip — the resident multinomial fit: whole fit_Adam iterations of the hierarchical
// multinomial module (multinomial_tensor_regression_hierarchical.py:449-464) in one launch.
//
// The module's real workload is small (kim_MultinomialTensorRegression.ipynb: X 227 x 8 x 12, 4
// classes, rank 6: 87 KB of X, 144 parameters) and long (12000 iterations).  The streamed route
// spends an iteration in six to eight launches around almost no work.  Here ONE 1024-thread workgroup
// keeps X, the dense B and G, Z / dZ, the factors and the Adam state in its CU's LDS and runs up to
// RES_MAX_ITERS complete iterations; parameters and state go back to global memory at the end.
//
// One iteration, every phase ending in a workgroup barrier:
//   1  phi = softplus(A) or A, dphi                                   (thread per parameter)
//   2  B[p, c] = sum_r (phi0[i0, r] w_r) (phi1[i1, r] phi2[c, r])     (thread per (p, c); cp_to_tensor's
//                                                                      association, r ascending)
//   3  Z[n, c] = sum_p X[n, p] B[p, c]                                (thread per (c, n), lanes over n)
//   4  S = softmax(Z); CrossEntropyLoss(S, y) (the reference's double softmax, unweighted mean);
//      dZ = S (dS - <dS, S>) over Z; the loss as fp64 per-wave partials  (thread per sample)
//   5  G[c, p] = sum_n X[n, p] dZ[n, c]                               (thread per (split, c, p), lanes over
//                                                                      p; the S splits added in order)
//   6  the three factor gradients from G with the softplus chain (thread per parameter);
//      ||A_f|| of the raw factors (one wave per factor)
//   7  L2 term + torch's _single_tensor_adam, one step size per factor (k_update<true>'s arithmetic, tr_adam.h)
//   8  thread 0: loss_hist[hist_base + iter] = data + lambda sum ||A_f||, then the plateau test by
//      np_pairwise_sum_absdiff (k_converge's) into one LDS word
// and after that barrier every thread reads the word, so all leave the loop together.
//
// All sums are fp32 fmaf chains in one fixed order (the loss in fp64), no atomics: two runs, and a
// fit cut into launches of any lengths, give the same bits.  lr is constant within a launch (the
// host cuts the chunk at a group_lr breakpoint).
//
// Two entry points run that one body (resident_fit): k_mnl_resident, one workgroup whose arguments are
// the kernel's own, and k_mnl_resident_many, a grid in which workgroup j fits member j of a table in
// global memory (a hyperparameter sweep: independent models, each with its own shape, data and
// optimizer settings).  The workgroups share nothing, so member j's bits are the single launch's.
//
// LDS image (ResGeom): X at an odd row pitch, so the Z pass (lanes over samples, stride XP) and the G
// pass (lanes over features, stride 1) both touch 32 distinct banks per half wave; Z at an odd pitch
// for the same reason; B and dZ are read at wave-uniform addresses (broadcast).
#include "tr_mnl_resident.h"

#include "tr_adam.h"
#include "tr_common.h"
#include "tr_np_sum.h"

namespace tr {

// The fit of one problem by the calling workgroup: load, phases 1-8 per iteration, write-back.  `a` is
// read through a wave-uniform address (the kernel arguments, or this workgroup's row of the member
// table in global memory), so its fields arrive by scalar loads; it is not copied into the LDS image.
static __device__ __forceinline__ void resident_fit(const ResArgs& a, const float* __restrict__ X, int64_t xld,
                                                    const int64_t* __restrict__ target, float* __restrict__ params,
                                                    const float* __restrict__ w, float* __restrict__ m,
                                                    float* __restrict__ v, float* __restrict__ vmax,
                                                    double* __restrict__ loss_hist, int32_t* __restrict__ stop) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const ResGeom& g = a.g;
  const int t = threadIdx.x, lane = t & (TR_WAVE - 1), q = t / TR_WAVE;
  constexpr int T = RES_T;
  const int N = g.N, I1 = g.I1, P = g.P, C = g.C, R = g.R, XP = g.XP, CP = g.CP, np = g.np, PC = g.P * g.C;
  double* dred = reinterpret_cast<double*>(lds);          // [16] per-wave loss partials
  int* ctrl = reinterpret_cast<int*>(lds + 32);           // [0] the stop word
  float* sX = lds + g.oX;
  float* sB = lds + g.oB;
  float* sG = lds + g.oG;
  float* sGp = lds + g.oGp;
  float* sZ = lds + g.oZ;
  int* sY = reinterpret_cast<int*>(lds + g.oY);
  float* sW = lds + g.oW;
  float* sPar = lds + g.oPar;
  float* sM = lds + g.oM;
  float* sV = lds + g.oV;
  float* sVm = lds + g.oVm;
  float* sPhi = lds + g.oPhi;
  float* sDphi = lds + g.oDphi;
  float* sGrad = lds + g.oGrad;
  float* sNorm = lds + g.oNorm;      // [0..2] ||A_f||, [4..6] lambda / (2 ||A_f||)
  const bool ams = a.amsgrad != 0;

  if (*stop != 0) return;  // (uniform: every thread reads the same word)
  // ---- load the problem ----
  for (int n = q; n < N; n += T / TR_WAVE) {  // one wave per row: coalesced reads, conflict-free writes
    const float* __restrict__ row = X + (int64_t)n * xld;
    for (int p = lane; p < P; p += TR_WAVE) sX[n * XP + p] = row[p];
  }
  for (int n = t; n < N; n += T) sY[n] = (int)target[n];
  for (int e = t; e < np; e += T) {
    sPar[e] = params[e];
    sM[e] = m[e];
    sV[e] = v[e];
    sVm[e] = ams ? vmax[e] : 0.f;
  }
  if (t < R) sW[t] = w[t];
  if (t == 0) ctrl[0] = 0;
  __syncthreads();

  const float* phi0 = sPhi;
  const float* phi1 = sPhi + g.off1;
  const float* phi2 = sPhi + g.off2;
  int done = 0;  // iterations completed by this launch
  for (int it = 0; it < a.n_iters; ++it) {
    // ---- 1: phi, dphi ----
    for (int e = t; e < np; e += T) {
      const int f = e < g.off1 ? 0 : (e < g.off2 ? 1 : 2);
      const float p = sPar[e];
      const bool soft = a.nonneg[f] != 0;
      sPhi[e] = soft ? tr_softplus(p, a.beta, a.thr) : p;
      sDphi[e] = soft ? tr_softplus_grad(p, a.beta, a.thr) : 1.0f;
    }
    __syncthreads();
    // ---- 2: dense B[p][c] ----
    for (int e = t; e < PC; e += T) {
      const int p = e / C, c = e - p * C;
      const int i0 = p / I1, i1 = p - i0 * I1;
      float acc = 0.f;
      for (int r = 0; r < R; ++r)
        acc = fmaf(phi0[i0 * R + r] * sW[r], phi1[i1 * R + r] * phi2[c * R + r], acc);
      sB[e] = acc;
    }
    __syncthreads();
    // ---- 3: Z = X . B ----
    for (int e = t; e < N * C; e += T) {
      const int c = e / N, n = e - c * N;
      const float* xr = sX + n * XP;
      float acc = 0.f;
      for (int p = 0; p < P; ++p) acc = fmaf(xr[p], sB[p * C + c], acc);
      sZ[n * CP + c] = acc;
    }
    __syncthreads();
    // ---- 4: double softmax, CE, dZ over Z ----
    double lsum = 0.0;
    for (int n = t; n < N; n += T) {
      float* z = sZ + n * CP;
      float s[RES_MAX_C];
      const float NEG = -__builtin_huge_valf();
      float mx = NEG;
#pragma unroll
      for (int c = 0; c < RES_MAX_C; ++c) {
        s[c] = c < C ? z[c] : NEG;
        mx = fmaxf(mx, s[c]);
      }
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < RES_MAX_C; ++c)
        if (c < C) {
          s[c] = expf(s[c] - mx);
          sum += s[c];
        }
      const float inv = 1.0f / sum;
      float m2 = NEG;
#pragma unroll
      for (int c = 0; c < RES_MAX_C; ++c)
        if (c < C) {
          s[c] = s[c] * inv;  // S = softmax(Z)
          m2 = fmaxf(m2, s[c]);
        }
      float s2 = 0.f;
#pragma unroll
      for (int c = 0; c < RES_MAX_C; ++c)
        if (c < C) s2 += expf(s[c] - m2);
      const float lse = logf(s2), inv2 = 1.0f / s2;
      const int yl = sY[n];
      float dS[RES_MAX_C];
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < RES_MAX_C; ++c)
        if (c < C) {
          dS[c] = (expf(s[c] - m2) * inv2 - (c == yl ? 1.0f : 0.0f)) * a.inv_n;
          dot = fmaf(dS[c], s[c], dot);
          if (c == yl) lsum += (double)(-((s[c] - m2) - lse));
        }
#pragma unroll
      for (int c = 0; c < RES_MAX_C; ++c)
        if (c < C) z[c] = s[c] * (dS[c] - dot);
    }
    lsum = wv_allreduce_d(lsum);
    if (lane == 0) dred[q] = lsum;
    __syncthreads();
    // ---- 5: G[c][p] = sum_n X[n][p] dZ[n][c], the samples in S contiguous splits ----
    {
      const int chunk = (N + g.S - 1) / g.S;
      for (int j = t; j < PC * g.S; j += T) {
        const int s = j / PC, e = j - s * PC;
        const int c = e / P, p = e - c * P;
        const int n0 = s * chunk, n1 = n0 + chunk < N ? n0 + chunk : N;
        float acc = 0.f;
        for (int n = n0; n < n1; ++n) acc = fmaf(sX[n * XP + p], sZ[n * CP + c], acc);
        if (g.S > 1)
          sGp[j] = acc;
        else
          sG[e] = acc;
      }
      if (g.S > 1) {
        __syncthreads();
        for (int e = t; e < PC; e += T) {
          float acc = sGp[e];
          for (int s = 1; s < g.S; ++s) acc += sGp[s * PC + e];
          sG[e] = acc;
        }
      }
    }
    __syncthreads();
    // ---- 6: factor gradients from G (softplus chain), norms of the raw factors ----
    for (int e = t; e < np; e += T) {
      float acc = 0.f;
      int r;
      if (e < g.off1) {
        const int i0 = e / R;
        r = e - i0 * R;
        for (int i1 = 0; i1 < I1; ++i1)
          for (int c = 0; c < C; ++c)
            acc = fmaf(sG[c * P + i0 * I1 + i1], phi1[i1 * R + r] * phi2[c * R + r], acc);
      } else if (e < g.off2) {
        const int x = e - g.off1, i1 = x / R;
        r = x - i1 * R;
        for (int i0 = 0; i0 < g.I0; ++i0)
          for (int c = 0; c < C; ++c)
            acc = fmaf(sG[c * P + i0 * I1 + i1], phi0[i0 * R + r] * phi2[c * R + r], acc);
      } else {
        const int x = e - g.off2, c = x / R;
        r = x - c * R;
        for (int i0 = 0; i0 < g.I0; ++i0)
          for (int i1 = 0; i1 < I1; ++i1)
            acc = fmaf(sG[c * P + i0 * I1 + i1], phi0[i0 * R + r] * phi1[i1 * R + r], acc);
      }
      sGrad[e] = acc * sW[r] * sDphi[e];
    }
    if (q < 3) {  // wave f: ||A_f||, its elements lane-strided in increasing order, then the butterfly
      const int b = q == 0 ? 0 : (q == 1 ? g.off1 : g.off2);
      const int e1 = q == 0 ? g.off1 : (q == 1 ? g.off2 : np);
      float acc = 0.f;
      for (int e = b + lane; e < e1; e += TR_WAVE) acc = fmaf(sPar[e], sPar[e], acc);
      acc = wv_allreduce(acc);
      if (lane == 0) {
        const float nrm = sqrtf(acc);
        sNorm[q] = nrm;
        sNorm[4 + q] = a.lambda_l2 / (2.0f * nrm);  // d/dA lambda ||A|| = (lambda / (2 ||A||)) * (2 A)
      }
    }
    __syncthreads();
    // ---- 7: L2 term + Adam / AMSGrad, one step size per factor ----
    for (int e = t; e < np; e += T) {
      const int f = e < g.off1 ? 0 : (e < g.off2 ? 1 : 2);
      float p = sPar[e];
      float gr = sGrad[e] + sNorm[4 + f] * (2.0f * p);
      float mm = sM[e], vv = sV[e];
      adam_moments(p, gr, mm, vv, a.weight_decay, a.one_minus_b1, a.beta2, a.one_minus_b2);
      float vm = 0.f;
      if (ams) {
        vm = fmaxf(sVm[e], vv);
        sVm[e] = vm;
      }
      p = adam_param(p, mm, ams ? vm : vv, a.bc2_sqrt[it], a.eps, a.step_size[f][it]);
      sM[e] = mm;
      sV[e] = vv;
      sPar[e] = p;
    }
    // ---- 8: the loss record and the plateau test ----
    if (t == 0) {
      double ds = 0.0;
      for (int k = 0; k < T / TR_WAVE; ++k) ds += dred[k];
      const float data = (float)(ds * (double)a.inv_n);
      float l2 = 0.f;
      for (int f = 0; f < 3; ++f) l2 = l2 + sNorm[f];
      const float total = data + a.lambda_l2 * l2;
      const int64_t iter = a.iter0 + it;
      loss_hist[a.hist_base + iter] = (double)total;
      if (a.tol > 0.0 && iter > a.patience) {  // loss_running[ii - patience:], hierarchical…py:461-464
        const int64_t s0 = iter - a.patience;
        const double d = np_pairwise_sum_absdiff(loss_hist + s0, a.hist_base + iter - s0);
        if (d < a.tol) ctrl[0] = (int)(iter + 1);
      }
    }
    __syncthreads();
    done = it + 1;
    if (ctrl[0] != 0) break;  // one LDS word read by every thread after the barrier
  }
  (void)done;
  // ---- parameters and Adam state back to global memory ----
  for (int e = t; e < np; e += T) {
    params[e] = sPar[e];
    m[e] = sM[e];
    v[e] = sV[e];
    if (ams) vmax[e] = sVm[e];
  }
  if (t == 0 && ctrl[0] != 0) *stop = ctrl[0];
}

__global__ __launch_bounds__(RES_T) void k_mnl_resident(ResArgs a, const float* __restrict__ X, int64_t xld,
                                                        const int64_t* __restrict__ target,
                                                        float* __restrict__ params, const float* __restrict__ w,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        float* __restrict__ vmax, double* __restrict__ loss_hist,
                                                        int32_t* __restrict__ stop) {
  resident_fit(a, X, xld, target, params, w, m, v, vmax, loss_hist, stop);
}

// Workgroup j fits member j of the table; the workgroups share nothing (no atomics, no waiting on one
// another), so the grid may exceed the CUs and run in waves.  A member with n_iters == 0 (finished, or
// fewer iterations than the others) and one whose stop word is set leave before any barrier; both
// tests are uniform over the workgroup.  The launch's dynamic LDS is the largest member's carve.
__global__ __launch_bounds__(RES_T) void k_mnl_resident_many(const ResMember* __restrict__ members, int n_members) {
  const int j = blockIdx.x;
  if (j >= n_members) return;
  const ResMember& mb = members[j];
  if (mb.a.n_iters <= 0) return;
  resident_fit(mb.a, mb.X, mb.xld, mb.target, mb.params, mb.w, mb.m, mb.v, mb.vmax, mb.loss_hist, mb.stop);
}

hipError_t prepare_resident() {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mnl_resident),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)RES_LDS_BYTES);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mnl_resident_many),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)RES_LDS_BYTES);
}

hipError_t launch_resident(const ResArgs& a, const float* X, int64_t xld, const int64_t* target, float* params,
                           const float* w, float* m, float* v, float* vmax, double* loss_hist, int32_t* stop,
                           hipStream_t st) {
  if (a.n_iters < 1 || a.n_iters > RES_MAX_ITERS || (int64_t)a.g.words * 4 > RES_LDS_BYTES || stop == nullptr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mnl_resident, dim3(1), dim3(RES_T), (size_t)a.g.words * 4, st, a, X, xld, target, params, w, m,
                     v, vmax, loss_hist, stop);
  return hipGetLastError();
}

hipError_t launch_resident_many(const ResMember* members, int n_members, int64_t lds_bytes, hipStream_t st) {
  if (members == nullptr || n_members < 1 || lds_bytes < 1 || lds_bytes > RES_LDS_BYTES) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mnl_resident_many, dim3(n_members), dim3(RES_T), (size_t)lds_bytes, st, members, n_members);
  return hipGetLastError();
}

hipError_t touch_code_object_mnl_resident() {
  hipFuncAttributes at;
  return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_mnl_resident));
}

}  // namespace tr
