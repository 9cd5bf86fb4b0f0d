// tr_conv_spectrum.hip — the output-spectrum penalty of the convolutional Fourier model
// (convolutional_fourier_tensor_regression.py: spectral_penalty 727-812, set up at 1040-1048 and
// 1260-1261; loss 1269-1282).  The model's update step is k_update_conv (tr_conv.hip), which adds
// this penalty's value (SpecBufs::val) into the total.
//
//   C[k,n] = sum_{t<rows} x[t,n] cos(2 pi k t / n_fft),  S[k,n] = sum_t x[t,n] sin(2 pi k t / n_fft)
//            (Y = rfft(x, n_fft) = C - i S; the series is zero-padded from rows to n_fft)     k < F
//   A      = |Y|
//   M[j,n] = sum_{s<S} A[j+s,n] g[s]                                                         j < Fs
//   pen    = lambda_sp mean_{j,n} ((M - M_y) / (M_y + 1e-8))^2
// and back:
//   dM[j,n] = 2 lambda_sp / (Fs N) (M - M_y) / (M_y + 1e-8)^2
//   dA[k,n] = sum_s dM[k-s,n] g[s]                       (0 <= k - s < Fs)
//   d pen / d x[t,n] = sum_{k<F} (dA / A)[k,n] (C[k,n] cos(2 pi k t / n_fft) + S[k,n] sin(2 pi k t / n_fft))
//            (torch's abs backward: 0 where A = 0; the F bins only, no factor 2 for the mirrored half)
//
//   k_dft<ADJ>   out[a,n] = sum_b in[b,n] {cos, sin}(2 pi a b / n_fft): one thread owns one output
//                index a and NC = 4 columns; the summation index b runs over tiles of 256 rows staged
//                in LDS (every lane reads the same row: broadcast).  The angle index (a b) mod n_fft
//                is exact: a 64-bit product once per (thread, split), then add-and-wrap by
//                (a RUN) mod n_fft per run of RUN = 8 terms.  Each run is seeded from the table
//                tw[i] = (cos, sin)(2 pi i / n_fft) (fp64 on the host, rounded once) and bridged by
//                the rotation by tw[a]: at most 7 rotations from an exact seed.  fp32 fmaf inside a
//                tile, the tiles' sums accumulated in fp64.  The b range is split over blockIdx.z
//                when a and n alone give too few workgroups; the splits' fp64 partials are added in
//                index order by k_dft_combine.  ADJ = 0: real in, C and S out; ADJ = 1: two ins, one out.
//   k_spec_smooth / k_spec_pen / k_spec_val / k_spec_back   the terms between the two DFT passes, one
//                thread per element, every sum in ascending index order; the mean's partials are fp64
//                (one per workgroup, added in index order), the value is fp32(mean) * lambda_sp.
// No float atomics; two runs on the same inputs are bitwise equal.  Every kernel returns at once when
// the device stop flag is set.
// Bounds: a thread with a >= A computes index 0 and stores nothing; tile rows >= the split's end are
// zero; every table index is < n_fft (a < A <= n_fft, wrapped sums < 2 n_fft <= 2^23).
#include <cmath>
#include <cstring>

#include "tr_conv_spectrum.h"
#include "tr_workspace.h"

namespace tr {

namespace {
constexpr int DFT_T = 256;   // threads of a workgroup = output indices
constexpr int DFT_BT = 256;  // summation indices per LDS tile
constexpr int DFT_NC = 4;    // columns per workgroup
constexpr int DFT_RUN = 8;   // terms per exact re-seed of the twiddle
constexpr int PEN_EPB = 1024;  // elements per workgroup of k_spec_pen
}  // namespace

template <int ADJ>
__global__ __launch_bounds__(DFT_T) void k_dft(int64_t A, int64_t B, int N, uint32_t nfft, int64_t bper,
                                               const float2* __restrict__ tw, const float* __restrict__ in0,
                                               const float* __restrict__ in1, double* __restrict__ part,
                                               const int32_t* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  __shared__ float4 s0[DFT_BT];
  __shared__ float4 s1[ADJ ? DFT_BT : 1];
  const int tid = threadIdx.x;
  const int64_t a = (int64_t)blockIdx.x * DFT_T + tid;
  const int n0 = blockIdx.y * DFT_NC;
  const int64_t b_begin = (int64_t)blockIdx.z * bper;
  const int64_t b_end = b_begin + bper < B ? b_begin + bper : B;
  const uint64_t ac = a < A ? (uint64_t)a : 0;
  const uint32_t step = (uint32_t)((ac * DFT_RUN) % nfft);
  uint32_t idx = (uint32_t)((ac * (uint64_t)b_begin) % nfft);
  const float2 w = tw[ac];
  double acc0[DFT_NC], acc1[DFT_NC];
#pragma unroll
  for (int i = 0; i < DFT_NC; ++i) acc0[i] = acc1[i] = 0.0;
  for (int64_t b0 = b_begin; b0 < b_end; b0 += DFT_BT) {
    __syncthreads();  // the tile's previous readers are done
    {
      const int64_t b = b0 + tid;
      float v0[DFT_NC], v1[DFT_NC];
#pragma unroll
      for (int i = 0; i < DFT_NC; ++i) {
        const bool ok = b < b_end && n0 + i < N;
        v0[i] = ok ? in0[b * N + n0 + i] : 0.f;
        v1[i] = ADJ && ok ? in1[b * N + n0 + i] : 0.f;
      }
      s0[tid] = make_float4(v0[0], v0[1], v0[2], v0[3]);
      if (ADJ) s1[tid] = make_float4(v1[0], v1[1], v1[2], v1[3]);
    }
    __syncthreads();
    float f0[DFT_NC], f1[DFT_NC];
#pragma unroll
    for (int i = 0; i < DFT_NC; ++i) f0[i] = f1[i] = 0.f;
    for (int j = 0; j < DFT_BT; j += DFT_RUN) {
      float2 cs = tw[idx];
      idx += step;
      if (idx >= nfft) idx -= nfft;
#pragma unroll
      for (int r = 0; r < DFT_RUN; ++r) {
        const float4 x4 = s0[j + r];
        const float x[DFT_NC] = {x4.x, x4.y, x4.z, x4.w};
        if (ADJ) {
          const float4 y4 = s1[j + r];
          const float y[DFT_NC] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
          for (int i = 0; i < DFT_NC; ++i) f0[i] = fmaf(y[i], cs.y, fmaf(x[i], cs.x, f0[i]));
        } else {
#pragma unroll
          for (int i = 0; i < DFT_NC; ++i) {
            f0[i] = fmaf(x[i], cs.x, f0[i]);
            f1[i] = fmaf(x[i], cs.y, f1[i]);
          }
        }
        if (r + 1 < DFT_RUN) {  // angle + 2 pi a / n_fft
          const float c = fmaf(cs.x, w.x, -(cs.y * w.y));
          const float s = fmaf(cs.y, w.x, cs.x * w.y);
          cs = make_float2(c, s);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < DFT_NC; ++i) {
      acc0[i] += (double)f0[i];
      acc1[i] += (double)f1[i];
    }
  }
  if (a >= A) return;
  const int nout = ADJ ? 1 : 2;
  double* p0 = part + (((int64_t)blockIdx.z * nout) * A + a) * N;
#pragma unroll
  for (int i = 0; i < DFT_NC; ++i) {
    if (n0 + i < N) {
      p0[n0 + i] = acc0[i];
      if (!ADJ) p0[A * N + n0 + i] = acc1[i];
    }
  }
}

// out[e] = sum over the splits, in index order; MAG: also |out0 + i out1| from the fp64 sums
template <int MAG>
__global__ __launch_bounds__(256) void k_dft_combine(int nsplit, int64_t AN, const double* __restrict__ part,
                                                     float* __restrict__ out0, float* __restrict__ out1,
                                                     float* __restrict__ mag, const int32_t* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= AN) return;
  const int nout = MAG ? 2 : 1;
  double s0 = 0.0, s1 = 0.0;
  for (int z = 0; z < nsplit; ++z) {
    s0 += part[((int64_t)z * nout) * AN + e];
    if (MAG) s1 += part[((int64_t)z * nout + 1) * AN + e];
  }
  out0[e] = (float)s0;
  if (MAG) {
    out1[e] = (float)s1;
    mag[e] = (float)sqrt(s0 * s0 + s1 * s1);
  }
}

// M[j,n] = sum_s A[j+s,n] g[s]   (conv1d: no flip)
__global__ __launch_bounds__(256) void k_spec_smooth(int64_t FsN, int N, int S, const float* __restrict__ A,
                                                     const float* __restrict__ g, float* __restrict__ M,
                                                     const int32_t* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= FsN) return;
  const float* a = A + e;  // A[(j + s) N + n] = A[e + s N]
  float m = 0.f;
  for (int s = 0; s < S; ++s) m = fmaf(a[(int64_t)s * N], g[s], m);
  M[e] = m;
}

// dM and the workgroup's partial sum of ((M - My) / (My + 1e-8))^2
__global__ __launch_bounds__(256) void k_spec_pen(int64_t FsN, float coef, const float* __restrict__ M,
                                                  const float* __restrict__ My, float* __restrict__ dM,
                                                  double* __restrict__ ppart, const int32_t* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  __shared__ double wl[4];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = 0; i < PEN_EPB / 256; ++i) {
    const int64_t e = (int64_t)blockIdx.x * PEN_EPB + i * 256 + tid;
    if (e < FsN) {
      const float den = My[e] + 1e-8f;
      const float r = (M[e] - My[e]) / den;
      acc += (double)r * (double)r;
      dM[e] = coef * (r / den);
    }
  }
  const double s = wv_allreduce_d(acc);
  if ((tid & 63) == 0) wl[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) ppart[blockIdx.x] = (wl[0] + wl[1]) + (wl[2] + wl[3]);
}

// val = fp32(mean) * lambda_sp   (torch.mean(...) * lam)
__global__ __launch_bounds__(64) void k_spec_val(int nb, double count, float lam, const double* __restrict__ ppart,
                                                 float* __restrict__ val, const int32_t* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += ppart[b];
  *val = (float)(s / count) * lam;
}

// dA[k,n] = sum_s dM[k-s,n] g[s]; (re, im) *= dA / A  (0 where A = 0)
__global__ __launch_bounds__(256) void k_spec_back(int64_t F, int64_t Fs, int N, int S, const float* __restrict__ dM,
                                                   const float* __restrict__ g, const float* __restrict__ A,
                                                   float* __restrict__ re, float* __restrict__ im,
                                                   const int32_t* __restrict__ stop) {
  if (stop != nullptr && *stop != 0) return;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= F * N) return;
  const int64_t k = e / N;
  const int64_t slo = k - Fs + 1 > 0 ? k - Fs + 1 : 0;
  const int64_t shi = k < S - 1 ? k : S - 1;
  float d = 0.f;
  for (int64_t s = slo; s <= shi; ++s) d = fmaf(dM[e - s * N], g[s], d);
  const float a = A[e];
  const float f = a > 0.f ? d / a : 0.f;
  re[e] *= f;
  im[e] *= f;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
namespace {
// splits of the summation range and rows per split (a multiple of the tile)
void dft_split(int64_t A, int64_t B, int N, int* nsplit, int64_t* bper) {
  const int64_t wg = ((A + DFT_T - 1) / DFT_T) * ((N + DFT_NC - 1) / DFT_NC);
  const int64_t tiles = (B + DFT_BT - 1) / DFT_BT;
  int64_t s = (1024 + wg - 1) / wg;
  if (s > SPEC_MAXSPLIT) s = SPEC_MAXSPLIT;
  if (s > tiles) s = tiles;
  if (s < 1) s = 1;
  const int64_t tper = (tiles + s - 1) / s;
  *bper = tper * DFT_BT;
  *nsplit = (int)((tiles + tper - 1) / tper);
}

template <int ADJ>
hipError_t launch_dft(const SpecPen& sp, const SpecBufs& b, int64_t A, int64_t B, const float* in0, const float* in1,
                      float* out0, float* out1, float* mag, const int32_t* stop, hipStream_t st) {
  int nsplit;
  int64_t bper;
  dft_split(A, B, sp.N, &nsplit, &bper);
  const dim3 grid((unsigned)((A + DFT_T - 1) / DFT_T), (unsigned)((sp.N + DFT_NC - 1) / DFT_NC), (unsigned)nsplit);
  hipLaunchKernelGGL(k_dft<ADJ>, grid, dim3(DFT_T), 0, st, A, B, sp.N, (uint32_t)sp.nfft, bper, b.tw, in0, in1, b.part,
                     stop);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t AN = A * sp.N;
  hipLaunchKernelGGL(k_dft_combine<ADJ ? 0 : 1>, dim3((unsigned)((AN + 255) / 256)), dim3(256), 0, st, nsplit, AN,
                     b.part, out0, out1, mag, stop);
  return hipGetLastError();
}
}  // namespace

size_t spec_carve(const SpecPen& sp, int64_t max_rows, char* base, SpecBufs* b) {
  const size_t FN = (size_t)sp.F * sp.N, FsN = (size_t)sp.Fs * sp.N, RN = (size_t)max_rows * sp.N;
  const size_t amax = FN > RN ? FN : RN;
  // splits * outputs <= 2^20 + A N (dft_split: splits <= 1024 / workgroups + 1, workgroups >= A N / 1024)
  SpecBufs sized;  // (size only: the slots of a call without a base)
  if (base == nullptr || b == nullptr) b = &sized;
  Carver c;
  c.add(&b->tw, (size_t)sp.nfft * 8);
  c.add(&b->g, (size_t)sp.S * 4);
  c.add(&b->re, FN * 4);
  c.add(&b->im, FN * 4);
  c.add(&b->A, FN * 4);
  c.add(&b->M, FsN * 4);
  c.add(&b->My, FsN * 4);
  c.add(&b->dM, FsN * 4);
  c.add(&b->part, 2 * (((size_t)1 << 20) + amax) * 8);
  c.add(&b->ppart, ((FsN + PEN_EPB - 1) / PEN_EPB) * 8);
  c.add(&b->val, 4);
  c.add(&b->yhat, RN * 4);
  c.add(&b->eadd, RN * 4);
  if (b != &sized) c.bind(base);
  return c.bytes();
}

void spec_build_twiddles(int64_t nfft, float2* tw) {
  const double pi = 3.14159265358979323846;
  for (int64_t i = 0; i < nfft; ++i) {
    const double th = 2.0 * pi * (double)i / (double)nfft;
    tw[i] = make_float2((float)std::cos(th), (float)std::sin(th));
  }
}

hipError_t launch_spectrum(const SpecPen& sp, const SpecBufs& b, const float* series, int64_t rows, float* M_out,
                           const int32_t* stop, hipStream_t st) {
  if (rows < 1 || rows > sp.nfft || sp.Fs < 1) return hipErrorInvalidValue;
  hipError_t e = launch_dft<0>(sp, b, sp.F, rows, series, nullptr, b.re, b.im, b.A, stop, st);
  if (e != hipSuccess) return e;
  const int64_t FsN = sp.Fs * sp.N;
  hipLaunchKernelGGL(k_spec_smooth, dim3((unsigned)((FsN + 255) / 256)), dim3(256), 0, st, FsN, sp.N, sp.S, b.A, b.g,
                     M_out, stop);
  return hipGetLastError();
}

hipError_t launch_spectrum_penalty(const SpecPen& sp, const SpecBufs& b, const float* series, int64_t rows,
                                   float* grad_out, const int32_t* stop, hipStream_t st) {
  hipError_t e = launch_spectrum(sp, b, series, rows, b.M, stop, st);
  if (e != hipSuccess) return e;
  const int64_t FsN = sp.Fs * sp.N, FN = sp.F * sp.N;
  const int nb = (int)((FsN + PEN_EPB - 1) / PEN_EPB);
  const float coef = (float)(2.0 * (double)sp.lam / (double)FsN);
  hipLaunchKernelGGL(k_spec_pen, dim3(nb), dim3(256), 0, st, FsN, coef, b.M, b.My, b.dM, b.ppart, stop);
  hipLaunchKernelGGL(k_spec_val, dim3(1), dim3(64), 0, st, nb, (double)FsN, sp.lam, b.ppart, b.val, stop);
  hipLaunchKernelGGL(k_spec_back, dim3((unsigned)((FN + 255) / 256)), dim3(256), 0, st, sp.F, sp.Fs, sp.N, sp.S, b.dM,
                     b.g, b.A, b.re, b.im, stop);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_dft<1>(sp, b, rows, sp.F, b.re, b.im, grad_out, nullptr, nullptr, stop, st);
}

}  // namespace tr
