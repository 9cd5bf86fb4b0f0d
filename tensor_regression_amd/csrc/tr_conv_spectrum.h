// tr_conv_spectrum.h — host-side interface of the output-spectrum penalty of the convolutional
// Fourier model (tr_conv_spectrum.hip).  The X pass is k_conv (tr_conv.h); these kernels
// compute |rfft(y_hat, n_fft)| of any length by a direct real DFT, smooth it, form the penalty and
// carry its gradient back into y_hat (k_conv's `eadd`).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tr_conv.h"

namespace tr {

constexpr int SPEC_MAXS = 4097;     // longest smoothing kernel (taps)
constexpr int SPEC_MAXSPLIT = 16;   // at most this many partial sums per DFT output
constexpr int64_t SPEC_MAXFFT = (int64_t)1 << 22;  // twiddle table entries at most

// Shapes of one spectrum path (fixed by tr_plan_set_spectrum_penalty).
struct SpecPen {
  int64_t nfft;   // transform length n (the series is zero-padded to it)
  int64_t F;      // n/2 + 1 bins
  int S;          // smoothing taps
  int64_t Fs;     // F - S + 1 rows of the smoothed spectrum
  int N;          // columns (n_out)
  float lam;      // lambda_sp
};

// Device buffers of the spectrum path, carved from one allocation.
struct SpecBufs {
  float2* tw;      // (nfft) (cos, sin)(2 pi i / nfft), computed in fp64 and rounded once
  float* g;        // (S) smoothing kernel
  float* re;       // (F, N)  sum_t x cos      (= Re Y); overwritten by dA * re / A
  float* im;       // (F, N)  sum_t x sin      (= -Im Y); overwritten by dA * im / A
  float* A;        // (F, N)  |Y|
  float* M;        // (Fs, N) smoothed |Y|
  float* My;       // (Fs, N) the target's, kept
  float* dM;       // (Fs, N)
  double* part;    // DFT partial sums: (split, 2, max(F, rows), N)
  double* ppart;   // penalty partial sums, one per workgroup of k_spec_pen
  float* val;      // the penalty value (lambda_sp * mean), plan-owned scalar
  float* yhat;     // (rows, N) y_hat of the forward pass
  float* eadd;     // (rows, N) d pen / d y_hat
};

// bytes of the allocation for series of at most max_rows rows; fills the pointers when base != nullptr
size_t spec_carve(const SpecPen& sp, int64_t max_rows, char* base, SpecBufs* b);
// tw[i] = (cos, sin)(2 pi i / nfft) in fp64, rounded once
void spec_build_twiddles(int64_t nfft, float2* tw_host);
// smoothed magnitude spectrum of series (rows, N) into M_out (Fs, N); leaves re / im / A of the series
hipError_t launch_spectrum(const SpecPen& sp, const SpecBufs& b, const float* series, int64_t rows, float* M_out,
                           const int32_t* stop, hipStream_t st);
// launch_spectrum into b.M, then the penalty value into b.val and d pen / d series into grad_out (rows, N)
hipError_t launch_spectrum_penalty(const SpecPen& sp, const SpecBufs& b, const float* series, int64_t rows,
                                   float* grad_out, const int32_t* stop, hipStream_t st);

}  // namespace tr
