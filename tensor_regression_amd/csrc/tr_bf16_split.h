// tr_bf16_split.h — an fp32 value as a sum of bf16 pieces, so that an fp32 GEMM runs as exact
// bf16 x bf16 products on v_mfma_f32_16x16x32_bf16 (wv_mfma_bf16, 16x the f32 MFMA rate).  Used by
// the column-slice spectral kernel (tr_spectral_slice.hip) and the split body of the
// two-workgroups-per-CU multinomial kernel (tr_mnl_duo.hip).
//
// x = x1 + x2 + x3 by round-to-nearest-even bf16 conversions (v_cvt_pk_bf16_f32, two values per
// instruction): x1 = bf16(x), r = x - x1 (exact: Sterbenz), x2 = bf16(r), x3 = r - x2 (exact, at
// most 8 significant bits: exactly a bf16), for every finite |x| below the bf16 overflow
// threshold (3.39e38) and above 2^-100.  |x2| <= 2^-8 |x|, |x3| <= 2^-17 |x|, and — unlike a
// truncating split, whose pieces all carry the sign of x — the pieces' signs are independent of
// x, so the terms a product drops are unbiased (a truncating split's are biased toward the sign of
// the product: over config 5's sums that bias reached 8-25x the f32 MFMA form's error).
// tests/test_split_numerics.py holds these bounds.
#pragma once

#include "tr_wave.h"

typedef __bf16 bfs_bf2 __attribute__((ext_vector_type(2)));

// two values -> one VGPR of packed RNE bf16 (element 0 = a in the low half), v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t bfs_pack_rne(float a, float b) {
  return __builtin_bit_cast(uint32_t, bfs_bf2{(__bf16)a, (__bf16)b});
}
// the two halves of a packed pair back as fp32 values (the low half by a byte permute: a shift of
// the packed word lets the compiler re-convert that value alone, one more cvt per pair)
__device__ __forceinline__ float bfs_lo_f32(uint32_t h) { return __uint_as_float(__builtin_amdgcn_perm(h, h, 0x01000c0cu)); }
__device__ __forceinline__ float bfs_hi_f32(uint32_t h) { return __uint_as_float(h & 0xffff0000u); }
// a (element 2m), b (element 2m + 1) -> three packed round-to-nearest pieces: x = x1 + x2 + x3 exactly
__device__ __forceinline__ void bfs_split2(float a, float b, uint32_t& h1, uint32_t& h2, uint32_t& h3) {
  h1 = bfs_pack_rne(a, b);
  const float ra = a - bfs_lo_f32(h1), rb = b - bfs_hi_f32(h1);
  h2 = bfs_pack_rne(ra, rb);
  h3 = bfs_pack_rne(ra - bfs_lo_f32(h2), rb - bfs_hi_f32(h2));
}
