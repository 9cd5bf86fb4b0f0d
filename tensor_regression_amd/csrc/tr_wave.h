// tr_wave.h — the wave-level building blocks every gfx950 kernel file shares: lane exchange and
// reductions, the LDS barrier and LDS-DMA pieces of the ring-buffer kernels, counted vmcnt waits and
// the MFMA wrappers.  One copy each, prefix wv_; every function is inlined, so a kernel's code is
// what it was with a private copy (tools/isa_cmp.sh compares the assembly of two trees).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float wv_f4 __attribute__((ext_vector_type(4)));     // an MFMA accumulator / a 16-B load
typedef uint32_t wv_u4 __attribute__((ext_vector_type(4)));  // eight packed 16-bit MFMA operands

// ---- lane exchange and reductions -----------------------------------------------------------
// Every reduction below adds (or maxes) the same two operands in both lanes of a pair at every
// step, so by commutativity of the IEEE operation all participating lanes end with the
// bitwise-identical value: the result is deterministic and may be read from any lane.

// One DPP move (row_mask = bank_mask = 0xF, no bound control): lane exchange inside a 16-lane row
// on the VALU's operand path, no LDS round trip.
template <int CTRL>
__device__ __forceinline__ float wv_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// 16-lane row reductions by DPP: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror,
// row_mirror.
__device__ __forceinline__ float wv_row_sum16(float v) {
  v += wv_dpp<0xB1>(v);
  v += wv_dpp<0x4E>(v);
  v += wv_dpp<0x141>(v);
  v += wv_dpp<0x140>(v);
  return v;
}
__device__ __forceinline__ float wv_row_max16(float v) {
  v = fmaxf(v, wv_dpp<0xB1>(v));
  v = fmaxf(v, wv_dpp<0x4E>(v));
  v = fmaxf(v, wv_dpp<0x141>(v));
  v = fmaxf(v, wv_dpp<0x140>(v));
  return v;
}
// v_permlane16_swap / v_permlane32_swap (CDNA4) of a value with itself: the two results hold, in
// every lane, the lane's own row pair / half and the partner's, so their sum is the xor-16 /
// xor-32 butterfly step without an LDS round trip (ds_bpermute).
__device__ __forceinline__ float wv_xor16_sum(float v) {
  const auto q = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(q[0]) + __uint_as_float(q[1]);
}
__device__ __forceinline__ float wv_xor32_sum(float v) {
  const auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(q[0]) + __uint_as_float(q[1]);
}
// (lower-half value, upper-half value) of v at lane (l mod 32) and (l mod 32) + 32, in every lane
__device__ __forceinline__ void wv_halves(float v, float& lo, float& hi) {
  const auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  lo = __uint_as_float(q[0]);
  hi = __uint_as_float(q[1]);
}
// One ds_swizzle step in bit-mask mode (offset = xor << 10 | and 0x1F): an xor butterfly inside
// each 32-lane half through the LDS crossbar, without address VGPRs and without touching LDS memory.
template <int PATTERN>
__device__ __forceinline__ float wv_swz(float v) {
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), PATTERN));
}
__device__ __forceinline__ float wv_swz_sum16(float v) {
  v += wv_swz<0x201F>(v);  // xor 8
  v += wv_swz<0x101F>(v);  // xor 4
  v += wv_swz<0x081F>(v);  // xor 2
  v += wv_swz<0x041F>(v);  // xor 1
  return v;
}
__device__ __forceinline__ float wv_swz_max16(float v) {
  v = fmaxf(v, wv_swz<0x201F>(v));
  v = fmaxf(v, wv_swz<0x101F>(v));
  v = fmaxf(v, wv_swz<0x081F>(v));
  v = fmaxf(v, wv_swz<0x041F>(v));
  return v;
}
// readfirstlane / readlane of a float (the result is a scalar: the same in every lane)
__device__ __forceinline__ float wv_rfl(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ float wv_rdl(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
// All-reduce across the 64 lanes of a wave: the swizzle butterfly inside each 32-lane half, then
// the two half results through readlane.
__device__ __forceinline__ float wv_allreduce(float v) {
  v += wv_swz<0x401F>(v);  // xor 16
  v += wv_swz<0x201F>(v);  // xor 8
  v += wv_swz<0x101F>(v);  // xor 4
  v += wv_swz<0x081F>(v);  // xor 2
  v += wv_swz<0x041F>(v);  // xor 1
  const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  return a + b;
}
__device__ __forceinline__ float wv_allreduce_max(float v) {
  v = fmaxf(v, wv_swz<0x401F>(v));
  v = fmaxf(v, wv_swz<0x201F>(v));
  v = fmaxf(v, wv_swz<0x101F>(v));
  v = fmaxf(v, wv_swz<0x081F>(v));
  v = fmaxf(v, wv_swz<0x041F>(v));
  const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  return fmaxf(a, b);
}
__device__ __forceinline__ double wv_allreduce_d(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- barriers -------------------------------------------------------------------------------
// Workgroup barrier on LDS alone: each wave retires its own LDS accesses (lgkmcnt), then
// s_barrier.  Global loads and LDS-DMA pieces (vmcnt) stay in flight across it; __syncthreads()
// would wait vmcnt(0) as well and drain the DMA these kernels overlap with their GEMMs.
__device__ __forceinline__ void wv_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// Not a workgroup barrier: one wave's own LDS writes before its lanes read each other's.  A wave
// executes in lockstep, so no s_barrier is needed and no other wave is ordered by it; the fences
// keep the compiler from moving the accesses across (wv_barrier orders all waves of the workgroup).
__device__ __forceinline__ void wv_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- LDS-DMA --------------------------------------------------------------------------------
// One LDS-DMA piece per lane (16 B or 4 B from gsrc, 4-B aligned is enough, to LDS byte address
// m0 + size * lane), issued from inline asm: the compiler then does not see an LDS write in flight.
// With the builtin it cannot tell the ring slot being filled from the one being read and puts an
// s_waitcnt vmcnt(0) in front of every later LDS read, draining the DMA the kernel overlaps with
// them.  The kernel orders the pieces itself: counted wv_wait_vm + wv_barrier before a slot is
// read, wv_barrier before it is refilled.  m0 is compiler-reserved: it is saved and restored inside
// the statement.  The "memory" clobber keeps the compiler from moving LDS reads across the piece.
//
// Two things differ between the kernels, and each call site states its choice:
//  - the cache policy: WV_NT issues the piece non-temporal (a sample streamed once per pass should
//    not displace the factors in L2 / Infinity Cache), WV_CACHED with the default policy.  Which
//    one is faster was measured per kernel (DESIGN.md "Wave-level primitives"); they are not
//    interchangeable without measuring again.
//  - the m0 operand: WV_DST_RFL passes the LDS address through readfirstlane, which states that it
//    is wave-uniform where it was computed from per-lane values; WV_DST_UNIFORM hands it to the
//    "s" operand as it is, for an address the compiler already holds in a scalar register.
__device__ __forceinline__ uint32_t wv_lds_addr(const float* p) {
  return (uint32_t)(uintptr_t)((const __attribute__((address_space(3))) float*)p);
}
constexpr bool WV_NT = true, WV_CACHED = false;
constexpr bool WV_DST_RFL = true, WV_DST_UNIFORM = false;
#define WV_DMA_PIECE(OP, POLICY)                                                                            \
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t" OP " %1, off" POLICY "\n\ts_mov_b32 m0, %0" \
               : "=&s"(keep)                                                                                \
               : "v"(gsrc), "s"(dst)                                                                        \
               : "memory")
template <bool NT, bool RFL>
__device__ __forceinline__ void wv_dma16(const float* gsrc, const float* lds_dst) {
  const uint32_t a = wv_lds_addr(lds_dst), dst = RFL ? __builtin_amdgcn_readfirstlane(a) : a;
  uint32_t keep;
  if constexpr (NT)
    WV_DMA_PIECE("global_load_lds_dwordx4", " nt");
  else
    WV_DMA_PIECE("global_load_lds_dwordx4", "");
}
template <bool NT, bool RFL>
__device__ __forceinline__ void wv_dma4(const float* gsrc, const float* lds_dst) {
  const uint32_t a = wv_lds_addr(lds_dst), dst = RFL ? __builtin_amdgcn_readfirstlane(a) : a;
  uint32_t keep;
  if constexpr (NT)
    WV_DMA_PIECE("global_load_lds_dword", " nt");
  else
    WV_DMA_PIECE("global_load_lds_dword", "");
}
#undef WV_DMA_PIECE

// s_waitcnt vmcnt(n) for a wave-uniform runtime n (the counter is an immediate, hence the switch).
// MAXN is the largest count a kernel asks for, 31 or 63 (the field is six bits wide); above it the
// wait is for MAXN, stricter than asked and still safe.  The cap is a template parameter and the
// operand is spelled as each cap's kernels always had it (k, or b + i in groups of eight), because
// the spelling reaches the assembly listing: no kernel's code or listing changes with the cap.
#define WV_VM(k) \
  case k:        \
    asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); \
    break;
#define WV_VM8(b) WV_VM(b) WV_VM(b + 1) WV_VM(b + 2) WV_VM(b + 3) WV_VM(b + 4) WV_VM(b + 5) WV_VM(b + 6) WV_VM(b + 7)
template <int MAXN>
__device__ __forceinline__ void wv_wait_vm(int n) {
  static_assert(MAXN == 31 || MAXN == 63, "caps in use");
  if constexpr (MAXN == 31) {
    switch (n < 0 ? 0 : n) {
      WV_VM(0) WV_VM(1) WV_VM(2) WV_VM(3) WV_VM(4) WV_VM(5) WV_VM(6) WV_VM(7)
      WV_VM(8) WV_VM(9) WV_VM(10) WV_VM(11) WV_VM(12) WV_VM(13) WV_VM(14) WV_VM(15)
      WV_VM(16) WV_VM(17) WV_VM(18) WV_VM(19) WV_VM(20) WV_VM(21) WV_VM(22) WV_VM(23)
      WV_VM(24) WV_VM(25) WV_VM(26) WV_VM(27) WV_VM(28) WV_VM(29) WV_VM(30) WV_VM(31)
      default:
        asm volatile("s_waitcnt vmcnt(31)" ::: "memory");
    }
  } else {
    switch (n < 0 ? 0 : n) {
      WV_VM8(0) WV_VM8(8) WV_VM8(16) WV_VM8(24) WV_VM8(32) WV_VM8(40) WV_VM8(48) WV_VM8(56)
      default:
        asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
    }
  }
}
#undef WV_VM8
#undef WV_VM

// ---- MFMA -----------------------------------------------------------------------------------
// v_mfma_f32_4x4x1_16b_f32: 16 blocks of 4x4 outer products (lane l = output row, four columns)
__device__ __forceinline__ wv_f4 wv_mfma_4x4(float a, float b, wv_f4 c) {
  return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0);
}
// v_mfma_f32_16x16x4_f32: exact fp32 products, lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15]
__device__ __forceinline__ wv_f4 wv_mfma_16x16x4(float a, float b, wv_f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// v_mfma_f32_16x16x32_bf16 / _f16 on operands held as four VGPRs of packed pairs
__device__ __forceinline__ wv_f4 wv_mfma_bf16(wv_u4 a, wv_u4 b, wv_f4 c) {
  typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
}
__device__ __forceinline__ wv_f4 wv_mfma_f16(wv_u4 a, wv_u4 b, wv_f4 c) {
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}
