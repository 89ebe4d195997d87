// The gfx950 primitives the MFMA kernels are built from: buffer resources and the
// out-of-range convention, LDS-DMA, counted waits and raw barriers, the transposed LDS
// fragment read, the 128-byte-row XOR swizzle and multiply-shift division.  Kernel files
// include this header; they do not copy from it.
#pragma once
#include "common.h"

// ------------------------------------------------------------------ buffer resources
// Every operand load is a branch-free raw buffer load: the per-thread 32-bit voffset is
// precomputed (relative to a wave-uniform base that moves per block / K-tile), and a
// load that must read zero (padding tap, row past M, K tail) gets voffset OOB, past
// num_records, so the hardware returns 0; a store with voffset OOB is dropped.  No
// exec-mask branches around loads means the compiler sees a fixed number of loads per
// K-tile and can wait with counted vmcnt instead of draining all of them, which is what
// lets loads stay in flight across the MFMA phase.
// The resource is raw (stride 0): an access is in range while voffset + its size stays
// within num_records bytes of `base`; num_records stays below 0x80000000, so OOB is out
// of range for every resource built here.  The flags word (the descriptor's fourth
// dword) 0x00020000 is DATA_FORMAT = 4 (BUF_DATA_FORMAT_32, bits 15..18) and every other
// field 0: no swizzle, no index stride, no typed conversion.
typedef __amdgpu_buffer_rsrc_t Rsrc;
constexpr unsigned OOB = 0x80000000u;
// the whole addressable range from `base` on: only an OOB voffset is out of range
static __device__ __forceinline__ Rsrc rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, 0x7ffffff0, 0x00020000);
}
// `bytes` from `base` on (e.g. from a tile's first row to the end of the tensor), so
// whatever the offsets are, the hardware confines every access to the tensor.  A long
// count is clamped to the whole-range value; an unsigned one is the caller's exact range.
static __device__ __forceinline__ Rsrc rsrc(const void* base, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0,
                                           (int)(bytes < 0x7ffffff0L ? bytes : 0x7ffffff0L), 0x00020000);
}
static __device__ __forceinline__ Rsrc rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, bytes, 0x00020000);
}
static __device__ __forceinline__ uint4 bload(Rsrc r, unsigned voff) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0));
}
// the same with a compile-time byte offset in the instruction (as bstore's `imm`)
static __device__ __forceinline__ uint4 bload(Rsrc r, unsigned voff, int imm) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, voff + imm, 0, 0));
}
// branch-free 16-byte store, dropped for an out-of-range voffset
static __device__ __forceinline__ void bstore(Rsrc r, unsigned voff, int imm, const uint4& v) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  __builtin_amdgcn_raw_buffer_store_b128(u32x4{v.x, v.y, v.z, v.w}, r, voff, imm, 0);
}
// 16-byte global load as an MFMA operand fragment
static __device__ __forceinline__ bf16x8 ldfrag(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

// ------------------------------------------------------------------ LDS-DMA, waits, barriers
// LDS-DMA (buffer_load ... lds): 16 B per lane straight into LDS, lane-linear from the
// wave-uniform destination `dst` (no VGPR round trip and no ds_write); an OOB voffset
// writes zeros.
static __device__ __forceinline__ void dma16(Rsrc rs, char* dst, unsigned voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, voff, 0, 0, 0);
}
// counted wait: at most N of this wave's vector-memory operations still in flight
template <int N>
static __device__ __forceinline__ void vmwait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// raw barriers: __syncthreads() would also wait for the global loads / LDS-DMA in flight
// (vmcnt(0)).  lds_barrier() makes this wave's LDS accesses complete first; s_barrier()
// waits for nothing (the caller has placed its own counted waits).
static __device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
static __device__ __forceinline__ void s_barrier() { asm volatile("s_barrier" ::: "memory"); }

// ------------------------------------------------------------------ transposed fragment read
// tr_read: one ds_read_b64_tr_b16 (4 k-rows) at an LDS address the caller computes from its
// image layout; tr_pair joins the read of 4 k-rows and that of the next 4 into one 8-deep
// MFMA operand fragment: tr_pair(tr_read(lo), tr_read(hi)).  The reads are the arguments,
// not the addresses, so that `hi` is computed after the first read is issued - the order
// every kernel here was written in and that its instruction schedule follows.
typedef short s16x8 __attribute__((ext_vector_type(8)));
static __device__ __forceinline__ s16x4 tr_read(const void* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(p));
}
static __device__ __forceinline__ bf16x8 tr_pair(s16x4 lo, s16x4 hi) {
  const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

// ------------------------------------------------------------------ 128-byte-row swizzle
// [rows][64 k] bf16 image, 128 B rows: 16 B chunk c of row r is stored in slot
// c ^ kc_swz(r), so the 16-lane groups of a ds_read_b128 hit 16 distinct slots.
static __device__ __forceinline__ int kc_swz(int r) { return (r >> 1) & 7; }
static __device__ __forceinline__ int kc_off(int r, int c) { return r * 128 + ((c ^ kc_swz(r)) << 4); }
// Source side, for an image filled by LDS-DMA: the destination is lane-linear (a lane's
// 16 B land at slot lane & 7 of some image row r), so the swizzle moves to the source and
// the lane fetches logical chunk (lane & 7) ^ kc_swz(r).  dma_chunk: the block-linear copy,
// thread tid of a 32-row round lands in row tid >> 3 (+ 32 per round, which kc_swz ignores).
static __device__ __forceinline__ int dma_chunk(int tid) { return (tid & 7) ^ kc_swz(tid >> 3); }

// ------------------------------------------------------------------ fast division
// n / d for 0 <= n < 2^31 as a multiply-high, an add and a shift, with the divisor's magic
// number computed on the host.  Passed by value inside kernel arguments: three unsigned
// fields, in this order.
struct FastDiv {
  unsigned d, mul, sh;
  __host__ __device__ FastDiv() : d(1), mul(0), sh(0) {}
  __host__ explicit FastDiv(unsigned dd) : d(dd) {
    sh = 0;
    while ((1u << sh) < d) ++sh;   // ceil(log2 d)
    mul = (unsigned)((((unsigned long long)1 << 32) * ((1ull << sh) - d)) / d + 1);
  }
  __device__ __forceinline__ unsigned div(unsigned n) const { return (__umulhi(n, mul) + n) >> sh; }
  __device__ __forceinline__ void divmod(unsigned n, unsigned& q, unsigned& r) const {
    q = div(n); r = n - q * d;
  }
};
