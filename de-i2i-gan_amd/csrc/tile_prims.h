// Device primitives shared by the MFMA tile kernels (conv_gemm, conv_gemm_v2, conv_halo, conv_halo16, thin_conv, wgrad_v2,
// wgrad_halo, wgrad_thin): the zero page, the two LDS-DMA issue forms, the XCD remap, counted waits, the LDS swizzles and the
// transposed fragment read -- one definition each.  Every .hip is its own translation unit (no -fgpu-rdc), so the `static`
// zero page below is one private copy per code object and makes no host symbol.
#pragma once
#include "common.h"

#if defined(__HIPCC__)
namespace dei2i {

// 256 bytes of zero-initialised device memory: rows that contribute zeros (tile edges, zero padding) fetch from here
static __device__ __attribute__((aligned(256))) unsigned char g_zero_page[256];

// bijective XCD-aware remap of the linear workgroup id (cdna_hip_programming.md T1)
DEI2I_D int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

// ------------------------------------------------------------------------------------------------
// LDS-DMA (global -> LDS, 16 bytes per lane, 1 KB per wave instruction): two issue forms, two rules.
//   glds16 (builtin)          : hipcc sees the LDS write and orders it itself -- s_waitcnt vmcnt(0) in front of the next LDS
//                               read and in every __syncthreads(); the kernel's own counted waits can only be stricter.
//                               Used by conv_gemm_v2, conv_halo and conv_halo16.
//   glds16_asm / glds16_asm_s : hipcc sees nothing and adds nothing: the kernel's own wait_vm<N>() and barriers are ALL that
//                               orders the DMA against the reads, and each has to be complete.
//                               Used by wgrad_v2, wgrad_halo, wgrad_thin and thin_conv.
// A kernel stays on the form its waits were written for.
// ------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

DEI2I_D void glds16(const void* gptr, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void_t*)gptr, (lds_void_t*)lds_wave_base, 16, 0, 0);
}

// The same as inline asm: M0 is written in the same statement and restored after it (hipcc reserves M0).  Issued through
// __builtin_amdgcn_global_load_lds, hipcc knows that LDS is being written and -- unable to tell that a prefetch into the NEXT
// buffer does not alias the buffer being read -- puts s_waitcnt vmcnt(0) in front of the next LDS read (and into every
// __syncthreads()): the multi-stage rings of wgrad_halo / wgrad_v2 / the thin convs then drain their prefetch before computing.
// With the asm form the kernels' own counted vmcnt waits and barriers are what order the DMA against the reads -- each of them
// has to be complete: hipcc adds nothing.
DEI2I_D void glds16_asm(const void* gptr, unsigned char* lds_wave_base) {
  typedef __attribute__((address_space(3))) unsigned char lds_byte_t;
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_byte_t*)lds_wave_base);   // wave-uniform by contract
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gptr), "s"(dst) : "memory");
}
// the same with a wave-uniform 64-bit base (SGPR pair) + a per-lane unsigned 32-bit BYTE offset: no 64-bit vector add per instruction
// (lds_dst: the LDS byte address of the wave's 1 KB piece, wave-uniform -- lds_addr_of(smem) + offset)
DEI2I_D unsigned lds_addr_of(const void* lds_ptr) {
  typedef __attribute__((address_space(3))) unsigned char lds_byte_t;
  return (unsigned)(uintptr_t)(lds_byte_t*)lds_ptr;
}
DEI2I_D void glds16_asm_s(const void* sbase, unsigned voff_bytes, unsigned lds_dst) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_dst);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)sbase);          // (the builtin returns int:
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((uintptr_t)sbase >> 32));  //  no sign extension into the high half)
  const unsigned long long sb = ((unsigned long long)hi << 32) | (unsigned long long)lo;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff_bytes), "s"(sb), "s"(dst) : "memory");
}

// Counted waits: at most N vector-memory operations (LDS-DMA, loads AND stores, in issue order) / N LDS or scalar-memory
// operations of this wave still in flight.
template <int N> DEI2I_D void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N> DEI2I_D void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }

// ------------------------------------------------------------------------------------------------
// LDS swizzles.  Each is an XOR applied alike where a tile is written and where it is read; LDS-DMA lands lane-linear, so
// there it goes onto the SOURCE address each lane fetches.
// ------------------------------------------------------------------------------------------------
// 128-byte rows read with ds_read_b128: the 16-byte chunk c of row r sits at slot c ^ chunk_swz128(r) -- conflict-free
// fragment reads of 16 or 32 consecutive rows from an aligned start (rows two apart would otherwise share their banks);
// tap-shifted reads (conv_halo.hip) start at any row and lose 5.9 % of their cycles to conflicts.
// (conv_gemm_v2.hip and conv_halo.hip use this image too but write the expression out: see their header comments)
DEI2I_D int chunk_swz128(int row) { return (row >> 1) & 7; }
// 64-byte rows read with ds_read_b128: chunk c of row r sits at slot c ^ chunk_swz64(r).  Every read of 16 consecutive rows x 4
// k-groups is conflict-free at ANY starting row (all lane groups of the instruction see 16 distinct (row & 3, slot) pairs), so
// tap-shifted pixel fragments never conflict.  The bit repeats every 8 rows: row r + 16 has the swizzle of row r.
DEI2I_D int chunk_swz64(int row) { return ((row >> 2) & 1) << 1; }
// Pixel-major tiles read with ds_read_b64_tr_b16 (byte offset within the row ^= tr_swz): a 32-lane half reads 4 consecutive
// rows x 64 bytes; spread the 4 rows over the four 64-byte quarters of the 256-byte bank row.
template <int ROWB> DEI2I_D int tr_swz(int row) {
  if constexpr (ROWB % 256 == 0) return (row & 3) << 6;
  else return ((row >> 1) & 1) << 6;    // 128-byte rows: rows r and r+2 alias, flip the 64-byte half
}

// Transposed fragment read: two ds_read_b64_tr_b16 (rows r and r+4 of a pixel-major tile) -> one 8 x bf16 MFMA fragment.
// Lane roles: lane i = 4q+p of a 16-lane group supplies row q, cols 4p..4p+3.
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;
DEI2I_D u32x4 tr_read_pair(lds_s16x4_ptr p0, lds_s16x4_ptr p1) {
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p0);
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p1);
  u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
  u32x4 r;
  r.x = l2.x; r.y = l2.y; r.z = h2.x; r.w = h2.y;
  return r;
}
DEI2I_D u32x4 tr_read_lds(unsigned a0, unsigned a1) {                     // two 32-bit LDS addresses
  return tr_read_pair((lds_s16x4_ptr)(uintptr_t)a0, (lds_s16x4_ptr)(uintptr_t)a1);
}
DEI2I_D u32x4 tr_read(const unsigned char* base, int o0, int o1) {        // a tile base in LDS + two byte offsets
  return tr_read_pair((lds_s16x4_ptr)(base + o0), (lds_s16x4_ptr)(base + o1));
}

}  // namespace dei2i
#endif  // __HIPCC__
