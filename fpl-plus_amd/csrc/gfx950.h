// Device-side primitives of the hand-written convolution kernels (gfx950 only): the vector types and every inline-asm
// sequence, each written once and explained where it is defined.  Device code only; conv_march.hip, conv_brick.hip,
// conv_wgrad.hip, conv_mfma.hip and conv_edge.hip include it, and no .hip file holds an asm statement of its own.
// Everything here is __forceinline__: a call compiles to the statement it wraps, at the place of the call.
#pragma once
#include "common.h"

// ---- vector types (MFMA fragments, 8- and 16-byte memory accesses)
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// ---- register pins.  An empty asm statement makes a value opaque at that point: hipcc can neither take it apart, nor fold
// it into constants, nor hoist what is derived from it out of a loop - addresses formed from an opaque base are computed
// next to their use (a few VALU ops under the MFMAs) instead of living in registers across the loop and being spilled.
// opaque_v pins a per-lane value in a VGPR, opaque_s a wave-uniform one in an SGPR, both in place.
template <class T> __device__ __forceinline__ void opaque_v(T& x) { asm volatile("" : "+v"(x)); }
template <class T> __device__ __forceinline__ void opaque_s(T& x) { asm volatile("" : "+s"(x)); }
// two values pinned by ONE statement (two statements are scheduled, and their registers allocated, differently)
template <class T> __device__ __forceinline__ void opaque_v(T& x, T& y) { asm volatile("" : "+v"(x), "+v"(y)); }

// ---- waits and the LDS-only barrier
// vmcnt counts this wave's outstanding vector-memory operations: LDS-DMA pieces, loads and stores share the counter.
// The LDS-DMA issues below are invisible to hipcc's own bookkeeping, so whoever issues them also retires them, by one of
// these waits in front of the barrier that publishes the data.  Where ordinary loads or stores of the wave are in flight
// too, only 0 is a safe count (they may complete out of order); a count N > 0 ("all but the N issued last have landed")
// is for waves that issue nothing but DMA pieces.
__device__ __forceinline__ void wait_vmcnt0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
// The same for a count that becomes a constant only after unrolling (the wait takes an immediate): one wait per value,
// of which the unrolled code keeps one.  Counts above 8 wait for everything.
__device__ __forceinline__ void wait_vmcnt_upto8(int n) {
  if (n == 1) wait_vmcnt<1>();
  else if (n == 2) wait_vmcnt<2>();
  else if (n == 3) wait_vmcnt<3>();
  else if (n == 4) wait_vmcnt<4>();
  else if (n == 5) wait_vmcnt<5>();
  else if (n == 6) wait_vmcnt<6>();
  else if (n == 7) wait_vmcnt<7>();
  else if (n == 8) wait_vmcnt<8>();
  else wait_vmcnt0();
}
// Barrier for LDS traffic only.  __syncthreads() also waits for vmcnt(0), i.e. for the acknowledgement of every global
// store the wave has in flight - at the end of a block that is the whole write-out of its last depth (2-3 us per block,
// 12-24 us per launch measured on the statistics forms) - and for LDS-DMA pieces a loop wants to keep in flight.  This
// one waits for the wave's LDS accesses alone; an LDS-DMA that the barrier is to publish needs its own vmcnt wait first.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- LDS addresses
// wave-uniform 32-bit LDS byte address of a pointer into shared memory (what M0 and the ds instructions take)
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return __builtin_amdgcn_readfirstlane((unsigned)(size_t)((__attribute__((address_space(3))) char*)p));
}

// ---- transposed LDS fragment read of a [voxel][32 channel] image with 64-byte voxel rows: two transposed 4 x 16 block
// reads (voxels +0..3 and +4..7 of a lane group's 8) spliced into the 8 k-values of an MFMA operand.  Lane geometry: group
// g = lane / 16 reads voxel rows 8 (g >> 1) + q, channels 16 (g & 1) + 4 p .. (q = (lane & 15) >> 2, p = lane & 3).
// Takes a pointer into shared memory, or a 32-bit LDS byte address (an opaque per-step base + a compile-time offset that
// lands in the instruction's 16-bit offset field).
__device__ __forceinline__ bf16x8 tr_splice(bf16x4 lo, bf16x4 hi) {
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wint-to-pointer-cast"      // LDS pointers are 32 bits wide
template <class A> __device__ __forceinline__ bf16x8 tr_frag(A base_lo) {      // A: const char* or unsigned
  return tr_splice(__builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(base_lo)),
                   __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(base_lo + 4 * 64)));
}
#pragma clang diagnostic pop

// ---- buffer resource descriptor over [base, base + bytes): base low, base high (16 bits; stride 0), the byte extent and
// the flags word of a raw buffer (0x00020000: 32-bit data format).  All four words are wave-uniform (readfirstlane): they
// live in SGPRs.  The hardware checks every lane's offset - per-lane offset + scalar offset - against the extent, and a
// lane out of range reads ZEROS (as LDS-DMA: writes zeros into LDS).  The kernels use that as their padding: a halo voxel
// outside the volume, the tail of a last piece, or a whole slab outside the volume gets the offset 0x40000000u - 1 GiB,
// beyond every extent (the launchers keep what a descriptor spans below 1 GiB) and small enough that per-lane + scalar
// offset does not wrap 32 bits even when both are out of range.  (Where the scalar offset is always 0, 0x80000000u
// serves as well.)
// The shape of the constructor is deliberate: hipcc's scalar schedule and register allocation follow the order and the form
// in which these operations are emitted, and profiles/device_header_codeobjects.txt holds every code object to what the
// written-out fields produced.  The base words are formed by converting the first argument (a pointer, or the address as
// an integer), i.e. - arguments being evaluated left to right - in front of whatever the extent expression computes, and
// the extent is narrowed to 32 bits at the call site, next to the arithmetic that forms it.
struct BufferBase {
  unsigned lo, hi;
  __device__ __forceinline__ BufferBase(uint64_t a)
      : lo(__builtin_amdgcn_readfirstlane((unsigned)a)), hi(__builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xFFFFu)) {}
  __device__ __forceinline__ BufferBase(const void* p) : BufferBase((uint64_t)(size_t)p) {}
};
__device__ __forceinline__ u32x4 buffer_rsrc(BufferBase base, unsigned bytes) {
  u32x4 r;
  r[0] = base.lo;
  r[1] = base.hi;
  r[2] = __builtin_amdgcn_readfirstlane(bytes);
  r[3] = 0x00020000u;
  return r;
}

// ---- LDS-DMA: global memory -> LDS without staging registers and without a ds_write pass.  A wave-instruction fills
// 1 KiB of LDS linearly, 16 bytes per lane, from M0's byte address on (lds: wave-uniform, see lds_addr); a layout
// other than linear is made by choosing each lane's SOURCE.
// M0 is reserved by the compiler and not preserved around a statement: it is saved, written, used and restored inside
// ONE statement (the s_nop 0 is the wait state between the SALU write of M0 and the instruction that reads it).
// Inline asm and not the builtin: with the builtin in a loop hipcc stops counting lgkmcnt and drains every ds_read with
// lgkmcnt(0), which defeats the fragment prefetch.  hipcc does not count these operations: retire them with a vmcnt wait
// above, then a barrier, before the data is read.
// Buffer form: source = descriptor (buffer_rsrc) + per-lane byte offset + scalar byte offset, range-checked (see above).
// (Vector arguments by value here and below: a reference keeps the caller's variable in memory until the call is inlined.)
__device__ __forceinline__ void lds_dma_buffer(u32x4 rsrc, unsigned lane_off, unsigned scalar_off, unsigned lds) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(lane_off), "s"(rsrc), "s"(scalar_off), "s"(lds) : "memory");
}
// Global form: source = each lane's own pointer (no range check: lanes with nothing to fetch point at a zero constant).
__device__ __forceinline__ void lds_dma_global(const void* src, unsigned lds) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(lds) : "memory");
}

// ---- 16-byte global store that hipcc does not know about.
// Inline asm: a store hipcc knows about makes it guard later register reuse with vmcnt(N) waits, and since it does not
// know about the DMA pieces in flight, those waits end up waiting for the DMA.
// s_nop 1: a VMEM store of more than 8 bytes reads its data VGPRs for two more cycles ("12-dword store" hazard: a VALU
// write of those registers needs 2 wait states on gfx940+); hipcc's hazard recognizer does not look inside inline asm,
// and the register allocator reuses the data registers at once.  Without the nop the first dword of the store's last
// lanes picked up the next instruction's result whenever another kernel's waves shared the SIMD
// (profiles/r02_race25_hazard_location.txt: the 2.5D stream-order hazard of round 1).
// The store is retired by the caller's next wait_vmcnt0().
__device__ __forceinline__ void global_store_16(void* dst, u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" :: "v"(dst), "v"(v) : "memory");
}
