// conv_prims.h — the device primitives the conv_*.hip kernels share, one copy each: MFMA operand / accumulator vector
// types, one LDS-DMA piece, the counted waits, LDS operand reads and MFMAs as inline asm, division by a host-computed
// reciprocal, and the XCD-contiguous static tile list of the persistent kernels.  Everything is __forceinline__: a
// kernel compiles to the instructions it had with a private copy (tools/isa_identity.py compares two checkouts).
#pragma once
#include <hip/hip_runtime.h>

#include "act_io.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_void_ptr;

// one LDS-DMA piece: 64 lanes x 16 bytes -> LDS [lds_off, lds_off + 1 KiB) (wave-uniform), source = buffer base +
// per-lane voff + wave-uniform soff; lanes whose voff is out of range write zeros
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, char* smem, int lds_off, unsigned voff, unsigned soff = 0) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_ptr)(smem + lds_off), 16, voff, soff, 0, 0);
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS operand reads as inline asm: hipcc sinks every compiler-visible ds_read to just before its MFMA and waits
// lgkmcnt(0) there (no software pipelining across taps); the asm forms pin the issue point, and the wait statement of
// the kernel that uses them (lds_wait in conv_pipe.hip ...) names every destination "+v" so that no consumer (and no
// register copy) is scheduled above it.
template <int OFF>
__device__ __forceinline__ void lds_read16(bf16x8& dst, int addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}

// MFMAs as inline asm too: the builtin is a pure value operation that instruction selection may place anywhere between
// its operands' definitions and its result's use — hipcc sank MFMAs across two and three taps, keeping their operands
// alive (36-42 spilled registers inside the loop).  asm volatile statements keep their program order.
// Hazards the compiler cannot see: a VALU read of an accumulator needs 12 wait states after the MFMA that wrote it
// (the epilogue is preceded by explicit s_nops); accumulate chains (D as the next C) need none.
__device__ __forceinline__ void mfma1(f32x16& acc, const bf16x8& a, const bf16x8& b) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}

// q = n / d for n * d < 2^32 with M = magic_of(d) = ceil(2^32 / d) from the host (tile indices: a few thousand);
// magic 0: d = 1
__device__ __forceinline__ int fastdiv(int n, unsigned magic) { return magic ? (int)__umulhi((unsigned)n, magic) : n; }
inline unsigned magic_of(int d) { return d <= 1 ? 0u : (unsigned)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d); }

// Static tile list of a persistent kernel launched with a multiple of 8 blocks: XCD x (blocks x, x+8, ...) owns a
// contiguous range of the total_tiles tiles and its blocks interleave inside it, so the CUs of an XCD work on
// consecutive tiles: xn of them, tile k of this block is xs + bslot + k * nslots.  A block with bslot >= xn has none and
// returns at once; the others walk xcd_my_tiles(xn, bslot, nslots) tiles.
// (Two steps with plain int references, and the return in the kernel: with the values in a struct, or with the return
// and the tile count inside the helper, hipcc's code for the kernels came out different from the private copies'.)
__device__ __forceinline__ void xcd_tile_span(int total_tiles, int& xs, int& xn, int& bslot, int& nslots) {
    const int xcd = blockIdx.x & 7;
    bslot = blockIdx.x >> 3, nslots = gridDim.x >> 3;
    const int tq = total_tiles >> 3, tr = total_tiles & 7;
    xs = xcd * tq + (xcd < tr ? xcd : tr), xn = tq + (xcd < tr ? 1 : 0);
}
__device__ __forceinline__ int xcd_my_tiles(int xn, int bslot, int nslots) { return (xn - bslot + nslots - 1) / nslots; }
