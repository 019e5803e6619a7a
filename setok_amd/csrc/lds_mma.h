// lds_mma.h — the primitives every hand-written MFMA kernel of the library stages and feeds its operands with (gfx950): the LDS-DMA requests,
// the hardware-transposing LDS read and the fp32 -> 16-bit operand pack.  ONE definition of each: a wrong constraint or a forgotten m0
// restore corrupts LDS silently, so no kernel writes its own.
#pragma once
#include "common.h"

// ---- LDS-DMA: global -> LDS without a VGPR round trip ------------------------------------------------------------------------------------
// The m0 contract of global_load_lds_*: lane l's `size` bytes (16 or 4) land at LDS byte address  m0 + l * size  — the destination is not
// per-lane: `dst` is the byte address of lane 0's piece and MUST be wave-uniform (it is moved into m0, a scalar register), the 64 pieces of a
// request are consecutive in LDS, and any swizzle is applied to the SOURCE address.  m0 is saved before and restored after the request, so
// the compiler's own uses of m0 (LDS instructions, readlane) around a request stay valid.  Every request is inline asm: the compiler does
// not know of it, so the kernel places its own `s_waitcnt vmcnt` before it reads what a request wrote.

// 16 bytes per lane from a per-lane pointer
__device__ inline void lds_dma16(const void* src, unsigned dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}
// 16 bytes per lane from a wave-uniform 64-bit base (made scalar here: two readfirstlane) plus a 32-bit per-lane byte offset
__device__ inline void lds_dma16_sbase(const char* sbase, unsigned off, unsigned dst) {
    unsigned keep;
    const unsigned long long b64 = (unsigned long long)sbase;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b64);          // (readfirstlane returns int: widen as unsigned)
    const unsigned hi32 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b64 >> 32));
    const unsigned long long sb64 = (unsigned long long)lo | ((unsigned long long)hi32 << 32);
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(off), "s"(sb64), "s"(dst) : "memory");
}
// 4 bytes per lane from a per-lane pointer
__device__ inline void lds_dma4(const void* src, unsigned dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}

// ---- the transposing LDS read (ds_read_b64_tr_b16) as an MFMA A operand ------------------------------------------------------------------
// Lanes 4 j + p of a 16-lane group supply row j, 8-byte piece p; lane i receives element i of rows 0 .. 3.  Two reads — `a0`, and `a1` for
// the rows that fill k-slots 4 .. 7 — make the eight k-slots of one lane's fragment.
typedef __attribute__((ext_vector_type(4))) short short4v;

__device__ inline bf16x8 lds_read_tr16(const char* a0, const char* a1) {
    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(a0));
    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(a1));
    union { short s8[8]; bf16x8 v; } u;
#pragma unroll
    for (int j = 0; j < 4; ++j) { u.s8[j] = lo[j]; u.s8[4 + j] = hi[j]; }
    return u.v;
}

// eight fp32 values -> one 16-bit MFMA operand (round to nearest even)
__device__ inline bf16x8 pack8(const float* p) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (bf16)p[i];
    return v;
}
