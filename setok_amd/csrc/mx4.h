// mx4.h — the e2m1 / e8m0 <-> fp32 helpers and the block-exponent rule of the MXFP4 storage contract (include/setok_hip.h, "MXFP4 weight-only
// decode"), shared by the weight path (gemm_mxfp4w.hip) and the KV-cache path (attn_decode.hip, attn_extend.hip): a weight row and a cache row
// are stored by the same rule.
#pragma once
#include "common.h"

// The converter's scale operand: an fp32 whose exponent field IS the e8m0 byte.  0xFF (the block is NaN) also sets a mantissa bit, so the operand
// is a NaN both as e8m0 and as fp32.
__device__ inline float mx4_scale(unsigned s) { return __builtin_bit_cast(float, (s << 23) | (s == 0xffu ? 0x400000u : 0u)); }

// the 8 values of one dword (elements 0..7: byte b holds element 2b in its low nibble, 2b + 1 in its high one), scaled, in fp32
__device__ inline void mx4_f32x8(unsigned w, float sc, float* f) {
    const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 0), p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 1);
    const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 2), p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 3);
    f[0] = p0[0]; f[1] = p0[1]; f[2] = p1[0]; f[3] = p1[1]; f[4] = p2[0]; f[5] = p2[1]; f[6] = p3[0]; f[7] = p3[1];
}

// The converter into the build's 16-bit element type (common.h): exact for every value(nibble) * 2^e with e in [-13, 13], the exponents the
// quantisers write (6 * 2^13 < 65504, 0.5 * 2^-13 is fp16's smallest normal).
#ifdef SETOK_HALF
#define MX4_CVT_PK16 __builtin_amdgcn_cvt_scalef32_pk_f16_fp4
#else
#define MX4_CVT_PK16 __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4
#endif

// the 8 values of one dword (mx4_f32x8's order), scaled, in the 16-bit element type: one 16-byte MFMA operand fragment
__device__ inline bf16x8 mx4_frag(unsigned w, float sc) {
    const bf16x2 p0 = MX4_CVT_PK16(w, sc, 0), p1 = MX4_CVT_PK16(w, sc, 1), p2 = MX4_CVT_PK16(w, sc, 2), p3 = MX4_CVT_PK16(w, sc, 3);
    return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// round-to-nearest, ties to the even code, to e2m1 (0, 0.5, 1, 1.5, 2, 3, 4, 6), saturating at +-6; v is finite.  The sign bit is v's own.
__device__ inline unsigned mx4_encode(float v) {
    const unsigned sign = (__builtin_bit_cast(unsigned, v) >> 28) & 0x8u;
    const float a = fabsf(v);
    const unsigned code = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
    return sign | code;
}

// the block exponent: floor(log2(amax)) - 2 by exponent arithmetic (an fp32 subnormal reads as -127: clamped), clamped to [-13, 13]; 0 for a
// block of zeros.  amax is finite and >= 0.
__device__ inline int mx4_exponent(float amax) {
    int e = 0;
    if (amax > 0.f) {
        e = (int)(__builtin_bit_cast(unsigned, amax) >> 23) - 127 - 2;
        e = e < -13 ? -13 : (e > 13 ? 13 : e);
    }
    return e;
}

__device__ inline float mx4_inv_scale(int e) { return __builtin_bit_cast(float, (unsigned)(127 - e) << 23); }      // 2^-e exactly, e in [-13, 13]
