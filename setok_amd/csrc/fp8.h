// fp8.h — the e4m3fn <-> fp32 helpers and the row-exponent rule of the fp8 storage contract (include/setok_hip.h, "FP8 weight-only decode"),
// shared by the weight path (gemm_fp8w.hip) and the KV-cache path (attn_decode.hip): a weight row and a cache row are stored by the same rule.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;      // 16 bytes as they come from memory

__device__ inline float fp8w_scale(int e) { return __builtin_bit_cast(float, (unsigned)(127 + e) << 23); }      // 2^e exactly, e in [-15, 7]

// the row exponent: the smallest e with amax <= 448 * 2^e = 1.75 * 2^(8 + e), clamped to [-15, 7], 0 for amax == 0: exponent arithmetic on
// amax = 1.m * 2^x (an fp32 subnormal reads as x = -127: clamped); amax is finite and >= 0
__device__ inline int fp8w_exponent(float amax) {
    int ex = 0;
    if (amax > 0.f) {
        const unsigned b = __builtin_bit_cast(unsigned, amax);
        ex = (int)(b >> 23) - 127 - 8 + ((b & 0x7fffffu) > 0x600000u ? 1 : 0);
        ex = ex < -15 ? -15 : (ex > 7 ? 7 : ex);
    }
    return ex;
}

// round-to-nearest-even to OCP e4m3fn (subnormals included), saturating at +-448; v is finite
__device__ inline unsigned fp8w_encode(float v) {
    const unsigned sign = (__builtin_bit_cast(unsigned, v) >> 24) & 0x80u;
    const float a = fminf(fabsf(v), 448.0f);
    unsigned code;
    if (a < 0.015625f) {                                           // below 2^-6: multiples of 2^-9 (8 rounds up into the first normal code, 0x08)
        code = (unsigned)rintf(a * 512.0f);
    } else {
        unsigned b = __builtin_bit_cast(unsigned, a);
        b += 0x7ffffu + ((b >> 20) & 1u);                          // nearest even at 3 mantissa bits; a carry walks into the exponent
        code = (((b >> 23) - 120u) << 3) | ((b >> 20) & 7u);       // biased exponent 127 + x -> 7 + x
    }
    return sign | code;
}

// the 16 values of a lane's 16 fp8 bytes, in byte order
__device__ inline void fp8w_decode16(const u32x4& w, float* f) {
    const unsigned u[4] = {w[0], w[1], w[2], w[3]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)u[i], false);
        const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)u[i], true);
        f[4 * i + 0] = lo[0]; f[4 * i + 1] = lo[1]; f[4 * i + 2] = hi[0]; f[4 * i + 3] = hi[1];
    }
}
