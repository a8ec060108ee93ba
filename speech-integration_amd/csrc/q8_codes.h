// The e4m3 codes with one power-of-two exponent byte of the header's "FP8 K/V cache" rule, as device code: the one copy that the K/V store, the
// decode walks (attention_decode.hip) and the weight quantiser and GEMMs (gemm_wq8.hip) share.  A "line" there is a row of a weight matrix here.
#pragma once
#include "common_hip.h"

// the bits of the larger finite magnitude: finite |x| order as unsigned integers, a NaN or an infinity never wins
__device__ __forceinline__ uint32_t q8_absmax_bits(uint32_t a, float x) {
    const uint32_t m = __float_as_uint(x) & 0x7fffffffu;
    return m < 0x7f800000u && m > a ? m : a;
}

// a = m * 2^E, m in [1, 2): e = E - 8, or E - 7 where m > 1.75, and b = max(e, -127) + 127 from a's exponent field E + 127 (a subnormal a,
// field 0, has E - 7 < -127: b = 0 as the formula gives it; e <= 120 never meets the upper clamp)
__device__ __forceinline__ int q8_exponent_byte(uint32_t a) {
    const int b = (int)(a >> 23) - 8 + ((a & 0x7fffffu) > 0x600000u ? 1 : 0);
    return a == 0 ? 127 : b < 0 ? 0 : b;
}

// four codes of f[0..3] under exponent byte b, element v in byte v: scaled (v_ldexp_f32: exact), converted (v_cvt_pk_fp8_f32: RNE); a NaN or
// an infinity stores the NaN code 0x7f, whatever the conversion makes of it
__device__ __forceinline__ uint32_t q8_encode4(float f0, float f1, float f2, float f3, int b) {
    const float f[4] = {f0, f1, f2, f3};
    float s[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) s[v] = ldexpf(f[v], 127 - b);
    int p = 0;
    p = __builtin_amdgcn_cvt_pk_fp8_f32(s[0], s[1], p, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(s[2], s[3], p, true);
    uint32_t u = (uint32_t)p;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const bool finite = (__float_as_uint(f[v]) & 0x7fffffffu) < 0x7f800000u;
        u = finite ? u : (u & ~(0xffu << (8 * v))) | (0x7fu << (8 * v));
    }
    return u;
}

// the values of the four codes of word c under e = b - 127 (v_cvt_pk_f32_fp8, v_ldexp_f32: both exact)
__device__ __forceinline__ void q8_decode4(uint32_t c, int e, float* f) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c, true);
    f[0] = ldexpf(lo[0], e);
    f[1] = ldexpf(lo[1], e);
    f[2] = ldexpf(hi[0], e);
    f[3] = ldexpf(hi[1], e);
}
