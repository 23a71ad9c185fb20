// ssdnerf_amd/csrc/cache_cvt.h -- the number formats of the 16-bit scene cache, on bit patterns.
//
// The cache keeps a scene's pre-activation code in fp16 and its two Adam moments in bf16 (scene_cache.py; the reference's cache_16bit,
// lib/core/utils/misc.py:43-128).  A value enters the cache as  _clamp_to(x, dtype).to(dtype) : clamped to the target's finite range, then
// rounded to nearest, ties to even.  On bit patterns:
//     NaN            stays NaN (quiet; the payload is not kept)
//     |x| > max      becomes +-max: 65504 = 0x7BFF in fp16, 0x7F7F in bf16 -- so does +-Inf, and so does 65519.9, which plain rounding would
//                    still bring down to 65504, and 65520, which plain rounding would make Inf
//     otherwise      round to nearest even, the sign of zero kept; below 2^-14 the fp16 result is a subnormal (2^-25 is a tie and goes to 0,
//                    anything above it to 2^-24); bf16 shares fp32's exponent range, so its subnormals come out of the same shift
// Leaving the cache a value is widened to fp32, which is exact for every pattern (subnormals, Inf and NaN included).
// Integer arithmetic only: the device and a gcc build give the same bits by construction, and no denormal mode can interfere.
// Plain C: compiled by hipcc into the kernels of scene_cache.hip and by gcc into the CPU test's harness (tests/host/cache_host.c).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SSCC_FN __device__ __forceinline__
#else
#define SSCC_FN static inline
#endif

#define SSCC_F16_MAX_AS_F32 0x477fe000u   // 65504
#define SSCC_BF16_MAX_AS_F32 0x7f7f0000u  // 3.3895e38

// fp32 bits -> fp16 bits, clamped to +-65504, round to nearest even
SSCC_FN uint16_t sscc_f32_to_f16_clamped(uint32_t u) {
    const uint32_t sign = (u >> 16) & 0x8000u;
    uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                 // NaN
    if (a > SSCC_F16_MAX_AS_F32) a = SSCC_F16_MAX_AS_F32;                   // the clamp (Inf included)
    if (a >= 0x38800000u) {                                                 // >= 2^-14: a normal fp16; the carry of the rounding walks into the exponent
        const uint32_t r = a - 0x38000000u + 0xfffu + ((a >> 13) & 1u);
        return (uint16_t)(sign | (r >> 13));
    }
    if (a < 0x33000000u) return (uint16_t)sign;                             // < 2^-25: zero
    // [2^-25, 2^-14): a multiple of 2^-24.  value = mant * 2^(e - 150), in units of 2^-24: mant >> (126 - e), e in [102, 112]
    const uint32_t e = a >> 23, mant = (a & 0x7fffffu) | 0x800000u, sh = 126u - e;
    uint32_t h = mant >> sh;
    const uint32_t rem = mant & ((1u << sh) - 1u), half = 1u << (sh - 1u);
    if (rem > half || (rem == half && (h & 1u))) ++h;                       // (h == 0x400 is 2^-14, the smallest normal: the right bits)
    return (uint16_t)(sign | h);
}

// fp32 bits -> bf16 bits, clamped to the largest finite bf16, round to nearest even
SSCC_FN uint16_t sscc_f32_to_bf16_clamped(uint32_t u) {
    const uint32_t sign = (u >> 16) & 0x8000u;
    uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7fc0u);                 // NaN
    if (a > SSCC_BF16_MAX_AS_F32) a = SSCC_BF16_MAX_AS_F32;                 // the clamp (Inf included): nothing above it is left to round up to Inf
    a += 0x7fffu + ((a >> 16) & 1u);
    return (uint16_t)(sign | (a >> 16));
}

// fp16 bits -> fp32 bits, exact
SSCC_FN uint32_t sscc_f16_to_f32(uint16_t h) {
    const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, e = ((uint32_t)h >> 10) & 0x1fu;
    uint32_t m = (uint32_t)h & 0x3ffu;
    if (e == 0x1fu) return sign | 0x7f800000u | (m << 13);                  // Inf, NaN (payload kept)
    if (e != 0u) return sign | ((e + 112u) << 23) | (m << 13);
    if (m == 0u) return sign;
    uint32_t k = 0;                                                         // subnormal: m * 2^-24, normalised
    while (!(m & 0x400u)) { m <<= 1; ++k; }
    return sign | ((113u - k) << 23) | ((m & 0x3ffu) << 13);
}

// bf16 bits -> fp32 bits, exact
SSCC_FN uint32_t sscc_bf16_to_f32(uint16_t b) { return (uint32_t)b << 16; }
