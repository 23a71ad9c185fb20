// ssdnerf_amd/csrc/philox.h -- the counter-based normal generator of the stochastic sampling steps (sampler_step.hip).
//
// Integer stream: Philox4x32-10 (Salmon et al. 2011, Random123) with the standard constants.  The key is the 64-bit seed, low word first.  The counter is
//     c0, c1   the low and high 32 bits of the quad index i4 (element i of the flattened latent belongs to quad i / 4)
//     c2       the draw index (0, 1, 2, ... in plan order within a sampling call)
//     c3       0 (reserved)
// so an element's noise depends on (seed, draw, its own index) alone: not on the launch shape, not on which kernel asks for it.
// Uniforms: u = ((r >> 9) + 0.5) 2^-23 -- 23 bits, exact in fp32, never 0 or 1.
// Normals: Box-Muller on the four words of a quad: (r0, r1) give elements 4 i4 and 4 i4 + 1 as R cos, R sin with R = sqrt(-2 ln u(r0)) and angle 2 pi u(r1);
// (r2, r3) give elements 4 i4 + 2 and 4 i4 + 3 in the same way.  |z| <= sqrt(-2 ln 2^-24) = 5.768.
// The integer part is plain C on integers: compiled by hipcc into the kernels and by gcc into the CPU test's harness (tests/host/philox_host.c), the same
// bits by construction.  The float part exists on the device only; tests/_philox_ref.py restates it in float64 and bounds the difference.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SSPH_FN __device__ __forceinline__
#else
#define SSPH_FN static inline
#endif

#define SSPH_M0 0xD2511F53u
#define SSPH_M1 0xCD9E8D57u
#define SSPH_W0 0x9E3779B9u
#define SSPH_W1 0xBB67AE85u

typedef struct { uint32_t r[4]; } ssph_words;

SSPH_FN uint32_t ssph_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

// Philox4x32-10: ten rounds, the key bumped between them
SSPH_FN ssph_words ssph_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = ssph_mulhi(SSPH_M0, c0), lo0 = SSPH_M0 * c0;
        const uint32_t hi1 = ssph_mulhi(SSPH_M1, c2), lo1 = SSPH_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += SSPH_W0;
        k1 += SSPH_W1;
    }
    ssph_words w;
    w.r[0] = c0; w.r[1] = c1; w.r[2] = c2; w.r[3] = c3;
    return w;
}

// the four words of quad i4 of draw `draw` under `seed`
SSPH_FN ssph_words ssph_quad_words(uint64_t seed, uint32_t draw, uint64_t i4) {
    return ssph_philox4x32_10((uint32_t)i4, (uint32_t)(i4 >> 32), draw, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// the 23 bits of a word that make its uniform: u = (m + 0.5) 2^-23
SSPH_FN uint32_t ssph_uniform_bits(uint32_t r) { return r >> 9; }

#ifdef __HIPCC__
// (m + 0.5) 2^-23: m < 2^23, so m + 0.5 has 24 significant bits and every step is exact
SSPH_FN float ssph_uniform(uint32_t m) { return ((float)m + 0.5f) * 0x1p-23f; }
// The three library functions of the normals, each behind one name so that tools/ubench/philox_ulp.hip measures exactly what the kernels call:
// ln u (u in (0, 1)), the square root of -2 ln u, and cos / sin of 2 pi u taken as cospi / sinpi of 2 u (2 u is exact; the reduction of the
// argument is exact too, so no rounded 2 pi enters).
SSPH_FN float ssph_log(float u) { return logf(u); }
SSPH_FN float ssph_sqrt(float t) { return sqrtf(t); }
SSPH_FN void ssph_sincos2pi(float u, float* s, float* c) { *s = sinpif(2.0f * u); *c = cospif(2.0f * u); }

// the four normals of quad i4: what ssdnerf_philox_normal_fill stores and what ssdnerf_sde_step_v adds, from this one function
SSPH_FN float4 ssph_normal4(uint64_t seed, uint32_t draw, uint64_t i4) {
    const ssph_words w = ssph_quad_words(seed, draw, i4);
    const float r0 = ssph_sqrt(-2.0f * ssph_log(ssph_uniform(ssph_uniform_bits(w.r[0]))));
    const float r1 = ssph_sqrt(-2.0f * ssph_log(ssph_uniform(ssph_uniform_bits(w.r[2]))));
    float s0, c0, s1, c1;
    ssph_sincos2pi(ssph_uniform(ssph_uniform_bits(w.r[1])), &s0, &c0);
    ssph_sincos2pi(ssph_uniform(ssph_uniform_bits(w.r[3])), &s1, &c1);
    float4 z;
    z.x = r0 * c0;
    z.y = r0 * s0;
    z.z = r1 * c1;
    z.w = r1 * s1;
    return z;
}
#endif
