// ssdnerf_amd/csrc/keyed_perm.h -- the keyed pseudo-random permutation that numbers the pixels of a training ray batch on the device
// (scene_store.hip: k_perm_indices, k_sample_rays_perm_u8; fitting.RayBatcher(index_source='device')).
//
// pi(seed, scene, draw, P) is a bijection of [0, P), 1 <= P < 2^32, that any lane evaluates at any position j on its own: no index array, no sort.
//
// Domain.  b is the smallest EVEN number >= 2 with 2^b >= P (so 2^b < 4 P), h = b / 2 (1 .. 16), m = 2^h - 1.  A value v of [0, 2^b) is the pair
//     L = v >> h,  R = v & m.
// Network.  A balanced Feistel network of SSKP_ROUNDS = 12 rounds on (L, R); round i = 0 .. 11 is
//     (L, R) <- (R, L ^ F(R, k[i])),         and afterwards  pihat(v) = (L << h) | R,
// a bijection of [0, 2^b) whatever F is.
// Round function.  On 32-bit unsigned integers, every operation modulo 2^32:
//     t = x + k;  t ^= t >> 16;  t *= 0x7FEB352D;  t ^= t >> 15;  t *= 0x846CA68B;  t ^= t >> 16;  F(x, k) = t & m
// (the two-multiply xor-shift finaliser "lowbias32" of C. Wellons' hash-prospector, applied to half + round key).
// Round keys.  k[4 q + e] = word e of the Philox4x32-10 block (philox.h: ssph_philox4x32_10) with
//     key     = the 64-bit seed, low word first
//     counter = {c0 = scene, c1 = draw, c2 = q, c3 = SSKP_TAG = 0x5045524D ("PERM")},      q = 0, 1, 2.
// The sampler's noise uses c3 = 0 (philox.h), so the two streams never meet, equal seeds included.  The keys depend on (seed, scene, draw) alone,
// not on P and not on the position.
// Cycle walking.  pi(j) for j < P:  v = pihat(j);  while (v >= P) v = pihat(v);  pi(j) = v.  pihat is a bijection, so j lies on a cycle of it and the
// walk from j comes back to j < P at the latest: it ends, and it ends on the first value below P.  Two positions cannot end on the same value (walk
// both backwards), so pi is a bijection of [0, P).  The walks of all j < P together evaluate pihat at most 2^b times -- once per element of the
// domain at the most -- so the mean number of evaluations per position is at most 2^b / P < 4.  P = 1 gives pi(0) = 0 (the walk from 0 ends on the
// only value below 1).
// Plain C on integers: compiled by hipcc into the kernels and by gcc into the CPU test's harness (tests/host/keyed_perm_host.c), the same bits by
// construction; tests/_perm_ref.py restates this text in numpy.
#pragma once
#include "philox.h"

#define SSKP_ROUNDS 12
#define SSKP_TAG 0x5045524Du

typedef struct { uint32_t k[SSKP_ROUNDS]; } sskp_keys;

#ifdef __HIPCC__
#define SSKP_HOST_FN __host__ __device__ __forceinline__       // the launcher works h out once and passes it in
#else
#define SSKP_HOST_FN static inline
#endif

// h = b / 2 for P in [1, 2^32): the smallest h >= 1 with 4^h >= P
SSKP_HOST_FN uint32_t sskp_half_bits(uint64_t P) {
    uint32_t h = 1;
    while (h < 16 && ((uint64_t)1 << (2 * h)) < P) ++h;
    return h;
}

SSPH_FN sskp_keys sskp_round_keys(uint64_t seed, uint32_t scene, uint32_t draw) {
    sskp_keys keys;
    for (uint32_t q = 0; q < SSKP_ROUNDS / 4; ++q) {
        const ssph_words w = ssph_philox4x32_10(scene, draw, q, SSKP_TAG, (uint32_t)seed, (uint32_t)(seed >> 32));
        for (int e = 0; e < 4; ++e) keys.k[4 * q + e] = w.r[e];
    }
    return keys;
}

SSPH_FN uint32_t sskp_mix(uint32_t t) {
    t ^= t >> 16;
    t *= 0x7FEB352Du;
    t ^= t >> 15;
    t *= 0x846CA68Bu;
    t ^= t >> 16;
    return t;
}

// pihat: one pass through the network, a bijection of [0, 4^h)
SSPH_FN uint32_t sskp_feistel(const sskp_keys* keys, uint32_t h, uint32_t v) {
    const uint32_t m = (1u << h) - 1u;
    uint32_t L = v >> h, R = v & m;
    for (int i = 0; i < SSKP_ROUNDS; ++i) {
        const uint32_t next = L ^ (sskp_mix(R + keys->k[i]) & m);
        L = R;
        R = next;
    }
    return (L << h) | R;
}

// pi(j), j < P; *evals (when not NULL) receives the number of passes the walk took
SSPH_FN uint32_t sskp_perm(const sskp_keys* keys, uint32_t h, uint32_t P, uint32_t j, uint32_t* evals) {
    uint32_t v = j, n = 0;
    do {
        v = sskp_feistel(keys, h, v);
        ++n;
    } while (v >= P);
    if (evals) *evals = n;
    return v;
}
