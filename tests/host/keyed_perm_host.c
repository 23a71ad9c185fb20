/* tests/host/keyed_perm_host.c -- TEST INFRASTRUCTURE.  Host build (gcc) of the keyed permutation the device kernels k_perm_indices /
 * k_sample_rays_perm_u8 number their pixels with (ssdnerf_amd/csrc/keyed_perm.h). */
#include <stddef.h>
#include "../../ssdnerf_amd/csrc/keyed_perm.h"

uint32_t perm_rounds(void) { return SSKP_ROUNDS; }
uint32_t perm_half_bits(uint64_t P) { return sskp_half_bits(P); }

/* the round keys of one (seed, scene, draw) */
void perm_round_keys(uint64_t seed, uint32_t scene, uint32_t draw, uint32_t* out) {
    const sskp_keys keys = sskp_round_keys(seed, scene, draw);
    for (int i = 0; i < SSKP_ROUNDS; ++i) out[i] = keys.k[i];
}

/* out[r] = pi(seed, scene, draw, P)(start + r), r < n; evals[r] (when not NULL) the passes of that walk */
void perm_range(uint64_t seed, uint32_t scene, uint32_t draw, uint64_t P, uint64_t start, size_t n, int64_t* out, uint32_t* evals) {
    const sskp_keys keys = sskp_round_keys(seed, scene, draw);
    const uint32_t h = sskp_half_bits(P);
    for (size_t r = 0; r < n; ++r) out[r] = (int64_t)sskp_perm(&keys, h, (uint32_t)P, (uint32_t)(start + r), evals ? evals + r : NULL);
}

/* out[d][r] = pi(seed, scene, first_draw + d, P)(r), r < n: many draws of the leading positions (the statistics) */
void perm_draws(uint64_t seed, uint32_t scene, uint32_t first_draw, size_t draws, uint64_t P, size_t n, int64_t* out) {
    const uint32_t h = sskp_half_bits(P);
    for (size_t d = 0; d < draws; ++d) {
        const sskp_keys keys = sskp_round_keys(seed, scene, first_draw + (uint32_t)d);
        for (size_t r = 0; r < n; ++r) out[d * n + r] = (int64_t)sskp_perm(&keys, h, (uint32_t)P, (uint32_t)r, NULL);
    }
}
