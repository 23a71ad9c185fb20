/* tests/host/philox_host.c -- TEST INFRASTRUCTURE.  Host build (gcc) of the integer stream the device kernels k_philox_normal_fill / k_step_v
 * draw their normals from (ssdnerf_amd/csrc/philox.h). */
#include <stddef.h>
#include "../../ssdnerf_amd/csrc/philox.h"

/* one raw Philox4x32-10 block (the known-answer vectors) */
void philox_block(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
    const ssph_words w = ssph_philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    for (int k = 0; k < 4; ++k) out[k] = w.r[k];
}

/* the words of quads first .. first + n - 1 of one draw, [n][4] */
void quad_words(uint64_t seed, uint32_t draw, uint64_t first, size_t n, uint32_t* out) {
    for (size_t i = 0; i < n; ++i) {
        const ssph_words w = ssph_quad_words(seed, draw, first + i);
        for (int k = 0; k < 4; ++k) out[4 * i + k] = w.r[k];
    }
}

/* the 23 uniform bits of each word */
void uniform_bits(const uint32_t* r, uint32_t* m, size_t n) { for (size_t i = 0; i < n; ++i) m[i] = ssph_uniform_bits(r[i]); }
