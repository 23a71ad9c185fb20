/* tests/host/decode_bwd_params_host.c -- TEST INFRASTRUCTURE.  Host build (gcc) of the arithmetic the device kernel k_decode_bwd_params runs
 * (ssdnerf_amd/csrc/decode_bwd_params_math.h), so that the CPU test suite can check it against the float64 reference and PyTorch autograd without a GPU. */
#include "../../ssdnerf_amd/csrc/decode_bwd_params_math.h"

/* planes (3,Hp,Wp,8) fp32 of ONE scene, P packed decoder parameters, xyzs (n,3), shs (n,16) SH values of the view directions, g_sigmas (n), g_rgbs (n,3)
 * -> grad (SSDP_PARAM_FLOATS, packed layout) ADDED to in place (one call per scene).  Samples whose upstream gradient is all zero are skipped, as the kernel skips them;
 * the samples are added in order, every hidden unit's accumulators as one lane of the kernel holds them. */
void decode_bwd_params_points(const float* planes, uint32_t Hp, uint32_t Wp, const float* P, const float* xyzs, const float* shs, uint32_t n, float sat,
                              const float* g_sigmas, const float* g_rgbs, float* grad) {
    static float acc[64][SSDP_ACC];
    float scene[SSDP_PARAM_FLOATS];
    for (int i = 0; i < 64; ++i)
        for (int q = 0; q < SSDP_ACC; ++q) acc[i][q] = 0.0f;
    for (uint32_t s = 0; s < n; ++s) {
        const float gs = g_sigmas[s], *gc = g_rgbs + 3 * (uint64_t)s;
        if (gs == 0.0f && gc[0] == 0.0f && gc[1] == 0.0f && gc[2] == 0.0f) continue;
        float f[18], dsa, dz[3];
        const float* sh = shs + 16 * (uint64_t)s;
        ssdb_gather18(planes, Hp, Wp, xyzs[3 * s], xyzs[3 * s + 1], xyzs[3 * s + 2], f);
        ssdb_heads(P, f, sh, sat, gs, gc, 1, &dsa, dz);
        for (int i = 0; i < 64; ++i) ssdp_unit_add(P + i * 24, P + SSDB_OFF_WD + i * 16, P[SSDB_OFF_BD + i], f, sh, dsa, dz, acc[i]);
    }
    for (int i = 0; i < 64; ++i) ssdp_store_row(acc[i], i, scene);
    for (int e = 0; e < SSDP_PARAM_FLOATS; ++e) grad[e] += scene[e];
}
