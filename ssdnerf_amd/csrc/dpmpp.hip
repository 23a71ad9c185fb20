// ssdnerf_amd/csrc/dpmpp.hip -- the per-step latent update of the DPM-Solver++(2M) loop (Lu et al. 2022, data prediction, multistep) as one
// elementwise kernel: the same x0 prediction and clamp as k_ddim_step_v (ddim.hip), then a three-term combination that also reads the
// x0 of the step before.  Nothing in the reference does this (the DPM-Solver++ section); the coefficients come from
// diffusion.SamplingPlan as host floats.
// HBM-bound streaming: 12 B read + 8 B written per element (8 B read on a first-order step), float4 per lane.
#include "common.h"

#define SSD_DPMPP_BLOCK_CAP 2048u     /* 256 CUs x 8 blocks of 256 lanes; the grid-stride loop takes the rest (tests/test_dpmpp_gpu.py sizes its last case by it) */

// (no __restrict__: the sampling loop runs this in place, xnext_out == x_t and, when x0 is not kept, x0_out == v; element i is read before it is
//  written.  x0_prev is another buffer than x0_out: the host refuses the call otherwise.)
// HAS_PREV = false: a first-order step (e == 0), x0_prev is not read and may be NULL.
template <bool HAS_PREV>
__global__ void k_dpmpp_step_v(const float4* x_t, const float4* v, const float4* x0_prev, uint64_t n4, float a, float b, float c, float d,
                               float e, float lo, float hi, float4* x0_out, float4* xnext_out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 xt = x_t[i], vv = v[i];
        float4 q = {0.0f, 0.0f, 0.0f, 0.0f};
        if (HAS_PREV) q = x0_prev[i];
        float4 x0, xn;
#define SSD_DPMPP_LANE(f)                                                                             \
        {                                                                                             \
            float p = a * xt.f - b * vv.f;               /* x0 = sqrt(ab) x_t - sqrt(1-ab) v      */ \
            p = fminf(fmaxf(p, lo), hi);                 /* clip_denoised                         */ \
            float s = c * p + d * xt.f;                  /* a_prev phi (1 + 1/2r) x0 + (b_prev / b) x_t */ \
            if (HAS_PREV) s = s + e * q.f;               /* - a_prev phi / 2r  x0 of the step before  */ \
            x0.f = p;                                                                                 \
            xn.f = s;                                                                                 \
        }
        SSD_DPMPP_LANE(x) SSD_DPMPP_LANE(y) SSD_DPMPP_LANE(z) SSD_DPMPP_LANE(w)
#undef SSD_DPMPP_LANE
        x0_out[i] = x0;
        xnext_out[i] = xn;
    }
}

extern "C" uint32_t ssdnerf_dpmpp_block_cap(void) { return SSD_DPMPP_BLOCK_CAP; }

extern "C" int ssdnerf_dpmpp_step_v(const float* x_t, const float* v, const float* x0_prev, uint64_t n, float sqrt_ab, float sqrt_1mab, float c,
                                    float d, float e, float clip_lo, float clip_hi, float* x0_out, float* xnext_out, void* stream) {
    if (n == 0) return SSDNERF_OK;
    SSD_REQUIRE(x_t && v && x0_out && xnext_out, "dpmpp_step_v: null pointer");
    SSD_REQUIRE(n % 4 == 0, "dpmpp_step_v: element count must be a multiple of 4 (latents are (S,18,128,128))");
    SSD_REQUIRE(x0_prev || e == 0.0f, "dpmpp_step_v: x0_prev may be NULL only when e == 0 (a first-order step reads no history)");
    SSD_REQUIRE(x0_out != x0_prev, "dpmpp_step_v: x0_out must not alias x0_prev (the two history buffers alternate)");
    const uint64_t n4 = n / 4;
    const unsigned blocks = (unsigned)((n4 + 255) / 256 < SSD_DPMPP_BLOCK_CAP ? (n4 + 255) / 256 : SSD_DPMPP_BLOCK_CAP);
    if (e != 0.0f)
        hipLaunchKernelGGL(k_dpmpp_step_v<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)x_t, (const float4*)v,
                           (const float4*)x0_prev, n4, sqrt_ab, sqrt_1mab, c, d, e, clip_lo, clip_hi, (float4*)x0_out, (float4*)xnext_out);
    else
        hipLaunchKernelGGL(k_dpmpp_step_v<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)x_t, (const float4*)v,
                           (const float4*)nullptr, n4, sqrt_ab, sqrt_1mab, c, d, e, clip_lo, clip_hi, (float4*)x0_out, (float4*)xnext_out);
    SSD_CHECK_LAUNCH("dpmpp_step_v");
    return SSDNERF_OK;
}
