// ssdnerf_amd/csrc/sde_step.hip -- the sampling steps that inject noise, as one elementwise kernel each, with the noise made in registers:
// the x0 prediction and clamp of k_dpmpp_step_v (dpmpp.hip), the update of the plan step's kind (diffusion.PlanStep), and n z with z from the
// counter-based generator of philox.h.  k_philox_normal_fill stores the same z for the branches that stay in tensor expressions (guidance,
// save_intermediates) -- one inline function serves both, so the two consume bit-identical noise.  Nothing in the reference does this (DESIGN.md,
// section 22); the coefficients come from diffusion.SamplingPlan as host floats.
// Streaming: 8 or 12 B read + 8 B written per element like the deterministic steps, float4 per lane; the generator costs VALU work only (ten Philox
// rounds, two logarithms, two square roots and two sine / cosine pairs per quad) and no memory traffic: z is never stored by the step.
#include "common.h"
#include "philox.h"

#define SSD_SDE_BLOCK_CAP 2048u       /* 256 CUs x 8 blocks of 256 lanes; the grid-stride loop takes the rest (tests/test_sde_gpu.py sizes its last case by it) */

__global__ void k_philox_normal_fill(float4* out, uint64_t n4, uint64_t seed, uint32_t draw) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) out[i] = ssph_normal4(seed, draw, i);
}

// (no __restrict__: the sampling loop runs this in place, xnext_out == x_t and, when x0 is not kept, x0_out == v; element i is read before it is
//  written.  x0_prev is another buffer than x0_out: the host refuses the call otherwise.)
// FORM 0: c p + d eps + nz z      ('ddim' with eta > 0;  eps = (x_t - a p) / b, as k_ddim_step_v forms it)
// FORM 1: x_t - d eps + nz z      ('langevin')
// FORM 2: c p + d x_t + e q + nz z  ('ddpm', 'dpmpp_sde'); HAS_PREV = false: e == 0, x0_prev is not read and may be NULL
template <int FORM, bool HAS_PREV>
__global__ void k_sde_step_v(const float4* x_t, const float4* v, const float4* x0_prev, uint64_t n4, float a, float b, float inv_b, float c, float d,
                             float e, float nz, float lo, float hi, uint64_t seed, uint32_t draw, float4* x0_out, float4* xnext_out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 xt = x_t[i], vv = v[i];
        float4 q = {0.0f, 0.0f, 0.0f, 0.0f};
        if (HAS_PREV) q = x0_prev[i];
        const float4 zz = ssph_normal4(seed, draw, i);
        float4 x0, xn;
#define SSD_SDE_LANE(f)                                                                               \
        {                                                                                             \
            float p = a * xt.f - b * vv.f;               /* x0 = sqrt(ab) x_t - sqrt(1-ab) v      */ \
            p = fminf(fmaxf(p, lo), hi);                 /* clip_denoised                         */ \
            float s;                                                                                  \
            if (FORM == 2) {                                                                          \
                s = c * p + d * xt.f;                                                                 \
                if (HAS_PREV) s = s + e * q.f;                                                        \
            } else {                                                                                  \
                const float eps = (xt.f - a * p) * inv_b; /* (x_t - sqrt(ab) x0) / sqrt(1-ab)     */ \
                s = FORM == 0 ? c * p + d * eps : xt.f - d * eps;                                     \
            }                                                                                         \
            x0.f = p;                                                                                 \
            xn.f = s + nz * zz.f;                                                                     \
        }
        SSD_SDE_LANE(x) SSD_SDE_LANE(y) SSD_SDE_LANE(z) SSD_SDE_LANE(w)
#undef SSD_SDE_LANE
        x0_out[i] = x0;
        xnext_out[i] = xn;
    }
}

static inline unsigned sde_blocks(uint64_t n4) { return (unsigned)((n4 + 255) / 256 < SSD_SDE_BLOCK_CAP ? (n4 + 255) / 256 : SSD_SDE_BLOCK_CAP); }

extern "C" uint32_t ssdnerf_sde_block_cap(void) { return SSD_SDE_BLOCK_CAP; }

extern "C" int ssdnerf_philox_normal_fill(float* out, uint64_t n, uint64_t seed, uint32_t draw, void* stream) {
    if (n == 0) return SSDNERF_OK;
    SSD_REQUIRE(out, "philox_normal_fill: null pointer");
    SSD_REQUIRE(n % 4 == 0, "philox_normal_fill: element count must be a multiple of 4 (a Philox block makes four normals)");
    const uint64_t n4 = n / 4;
    hipLaunchKernelGGL(k_philox_normal_fill, dim3(sde_blocks(n4)), dim3(256), 0, (hipStream_t)stream, (float4*)out, n4, seed, draw);
    SSD_CHECK_LAUNCH("philox_normal_fill");
    return SSDNERF_OK;
}

extern "C" int ssdnerf_sde_step_v(const float* x_t, const float* v, const float* x0_prev, uint64_t n, int form, float sqrt_ab, float sqrt_1mab, float c,
                                  float d, float e, float nz, float clip_lo, float clip_hi, uint64_t seed, uint32_t draw, float* x0_out,
                                  float* xnext_out, void* stream) {
    if (n == 0) return SSDNERF_OK;
    SSD_REQUIRE(x_t && v && x0_out && xnext_out, "sde_step_v: null pointer");
    SSD_REQUIRE(n % 4 == 0, "sde_step_v: element count must be a multiple of 4 (latents are (S,18,128,128))");
    SSD_REQUIRE(form >= 0 && form <= 2, "sde_step_v: form must be 0 (ddim), 1 (langevin) or 2 (ddpm / dpmpp_sde), not %d", form);
    SSD_REQUIRE(x0_prev || e == 0.0f, "sde_step_v: x0_prev may be NULL only when e == 0 (a first-order step reads no history)");
    SSD_REQUIRE(x0_out != x0_prev, "sde_step_v: x0_out must not alias x0_prev (the two history buffers alternate)");
    const uint64_t n4 = n / 4;
    const dim3 grid(sde_blocks(n4)), block(256);
    const float inv_b = 1.0f / sqrt_1mab;
#define SSD_SDE_LAUNCH(FORM, HAS_PREV)                                                                                                              \
    hipLaunchKernelGGL((k_sde_step_v<FORM, HAS_PREV>), grid, block, 0, (hipStream_t)stream, (const float4*)x_t, (const float4*)v,                  \
                       (const float4*)(HAS_PREV ? x0_prev : nullptr), n4, sqrt_ab, sqrt_1mab, inv_b, c, d, e, nz, clip_lo, clip_hi, seed, draw,    \
                       (float4*)x0_out, (float4*)xnext_out)
    if (form == 0) SSD_SDE_LAUNCH(0, false);
    else if (form == 1) SSD_SDE_LAUNCH(1, false);
    else if (e != 0.0f) SSD_SDE_LAUNCH(2, true);
    else SSD_SDE_LAUNCH(2, false);
#undef SSD_SDE_LAUNCH
    SSD_CHECK_LAUNCH("sde_step_v");
    return SSDNERF_OK;
}
