// ssdnerf_amd/csrc/sampler_step.hip -- the per-step latent update of every sampling loop (diffusion.PlanStep) as ONE elementwise kernel template:
// the V-parameterised x0 prediction and clamp (reference: lib/models/diffusions/gaussian_diffusion.py:213, :235; ~10 eager PyTorch kernels and as
// many HBM round trips over the (S,18,128,128) latent per step there), the update of the plan step's kind, and -- in the instantiations that inject
// noise -- n z with z made in registers by the counter-based generator of philox.h.  k_philox_normal_fill stores the same z for the branches that
// stay in tensor expressions (guidance, save_intermediates): one inline function serves both, so the two consume bit-identical noise.  The
// DPM-Solver++ and device-noise steps are not in the reference (DESIGN.md sections 20 and 22); the coefficients come from diffusion.SamplingPlan
// as host floats.
// HBM-bound streaming: 8 B read (12 B with a history term) + 8 B written per element, float4 per lane; the generator costs VALU work only (ten
// Philox rounds, two logarithms, two square roots and two sine / cosine pairs per quad) and no memory traffic: z is never stored by the step.
#include "common.h"
#include "philox.h"

#define SSD_STEP_BLOCK_CAP 2048u      /* 256 CUs x 8 blocks of 256 lanes; the grid-stride loop takes the rest (tests/test_dpmpp_gpu.py and tests/test_sde_gpu.py size their last case by it) */

static inline unsigned step_blocks(uint64_t n4) { return (unsigned)((n4 + 255) / 256 < SSD_STEP_BLOCK_CAP ? (n4 + 255) / 256 : SSD_STEP_BLOCK_CAP); }

__global__ void k_philox_normal_fill(float4* out, uint64_t n4, uint64_t seed, uint32_t draw) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) out[i] = ssph_normal4(seed, draw, i);
}

// (no __restrict__: the sampling loop runs this in place, xnext_out == x_t and, when x0 is not kept, x0_out == v; element i is read before it is
//  written.  x0_prev is another buffer than x0_out: the host refuses the call otherwise.)
// FORM 0: c p + d eps [+ nz z]        ('ddim';  eps = (x_t - a p) / b)
// FORM 1: x_t - d eps [+ nz z]        ('langevin')
// FORM 2: c p + d x_t + e q [+ nz z]  ('ddpm', 'dpmpp', 'dpmpp_sde'); HAS_PREV = false: e == 0, x0_prev is not read and may be NULL
// NOISE = false: the generator is not evaluated and nothing is added (not + 0 z: that would turn a -0 sum into +0 and an infinite z into NaN)
template <int FORM, bool HAS_PREV, bool NOISE>
__global__ void k_step_v(const float4* x_t, const float4* v, const float4* x0_prev, uint64_t n4, float a, float b, float inv_b, float c, float d,
                         float e, float nz, float lo, float hi, uint64_t seed, uint32_t draw, float4* x0_out, float4* xnext_out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 xt = x_t[i], vv = v[i];
        float4 q = {0.0f, 0.0f, 0.0f, 0.0f}, zz = {0.0f, 0.0f, 0.0f, 0.0f};
        if (HAS_PREV) q = x0_prev[i];
        if (NOISE) zz = ssph_normal4(seed, draw, i);
        float4 x0, xn;
#define SSD_STEP_LANE(f)                                                                              \
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
            if (NOISE) s = s + nz * zz.f;                                                             \
            x0.f = p;                                                                                 \
            xn.f = s;                                                                                 \
        }
        SSD_STEP_LANE(x) SSD_STEP_LANE(y) SSD_STEP_LANE(z) SSD_STEP_LANE(w)
#undef SSD_STEP_LANE
        x0_out[i] = x0;
        xnext_out[i] = xn;
    }
}

// the argument checks every step entry shares (the messages name the entry), then one launch of the instantiation (form, e != 0, noise) selects;
// only the seven combinations the three entries can ask for are instantiated
static int step_launch(const char* entry, int form, bool noise, const float* x_t, const float* v, const float* x0_prev, uint64_t n, float a, float b,
                       float c, float d, float e, float nz, float lo, float hi, uint64_t seed, uint32_t draw, float* x0_out, float* xnext_out,
                       void* stream) {
    if (n == 0) return SSDNERF_OK;
    SSD_REQUIRE(x_t && v && x0_out && xnext_out, "%s: null pointer", entry);
    SSD_REQUIRE(n % 4 == 0, "%s: element count must be a multiple of 4 (latents are (S,18,128,128))", entry);
    SSD_REQUIRE(form >= 0 && form <= 2, "%s: form must be 0 (ddim), 1 (langevin) or 2 (ddpm / dpmpp_sde), not %d", entry, form);
    SSD_REQUIRE(x0_prev || e == 0.0f, "%s: x0_prev may be NULL only when e == 0 (a first-order step reads no history)", entry);
    SSD_REQUIRE(x0_out != x0_prev, "%s: x0_out must not alias x0_prev (the two history buffers alternate)", entry);
    const uint64_t n4 = n / 4;
    const dim3 grid(step_blocks(n4)), block(256);
    const float inv_b = 1.0f / b;
#define SSD_STEP_LAUNCH(FORM, HAS_PREV, NOISE)                                                                                                      \
    hipLaunchKernelGGL((k_step_v<FORM, HAS_PREV, NOISE>), grid, block, 0, (hipStream_t)stream, (const float4*)x_t, (const float4*)v,               \
                       (const float4*)(HAS_PREV ? x0_prev : nullptr), n4, a, b, inv_b, c, d, e, nz, lo, hi, seed, draw, (float4*)x0_out,           \
                       (float4*)xnext_out)
    if (form == 1) SSD_STEP_LAUNCH(1, false, true);
    else if (form == 0 && noise) SSD_STEP_LAUNCH(0, false, true);
    else if (form == 0) SSD_STEP_LAUNCH(0, false, false);
    else if (noise && e != 0.0f) SSD_STEP_LAUNCH(2, true, true);
    else if (noise) SSD_STEP_LAUNCH(2, false, true);
    else if (e != 0.0f) SSD_STEP_LAUNCH(2, true, false);
    else SSD_STEP_LAUNCH(2, false, false);
#undef SSD_STEP_LAUNCH
    SSD_CHECK_LAUNCH(entry);
    return SSDNERF_OK;
}

extern "C" uint32_t ssdnerf_dpmpp_block_cap(void) { return SSD_STEP_BLOCK_CAP; }
extern "C" uint32_t ssdnerf_sde_block_cap(void) { return SSD_STEP_BLOCK_CAP; }

extern "C" int ssdnerf_philox_normal_fill(float* out, uint64_t n, uint64_t seed, uint32_t draw, void* stream) {
    if (n == 0) return SSDNERF_OK;
    SSD_REQUIRE(out, "philox_normal_fill: null pointer");
    SSD_REQUIRE(n % 4 == 0, "philox_normal_fill: element count must be a multiple of 4 (a Philox block makes four normals)");
    const uint64_t n4 = n / 4;
    hipLaunchKernelGGL(k_philox_normal_fill, dim3(step_blocks(n4)), dim3(256), 0, (hipStream_t)stream, (float4*)out, n4, seed, draw);
    SSD_CHECK_LAUNCH("philox_normal_fill");
    return SSDNERF_OK;
}

// form 0, no history, no noise
extern "C" int ssdnerf_ddim_step_v(const float* x_t, const float* v, uint64_t n, float sqrt_ab, float sqrt_1mab, float sqrt_ab_prev, float dir_coef,
                                   float clip_lo, float clip_hi, float* x0_out, float* xprev_out, void* stream) {
    return step_launch("ddim_step_v", 0, false, x_t, v, nullptr, n, sqrt_ab, sqrt_1mab, sqrt_ab_prev, dir_coef, 0.0f, 0.0f, clip_lo, clip_hi, 0, 0,
                       x0_out, xprev_out, stream);
}

// form 2, no noise
extern "C" int ssdnerf_dpmpp_step_v(const float* x_t, const float* v, const float* x0_prev, uint64_t n, float sqrt_ab, float sqrt_1mab, float c,
                                    float d, float e, float clip_lo, float clip_hi, float* x0_out, float* xnext_out, void* stream) {
    return step_launch("dpmpp_step_v", 2, false, x_t, v, x0_prev, n, sqrt_ab, sqrt_1mab, c, d, e, 0.0f, clip_lo, clip_hi, 0, 0, x0_out, xnext_out,
                       stream);
}

extern "C" int ssdnerf_sde_step_v(const float* x_t, const float* v, const float* x0_prev, uint64_t n, int form, float sqrt_ab, float sqrt_1mab, float c,
                                  float d, float e, float nz, float clip_lo, float clip_hi, uint64_t seed, uint32_t draw, float* x0_out,
                                  float* xnext_out, void* stream) {
    return step_launch("sde_step_v", form, true, x_t, v, x0_prev, n, sqrt_ab, sqrt_1mab, c, d, e, nz, clip_lo, clip_hi, seed, draw, x0_out,
                       xnext_out, stream);
}
