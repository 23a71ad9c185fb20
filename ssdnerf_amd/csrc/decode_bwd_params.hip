// ssdnerf_amd/csrc/decode_bwd_params.hip -- Part 2 of the C ABI, continued: the gradient of the point decode (decode.hip) w.r.t. the DECODER's parameters, all scenes
// of a batch in two launches, for gfx950.  It is a reduction over all samples (three small matrix products with K = samples); the arithmetic is decode_bwd_params_math.h.
//
//   k_decode_bwd_params      persistent blocks of four waves in a grid-stride loop over 256-sample groups; wave w of a block takes samples [64 w, 64 w + 64) of a group.
//                            STAGE 1, lane = sample: the samples WITH an upstream gradient (not the alignment padding, not the samples behind the T_thresh cut)
//                            re-gather their 18 features, evaluate the SH basis and run ssdb_heads (the hidden units once, to dL/dsa and dL/dz); they leave
//                            {f[18], SH[16], dsa, dz[3]} in the wave's own LDS rows, compacted in sample order.
//                            STAGE 2, the wave turns round, lane = hidden unit i: the lane holds its unit's 40 weights in registers and walks the wave's rows in order
//                            with broadcast LDS reads (every lane reads the same address); per sample it recomputes h_i and u_i (34 fmas, two sigmoids) and adds the
//                            sample's terms into SSDP_ACC = 44 register accumulators (ssdp_unit_add), which live across the whole loop.  Nothing but 40 floats per sample
//                            is staged: the per-(sample, unit) factors a_i + e_i, e_i, silu(h_i), silu(u_i) are formed where they are used.
//                            At the end the block's waves are added in wave order, ((w0 + w1) + w2) + w3, through one LDS image, and the block STORES one record of
//                            MLP_PARAM_FLOATS to partial[block] (every float of every record is written: nothing to zero-fill).
//   k_decode_bwd_params_sum  grad_params[e] = sum over the blocks, in block order.
//
// No floating-point atomics, neither global nor LDS.  The assignment of samples to blocks, waves and rows is static (group g -> block g mod gridDim.x) and every sum is
// formed in a fixed order: two calls on the same inputs with the same block count give the same bits.  Plain fp32 fmas: the arithmetic class of k_decode_bwd_feat.
#include "decode_core.h"
#include "decode_bwd_params_math.h"

static constexpr unsigned DBP_TPB = 256;
static constexpr unsigned DBP_WAVES = DBP_TPB / 64;
static constexpr unsigned DBP_ROW = 40;                       // floats per staged sample: f[18], SH[16], dsa, dz[3], two of padding (rows of whole float4)
static constexpr uint32_t DBP_MAX_BLOCKS = 4096;              // cap of max_blocks: 42 MB of partial records

// blocks of one launch: one per 256-sample group, at most max_blocks (0: two per compute unit)
static uint32_t dbp_blocks(uint32_t total, uint32_t max_blocks) {
    static int n_cu = 0;
    if (max_blocks == 0) {
        if (n_cu == 0) {
            int dev = 0;
            hipDeviceProp_t prop;
            n_cu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
        }
        max_blocks = (uint32_t)n_cu * 2u;
    }
    if (max_blocks > DBP_MAX_BLOCKS) max_blocks = DBP_MAX_BLOCKS;
    const uint32_t groups = ssd_blocks(total, DBP_TPB);
    return groups < max_blocks ? (groups ? groups : 1u) : max_blocks;
}

extern "C" size_t ssdnerf_point_decode_backward_params_workspace(uint32_t S, uint32_t total, uint32_t max_blocks) {
    (void)S;
    return (size_t)dbp_blocks(total, max_blocks) * SSDP_PARAM_FLOATS * sizeof(float);
}

// the scene of sample i: the last s with offsets[s] <= i (empty scenes share their offset with the next one and are never the answer)
SSD_DEV uint32_t dbp_scene_of(const uint32_t* __restrict__ offsets, uint32_t S, uint32_t i) {
    uint32_t lo = 0, hi = S;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

SSD_DEV void dbp_wave_sync() {                                // the wave's LDS rows change hands between its two stages (LDS instructions of a wave execute in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename PT>
__global__ void __launch_bounds__(DBP_TPB, 2) k_decode_bwd_params(const PT* __restrict__ planes, PlaneGeom g, uint64_t plane_stride, const float* __restrict__ P,
                                                                  const float* __restrict__ xyzs, const float* __restrict__ dirs,
                                                                  const uint32_t* __restrict__ offsets, uint32_t S, uint32_t total, float sat,
                                                                  const float* __restrict__ g_sigmas, const float* __restrict__ g_rgbs,
                                                                  float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float rows[DBP_WAVES][64][DBP_ROW];      // 40 KiB
    __shared__ float image[SSDP_ACC][64];                                             // 11 KiB: the running sum over the block's waves
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // stage 2's operands: the weights of hidden unit `lane`
    float rec[23], wd[16];
#pragma unroll
    for (int k = 0; k < 23; ++k) rec[k] = P[lane * 24 + k];
#pragma unroll
    for (int m = 0; m < 16; ++m) wd[m] = P[SSDB_OFF_WD + lane * 16 + m];
    const float bd = P[SSDB_OFF_BD + lane];
    float acc[SSDP_ACC];
#pragma unroll
    for (int q = 0; q < SSDP_ACC; ++q) acc[q] = 0.0f;
    float* const my_rows = &rows[wave][0][0];
    const uint32_t groups = (total + DBP_TPB - 1u) / DBP_TPB;
    for (uint32_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const uint32_t i = grp * DBP_TPB + threadIdx.x;
        float gs = 0.0f, gc[3] = {0.0f, 0.0f, 0.0f};
        if (i < total) {
            gs = g_sigmas ? g_sigmas[i] : 0.0f;
            gc[0] = g_rgbs[3ull * i]; gc[1] = g_rgbs[3ull * i + 1]; gc[2] = g_rgbs[3ull * i + 2];
        }
        const bool active = gs != 0.0f || gc[0] != 0.0f || gc[1] != 0.0f || gc[2] != 0.0f;
        const uint64_t am = __ballot(active);
        const uint32_t n = (uint32_t)__popcll(am);
        if (n == 0u) continue;                                                        // (wave-uniform; there is no block barrier inside the loop)
        if (active) {                                                                 // ---- stage 1: lane = sample
            const uint32_t scene = dbp_scene_of(offsets, S, i);
            float f[18], sh[16], dsa, dz[3];
            ssd_gather18<PT>(planes + scene * plane_stride, g, xyzs[3ull * i], xyzs[3ull * i + 1], xyzs[3ull * i + 2], f);
            shb::eval<4, false>(dirs[3ull * i], dirs[3ull * i + 1], dirs[3ull * i + 2], sh, nullptr, nullptr, nullptr);
            ssdb_heads(P, f, sh, sat, gs, gc, 1, &dsa, dz);
            const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(am >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)am, 0u));     // rank among the wave's samples with a gradient
            float4* dst = reinterpret_cast<float4*>(my_rows + slot * DBP_ROW);
            dst[0] = make_float4(f[0], f[1], f[2], f[3]);
            dst[1] = make_float4(f[4], f[5], f[6], f[7]);
            dst[2] = make_float4(f[8], f[9], f[10], f[11]);
            dst[3] = make_float4(f[12], f[13], f[14], f[15]);
            dst[4] = make_float4(f[16], f[17], dsa, dz[0]);
            dst[5] = make_float4(dz[1], dz[2], 0.0f, 0.0f);
            dst[6] = make_float4(sh[0], sh[1], sh[2], sh[3]);
            dst[7] = make_float4(sh[4], sh[5], sh[6], sh[7]);
            dst[8] = make_float4(sh[8], sh[9], sh[10], sh[11]);
            dst[9] = make_float4(sh[12], sh[13], sh[14], sh[15]);
        }
        dbp_wave_sync();
#pragma unroll 1
        for (uint32_t r = 0; r < n; ++r) {                                            // ---- stage 2: lane = hidden unit, the wave's rows in sample order
            const float4* src = reinterpret_cast<const float4*>(my_rows + r * DBP_ROW);
            const float4 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3], v4 = src[4], v5 = src[5], v6 = src[6], v7 = src[7], v8 = src[8], v9 = src[9];
            const float f[18] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w, v4.x, v4.y};
            const float sh[16] = {v6.x, v6.y, v6.z, v6.w, v7.x, v7.y, v7.z, v7.w, v8.x, v8.y, v8.z, v8.w, v9.x, v9.y, v9.z, v9.w};
            const float dz[3] = {v4.w, v5.x, v5.y};
            ssdp_unit_add(rec, wd, bd, f, sh, v4.z, dz, acc);
        }
        dbp_wave_sync();                                                              // (the next trip's stage 1 writes the rows this trip read)
    }
    // ---- the block's waves, added in wave order
#pragma unroll
    for (unsigned w = 0; w < DBP_WAVES; ++w) {
        if ((unsigned)wave == w) {
            if (w > 0) {
#pragma unroll
                for (int q = 0; q < SSDP_ACC; ++q) acc[q] = image[q][lane] + acc[q];
            }
            if (w + 1 < DBP_WAVES) {
#pragma unroll
                for (int q = 0; q < SSDP_ACC; ++q) image[q][lane] = acc[q];
            }
        }
        __syncthreads();
    }
    if ((unsigned)wave == DBP_WAVES - 1) ssdp_store_row(acc, lane, partial + (uint64_t)blockIdx.x * SSDP_PARAM_FLOATS);
}

__global__ void __launch_bounds__(DBP_TPB) k_decode_bwd_params_sum(const float* __restrict__ partial, uint32_t blocks, float* __restrict__ grad_params) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= SSDP_PARAM_FLOATS) return;
    float s = 0.0f;
#pragma unroll 8
    for (uint32_t b = 0; b < blocks; ++b) s += partial[(uint64_t)b * SSDP_PARAM_FLOATS + e];
    grad_params[e] = s;
}

extern "C" int ssdnerf_point_decode_backward_params(const void* planes, int planes_dtype, uint32_t S, uint32_t Hp, uint32_t Wp, const float* mlp_params,
                                                    const float* xyzs, const float* dirs, const uint32_t* offsets, uint32_t total, float sigmoid_saturation,
                                                    const float* grad_sigmas, const float* grad_rgbs, float* grad_params, uint32_t max_blocks, void* workspace,
                                                    size_t workspace_bytes, void* stream) {
    SSD_REQUIRE(grad_params, "point_decode_backward_params: null grad_params");
    hipStream_t s = (hipStream_t)stream;
    if (S == 0 || total == 0) {
        if (hipMemsetAsync(grad_params, 0, SSDP_PARAM_FLOATS * sizeof(float), s) != hipSuccess)
            return ssdnerf_fail(SSDNERF_E_LAUNCH, "point_decode_backward_params: memset failed");
        return SSDNERF_OK;
    }
    SSD_REQUIRE(Hp >= 1 && Wp >= 1 && Hp <= 32768 && Wp <= 32768, "point_decode_backward_params: plane size out of range");
    SSD_REQUIRE(total <= 0xffffff00u, "point_decode_backward_params: too many samples");
    SSD_REQUIRE(planes && mlp_params && xyzs && dirs && offsets && grad_rgbs && workspace, "point_decode_backward_params: null pointer");
    SSD_REQUIRE(planes_dtype == SSDNERF_DTYPE_F32 || planes_dtype == SSDNERF_DTYPE_F16, "point_decode_backward_params: unsupported plane dtype");
    const uint32_t blocks = dbp_blocks(total, max_blocks);
    if (workspace_bytes < (size_t)blocks * SSDP_PARAM_FLOATS * sizeof(float))
        return ssdnerf_fail(SSDNERF_E_WORKSPACE, "point_decode_backward_params: workspace too small");
    float* partial = (float*)workspace;
    const PlaneGeom g = ssd_plane_geom(Hp, Wp);
    const uint64_t plane_stride = (uint64_t)3 * Hp * Wp * 8;
    if (planes_dtype == SSDNERF_DTYPE_F32)
        hipLaunchKernelGGL((k_decode_bwd_params<float>), dim3(blocks), dim3(DBP_TPB), 0, s, (const float*)planes, g, plane_stride, mlp_params, xyzs, dirs, offsets, S, total,
                           sigmoid_saturation, grad_sigmas, grad_rgbs, partial);
    else
        hipLaunchKernelGGL((k_decode_bwd_params<__half>), dim3(blocks), dim3(DBP_TPB), 0, s, (const __half*)planes, g, plane_stride, mlp_params, xyzs, dirs, offsets, S, total,
                           sigmoid_saturation, grad_sigmas, grad_rgbs, partial);
    SSD_CHECK_LAUNCH("point_decode_backward_params (blocks)");
    hipLaunchKernelGGL(k_decode_bwd_params_sum, dim3(ssd_blocks(SSDP_PARAM_FLOATS, DBP_TPB)), dim3(DBP_TPB), 0, s, partial, blocks, grad_params);
    SSD_CHECK_LAUNCH("point_decode_backward_params (sum)");
    return SSDNERF_OK;
}
