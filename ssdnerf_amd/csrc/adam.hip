// ssdnerf_amd/csrc/adam.hip -- one Adam step of up to SSDNERF_ADAM_MAX_TENSORS fp32 tensors in ONE launch (the per-scene code leaves of
// stage-1 fitting and the decoder's weights: MultiSceneNeRF.train_step steps 8 scenes x 16 iterations, each of which used to be a handful of
// library kernels with their own dispatch).  The arithmetic of one element is csrc/adam_math.h; this file is the streaming pass around it.
//
// The table travels BY VALUE in the kernel arguments (56 bytes per tensor, 32 tensors: 1.9 KB, well inside the 4 KB a launch may carry): no device
// table, no copy, no allocation, no host synchronisation, nothing to keep alive after the call returns.
//
// Shape: a block of ADAM_THREADS lanes owns one chunk of ADAM_CHUNK consecutive elements of ONE tensor; the grid is the concatenation of
// every tensor's chunks (first_block[] is the prefix sum, a block finds its tensor by bisection over at most 5 wave-uniform steps), so one
// large and many small tensors share a launch.  A lane handles ADAM_GROUPS groups of 4 consecutive elements, ADAM_THREADS * 4 apart, and
// issues every load before the first use.  Where the tensor's four pointers are 16-byte aligned a group is one 16-byte load per array and
// one 16-byte store per written array (a chunk starts at a multiple of 4 elements, so a group never straddles the alignment); the last,
// partial group of such a tensor and every group of a tensor that is only 4-byte aligned go element by element under `i < numel`.
// Every array is read once, param / exp_avg / exp_avg_sq are written once, grad is never written, nothing outside [0, numel) is touched.
#include "common.h"
#include "adam_math.h"

#define ADAM_THREADS 256
#define ADAM_GROUPS 2
#define ADAM_CHUNK (ADAM_THREADS * 4 * ADAM_GROUPS)     // elements per block (2048)

struct AdamTable {
    ssdnerf_adam_tensor t[SSDNERF_ADAM_MAX_TENSORS];
    uint32_t first_block[SSDNERF_ADAM_MAX_TENSORS + 1];  // first_block[k] = blocks of tensors 0 .. k-1; entries past T repeat the total
    uint32_t T;
};

// four consecutive elements held as one 16-byte group per array
SSD_DEV void adam_step4(float4& p, const float4& g, float4& m, float4& v, const ssda_hyper h, float step_size, float bc2_sqrt, float wd) {
    float pa[4] = {p.x, p.y, p.z, p.w}, ma[4] = {m.x, m.y, m.z, m.w}, va[4] = {v.x, v.y, v.z, v.w};
    const float ga[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) ssda_step(&pa[c], ga[c], &ma[c], &va[c], h, step_size, bc2_sqrt, wd);
    p = make_float4(pa[0], pa[1], pa[2], pa[3]);
    m = make_float4(ma[0], ma[1], ma[2], ma[3]);
    v = make_float4(va[0], va[1], va[2], va[3]);
}

__global__ void __launch_bounds__(ADAM_THREADS) k_adam_multi(const AdamTable tab, const ssda_hyper h) {
    // the tensor of this block: the last k with first_block[k] <= blockIdx.x (wave-uniform: scalar loads from the argument segment)
    uint32_t lo = 0, hi = tab.T;                             // invariant: first_block[lo] <= blockIdx.x < first_block[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab.first_block[mid] <= blockIdx.x) lo = mid; else hi = mid;
    }
    const ssdnerf_adam_tensor e = tab.t[lo];
    const uint64_t numel = e.numel;
    const uint64_t base = (uint64_t)(blockIdx.x - tab.first_block[lo]) * ADAM_CHUNK;
    float* __restrict__ P = e.param;
    const float* __restrict__ G = e.grad;
    float* __restrict__ M = e.exp_avg;
    float* __restrict__ V = e.exp_avg_sq;
    const bool vec = (((uintptr_t)P | (uintptr_t)G | (uintptr_t)M | (uintptr_t)V) & 15u) == 0;

    if (vec) {
        float4 p[ADAM_GROUPS], g[ADAM_GROUPS], m[ADAM_GROUPS], v[ADAM_GROUPS];
        uint64_t i0[ADAM_GROUPS];
        bool full[ADAM_GROUPS];
#pragma unroll
        for (int k = 0; k < ADAM_GROUPS; ++k) {
            i0[k] = base + (uint64_t)(k * ADAM_THREADS + threadIdx.x) * 4;
            full[k] = i0[k] + 4 <= numel;
            if (full[k]) {
                p[k] = *reinterpret_cast<const float4*>(P + i0[k]);
                g[k] = *reinterpret_cast<const float4*>(G + i0[k]);
                m[k] = *reinterpret_cast<const float4*>(M + i0[k]);
                v[k] = *reinterpret_cast<const float4*>(V + i0[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < ADAM_GROUPS; ++k) {
            if (full[k]) {
                adam_step4(p[k], g[k], m[k], v[k], h, e.step_size, e.bc2_sqrt, e.weight_decay);
                *reinterpret_cast<float4*>(P + i0[k]) = p[k];
                *reinterpret_cast<float4*>(M + i0[k]) = m[k];
                *reinterpret_cast<float4*>(V + i0[k]) = v[k];
            } else {
                for (uint64_t i = i0[k]; i < numel && i < i0[k] + 4; ++i) {      // the tail of numel % 4 elements (one lane of one block)
                    float ps = P[i], ms = M[i], vs = V[i];
                    ssda_step(&ps, G[i], &ms, &vs, h, e.step_size, e.bc2_sqrt, e.weight_decay);
                    P[i] = ps; M[i] = ms; V[i] = vs;
                }
            }
        }
    } else {
        // 4-byte aligned only: consecutive lanes take consecutive elements
#pragma unroll
        for (int k = 0; k < ADAM_GROUPS * 4; ++k) {
            const uint64_t i = base + (uint64_t)(k * ADAM_THREADS + threadIdx.x);
            if (i < numel) {
                float ps = P[i], ms = M[i], vs = V[i];
                ssda_step(&ps, G[i], &ms, &vs, h, e.step_size, e.bc2_sqrt, e.weight_decay);
                P[i] = ps; M[i] = ms; V[i] = vs;
            }
        }
    }
}

extern "C" uint32_t ssdnerf_adam_max_tensors(void) { return SSDNERF_ADAM_MAX_TENSORS; }

extern "C" int ssdnerf_adam_step_multi(const ssdnerf_adam_tensor* tensors, uint32_t T, double beta1, double beta2, double eps, void* stream) {
    SSD_REQUIRE(tensors != nullptr, "adam_step_multi: null pointer (the table)");
    SSD_REQUIRE(T > 0, "adam_step_multi: T == 0 (no tensors)");
    SSD_REQUIRE(T <= SSDNERF_ADAM_MAX_TENSORS, "adam_step_multi: %u tensors, one call takes at most %u", T, (unsigned)SSDNERF_ADAM_MAX_TENSORS);
    AdamTable tab;
    uint64_t blocks = 0;
    for (uint32_t k = 0; k < T; ++k) {
        const ssdnerf_adam_tensor& e = tensors[k];
        SSD_REQUIRE(e.param && e.grad && e.exp_avg && e.exp_avg_sq, "adam_step_multi: null pointer in tensor %u", k);
        SSD_REQUIRE(e.numel > 0, "adam_step_multi: numel == 0 in tensor %u", k);
        SSD_REQUIRE(e.numel <= ((uint64_t)1 << 40), "adam_step_multi: tensor %u has more than 2^40 elements", k);
        SSD_REQUIRE((((uintptr_t)e.param | (uintptr_t)e.grad | (uintptr_t)e.exp_avg | (uintptr_t)e.exp_avg_sq) & 3u) == 0,
                    "adam_step_multi: tensor %u has a pointer that is not 4-byte aligned", k);
        tab.t[k] = e;
        tab.first_block[k] = (uint32_t)blocks;
        blocks += (e.numel + ADAM_CHUNK - 1) / ADAM_CHUNK;
        SSD_REQUIRE(blocks <= 0x7fffffffu, "adam_step_multi: more than 2^31 - 1 blocks of %u elements up to tensor %u", (unsigned)ADAM_CHUNK, k);
    }
    for (uint32_t k = T; k <= SSDNERF_ADAM_MAX_TENSORS; ++k) {
        if (k < SSDNERF_ADAM_MAX_TENSORS) tab.t[k] = ssdnerf_adam_tensor{};
        tab.first_block[k] = (uint32_t)blocks;
    }
    tab.T = T;
    const ssda_hyper h = ssda_make_hyper(beta1, beta2, eps);
    hipLaunchKernelGGL(k_adam_multi, dim3((uint32_t)blocks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, tab, h);
    SSD_CHECK_LAUNCH("adam_step_multi");
    return SSDNERF_OK;
}
