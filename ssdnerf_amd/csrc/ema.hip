// ssdnerf_amd/csrc/ema.hip -- the EMA copies of denoiser and decoder (the reference's ExponentialMovingAverageHook, interp_mode='lerp') updated
// in ONE launch: every entry of every (source, EMA) module pair on a device.  The arithmetic of one element is csrc/ema_math.h; this file is the
// streaming pass around it and the host-side check of the table.
//
// The cars denoiser alone has several hundred tensors, far past the 32 rows that adam.hip carries by value in the kernel arguments, and the
// (source, EMA) pairs do not change from iteration to iteration.  So the rows live in a DEVICE-RESIDENT PLAN: an array of ssdnerf_ema_row
// in memory the caller owns, validated and completed (first_block, the prefix sum of the rows' block counts) ONCE on the host by
// ssdnerf_ema_plan_build, uploaded by the caller, and read by every launch.  The library allocates no device memory and keeps nothing.
//
// Shape (adam.hip's): a block of EMA_THREADS lanes owns one chunk of EMA_CHUNK consecutive elements of ONE row; the grid is the concatenation
// of every row's chunks, and a block finds its row by bisection over first_block (wave-uniform loads; ~9 steps for 300 rows, the whole plan
// stays in the scalar cache).  A lane handles EMA_GROUPS groups of 4 consecutive elements, EMA_THREADS * 4 apart, and issues every load
// before the first use.  Where src and dst are both 16-byte aligned a group is one 16-byte load per array and one 16-byte store (a chunk
// starts at a multiple of 4 elements, so a group never straddles the alignment); the last, partial group of such a row and every group of a
// row that is only 4-byte aligned go element by element under `i < numel`.  src is never written; nothing outside [0, numel) is touched.
#include <algorithm>
#include <vector>

#include "common.h"
#include "ema_math.h"

#define EMA_THREADS 256
#define EMA_GROUPS 4
#define EMA_CHUNK (EMA_THREADS * 4 * EMA_GROUPS)        // elements per block (4096)

// The rows' pointers come out of memory, so the compiler cannot tell they are global addresses and would emit flat loads and stores; they are
// device allocations by contract (include/ssdnerf_hip.h), hence the address-space casts below (global_load / global_store).
#define EMA_GLOBAL __attribute__((address_space(1)))
typedef float ema_f4 __attribute__((ext_vector_type(4)));

static_assert(sizeof(ssdnerf_ema_row) == 32, "ssdnerf_ema_row is 32 bytes (ssdnerf_amd/_cabi.py EmaRow)");

__global__ void __launch_bounds__(EMA_THREADS) k_ema_multi(const ssdnerf_ema_row* __restrict__ plan, uint32_t T, float m_trainable, float m_other) {
    // the row of this block: the last k with first_block[k] <= blockIdx.x (the grid is exactly the plan's block count, so one exists)
    uint32_t lo = 0, hi = T;                                 // invariant: first_block[lo] <= blockIdx.x, and blockIdx.x < first_block[hi] where hi < T
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (plan[mid].first_block <= blockIdx.x) lo = mid; else hi = mid;
    }
    const ssdnerf_ema_row e = plan[lo];
    const uint64_t numel = e.numel;
    const uint64_t base = (uint64_t)(blockIdx.x - e.first_block) * EMA_CHUNK;
    if (base >= numel) return;                               // (never with a plan from ssdnerf_ema_plan_build and its block count)
    const float m = e.trainable ? m_trainable : m_other;
    const EMA_GLOBAL float* __restrict__ S = (const EMA_GLOBAL float*)e.src;
    EMA_GLOBAL float* __restrict__ D = (EMA_GLOBAL float*)e.dst;

    if ((((uintptr_t)S | (uintptr_t)D) & 15u) == 0) {
        ema_f4 s[EMA_GROUPS], d[EMA_GROUPS];
        uint64_t i0[EMA_GROUPS];
        bool full[EMA_GROUPS];
#pragma unroll
        for (int k = 0; k < EMA_GROUPS; ++k) {
            i0[k] = base + (uint64_t)(k * EMA_THREADS + threadIdx.x) * 4;
            full[k] = i0[k] + 4 <= numel;
            if (full[k]) {
                s[k] = *(const EMA_GLOBAL ema_f4*)(S + i0[k]);
                d[k] = *(const EMA_GLOBAL ema_f4*)(D + i0[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < EMA_GROUPS; ++k) {
            if (full[k]) {
                ema_f4 o;
                o.x = ssde_update(d[k].x, s[k].x, m);
                o.y = ssde_update(d[k].y, s[k].y, m);
                o.z = ssde_update(d[k].z, s[k].z, m);
                o.w = ssde_update(d[k].w, s[k].w, m);
                *(EMA_GLOBAL ema_f4*)(D + i0[k]) = o;
            } else {
                for (uint64_t i = i0[k]; i < numel && i < i0[k] + 4; ++i) D[i] = ssde_update(D[i], S[i], m);   // the tail of numel % 4 elements
            }
        }
    } else {
        // 4-byte aligned only: consecutive lanes take consecutive elements
        float s[EMA_GROUPS * 4], d[EMA_GROUPS * 4];
#pragma unroll
        for (int k = 0; k < EMA_GROUPS * 4; ++k) {
            const uint64_t i = base + (uint64_t)(k * EMA_THREADS + threadIdx.x);
            if (i < numel) { s[k] = S[i]; d[k] = D[i]; }
        }
#pragma unroll
        for (int k = 0; k < EMA_GROUPS * 4; ++k) {
            const uint64_t i = base + (uint64_t)(k * EMA_THREADS + threadIdx.x);
            if (i < numel) D[i] = ssde_update(d[k], s[k], m);
        }
    }
}

extern "C" uint32_t ssdnerf_ema_chunk(void) { return EMA_CHUNK; }

namespace {
struct EmaSpan { uintptr_t begin, end; uint32_t row; bool is_dst; };
}

extern "C" int ssdnerf_ema_plan_build(ssdnerf_ema_row* rows, uint32_t T, uint32_t* blocks_out) {
    SSD_REQUIRE(rows != nullptr && blocks_out != nullptr, "ema_plan_build: null pointer (the rows or blocks_out)");
    SSD_REQUIRE(T > 0, "ema_plan_build: T == 0 (no rows)");
    SSD_REQUIRE(T <= SSDNERF_EMA_MAX_ROWS, "ema_plan_build: %u rows, a plan holds at most %u", T, (unsigned)SSDNERF_EMA_MAX_ROWS);
    uint64_t blocks = 0;
    for (uint32_t k = 0; k < T; ++k) {
        const ssdnerf_ema_row& e = rows[k];
        SSD_REQUIRE(e.src && e.dst, "ema_plan_build: null pointer in row %u", k);
        SSD_REQUIRE(e.numel > 0, "ema_plan_build: numel == 0 in row %u", k);
        SSD_REQUIRE(e.numel <= ((uint64_t)1 << 40), "ema_plan_build: row %u has more than 2^40 elements", k);
        SSD_REQUIRE((((uintptr_t)e.src | (uintptr_t)e.dst) & 3u) == 0, "ema_plan_build: row %u has a pointer that is not 4-byte aligned", k);
        SSD_REQUIRE(e.trainable <= 1u, "ema_plan_build: row %u has trainable = %u (0 or 1)", k, e.trainable);
        blocks += (e.numel + EMA_CHUNK - 1) / EMA_CHUNK;
        SSD_REQUIRE(blocks <= 0x7fffffffu, "ema_plan_build: more than 2^31 - 1 blocks of %u elements up to row %u", (unsigned)EMA_CHUNK, k);
    }
    // a written range may meet no other range: sweep the 2 T byte ranges in address order, remembering how far the ranges seen so far reach
    std::vector<EmaSpan> spans;
    spans.reserve((size_t)T * 2);
    for (uint32_t k = 0; k < T; ++k) {
        const uintptr_t s = (uintptr_t)rows[k].src, d = (uintptr_t)rows[k].dst;
        spans.push_back({s, s + (uintptr_t)rows[k].numel * 4, k, false});
        spans.push_back({d, d + (uintptr_t)rows[k].numel * 4, k, true});
    }
    std::sort(spans.begin(), spans.end(), [](const EmaSpan& a, const EmaSpan& b) { return a.begin != b.begin ? a.begin < b.begin : a.row < b.row; });
    uintptr_t dst_end = 0, src_end = 0, dst_begin = 0;      // the furthest end of the dst / src ranges that start at or before the current one
    uint32_t dst_row = 0, src_row = 0;
    bool have_dst = false;
    for (const EmaSpan& sp : spans) {
        if (sp.is_dst) {
            SSD_REQUIRE(!(have_dst && dst_begin == sp.begin), "ema_plan_build: rows %u and %u have the same dst (a dst appears twice)", dst_row, sp.row);
            SSD_REQUIRE(sp.begin >= dst_end, "ema_plan_build: dst of row %u overlaps dst of row %u", sp.row, dst_row);
            SSD_REQUIRE(sp.begin >= src_end, "ema_plan_build: dst of row %u overlaps src of row %u", sp.row, src_row);
            if (sp.end > dst_end) { dst_end = sp.end; dst_row = sp.row; }
            dst_begin = sp.begin; have_dst = true;
        } else {
            SSD_REQUIRE(sp.begin >= dst_end, "ema_plan_build: dst of row %u overlaps src of row %u", dst_row, sp.row);
            if (sp.end > src_end) { src_end = sp.end; src_row = sp.row; }
        }
    }
    blocks = 0;
    for (uint32_t k = 0; k < T; ++k) {
        rows[k].first_block = (uint32_t)blocks;
        blocks += (rows[k].numel + EMA_CHUNK - 1) / EMA_CHUNK;
    }
    *blocks_out = (uint32_t)blocks;
    return SSDNERF_OK;
}

extern "C" int ssdnerf_ema_update_multi(const ssdnerf_ema_row* plan, uint32_t T, uint32_t blocks, float momentum, float momentum_nontrainable,
                                        void* stream) {
    SSD_REQUIRE(plan != nullptr, "ema_update_multi: null pointer (the plan)");
    SSD_REQUIRE(((uintptr_t)plan & 7u) == 0, "ema_update_multi: the plan is not 8-byte aligned");
    SSD_REQUIRE(T > 0 && T <= SSDNERF_EMA_MAX_ROWS, "ema_update_multi: T = %u (1 .. %u rows)", T, (unsigned)SSDNERF_EMA_MAX_ROWS);
    SSD_REQUIRE(blocks >= T && blocks <= 0x7fffffffu, "ema_update_multi: %u blocks for %u rows (the count ssdnerf_ema_plan_build returned)", blocks, T);
    hipLaunchKernelGGL(k_ema_multi, dim3(blocks), dim3(EMA_THREADS), 0, (hipStream_t)stream, plan, T, momentum, momentum_nontrainable);
    SSD_CHECK_LAUNCH("ema_update_multi");
    return SSDNERF_OK;
}
