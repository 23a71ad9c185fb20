// ssdnerf_amd/csrc/scene_store.hip -- a batch of views out of the device-resident image store (datasets.SceneStore): the images of a dataset
// are kept as uint8, back to back; one launch picks `count` of them by index and writes them as the fp32 the fitting code reads,
//     out[k][b] = (float)store[index[k]][b] / 255.0f,
// which is what the reference's dataset computes per image on the host (lib/datasets/shapenet_srn.py:160, numpy `astype(float32) / 255`).
//
// Arithmetic: ONE IEEE fp32 division per element (the library is built with -fno-fast-math; hipcc's fp32 division is correctly rounded), so
// the result is numpy's quotient bit for bit for all 256 byte values.  `x * (1 / 255.f)` is NOT: it differs at 126 of the 256 values.
//
// Shape: a pure stream, 1 byte in and 4 bytes out per element, no LDS, no atomics.  The output is one array of count * image_bytes elements; a
// block of GV_THREADS lanes owns GV_CHUNK consecutive ones.  Every lane finds the image of its elements by integer division of the element
// offset (a chunk may span several small images, and an image many chunks).
//   vector path  (image_bytes % 16 == 0, store and out 16-byte aligned: the 128 x 128 and 64 x 64 views): a lane takes 4 * GV_GROUPS groups of 4
//                consecutive source bytes, GV_THREADS * 4 apart -- one 4-byte load each, all issued before the first use -- and writes each group
//                as one 16-byte non-temporal store, so a wave's store instruction covers 1 KB of `out` without gaps.  A group never straddles an
//                image, because image_bytes is a multiple of 4.  Measured on the training batch, 8 x 50 views of 128 x 128 (profiles/dataset.json,
//                DESIGN.md section 16): about 16 us, against 19 us with plain stores (-DGV_PLAIN_STORES), 29 us for one 16-byte load and four
//                16-byte stores per lane with plain stores (-DGV_LOAD16 -DGV_PLAIN_STORES: every store instruction of a wave then writes 16
//                of every 64 bytes) and 106 us for that form with non-temporal stores (-DGV_LOAD16).
//   element path (everything else: 5 x 7 x 3 = 105-byte images, whose starts are misaligned, or a store pointer that is only 1-byte aligned):
//                consecutive lanes take consecutive elements, under `i < total`.
// `store` and `index` are only read; nothing outside [0, count * image_bytes) of `out` is written.  The indices are NOT checked here: the Python
// layer validates them on the host before it uploads them.
//
// k_sample_rays_u8 (ssdnerf_sample_rays_u8, datasets.StoredViews.sample) is the other way out of the store: not whole views but R sampled PIXELS
// per scene, each with its camera ray -- what fitting.RayBatcher hands to the renderer -- so that a training batch never exists as fp32 images
// and (S, V, h, w, 3) ray arrays.  One lane per ray: the pixel index picks the view, ssd_cam_ray (common.h) makes the ray from that view's pose
// and intrinsics, gv_unit (below) makes the colour from the pixel's three bytes; the same two functions the dense kernels call, so all nine
// floats are the dense path's bit for bit.  No LDS, no atomics; the pose table (S * V * 80 B) is a per-lane load that stays in cache, the
// bytes are a random gather, 36 B are written per lane.  About 1.3 MB moves at the training batch (8 x 4096 rays): launch-bound.
//
// k_sample_rays_perm_u8 (ssdnerf_sample_rays_perm_u8, datasets.StoredViews.sample_permuted) is that kernel without the index array: ray r of scene s is
// pixel pi(seed, s, draw, V h w)(start + r) of the keyed permutation of keyed_perm.h, which every lane evaluates for itself.  A
// block belongs to ONE scene (blocks_per_scene = ceil(R / 256) blocks each), so the twelve round keys -- three Philox blocks on (seed, scene, draw) --
// are wave-uniform; the cycle walk is a per-lane loop of < 4 passes in the mean.  The pixel found goes through the same ssd_cam_ray and gv_unit as in
// k_sample_rays_u8, so the nine floats are that kernel's bit for bit.  k_perm_indices (ssdnerf_perm_indices) writes the same pi as int64 for the
// consumers that index dense arrays.  No LDS, no atomics, no workspace in either.
#include "common.h"
#include "keyed_perm.h"

#define GV_THREADS 256
#define GV_GROUPS 2
#define GV_CHUNK (GV_THREADS * 16 * GV_GROUPS)          // elements per block (8192)

#ifdef GV_PLAIN_STORES                                   // A/B builds only
#define GV_STORE4(p, v) (*(p) = (v))
#else                                                    // the output is written once and read by later kernels
#define GV_STORE4(p, v) __builtin_nontemporal_store((v), (p))
#endif

typedef float gv_float4 __attribute__((ext_vector_type(4)));

SSD_DEV float gv_unit(uint32_t byte) { return (float)byte / 255.0f; }

SSD_DEV gv_float4 gv_unit4(uint32_t word) {
    gv_float4 r;
    r.x = gv_unit(word & 0xffu);
    r.y = gv_unit((word >> 8) & 0xffu);
    r.z = gv_unit((word >> 16) & 0xffu);
    r.w = gv_unit(word >> 24);
    return r;
}

__global__ void __launch_bounds__(GV_THREADS) k_gather_views_u8_vec(const uint8_t* __restrict__ store, uint64_t image_bytes, const int32_t* __restrict__ index,
                                                                    uint64_t total, float* __restrict__ out) {
    const uint64_t base = (uint64_t)blockIdx.x * GV_CHUNK;
#ifndef GV_LOAD16
    uint32_t word[GV_GROUPS * 4];
    uint64_t ew[GV_GROUPS * 4];
#pragma unroll
    for (int g = 0; g < GV_GROUPS * 4; ++g) {
        ew[g] = base + (uint64_t)(g * GV_THREADS + threadIdx.x) * 4;
        if (ew[g] < total) {
            const uint64_t k = ew[g] / image_bytes;
            const uint64_t b = ew[g] - k * image_bytes;
            word[g] = *reinterpret_cast<const uint32_t*>(store + (uint64_t)index[k] * image_bytes + b);
        }
    }
#pragma unroll
    for (int g = 0; g < GV_GROUPS * 4; ++g)
        if (ew[g] < total) GV_STORE4(reinterpret_cast<gv_float4*>(out + ew[g]), gv_unit4(word[g]));
#else                                                    // A/B builds only: one 16-byte load and four 16-byte stores per lane and group
    uint4 src[GV_GROUPS];
    uint64_t e[GV_GROUPS];
#pragma unroll
    for (int g = 0; g < GV_GROUPS; ++g) {
        e[g] = base + (uint64_t)(g * GV_THREADS + threadIdx.x) * 16;
        if (e[g] < total) {                                          // total is a multiple of 16: a group is whole or absent
            const uint64_t k = e[g] / image_bytes;
            const uint64_t b = e[g] - k * image_bytes;
            src[g] = *reinterpret_cast<const uint4*>(store + (uint64_t)index[k] * image_bytes + b);
        }
    }
#pragma unroll
    for (int g = 0; g < GV_GROUPS; ++g) {
        if (e[g] < total) {
            gv_float4* dst = reinterpret_cast<gv_float4*>(out + e[g]);
            GV_STORE4(dst + 0, gv_unit4(src[g].x));
            GV_STORE4(dst + 1, gv_unit4(src[g].y));
            GV_STORE4(dst + 2, gv_unit4(src[g].z));
            GV_STORE4(dst + 3, gv_unit4(src[g].w));
        }
    }
#endif
}

__global__ void __launch_bounds__(GV_THREADS) k_gather_views_u8_elem(const uint8_t* __restrict__ store, uint64_t image_bytes, const int32_t* __restrict__ index,
                                                                     uint64_t total, float* __restrict__ out) {
    const uint64_t base = (uint64_t)blockIdx.x * GV_CHUNK;
    for (int j = 0; j < GV_CHUNK / GV_THREADS; ++j) {
        const uint64_t i = base + (uint64_t)(j * GV_THREADS + threadIdx.x);
        if (i < total) {
            const uint64_t k = i / image_bytes;
            const uint64_t b = i - k * image_bytes;
            out[i] = gv_unit(store[(uint64_t)index[k] * image_bytes + b]);
        }
    }
}

extern "C" int ssdnerf_gather_views_u8(const uint8_t* store, uint64_t image_bytes, uint64_t num_images, const int32_t* index, uint64_t count, float* out,
                                       void* stream) {
    SSD_REQUIRE(store != nullptr && index != nullptr && out != nullptr, "gather_views_u8: null pointer");
    SSD_REQUIRE(count > 0, "gather_views_u8: count == 0 (no views)");
    SSD_REQUIRE(image_bytes > 0, "gather_views_u8: image_bytes == 0");
    SSD_REQUIRE(num_images > 0, "gather_views_u8: num_images == 0 (an empty store)");
    SSD_REQUIRE(num_images <= 0x7fffffffull, "gather_views_u8: %llu images, the int32 indices reach 2^31 - 1", (unsigned long long)num_images);
    const uint64_t limit = (uint64_t)1 << 40;
    SSD_REQUIRE(image_bytes <= limit && count <= limit / image_bytes, "gather_views_u8: count * image_bytes is more than 2^40 elements");
    SSD_REQUIRE((((uintptr_t)index | (uintptr_t)out) & 3u) == 0, "gather_views_u8: index or out is not 4-byte aligned");
    const uint64_t total = count * image_bytes;
    const uint32_t blocks = (uint32_t)((total + GV_CHUNK - 1) / GV_CHUNK);      // <= 2^27
    const bool vec = image_bytes % 16 == 0 && (((uintptr_t)store | (uintptr_t)out) & 15u) == 0;
    if (vec) hipLaunchKernelGGL(k_gather_views_u8_vec, dim3(blocks), dim3(GV_THREADS), 0, (hipStream_t)stream, store, image_bytes, index, total, out);
    else hipLaunchKernelGGL(k_gather_views_u8_elem, dim3(blocks), dim3(GV_THREADS), 0, (hipStream_t)stream, store, image_bytes, index, total, out);
    SSD_CHECK_LAUNCH("gather_views_u8");
    return SSDNERF_OK;
}

// ------------------------------------------------------------------------------------------------
// sampled pixels of a batch's views, with their rays: out[s][r] for pixel p = inds[s][r] (or r, inds == NULL) of scene s, p = view * hw + pixel
#define RS_THREADS 256

__global__ void __launch_bounds__(RS_THREADS) k_sample_rays_u8(const uint8_t* __restrict__ store, uint32_t hw, uint32_t w, const int32_t* __restrict__ view_image,
                                                               const float* __restrict__ c2w, const float* __restrict__ intr, uint32_t V,
                                                               const int64_t* __restrict__ inds, uint32_t R, uint64_t total, float* __restrict__ rays_o,
                                                               float* __restrict__ rays_d, float* __restrict__ target) {
    const uint64_t i = (uint64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= total) return;
    const uint64_t s = i / R;
    const int64_t p = inds != nullptr ? inds[i] : (int64_t)(i - s * R);
    float o[3], d[3], c[3];
    if ((uint64_t)p < (uint64_t)V * hw) {                            // (a negative p is a huge unsigned one)
        const uint32_t v = (uint32_t)p / hw, q = (uint32_t)p - v * hw;
        const uint64_t cam = s * V + v;
        ssd_cam_ray(c2w + cam * 16, intr + cam * 4, q % w, q / w, o, d);
        const uint8_t* px = store + ((uint64_t)view_image[cam] * hw + q) * 3;
        c[0] = gv_unit(px[0]); c[1] = gv_unit(px[1]); c[2] = gv_unit(px[2]);
    } else {                                                         // outside the views: nothing is read, the ray is NaN
        const float nan = __builtin_nanf("");
        o[0] = o[1] = o[2] = d[0] = d[1] = d[2] = c[0] = c[1] = c[2] = nan;
    }
    rays_o[3 * i + 0] = o[0]; rays_o[3 * i + 1] = o[1]; rays_o[3 * i + 2] = o[2];
    rays_d[3 * i + 0] = d[0]; rays_d[3 * i + 1] = d[1]; rays_d[3 * i + 2] = d[2];
    target[3 * i + 0] = c[0]; target[3 * i + 1] = c[1]; target[3 * i + 2] = c[2];
}

extern "C" int ssdnerf_sample_rays_u8(const uint8_t* store, uint64_t num_images, uint32_t h, uint32_t w, const int32_t* view_image, const float* c2w,
                                      const float* intr, uint32_t S, uint32_t V, const int64_t* inds, uint32_t R, float* rays_o, float* rays_d,
                                      float* target, void* stream) {
    SSD_REQUIRE(store != nullptr && view_image != nullptr && c2w != nullptr && intr != nullptr, "sample_rays_u8: null input pointer");
    SSD_REQUIRE(rays_o != nullptr && rays_d != nullptr && target != nullptr, "sample_rays_u8: null output pointer");
    SSD_REQUIRE(S > 0 && V > 0 && R > 0, "sample_rays_u8: S, V and R must be positive (S = %u, V = %u, R = %u)", S, V, R);
    SSD_REQUIRE(h > 0 && w > 0, "sample_rays_u8: an empty view (h = %u, w = %u)", h, w);
    SSD_REQUIRE(num_images > 0, "sample_rays_u8: num_images == 0 (an empty store)");
    SSD_REQUIRE(num_images <= 0x7fffffffull, "sample_rays_u8: %llu images, the int32 table reaches 2^31 - 1", (unsigned long long)num_images);
    const uint64_t hw = (uint64_t)h * w, P = hw * V;
    SSD_REQUIRE(hw < ((uint64_t)1 << 32) && P < ((uint64_t)1 << 32), "sample_rays_u8: V * h * w is 2^32 pixels per scene or more");
    SSD_REQUIRE(inds != nullptr || R == P, "sample_rays_u8: inds == NULL takes every pixel, R must be V * h * w = %llu, got %u", (unsigned long long)P, R);
    SSD_REQUIRE((((uintptr_t)rays_o | (uintptr_t)rays_d | (uintptr_t)target | (uintptr_t)view_image | (uintptr_t)c2w | (uintptr_t)intr) & 3u) == 0,
                "sample_rays_u8: an output or a table is not 4-byte aligned");
    SSD_REQUIRE(((uintptr_t)inds & 7u) == 0, "sample_rays_u8: inds is not 8-byte aligned");
    const uint64_t total = (uint64_t)S * R;
    SSD_REQUIRE(total <= ((uint64_t)1 << 38), "sample_rays_u8: S * R is more than 2^38 rays");
    hipLaunchKernelGGL(k_sample_rays_u8, dim3((uint32_t)((total + RS_THREADS - 1) / RS_THREADS)), dim3(RS_THREADS), 0, (hipStream_t)stream, store, (uint32_t)hw, w,
                       view_image, c2w, intr, V, inds, R, total, rays_o, rays_d, target);
    SSD_CHECK_LAUNCH("sample_rays_u8");
    return SSDNERF_OK;
}

// ------------------------------------------------------------------------------------------------
// the same batch with its pixels numbered on the device: p = pi(seed, s, draw, V * hw)(start + r), keyed_perm.h.  Block b of the grid is block
// b % bps of scene b / bps: s, the round keys and h are uniform over the block, r and the walk are per lane.
SSD_DEV bool rp_locate(uint32_t R, uint32_t bps, uint32_t& s, uint32_t& r) {
    s = blockIdx.x / bps;
    r = (blockIdx.x - s * bps) * RS_THREADS + threadIdx.x;
    return r < R;
}

__global__ void __launch_bounds__(RS_THREADS) k_perm_indices(int64_t* __restrict__ out, uint32_t P, uint32_t start, uint32_t R, uint32_t bps, uint32_t hbits,
                                                             uint64_t seed, uint32_t draw) {
    uint32_t s, r;
    const bool live = rp_locate(R, bps, s, r);
    const sskp_keys keys = sskp_round_keys(seed, s, draw);
    if (!live) return;
    out[(uint64_t)s * R + r] = (int64_t)sskp_perm(&keys, hbits, P, start + r, nullptr);
}

__global__ void __launch_bounds__(RS_THREADS) k_sample_rays_perm_u8(const uint8_t* __restrict__ store, uint32_t hw, uint32_t w, const int32_t* __restrict__ view_image,
                                                                    const float* __restrict__ c2w, const float* __restrict__ intr, uint32_t V, uint32_t P,
                                                                    uint32_t start, uint32_t R, uint32_t bps, uint32_t hbits, uint64_t seed, uint32_t draw,
                                                                    float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ target) {
    uint32_t s, r;
    const bool live = rp_locate(R, bps, s, r);
    const sskp_keys keys = sskp_round_keys(seed, s, draw);
    if (!live) return;
    const uint32_t p = sskp_perm(&keys, hbits, P, start + r, nullptr);            // < P = V * hw: always inside the views
    const uint32_t v = p / hw, q = p - v * hw;
    const uint64_t cam = (uint64_t)s * V + v, i = (uint64_t)s * R + r;
    float o[3], d[3];
    ssd_cam_ray(c2w + cam * 16, intr + cam * 4, q % w, q / w, o, d);
    const uint8_t* px = store + ((uint64_t)view_image[cam] * hw + q) * 3;
    const float c0 = gv_unit(px[0]), c1 = gv_unit(px[1]), c2 = gv_unit(px[2]);
    rays_o[3 * i + 0] = o[0]; rays_o[3 * i + 1] = o[1]; rays_o[3 * i + 2] = o[2];
    rays_d[3 * i + 0] = d[0]; rays_d[3 * i + 1] = d[1]; rays_d[3 * i + 2] = d[2];
    target[3 * i + 0] = c0; target[3 * i + 1] = c1; target[3 * i + 2] = c2;
}

// the checks the two entry points share; on success *bps_out is the blocks per scene and S * *bps_out fits the grid
static int rp_check(const char* what, uint32_t S, uint64_t P, uint64_t start, uint32_t R, uint32_t* bps_out) {
    SSD_REQUIRE(S > 0 && R > 0 && P > 0, "%s: S, R and P must be positive (S = %u, R = %u, P = %llu)", what, S, R, (unsigned long long)P);
    SSD_REQUIRE(P < ((uint64_t)1 << 32), "%s: P = %llu, the permutation is defined below 2^32", what, (unsigned long long)P);
    SSD_REQUIRE(start <= P && R <= P - start, "%s: positions [%llu, %llu + %u) leave [0, P = %llu)", what, (unsigned long long)start,
                (unsigned long long)start, R, (unsigned long long)P);
    const uint32_t bps = (R + RS_THREADS - 1) / RS_THREADS;                         // R <= P < 2^32: no overflow, bps <= 2^24
    SSD_REQUIRE((uint64_t)S * bps <= 0x7fffffffull, "%s: S * ceil(R / %d) is more than 2^31 - 1 blocks", what, RS_THREADS);
    *bps_out = bps;
    return SSDNERF_OK;
}

extern "C" int ssdnerf_perm_indices(int64_t* out, uint32_t S, uint64_t P, uint64_t start, uint32_t R, uint64_t seed, uint32_t draw, void* stream) {
    SSD_REQUIRE(out != nullptr, "perm_indices: null pointer");
    uint32_t bps = 0;
    const int status = rp_check("perm_indices", S, P, start, R, &bps);
    if (status != SSDNERF_OK) return status;
    SSD_REQUIRE(((uintptr_t)out & 7u) == 0, "perm_indices: out is not 8-byte aligned");
    hipLaunchKernelGGL(k_perm_indices, dim3(S * bps), dim3(RS_THREADS), 0, (hipStream_t)stream, out, (uint32_t)P, (uint32_t)start, R, bps, sskp_half_bits(P),
                       seed, draw);
    SSD_CHECK_LAUNCH("perm_indices");
    return SSDNERF_OK;
}

extern "C" int ssdnerf_sample_rays_perm_u8(const uint8_t* store, uint64_t num_images, uint32_t h, uint32_t w, const int32_t* view_image, const float* c2w,
                                           const float* intr, uint32_t S, uint32_t V, uint64_t seed, uint32_t draw, uint64_t start, uint32_t R,
                                           float* rays_o, float* rays_d, float* target, void* stream) {
    SSD_REQUIRE(store != nullptr && view_image != nullptr && c2w != nullptr && intr != nullptr, "sample_rays_perm_u8: null input pointer");
    SSD_REQUIRE(rays_o != nullptr && rays_d != nullptr && target != nullptr, "sample_rays_perm_u8: null output pointer");
    SSD_REQUIRE(V > 0 && h > 0 && w > 0, "sample_rays_perm_u8: no pixels (V = %u, h = %u, w = %u)", V, h, w);
    SSD_REQUIRE(num_images > 0, "sample_rays_perm_u8: num_images == 0 (an empty store)");
    SSD_REQUIRE(num_images <= 0x7fffffffull, "sample_rays_perm_u8: %llu images, the int32 table reaches 2^31 - 1", (unsigned long long)num_images);
    const uint64_t hw = (uint64_t)h * w;
    SSD_REQUIRE(hw < ((uint64_t)1 << 32) && hw * V < ((uint64_t)1 << 32), "sample_rays_perm_u8: V * h * w is 2^32 pixels per scene or more");
    uint32_t bps = 0;
    const int status = rp_check("sample_rays_perm_u8", S, hw * V, start, R, &bps);
    if (status != SSDNERF_OK) return status;
    SSD_REQUIRE((((uintptr_t)rays_o | (uintptr_t)rays_d | (uintptr_t)target | (uintptr_t)view_image | (uintptr_t)c2w | (uintptr_t)intr) & 3u) == 0,
                "sample_rays_perm_u8: an output or a table is not 4-byte aligned");
    hipLaunchKernelGGL(k_sample_rays_perm_u8, dim3(S * bps), dim3(RS_THREADS), 0, (hipStream_t)stream, store, (uint32_t)hw, w, view_image, c2w, intr, V,
                       (uint32_t)(hw * V), (uint32_t)start, R, bps, sskp_half_bits(hw * V), seed, draw, rays_o, rays_d, target);
    SSD_CHECK_LAUNCH("sample_rays_perm_u8");
    return SSDNERF_OK;
}
