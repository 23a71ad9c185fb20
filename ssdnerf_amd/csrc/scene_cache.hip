// ssdnerf_amd/csrc/scene_cache.hip -- the per-scene training cache on the device: a batch of scenes out of the store into the batch buffers of a
// training step (ssdnerf_cache_load_multi) and back (ssdnerf_cache_store_multi), ONE launch each way (scene_cache.DeviceSceneCache;
// MultiSceneNeRF.load_cache / save_cache with cache_store='device').  The conversions of the 16-bit store are csrc/cache_cvt.h, integer code that
// a gcc build repeats bit for bit; this file is the streaming pass around them.
//
// The entries travel BY VALUE in the kernel arguments (16 bytes each, 32 of them, with the prefix sums and the ten array pointers under 1 KB):
// no device table, no copy, no allocation, no host synchronisation, nothing to keep alive after the call returns.
//
// Shape: the work of one entry is five segments back to back -- code, [exp_avg, exp_avg_sq when has_state,] density grid, bitfield -- and a
// block of SC_THREADS lanes owns one chunk of one segment: SC_ELEMS elements of a float array, SC_BYTES bytes of the grid or the bitfield.  The
// grid is the concatenation of every entry's chunks (first_block[] is the prefix sum; a block finds its entry by bisection over at most 5
// wave-uniform steps, then its segment by three comparisons).  Where both sides of a segment's row are 16-byte aligned a lane moves 16-byte
// groups (one 16-byte access on the 16-bit side against two on the fp32 side when converting) and every load is issued before the first use; a
// chunk starts at a multiple of the group, so a group never straddles the alignment.  The last, partial group of such a row and every element
// of a row that is not aligned (an odd numel moves every second row off) go element by element under `i < n`.  Every source byte is read
// once, every destination byte written once, nothing outside the named rows is touched.
#include "common.h"
#include "cache_cvt.h"

#define SC_THREADS 256
#ifndef SC_WIDE
// 16-byte groups per lane: 2 * SC_WIDE when copying, SC_WIDE (of 8 elements) when converting.  Measured on one MI355X at 8 scenes of 3 x 6 x 128^2,
// side builds back to back (tools/bench_scene_cache.py): the 16-bit load takes 17.8 / 11.9 / 13.9 us at SC_WIDE 1 / 2 / 4
#define SC_WIDE 2
#endif
#define SC_ELEMS (2048 * SC_WIDE)      // elements of code / exp_avg / exp_avg_sq per block
#define SC_BYTES (8192 * SC_WIDE)      // bytes of density_grid / density_bitfield per block

struct CacheArgs {
    ssdnerf_cache_row rows[SSDNERF_CACHE_MAX_SCENES];
    uint32_t first_block[SSDNERF_CACHE_MAX_SCENES + 1];  // first_block[k] = blocks of entries 0 .. k-1; entries past S repeat the total
    uint32_t S;
    uint32_t nb_float, nb_grid, nb_bits;                 // chunks per segment
    uint64_t numel, grid_bytes, bits_bytes;
    uint8_t* st_code; uint8_t* st_m; uint8_t* st_v; uint8_t* st_grid; uint8_t* st_bits;      // the store
    uint8_t* b_leaves; uint8_t* b_m; uint8_t* b_v; uint8_t* b_grid; uint8_t* b_bits;         // the batch buffers
};

enum { SC_F16 = 1, SC_BF16 = 2 };

template <int FMT> SSD_DEV uint32_t sc_widen(uint16_t h) { return FMT == SC_F16 ? sscc_f16_to_f32(h) : sscc_bf16_to_f32(h); }
template <int FMT> SSD_DEV uint16_t sc_narrow(uint32_t u) { return FMT == SC_F16 ? sscc_f32_to_f16_clamped(u) : sscc_f32_to_bf16_clamped(u); }

// elements [base, base + 2 * SC_WIDE * SC_THREADS * (16 / sizeof(T))) of a row of n elements, copied as they are (T: uint32_t for fp32, uint8_t for bytes)
template <typename T> SSD_DEV void sc_copy_chunk(const T* __restrict__ src, T* __restrict__ dst, uint64_t n, uint64_t base) {
    constexpr uint32_t G = 16 / sizeof(T);                   // elements per 16-byte group
    constexpr int NG = 2 * SC_WIDE;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
        uint4 r[NG];
        uint64_t i0[NG];
        bool full[NG];
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            i0[k] = base + (uint64_t)(k * SC_THREADS + threadIdx.x) * G;
            full[k] = i0[k] + G <= n;
            if (full[k]) r[k] = *reinterpret_cast<const uint4*>(src + i0[k]);
        }
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            if (full[k]) {
                *reinterpret_cast<uint4*>(dst + i0[k]) = r[k];
            } else {
                for (uint64_t i = i0[k]; i < n && i < i0[k] + G; ++i) dst[i] = src[i];       // the tail of n % G elements (one lane of one block)
            }
        }
    } else {
#pragma unroll 4
        for (uint32_t k = 0; k < NG * G; ++k) {              // consecutive lanes take consecutive elements
            const uint64_t i = base + (uint64_t)(k * SC_THREADS + threadIdx.x);
            if (i < n) dst[i] = src[i];
        }
    }
}

// elements [base, base + SC_ELEMS) of a 16-bit row of n elements, widened to fp32
template <int FMT> SSD_DEV void sc_widen_chunk(const uint16_t* __restrict__ src, uint32_t* __restrict__ dst, uint64_t n, uint64_t base) {
    if ((((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
        uint4 r[SC_WIDE];
        uint64_t i0[SC_WIDE];
        bool full[SC_WIDE];
#pragma unroll
        for (int k = 0; k < SC_WIDE; ++k) {
            i0[k] = base + (uint64_t)(k * SC_THREADS + threadIdx.x) * 8;
            full[k] = i0[k] + 8 <= n;
            if (full[k]) r[k] = *reinterpret_cast<const uint4*>(src + i0[k]);
        }
#pragma unroll
        for (int k = 0; k < SC_WIDE; ++k) {
            if (full[k]) {
                const uint32_t w[4] = {r[k].x, r[k].y, r[k].z, r[k].w};
                uint32_t o[8];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    o[2 * c] = sc_widen<FMT>((uint16_t)(w[c] & 0xffffu));
                    o[2 * c + 1] = sc_widen<FMT>((uint16_t)(w[c] >> 16));
                }
                *reinterpret_cast<uint4*>(dst + i0[k]) = make_uint4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<uint4*>(dst + i0[k] + 4) = make_uint4(o[4], o[5], o[6], o[7]);
            } else {
                for (uint64_t i = i0[k]; i < n && i < i0[k] + 8; ++i) dst[i] = sc_widen<FMT>(src[i]);     // fewer than 8 left (one lane of one block)
            }
        }
    } else {
#pragma unroll 8
        for (uint32_t k = 0; k < SC_ELEMS / SC_THREADS; ++k) {
            const uint64_t i = base + (uint64_t)(k * SC_THREADS + threadIdx.x);
            if (i < n) dst[i] = sc_widen<FMT>(src[i]);
        }
    }
}

// elements [base, base + SC_ELEMS) of an fp32 row of n elements, clamped and rounded to the 16-bit format
template <int FMT> SSD_DEV void sc_narrow_chunk(const uint32_t* __restrict__ src, uint16_t* __restrict__ dst, uint64_t n, uint64_t base) {
    if ((((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
        uint4 a[SC_WIDE], b[SC_WIDE];
        uint64_t i0[SC_WIDE];
        bool full[SC_WIDE];
#pragma unroll
        for (int k = 0; k < SC_WIDE; ++k) {
            i0[k] = base + (uint64_t)(k * SC_THREADS + threadIdx.x) * 8;
            full[k] = i0[k] + 8 <= n;
            if (full[k]) {
                a[k] = *reinterpret_cast<const uint4*>(src + i0[k]);
                b[k] = *reinterpret_cast<const uint4*>(src + i0[k] + 4);
            }
        }
#pragma unroll
        for (int k = 0; k < SC_WIDE; ++k) {
            if (full[k]) {
                const uint32_t w[8] = {a[k].x, a[k].y, a[k].z, a[k].w, b[k].x, b[k].y, b[k].z, b[k].w};
                uint32_t o[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = (uint32_t)sc_narrow<FMT>(w[2 * c]) | ((uint32_t)sc_narrow<FMT>(w[2 * c + 1]) << 16);
                *reinterpret_cast<uint4*>(dst + i0[k]) = make_uint4(o[0], o[1], o[2], o[3]);
            } else {
                for (uint64_t i = i0[k]; i < n && i < i0[k] + 8; ++i) dst[i] = sc_narrow<FMT>(src[i]);
            }
        }
    } else {
#pragma unroll 8
        for (uint32_t k = 0; k < SC_ELEMS / SC_THREADS; ++k) {
            const uint64_t i = base + (uint64_t)(k * SC_THREADS + threadIdx.x);
            if (i < n) dst[i] = sc_narrow<FMT>(src[i]);
        }
    }
}

// one chunk of a float array: row `slot` of the store's array (fp32, or FMT when HALF) against row `row` of the fp32 batch buffer
template <bool HALF, bool STORE, int FMT>
SSD_DEV void sc_float_chunk(uint8_t* store, uint8_t* batch, uint64_t numel, uint32_t slot, uint32_t row, uint32_t chunk) {
    const uint64_t base = (uint64_t)chunk * SC_ELEMS;
    uint32_t* b = reinterpret_cast<uint32_t*>(batch) + (uint64_t)row * numel;
    if (HALF) {
        uint16_t* s = reinterpret_cast<uint16_t*>(store) + (uint64_t)slot * numel;
        if (STORE) sc_narrow_chunk<FMT>(b, s, numel, base); else sc_widen_chunk<FMT>(s, b, numel, base);
    } else {
        uint32_t* s = reinterpret_cast<uint32_t*>(store) + (uint64_t)slot * numel;
        if (STORE) sc_copy_chunk<uint32_t>(b, s, numel, base); else sc_copy_chunk<uint32_t>(s, b, numel, base);
    }
}

template <bool HALF, bool STORE> __global__ void __launch_bounds__(SC_THREADS) k_cache_move(const CacheArgs a) {
    // the entry of this block: the last k with first_block[k] <= blockIdx.x (wave-uniform: scalar loads from the argument segment)
    uint32_t lo = 0, hi = a.S;                               // invariant: first_block[lo] <= blockIdx.x < first_block[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.first_block[mid] <= blockIdx.x) lo = mid; else hi = mid;
    }
    const ssdnerf_cache_row e = a.rows[lo];
    uint32_t b = blockIdx.x - a.first_block[lo];
    const uint32_t nf = a.nb_float;
    if (b < nf) {
        sc_float_chunk<HALF, STORE, SC_F16>(a.st_code, a.b_leaves, a.numel, e.slot, e.row, b);
        return;
    }
    b -= nf;
    if (e.has_state) {
        if (b < nf) {
            sc_float_chunk<HALF, STORE, SC_BF16>(a.st_m, a.b_m, a.numel, e.slot, e.row, b);
            return;
        }
        b -= nf;
        if (b < nf) {
            sc_float_chunk<HALF, STORE, SC_BF16>(a.st_v, a.b_v, a.numel, e.slot, e.row, b);
            return;
        }
        b -= nf;
    }
    uint8_t* s;
    uint8_t* t;
    uint64_t n;
    if (b < a.nb_grid) {
        n = a.grid_bytes;
        s = a.st_grid + (uint64_t)e.slot * n; t = a.b_grid + (uint64_t)e.row * n;
    } else {
        b -= a.nb_grid;
        n = a.bits_bytes;
        s = a.st_bits + (uint64_t)e.slot * n; t = a.b_bits + (uint64_t)e.row * n;
    }
    if (STORE) sc_copy_chunk<uint8_t>(t, s, n, (uint64_t)b * SC_BYTES); else sc_copy_chunk<uint8_t>(s, t, n, (uint64_t)b * SC_BYTES);
}

extern "C" uint32_t ssdnerf_cache_max_scenes(void) { return SSDNERF_CACHE_MAX_SCENES; }

// validates a call and fills in the kernel arguments; `name` prefixes the messages
static int sc_prepare(const char* name, bool store_dir, const ssdnerf_cache_store* st, const ssdnerf_cache_row* rows, uint32_t S, const void* leaves,
                      const void* m, const void* v, const void* grid, const void* bits, CacheArgs& a, uint64_t& blocks, bool& half) {
    SSD_REQUIRE(st != nullptr && rows != nullptr, "%s: null pointer (the store or the rows)", name);
    SSD_REQUIRE(S > 0, "%s: S == 0 (no scenes)", name);
    SSD_REQUIRE(S <= SSDNERF_CACHE_MAX_SCENES, "%s: %u scenes, one call takes at most %u", name, S, (unsigned)SSDNERF_CACHE_MAX_SCENES);
    SSD_REQUIRE(st->code && st->exp_avg && st->exp_avg_sq && st->density_grid && st->density_bitfield, "%s: null pointer in the store", name);
    SSD_REQUIRE(leaves && grid && bits, "%s: null pointer (a batch buffer)", name);
    SSD_REQUIRE((st->code_dtype == 0 && st->moment_dtype == 0) || (st->code_dtype == 1 && st->moment_dtype == 2),
                "%s: dtype pair (%d, %d) is not supported: (0, 0) fp32 codes and moments, or (1, 2) fp16 codes and bf16 moments", name, st->code_dtype,
                st->moment_dtype);
    half = st->code_dtype == 1;
    SSD_REQUIRE(st->slots > 0 && st->slots <= 0xffffffffull, "%s: zero size (slots) or more than 2^32 - 1 slots", name);
    SSD_REQUIRE(st->numel > 0 && st->grid_bytes > 0 && st->bits_bytes > 0, "%s: zero size (numel %llu, grid_bytes %llu, bits_bytes %llu)", name,
                (unsigned long long)st->numel, (unsigned long long)st->grid_bytes, (unsigned long long)st->bits_bytes);
    SSD_REQUIRE(st->numel <= ((uint64_t)1 << 40) && st->grid_bytes <= ((uint64_t)1 << 40) && st->bits_bytes <= ((uint64_t)1 << 40),
                "%s: a row of more than 2^40 elements", name);
    const uintptr_t store_mask = half ? 1u : 3u;
    SSD_REQUIRE((((uintptr_t)st->code | (uintptr_t)st->exp_avg | (uintptr_t)st->exp_avg_sq) & store_mask) == 0,
                "%s: a float array of the store is not aligned to its element size", name);
    SSD_REQUIRE((((uintptr_t)leaves | (uintptr_t)m | (uintptr_t)v) & 3u) == 0, "%s: a float batch buffer is not 4-byte aligned", name);
    a.nb_float = (uint32_t)((st->numel + SC_ELEMS - 1) / SC_ELEMS);
    a.nb_grid = (uint32_t)((st->grid_bytes + SC_BYTES - 1) / SC_BYTES);
    a.nb_bits = (uint32_t)((st->bits_bytes + SC_BYTES - 1) / SC_BYTES);
    uint32_t seen_slot[SSDNERF_CACHE_MAX_SCENES], seen_row = 0;
    blocks = 0;
    for (uint32_t k = 0; k < S; ++k) {
        const ssdnerf_cache_row& e = rows[k];
        SSD_REQUIRE(e.slot < st->slots, "%s: entry %u names slot %u of %llu", name, k, e.slot, (unsigned long long)st->slots);
        SSD_REQUIRE(e.row < S, "%s: entry %u names batch row %u of %u", name, k, e.row, S);
        SSD_REQUIRE(e.has_state <= 1, "%s: entry %u has has_state %u (0 or 1)", name, k, e.has_state);
        SSD_REQUIRE(!e.has_state || (m && v), "%s: null pointer (m or v) while entry %u has has_state set", name, k);
        if (store_dir) {
            for (uint32_t j = 0; j < k; ++j) SSD_REQUIRE(seen_slot[j] != e.slot, "%s: slot %u twice (entries %u and %u)", name, e.slot, j, k);
        } else {
            SSD_REQUIRE(!((seen_row >> e.row) & 1u), "%s: batch row %u twice (entry %u)", name, e.row, k);
            seen_row |= 1u << e.row;
        }
        seen_slot[k] = e.slot;
        a.rows[k] = e;
        a.first_block[k] = (uint32_t)blocks;
        blocks += (uint64_t)a.nb_float * (e.has_state ? 3 : 1) + a.nb_grid + a.nb_bits;
        SSD_REQUIRE(blocks <= 0x7fffffffu, "%s: more than 2^31 - 1 blocks up to entry %u", name, k);
    }
    for (uint32_t k = S; k <= SSDNERF_CACHE_MAX_SCENES; ++k) {
        if (k < SSDNERF_CACHE_MAX_SCENES) a.rows[k] = ssdnerf_cache_row{};
        a.first_block[k] = (uint32_t)blocks;
    }
    a.S = S;
    a.numel = st->numel; a.grid_bytes = st->grid_bytes; a.bits_bytes = st->bits_bytes;
    a.st_code = (uint8_t*)st->code; a.st_m = (uint8_t*)st->exp_avg; a.st_v = (uint8_t*)st->exp_avg_sq;
    a.st_grid = (uint8_t*)st->density_grid; a.st_bits = (uint8_t*)st->density_bitfield;
    a.b_leaves = (uint8_t*)leaves; a.b_m = (uint8_t*)m; a.b_v = (uint8_t*)v; a.b_grid = (uint8_t*)grid; a.b_bits = (uint8_t*)bits;
    return SSDNERF_OK;
}

extern "C" int ssdnerf_cache_load_multi(const ssdnerf_cache_store* store, const ssdnerf_cache_row* rows, uint32_t S, float* leaves, float* m, float* v,
                                        void* grid, void* bits, void* stream) {
    CacheArgs a;
    uint64_t blocks;
    bool half;
    const int rc = sc_prepare("cache_load_multi", false, store, rows, S, leaves, m, v, grid, bits, a, blocks, half);
    if (rc != SSDNERF_OK) return rc;
    if (half) hipLaunchKernelGGL((k_cache_move<true, false>), dim3((uint32_t)blocks), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_cache_move<false, false>), dim3((uint32_t)blocks), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    SSD_CHECK_LAUNCH("cache_load_multi");
    return SSDNERF_OK;
}

extern "C" int ssdnerf_cache_store_multi(const ssdnerf_cache_store* store, const ssdnerf_cache_row* rows, uint32_t S, const float* leaves, const float* m,
                                         const float* v, const void* grid, const void* bits, void* stream) {
    CacheArgs a;
    uint64_t blocks;
    bool half;
    const int rc = sc_prepare("cache_store_multi", true, store, rows, S, leaves, m, v, grid, bits, a, blocks, half);
    if (rc != SSDNERF_OK) return rc;
    if (half) hipLaunchKernelGGL((k_cache_move<true, true>), dim3((uint32_t)blocks), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_cache_move<false, true>), dim3((uint32_t)blocks), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    SSD_CHECK_LAUNCH("cache_store_multi");
    return SSDNERF_OK;
}
