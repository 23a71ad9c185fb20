// ssdnerf_amd/csrc/lpips.hip -- what LPIPS v0.1 (net = 'vgg') does around its thirteen 3 x 3 convolutions.  The convolutions are
// csrc/conv_igemm.hip's fp32-class kernels, called as they are; this file is the memory-bound rest, one pass over each activation:
//
//   k_lpips_input   two fp32 image sets (n, h, w, 3) in [0, 1] -> one channel-last tensor [2n][h][w][8], predictions first:
//                   x = ((2 img - 1) - shift) / scale per channel (the scaling layer of the lpips package), channels 3 .. 7 exactly zero (the
//                   convolution kernels take channel counts that are multiples of 8)
//   k_relu_pool     a convolution's raw output [N][H][W][C] -> ReLU, optionally the 2 x 2 / stride 2 max-pool (floor mode: an odd last row / column is
//                   dropped), written as fp32 or in the PRE-SPLIT operand layout of ssdnerf_conv2d_nhwc_f32x2_presplit
//   k_lpips_layer   a tap: the raw output [2n][H][W][C] of convolution 2 / 4 / 7 / 10 / 13.  Per pair (i, n + i) and pixel, with f = ReLU(x):
//                   fh = f / (sqrt(sum_c f_c^2) + 1e-10),  d = sum_c w_c (fh_p - fh_t)^2;  the pair's value is the mean of d over the pixels.  The
//                   same pass writes the pooled ReLU output for the next stage (k_relu_pool's bytes), so the largest tensors are read once.
//   k_lpips_finish  acc[i] += mean: the blocks' fp64 partial sums of a pair, added in block order
//
// Numerics: everything per pixel is fp32 (the channel sums: 8 terms serially per lane, then a butterfly over the lanes of the pixel); sums over pixels
// are fp64 in a fixed order -- lane group, wave, block, then the blocks in index order.  No atomics: two calls on the same input return the same bits.
// A NaN in a convolution's output stays one through ReLU and pool, and makes its pair's value NaN.
//
// Shape: a lane owns 8 consecutive channels (two 16-byte loads per pixel), L = C / 8 lanes own a pixel, so a wave holds 64 / L pixels' channel
// vectors at once and reduces over channels with DPP (within 16 lanes) and two cross-row shuffles.  k_lpips_layer's unit of work is a 2 x 2 QUAD of
// pixels of both images of a pair (16 loads in flight per lane), which is also one pooled output pixel.
#include "common.h"

#define LP_THREADS 256
#define LP_MAX_BLOCKS_PER_PAIR 64          // fp64 partial sums per pair (the workspace), and with 32 pairs a grid of 2048 blocks

namespace {

// ReLU and max as torch.relu and torch's max_pool2d take them: a NaN stays a NaN (fmaxf would drop it, and a broken image would score a plausible
// finite LPIPS); -0 -> +0
SSD_DEV float lp_relu(float v) { return !(v <= 0.f) ? v : 0.f; }
SSD_DEV float lp_max(float a, float b) { return (a != a || a > b) ? a : b; }
SSD_DEV float lp_max4(float a, float b, float c, float d) { return lp_max(lp_max(a, b), lp_max(c, d)); }

SSD_DEV void lp_load8(const float* __restrict__ p, float* f) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

SSD_DEV void lp_store8(float* __restrict__ p, const float* f) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}

// 8 consecutive channels [8 j, 8 j + 8) of one pixel in the PRE-SPLIT layout (include/ssdnerf_hip.h, ssdnerf_conv2d_nhwc_f32x2_presplit): per pixel and block
// of 32 channels 128 bytes = [32 hi | 32 lo] bf16, hi = truncation of the value, lo = truncation of the exact remainder -- the bytes of
// csrc/groupnorm.hip's store_split, 16 of each per lane.  pix_base: the pixel's first byte (pixel index * C * 4).
SSD_DEV void lp_store8_split(unsigned char* __restrict__ pix_base, uint32_t j, const float* f) {
    uint32_t hi[8], lo[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        hi[i] = __float_as_uint(f[i]) & 0xffff0000u;
        lo[i] = __float_as_uint(f[i] - __uint_as_float(hi[i]));
    }
    unsigned char* base = pix_base + (size_t)(j >> 2) * 128 + (j & 3) * 16;
    *reinterpret_cast<uint4*>(base) = make_uint4(__builtin_amdgcn_perm(hi[1], hi[0], 0x07060302u), __builtin_amdgcn_perm(hi[3], hi[2], 0x07060302u),
                                                 __builtin_amdgcn_perm(hi[5], hi[4], 0x07060302u), __builtin_amdgcn_perm(hi[7], hi[6], 0x07060302u));
    *reinterpret_cast<uint4*>(base + 64) = make_uint4(__builtin_amdgcn_perm(lo[1], lo[0], 0x07060302u), __builtin_amdgcn_perm(lo[3], lo[2], 0x07060302u),
                                                      __builtin_amdgcn_perm(lo[5], lo[4], 0x07060302u), __builtin_amdgcn_perm(lo[7], lo[6], 0x07060302u));
}

// ---------------------------------------------------------------------------------------------------------------------------------- input scaling
// shift and scale as the fp32 values nearest to the decimals the lpips package stores in fp32 tensors
__global__ void __launch_bounds__(LP_THREADS) k_lpips_input(const float* __restrict__ pred, const float* __restrict__ target, uint32_t n_pix, float* __restrict__ out) {
    const uint32_t p = blockIdx.x * LP_THREADS + threadIdx.x;                // pixel of [2n][h][w]; n_pix = n * h * w pixels per image set
    if (p >= 2 * n_pix) return;
    const float* __restrict__ src = p < n_pix ? pred + (size_t)p * 3 : target + (size_t)(p - n_pix) * 3;
    const float r = ((2.f * src[0] - 1.f) - -0.030f) / 0.458f;
    const float g = ((2.f * src[1] - 1.f) - -0.088f) / 0.448f;
    const float b = ((2.f * src[2] - 1.f) - -0.188f) / 0.450f;
    float4* __restrict__ o = reinterpret_cast<float4*>(out + (size_t)p * 8);
    o[0] = make_float4(r, g, b, 0.f);
    o[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------------------- ReLU (+ pool)
// one thread per (output pixel, 8 channels), grid-stride; cpp = C / 8
template <bool POOL, bool SPLIT>
__global__ void __launch_bounds__(LP_THREADS) k_relu_pool(const float* __restrict__ x, uint32_t H, uint32_t W, uint32_t Ho, uint32_t Wo, uint32_t cpp, uint64_t total,
                                                          void* __restrict__ y) {
    const uint32_t C = cpp * 8;
    for (uint64_t i = (uint64_t)blockIdx.x * LP_THREADS + threadIdx.x; i < total; i += (uint64_t)gridDim.x * LP_THREADS) {
        const uint64_t opix = i / cpp;
        const uint32_t j = (uint32_t)(i - opix * cpp);
        float f[8];
        if (POOL) {
            const uint64_t row = opix / Wo;                                  // image * Ho + yo
            const uint32_t xo = (uint32_t)(opix - row * Wo), yo = (uint32_t)(row % Ho);
            const uint64_t img = row / Ho;
            const float* __restrict__ p00 = x + (((img * H + 2 * yo) * W + 2 * xo) * C + 8 * j);
            float a[8], b[8], c[8], d[8];
            lp_load8(p00, a);
            lp_load8(p00 + C, b);
            lp_load8(p00 + (size_t)W * C, c);
            lp_load8(p00 + (size_t)W * C + C, d);
#pragma unroll
            for (int k = 0; k < 8; ++k) f[k] = lp_max4(lp_relu(a[k]), lp_relu(b[k]), lp_relu(c[k]), lp_relu(d[k]));
        } else {
            lp_load8(x + opix * C + 8 * j, f);
#pragma unroll
            for (int k = 0; k < 8; ++k) f[k] = lp_relu(f[k]);
        }
        if (SPLIT) lp_store8_split(reinterpret_cast<unsigned char*>(y) + opix * C * 4, j, f);
        else lp_store8(reinterpret_cast<float*>(y) + opix * C + 8 * j, f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------- tap
// v + (v of lane ^ m) for m = 1, 2 (quad permutes); for m = 4, 8 the mirrored half row / row, whose lanes hold the same value as lane ^ m once the
// narrower steps have been taken (every lane of a group of m lanes then holds that group's sum); m = 16, 32 cross the 16-lane rows through the
// LDS crossbar.  Taken in the order 1, 2, 4, ... this is the butterfly sum over L lanes, the same bits in every lane of the group.
template <int CTRL>
SSD_DEV float lp_dpp(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false)); }

template <int L>
SSD_DEV float lp_group_sum(float v) {
    if (L > 1) v += lp_dpp<0xB1>(v);                                         // quad_perm [1, 0, 3, 2]
    if (L > 2) v += lp_dpp<0x4E>(v);                                         // quad_perm [2, 3, 0, 1]
    if (L > 4) v += lp_dpp<0x141>(v);                                        // row_half_mirror
    if (L > 8) v += lp_dpp<0x140>(v);                                        // row_mirror
    if (L > 16) v += __shfl_xor(v, 16, 64);
    if (L > 32) v += __shfl_xor(v, 32, 64);
    return v;
}

// L = C / 8 lanes per pixel.  grid (blocks per pair, n); a lane group walks the pair's quads q = qy * Wq + qx (Hq x Wq = ceil(H / 2) x ceil(W / 2)); a pixel of
// the quad outside the image contributes nothing, and the pooled pixel (qy, qx) exists when the whole quad is inside (qy < Ho = H / 2, qx < Wo = W / 2).
// y == nullptr: no pooled output (the last tap).
template <int L, bool SPLIT>
__global__ void __launch_bounds__(LP_THREADS) k_lpips_layer(const float* __restrict__ x, uint32_t n, uint32_t H, uint32_t W, const float* __restrict__ lin_w,
                                                            void* __restrict__ y, double* __restrict__ partial) {
    constexpr uint32_t C = L * 8, GPB = LP_THREADS / L;                      // groups (quads in flight) per block
    __shared__ double red[LP_THREADS / 64];
    const uint32_t t = threadIdx.x, g = t / L, l = t % L;
    const uint32_t pair = blockIdx.y;
    const uint32_t Hq = (H + 1) / 2, Wq = (W + 1) / 2, Q = Hq * Wq, Ho = H / 2, Wo = W / 2;
    const float* __restrict__ xp = x + (size_t)pair * H * W * C + 8 * l;
    const float* __restrict__ xt = x + (size_t)(n + pair) * H * W * C + 8 * l;
    float wl[8];
    lp_load8(lin_w + 8 * l, wl);
    double acc = 0.0;
    // (the trip count is the same for every lane of the block: the shuffles below need all lanes of a wave)
    for (uint32_t q0 = blockIdx.x * GPB; q0 < Q; q0 += gridDim.x * GPB) {
        const uint32_t q = q0 + g;
        const bool q_ok = q < Q;
        const uint32_t qy = q / Wq, qx = q - qy * Wq;
        float fp[4][8], ft[4][8];
        bool ok[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t py = 2 * qy + (k >> 1), px = 2 * qx + (k & 1);
            ok[k] = q_ok && py < H && px < W;
            if (ok[k]) {
                const size_t off = ((size_t)py * W + px) * C;
                lp_load8(xp + off, fp[k]);
                lp_load8(xt + off, ft[k]);
            } else {
#pragma unroll
                for (int c = 0; c < 8; ++c) { fp[k][c] = 0.f; ft[k][c] = 0.f; }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float sp = 0.f, st = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                fp[k][c] = lp_relu(fp[k][c]);
                ft[k][c] = lp_relu(ft[k][c]);
                sp += fp[k][c] * fp[k][c];
                st += ft[k][c] * ft[k][c];
            }
            sp = lp_group_sum<L>(sp);
            st = lp_group_sum<L>(st);
            const float rp = 1.f / (sqrtf(sp) + 1e-10f), rt = 1.f / (sqrtf(st) + 1e-10f);
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float e = fp[k][c] * rp - ft[k][c] * rt;
                d += wl[c] * (e * e);
            }
            d = lp_group_sum<L>(d);
            if (ok[k]) acc += (double)d;                                     // (every lane of the group holds d: lane 0's copy is the one summed below)
        }
        if (y && q_ok && qy < Ho && qx < Wo) {
            float mp[8], mt[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                mp[c] = lp_max4(fp[0][c], fp[1][c], fp[2][c], fp[3][c]);
                mt[c] = lp_max4(ft[0][c], ft[1][c], ft[2][c], ft[3][c]);
            }
            const size_t op = ((size_t)pair * Ho + qy) * Wo + qx, ot = ((size_t)(n + pair) * Ho + qy) * Wo + qx;
            if (SPLIT) {
                lp_store8_split(reinterpret_cast<unsigned char*>(y) + op * C * 4, l, mp);
                lp_store8_split(reinterpret_cast<unsigned char*>(y) + ot * C * 4, l, mt);
            } else {
                lp_store8(reinterpret_cast<float*>(y) + op * C + 8 * l, mp);
                lp_store8(reinterpret_cast<float*>(y) + ot * C + 8 * l, mt);
            }
        }
    }
    // fixed order: the groups of a wave (one copy each: lane 0 of the group), butterfly over the wave, then the waves in index order
    if (l != 0) acc = 0.0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        double s = red[0];
        for (int k = 1; k < LP_THREADS / 64; ++k) s += red[k];
        partial[(size_t)pair * gridDim.x + blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(64) k_lpips_finish(const double* __restrict__ partial, uint32_t n, uint32_t blocks, double inv_pixels, float* __restrict__ acc) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (uint32_t b = 0; b < blocks; ++b) s += partial[(size_t)i * blocks + b];
    acc[i] += (float)(s * inv_pixels);
}

uint32_t lp_blocks_per_pair(uint32_t H, uint32_t W, uint32_t C) {
    const uint32_t Q = ((H + 1) / 2) * ((W + 1) / 2), gpb = LP_THREADS / (C / 8), b = (Q + gpb - 1) / gpb;
    return b < LP_MAX_BLOCKS_PER_PAIR ? b : LP_MAX_BLOCKS_PER_PAIR;
}

template <int L>
void lp_launch_layer(const float* x, uint32_t n, uint32_t H, uint32_t W, const float* lin_w, void* y, int split_out, double* partial, hipStream_t st) {
    const dim3 grid(lp_blocks_per_pair(H, W, L * 8), n);
    if (split_out) hipLaunchKernelGGL((k_lpips_layer<L, true>), grid, dim3(LP_THREADS), 0, st, x, n, H, W, lin_w, y, partial);
    else hipLaunchKernelGGL((k_lpips_layer<L, false>), grid, dim3(LP_THREADS), 0, st, x, n, H, W, lin_w, y, partial);
}

}  // namespace

extern "C" int ssdnerf_lpips_input(const float* pred, const float* target, uint32_t n, uint32_t h, uint32_t w, float* out, void* stream) {
    if (n == 0) return SSDNERF_OK;
    SSD_REQUIRE(pred && target && out, "lpips_input: null pointer");
    SSD_REQUIRE(h > 0 && w > 0 && (uint64_t)2 * n * h * w * 32 < (1ull << 31), "lpips_input: 2 x %u images of %u x %u x 8 floats do not stay below 2^31 bytes", n, h, w);
    SSD_REQUIRE((uintptr_t)out % 16 == 0, "lpips_input: the output must be 16-byte aligned");
    const uint32_t n_pix = n * h * w;
    hipLaunchKernelGGL(k_lpips_input, dim3(ssd_blocks((uint64_t)2 * n_pix, LP_THREADS)), dim3(LP_THREADS), 0, (hipStream_t)stream, pred, target, n_pix, out);
    SSD_CHECK_LAUNCH("lpips_input");
    return SSDNERF_OK;
}

extern "C" int ssdnerf_relu_pool_nhwc(const float* x, uint32_t N, uint32_t H, uint32_t W, uint32_t C, int pool, int split_out, void* y, void* stream) {
    if (N == 0) return SSDNERF_OK;
    SSD_REQUIRE(x && y, "relu_pool_nhwc: null pointer");
    SSD_REQUIRE(C > 0 && C % 8 == 0 && (!split_out || C % 32 == 0), "relu_pool_nhwc: C = %u must be a multiple of 8 (of 32 for the pre-split output)", C);
    SSD_REQUIRE(H > 0 && W > 0 && (!pool || (H >= 2 && W >= 2)), "relu_pool_nhwc: %u x %u is too small", H, W);
    SSD_REQUIRE((uint64_t)N * H * W * C * 4 < (1ull << 31), "relu_pool_nhwc: tensor of 2^31 bytes or more");
    SSD_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0, "relu_pool_nhwc: pointers must be 16-byte aligned");
    const uint32_t Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W, cpp = C / 8;
    const uint64_t total = (uint64_t)N * Ho * Wo * cpp, blocks = (total + LP_THREADS - 1) / LP_THREADS;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
    hipStream_t st = (hipStream_t)stream;
    if (pool && split_out) hipLaunchKernelGGL((k_relu_pool<true, true>), grid, dim3(LP_THREADS), 0, st, x, H, W, Ho, Wo, cpp, total, y);
    else if (pool) hipLaunchKernelGGL((k_relu_pool<true, false>), grid, dim3(LP_THREADS), 0, st, x, H, W, Ho, Wo, cpp, total, y);
    else if (split_out) hipLaunchKernelGGL((k_relu_pool<false, true>), grid, dim3(LP_THREADS), 0, st, x, H, W, Ho, Wo, cpp, total, y);
    else hipLaunchKernelGGL((k_relu_pool<false, false>), grid, dim3(LP_THREADS), 0, st, x, H, W, Ho, Wo, cpp, total, y);
    SSD_CHECK_LAUNCH("relu_pool_nhwc");
    return SSDNERF_OK;
}

extern "C" size_t ssdnerf_lpips_layer_workspace(uint32_t n) { return (size_t)n * LP_MAX_BLOCKS_PER_PAIR * sizeof(double); }

extern "C" int ssdnerf_lpips_layer(const float* x, uint32_t n, uint32_t H, uint32_t W, uint32_t C, const float* lin_w, float* acc, void* y_pool, int split_out,
                                   void* workspace, void* stream) {
    if (n == 0) return SSDNERF_OK;
    SSD_REQUIRE(x && lin_w && acc && workspace, "lpips_layer: null pointer");
    SSD_REQUIRE(C == 64 || C == 128 || C == 256 || C == 512, "lpips_layer: C = %u is not a VGG16 tap width (64, 128, 256, 512)", C);
    SSD_REQUIRE(H > 0 && W > 0 && n <= 65535u, "lpips_layer: needs H, W > 0 and at most 65535 pairs");
    SSD_REQUIRE(!y_pool || (H >= 2 && W >= 2), "lpips_layer: %u x %u is too small to pool", H, W);
    SSD_REQUIRE((uint64_t)2 * n * H * W * C * 4 < (1ull << 31), "lpips_layer: tensor of 2^31 bytes or more");
    SSD_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)lin_w % 16 == 0 && (uintptr_t)y_pool % 16 == 0 && (uintptr_t)workspace % 8 == 0, "lpips_layer: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)workspace;
    switch (C) {
        case 64: lp_launch_layer<8>(x, n, H, W, lin_w, y_pool, split_out, partial, st); break;
        case 128: lp_launch_layer<16>(x, n, H, W, lin_w, y_pool, split_out, partial, st); break;
        case 256: lp_launch_layer<32>(x, n, H, W, lin_w, y_pool, split_out, partial, st); break;
        default: lp_launch_layer<64>(x, n, H, W, lin_w, y_pool, split_out, partial, st); break;
    }
    hipLaunchKernelGGL(k_lpips_finish, dim3((n + 63) / 64), dim3(64), 0, st, (const double*)partial, n, lp_blocks_per_pair(H, W, C), 1.0 / ((double)H * W), acc);
    SSD_CHECK_LAUNCH("lpips_layer");
    return SSDNERF_OK;
}
