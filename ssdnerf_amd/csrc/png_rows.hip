// ssdnerf_amd/csrc/png_rows.hip -- what a PNG file needs per pixel and per row, in front of the host's deflate (ssdnerf_amd/viz.py):
//   k_png_filter_rows : N images (h, w, 3), fp32 or uint8, optionally beside a target on their left -> N streams of h filtered scanlines
//                       [type, 3 W bytes], the filter chosen per row by the PNG specification's minimum-sum-of-absolute-differences heuristic
//   k_code_plane_rgb  : triplane codes (S, 3, C, h, w) fp32 -> the reference's (3h, C w) plane sheet through a 256-entry colour table, uint8 RGB
// Nothing here compresses: every byte is a function of at most four input bytes (x, left, above, above-left) plus one choice per row.
//
// k_png_filter_rows: ONE WAVE PER ROW, four consecutive bytes of the row per lane and pass (256 bytes per wave-instruction: one float4 per lane from an
// fp32 operand, one dword from a uint8 one, where 3 w is a multiple of 4 and the operands are 16-byte aligned; byte by byte otherwise -- the same values).
// The bytes travel packed in a dword: the left neighbours (3 bytes back) of a lane's four bytes are its own dword and the lane below's, funnelled; lane 0
// takes lane 63 of the pass before.  The row is read twice -- once to score the five filters (five wave sums), once to write the winner -- and the row
// above is read by the wave of this row as well as by its own: per row 4 row-reads of which 3 hit in L2 (a 128 x 256 pair of rows is 6 KB of fp32).
// No atomics, no LDS; stores are byte stores because a stream's rows are 1 + 3 W bytes apart, which is odd.
#include "common.h"

#define SSD_PNG_BLOCK_CAP 2048u       /* 256 CUs x 8 blocks of 4 waves; the row loop strides over the rest */

struct PngOperand { const void* ptr; int is_u8; };

// bytes of fp32 operands.  pred: ssd_quant_u8 (clamp, x 255, round half to even: nerf's quantisation, k / 255 gives k back).  target: the reference's
// `(t * 255).to(torch.uint8)`, a truncation, behind a clamp of ours.  NaN -> 0 in both.
SSD_DEV uint32_t png_byte_pred(float v) { return v == v ? (uint32_t)ssd_quant_u8(v) : 0u; }
SSD_DEV uint32_t png_byte_target(float v) { return v == v ? (uint32_t)(uint8_t)(fminf(fmaxf(v, 0.f), 1.f) * 255.f) : 0u; }

// byte `e` (an element index) of an operand
template <bool TARGET>
SSD_DEV uint32_t png_load1(const PngOperand& op, uint64_t e) {
    if (op.is_u8) return ((const uint8_t*)op.ptr)[e];
    const float v = ((const float*)op.ptr)[e];
    return TARGET ? png_byte_target(v) : png_byte_pred(v);
}
// elements e .. e + 3 packed low byte first; e is a multiple of 4 and the operand 16-byte aligned
template <bool TARGET>
SSD_DEV uint32_t png_load4(const PngOperand& op, uint64_t e) {
    if (op.is_u8) return *(const uint32_t*)((const uint8_t*)op.ptr + e);
    const float4 v = *(const float4*)((const float*)op.ptr + e);
    if (TARGET) return png_byte_target(v.x) | png_byte_target(v.y) << 8 | png_byte_target(v.z) << 16 | png_byte_target(v.w) << 24;
    return png_byte_pred(v.x) | png_byte_pred(v.y) << 8 | png_byte_pred(v.z) << 16 | png_byte_pred(v.w) << 24;
}

// bytes i0 .. i0 + 3 of image row `row` (a row index over all images: its operand rows start at element row * w3) of the concatenated line
// [target (split bytes) | pred (L - split bytes)]; bytes at or beyond L are 0
template <bool VEC>
SSD_DEV uint32_t png_line4(const PngOperand& pred, const PngOperand& target, uint64_t row, uint32_t w3, uint32_t split, uint32_t L, uint32_t i0) {
    const uint64_t base = row * w3;
    if (VEC) {                                                          // split and L are multiples of 4: the four bytes share a side and a fate
        if (i0 >= L) return 0u;
        return i0 < split ? png_load4<true>(target, base + i0) : png_load4<false>(pred, base + (i0 - split));
    }
    uint32_t x = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = i0 + k;
        if (i < L) x |= (i < split ? png_load1<true>(target, base + i) : png_load1<false>(pred, base + (i - split))) << (8 * k);
    }
    return x;
}

SSD_DEV int png_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the five filtered values of byte x with left a, above b, above-left c (PNG specification, section 9: None, Sub, Up, Average, Paeth)
SSD_DEV void png_filter5(int x, int a, int b, int c, int r[5]) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    r[0] = x; r[1] = (x - a) & 255; r[2] = (x - b) & 255; r[3] = (x - ((a + b) >> 1)) & 255; r[4] = (x - paeth) & 255;
}

// the one of them a row was given; `type` is the same in every lane of the wave
SSD_DEV int png_filter1(int type, int x, int a, int b, int c) {
    if (type == 0) return x;
    if (type == 1) return (x - a) & 255;
    if (type == 2) return (x - b) & 255;
    if (type == 3) return (x - ((a + b) >> 1)) & 255;
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (x - ((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c))) & 255;
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_png_filter_rows(PngOperand pred, PngOperand target, uint64_t rows, uint32_t h, uint32_t w3, uint8_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t split = target.ptr ? w3 : 0u, L = split + w3;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t row = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < rows; row += waves) {
        const bool has_up = row % h != 0;
        int score[5] = {0, 0, 0, 0, 0};
        int type = 0;
        uint8_t* line = out + row * ((uint64_t)L + 1u);
        for (int phase = 0; phase < 2; ++phase) {                        // 0: score the five filters; 1: write the winner
            uint32_t carry_x = 0u, carry_b = 0u;                         // the dword in front of lane 0's: nothing in front of the first pixel
            for (uint32_t p0 = 0; p0 < L; p0 += 256u) {
                const uint32_t i0 = p0 + 4u * lane;
                const uint32_t x4 = png_line4<VEC>(pred, target, row, w3, split, L, i0);
                const uint32_t b4 = has_up ? png_line4<VEC>(pred, target, row - 1, w3, split, L, i0) : 0u;
                uint32_t px = __shfl_up(x4, 1, 64), pb = __shfl_up(b4, 1, 64);
                if (lane == 0) { px = carry_x; pb = carry_b; }
                carry_x = __shfl(x4, 63, 64);
                carry_b = __shfl(b4, 63, 64);
                const uint32_t a4 = px >> 8 | x4 << 24, c4 = pb >> 8 | b4 << 24;      // bytes i0 - 3 .. i0 of the line and of the line above
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = x4 >> (8 * k) & 255, a = a4 >> (8 * k) & 255, b = b4 >> (8 * k) & 255, c = c4 >> (8 * k) & 255;
                    if (i0 + k >= L) continue;
                    if (phase == 0) {
                        int r[5];
                        png_filter5(x, a, b, c, r);
#pragma unroll
                        for (int t = 0; t < 5; ++t) score[t] += r[t] < 256 - r[t] ? r[t] : 256 - r[t];
                    } else {
                        line[1u + i0 + k] = (uint8_t)png_filter1(type, x, a, b, c);
                    }
                }
            }
            if (phase == 0) {
                int best = png_wave_sum(score[0]);
#pragma unroll
                for (int t = 1; t < 5; ++t) {
                    const int s = png_wave_sum(score[t]);
                    if (s < best) { best = s; type = t; }               // strictly less: a tie stays with the lower filter number
                }
                if (lane == 0) line[0] = (uint8_t)type;
            }
        }
    }
}

extern "C" int ssdnerf_png_filter_rows(const void* pred, int pred_is_u8, const void* target, int target_is_u8, uint32_t n, uint32_t h, uint32_t w,
                                       uint8_t* out, void* stream) {
    if (n == 0) return SSDNERF_OK;
    SSD_REQUIRE(pred && out, "png_filter_rows: null pointer");
    SSD_REQUIRE(h >= 1 && w >= 1 && w <= (1u << 28), "png_filter_rows: h >= 1 and 1 <= w <= 2^28 are needed (got %u x %u)", h, w);
    const PngOperand p = {pred, pred_is_u8 != 0}, t = {target, target_is_u8 != 0};
    const uint32_t w3 = 3u * w;
    const uint64_t rows = (uint64_t)n * h;
    auto aligned = [](const PngOperand& o) { return o.ptr == nullptr || (uintptr_t)o.ptr % (o.is_u8 ? 4u : 16u) == 0; };
    const bool vec = w3 % 4u == 0 && aligned(p) && aligned(t);
    const unsigned blocks = (unsigned)((rows + 3) / 4 < SSD_PNG_BLOCK_CAP ? (rows + 3) / 4 : SSD_PNG_BLOCK_CAP);
    if (vec) hipLaunchKernelGGL(k_png_filter_rows<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, t, rows, h, w3, out);
    else hipLaunchKernelGGL(k_png_filter_rows<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, t, rows, h, w3, out);
    SSD_CHECK_LAUNCH("png_filter_rows");
    return SSDNERF_OK;
}

// ---- code planes ---------------------------------------------------------------------------------------------------------------------------------
// decoder.visualize (triplane_decoder.py:186-194): rows reversed within each plane unless flip_z, (S, 3, C, h, w) -> (S, 3, h, C, w) -> (S, 3h, C w),
// then matplotlib's mapping of a float32 array through a 256-entry table: t = (x - vmin) / (vmax - vmin) in fp32 (IEEE division), NaN -> black,
// t < 0 -> entry 0, t >= 1 -> entry 255, else entry (int)(t * 256) (the product by 256 is exact).  One lane per output pixel; x runs fastest.
__global__ void __launch_bounds__(256) k_code_plane_rgb(const float* __restrict__ code, const uint8_t* __restrict__ table, uint64_t pixels, uint32_t C,
                                                        uint32_t h, uint32_t w, float vmin, float vmax, int flip_z, uint8_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const float range = vmax - vmin;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {
        const uint32_t x = (uint32_t)(i % w);
        uint64_t q = i / w;
        const uint32_t c = (uint32_t)(q % C); q /= C;
        const uint32_t y = (uint32_t)(q % h); q /= h;                    // q = s * 3 + plane
        const uint32_t ys = flip_z ? y : h - 1u - y;
        const float v = code[((q * C + c) * h + ys) * w + x];
        const float t = (v - vmin) / range;
        uint32_t r = 0u, g = 0u, b = 0u;
        if (t == t) {
            const uint32_t e = t < 0.f ? 0u : t >= 1.f ? 255u : (uint32_t)(t * 256.f);
            r = table[3u * e]; g = table[3u * e + 1u]; b = table[3u * e + 2u];
        }
        out[3u * i] = (uint8_t)r; out[3u * i + 1u] = (uint8_t)g; out[3u * i + 2u] = (uint8_t)b;
    }
}

extern "C" int ssdnerf_code_plane_rgb(const float* code, const uint8_t* table, uint32_t S, uint32_t C, uint32_t h, uint32_t w, float vmin, float vmax,
                                      int flip_z, uint8_t* out, void* stream) {
    if (S == 0) return SSDNERF_OK;
    SSD_REQUIRE(code && table && out, "code_plane_rgb: null pointer");
    SSD_REQUIRE(C >= 1 && h >= 1 && w >= 1, "code_plane_rgb: C, h, w >= 1 are needed");
    const uint64_t pixels = (uint64_t)S * 3u * C * h * w;
    SSD_REQUIRE(pixels < (1ull << 40), "code_plane_rgb: %llu pixels", (unsigned long long)pixels);
    const unsigned blocks = (unsigned)((pixels + 255) / 256 < SSD_PNG_BLOCK_CAP ? (pixels + 255) / 256 : SSD_PNG_BLOCK_CAP);
    hipLaunchKernelGGL(k_code_plane_rgb, dim3(blocks), dim3(256), 0, (hipStream_t)stream, code, table, pixels, C, h, w, vmin, vmax, flip_z, out);
    SSD_CHECK_LAUNCH("code_plane_rgb");
    return SSDNERF_OK;
}
