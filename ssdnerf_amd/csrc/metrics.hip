// ssdnerf_amd/csrc/metrics.hip -- test-view scores of a reconstruction (reference: eval_psnr / eval_ssim_skimage, lib/core/evaluation/metrics.py:52-71,
// as BaseNeRF.eval_and_viz calls them, lib/models/autodecoders/base_nerf.py:555-558).
//
// For each of n image pairs a, b ([n][h][w][3] fp32, channel-last) one pass gives
//   mse[i]  = mean over h*w*3 of (a - b)^2                                      (fp64 accumulation)
//   ssim[i] = skimage.metrics.structural_similarity(channel_axis, data_range=1): per channel the mean over the pixels whose 7 x 7 window lies
//             inside the image (rows and columns [3, h-4] / [3, w-4]) of
//                 S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),   C1 = 0.01^2, C2 = 0.03^2,
//             u* = 7 x 7 window means of x, y, x^2, y^2, xy, vx = 49/48 (uxx - ux^2), vy, vxy alike; then the mean of the 3 channel values.
// Numerics: the five window sums and the three covariances are fp64 -- the products of fp32 values are exact there, and the
// E[x^2] - E[x]^2 cancellation of a bright, nearly flat window (+-1/255) costs fp32 up to 6.5e-5 of SSIM per image; S itself is fp32.
//
// Shape: one workgroup per image, one thread per (output column, channel) of a tile of IM_P columns.  The workgroup slides down the rows: row r of
// the tile (plus 3 halo columns on each side) is staged once in LDS as fp64, each thread forms its 7-tap horizontal sums from LDS into a 7-row
// ring in registers, and from row 6 on sums the ring vertically (recomputed each row, never kept running).  Images wider than IM_P + 6 columns
// are walked tile by tile.  The sums end in a fixed-order block reduction: no atomics, bit-identical from run to run.
#include "common.h"

#define IM_P 128                      // output columns per tile
#define IM_THREADS (3 * IM_P)         // one thread per (column, channel) of the tile
#define IM_ROW (3 * (IM_P + 6))       // values of one staged tile row: the tile's columns and 3 halo columns on each side

__global__ void __launch_bounds__(IM_THREADS) k_image_metrics(const float* __restrict__ a, const float* __restrict__ b, uint32_t h, uint32_t w,
                                                              float* __restrict__ mse, float* __restrict__ ssim) {
    __shared__ double sx[2][IM_ROW], sy[2][IM_ROW];        // double-buffered rows: one barrier per row
    __shared__ double red[2][IM_THREADS / 64];
    const uint32_t t = threadIdx.x;
    const size_t row_len = (size_t)w * 3;
    const float* __restrict__ A = a + (size_t)blockIdx.x * h * row_len;
    const float* __restrict__ B = b + (size_t)blockIdx.x * h * row_len;
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const double cov = (49.0 / 48.0) / (49.0 * 49.0);       // vx = cov * (49 Sxx - Sx^2) with window sums S*

    double sse = 0.0, s_sum = 0.0;
    const uint32_t tiles = (w - 7) / IM_P + 1;               // tile k: output columns 3 + k P ... ; the last tile holds column w - 4
    for (uint32_t tile = 0; tile < tiles; ++tile) {
        const uint32_t x0 = tile * IM_P;
        const uint32_t cnt = 3 * min((uint32_t)(IM_P + 6), w - x0);      // staged values of a row
        const uint32_t own = tile + 1 == tiles ? cnt : 3 * IM_P;   // of which this tile counts into mse (the halo belongs to the next tile)
        const bool valid = x0 + 3 + t / 3 <= w - 4;          // this thread's output column has its window inside the image
        float xa0, xa1, yb0, yb1;                            // row prefetch: values t and t + IM_THREADS of the staged row
        auto fetch = [&](uint32_t r) {
            const float* ra = A + r * row_len + 3 * x0;
            const float* rb = B + r * row_len + 3 * x0;
            xa0 = t < cnt ? ra[t] : 0.f;
            yb0 = t < cnt ? rb[t] : 0.f;
            xa1 = t + IM_THREADS < cnt ? ra[t + IM_THREADS] : 0.f;
            yb1 = t + IM_THREADS < cnt ? rb[t + IM_THREADS] : 0.f;
        };
        fetch(0);
        double hx[7], hy[7], hxx[7], hyy[7], hxy[7];         // horizontal sums of the last 7 rows (slot k: rows r with r % 7 == k)
        for (uint32_t r0 = 0; r0 < h; r0 += 7) {
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const uint32_t r = r0 + k;
                if (r >= h) break;
                const int buf = r & 1;
                sx[buf][t] = (double)xa0;
                sy[buf][t] = (double)yb0;
                if (t + IM_THREADS < IM_ROW) {
                    sx[buf][t + IM_THREADS] = (double)xa1;
                    sy[buf][t + IM_THREADS] = (double)yb1;
                }
                if (t < own) {
                    const double d = (double)xa0 - (double)yb0;
                    sse = __builtin_fma(d, d, sse);
                }
                if (t + IM_THREADS < own) {
                    const double d = (double)xa1 - (double)yb1;
                    sse = __builtin_fma(d, d, sse);
                }
                if (r + 1 < h) fetch(r + 1);                 // in flight while this row is summed
                __syncthreads();
                // 7-tap horizontal sums around column x0 + 3 + t / 3: values t, t + 3, ..., t + 18 of the staged row (fp32 products are exact in fp64)
                double x = sx[buf][t], y = sy[buf][t];
                double px = x, py = y, pxx = x * x, pyy = y * y, pxy = x * y;
#pragma unroll
                for (int j = 1; j < 7; ++j) {
                    x = sx[buf][t + 3 * j];
                    y = sy[buf][t + 3 * j];
                    px += x;
                    py += y;
                    pxx = __builtin_fma(x, x, pxx);
                    pyy = __builtin_fma(y, y, pyy);
                    pxy = __builtin_fma(x, y, pxy);
                }
                hx[k] = px; hy[k] = py; hxx[k] = pxx; hyy[k] = pyy; hxy[k] = pxy;
                if (r >= 6 && valid) {
                    double Sx = hx[0], Sy = hy[0], Sxx = hxx[0], Syy = hyy[0], Sxy = hxy[0];
#pragma unroll
                    for (int q = 1; q < 7; ++q) {
                        Sx += hx[q]; Sy += hy[q]; Sxx += hxx[q]; Syy += hyy[q]; Sxy += hxy[q];
                    }
                    const float ux = (float)(Sx * (1.0 / 49.0)), uy = (float)(Sy * (1.0 / 49.0));
                    const float vx = (float)(__builtin_fma(-Sx, Sx, 49.0 * Sxx) * cov);
                    const float vy = (float)(__builtin_fma(-Sy, Sy, 49.0 * Syy) * cov);
                    const float vxy = (float)(__builtin_fma(-Sx, Sy, 49.0 * Sxy) * cov);
                    const float num = (2.f * ux * uy + C1) * (2.f * vxy + C2);
                    const float den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
                    s_sum += (double)(num / den);
                }
            }
        }
        __syncthreads();                                     // the next tile's first row overwrites a buffer this tile's last row may still be read from
    }

    // fixed-order reduction: butterfly within each wave, then the waves in index order
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sse += __shfl_xor(sse, m);
        s_sum += __shfl_xor(s_sum, m);
    }
    if ((t & 63) == 0) {
        red[0][t >> 6] = sse;
        red[1][t >> 6] = s_sum;
    }
    __syncthreads();
    if (t == 0) {
        double e = red[0][0], s = red[1][0];
        for (int i = 1; i < IM_THREADS / 64; ++i) {
            e += red[0][i];
            s += red[1][i];
        }
        mse[blockIdx.x] = (float)(e / ((double)h * w * 3));
        ssim[blockIdx.x] = (float)(s / (3.0 * (h - 6) * (w - 6)));
    }
}

extern "C" int ssdnerf_image_metrics(const float* a, const float* b, uint32_t n, uint32_t h, uint32_t w, float* mse, float* ssim, void* stream) {
    SSD_REQUIRE(a && b && mse && ssim, "image_metrics: null pointer");
    SSD_REQUIRE(n > 0, "image_metrics: n == 0 (no image pairs)");
    SSD_REQUIRE(h >= 7 && w >= 7, "image_metrics: images of %u x %u are smaller than the 7 x 7 SSIM window", h, w);
    hipLaunchKernelGGL(k_image_metrics, dim3(n), dim3(IM_THREADS), 0, (hipStream_t)stream, a, b, h, w, mse, ssim);
    SSD_CHECK_LAUNCH("image_metrics");
    return SSDNERF_OK;
}
