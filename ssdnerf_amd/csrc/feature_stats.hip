// ssdnerf_amd/csrc/feature_stats.hip -- everything behind the feature extractor of FID / KID (reference: FIDKID, lib/core/evaluation/metrics.py:135-215,
// which keeps all features on the host, runs np.cov over them and forms 100 x 3 Gram matrices of 1000 x 1000 in float32 numpy).
//
//   k_feature_moments   sum[D] += sum_k x_k,  outer[D][D] += X^T X  of one (n, D) fp32 batch, in fp64: what mean and np.cov need, accumulated as the
//                       views are rendered.
//   k_kid_tiles /       per subset the three sums of KID's cubic kernel  (x_i . y_j / D + 1)^3  over gathered rows of the two feature stores, in fp64,
//   k_kid_finish        without a Gram matrix in memory.
//
// Both run on v_mfma_f64_16x16x4_f64.  Every fp32 input is converted to fp64 once, on its way into LDS; the product of two fp32 values is exact in fp64, so
// only the summation rounds.  Operand / result layout of this instruction (it is NOT the one of the f32 / bf16 forms used by conv_igemm.hip):
//   A: lane l holds A[row l & 15][k = l >> 4]      B: lane l holds B[k = l >> 4][col l & 15]
//   C/D: register r of lane l is element [row (l >> 4) + 4 r][col l & 15]
// Shape of both: a workgroup of 4 waves owns one 64 x 64 tile of the result, a wave one 32 x 32 quadrant of it as 2 x 2 MFMA tiles (16 fp64 accumulators per
// lane); the K dimension is walked FS_KC values at a time through LDS, the next step's global loads in flight in registers while this one is multiplied.
// No atomics anywhere: a result element has one owner, partial sums are added in a fixed order -- bit-identical from run to run.
#include "common.h"

typedef double fs_d4 __attribute__((ext_vector_type(4)));

#define FS_TILE 64
#define FS_THREADS 256
#define FS_KC 32                       // K values staged per step
#define FS_PER_THREAD (FS_TILE * FS_KC / FS_THREADS)
// LDS row strides in doubles, chosen so that the 32 lanes of one ds_read_b64 pass (16 rows / columns x 2 k) fall into 64 distinct 4-byte banks:
#define FM_LD 80                       // moments: [k][column]; k and k + 1 are 640 B apart = 128 B modulo the 256 B of all banks
#define KS_LD 34                       // KID:     [row][k];    rows are 272 B apart = 4 banks modulo 64, k and k + 1 two banks

SSD_DEV fs_d4 fs_mfma(double a, double b, fs_d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// tile t of the upper triangle of a T x T tile grid, row by row: (0,0) (0,1) ... (0,T-1) (1,1) ...
SSD_DEV void fs_tri_tile(uint32_t t, uint32_t T, uint32_t& ti, uint32_t& tj) {
    ti = 0;
    while (t >= T - ti) {
        t -= T - ti;
        ++ti;
    }
    tj = ti + t;
}

// ------------------------------------------------------------------------------------------------ (a) moments
// outer = X^T X: A = X^T (A[row i][k] = x[k][i]), B = X (B[k][col j] = x[k][j]); tiles with tj >= ti only (diagonal tiles are written whole).  The diagonal
// tiles also own the column sums of their 64 columns: every thread adds the values it stages (rows sr, sr + 4, ... of its column) as they pass, and the four
// row classes of a column are added in index order at the end.
__global__ void __launch_bounds__(FS_THREADS) k_feature_moments(const float* __restrict__ x, uint32_t n, uint32_t D, uint32_t T, double* __restrict__ sum,
                                                                double* __restrict__ outer) {
    __shared__ double sa[FS_KC][FM_LD], sb[FS_KC][FM_LD];
    uint32_t ti, tj;
    fs_tri_tile(blockIdx.x, T, ti, tj);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t i0 = ti * FS_TILE, j0 = tj * FS_TILE;
    const uint32_t wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    const uint32_t sr = tid >> 6, sc = tid & 63;              // staging: value e of this thread is row sr + 4 e, column sc of the step
    const bool in_i = i0 + sc < D, in_j = j0 + sc < D;

    fs_d4 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = fs_d4{0.0, 0.0, 0.0, 0.0};
    const bool diag = ti == tj;
    double csum = 0.0;
    float pa[FS_PER_THREAD], pb[FS_PER_THREAD];
    auto fetch = [&](uint32_t k0) {
#pragma unroll
        for (int e = 0; e < FS_PER_THREAD; ++e) {
            const uint32_t row = k0 + sr + 4 * e;
            const float* xr = x + (size_t)row * D;
            pa[e] = (row < n && in_i) ? xr[i0 + sc] : 0.f;      // rows past n and columns past D are zero: they add +0 exactly
            pb[e] = (row < n && in_j) ? xr[j0 + sc] : 0.f;
        }
    };
    fetch(0);
    for (uint32_t k0 = 0; k0 < n; k0 += FS_KC) {
#pragma unroll
        for (int e = 0; e < FS_PER_THREAD; ++e) {
            sa[sr + 4 * e][sc] = (double)pa[e];
            sb[sr + 4 * e][sc] = (double)pb[e];
            if (diag) csum += (double)pa[e];
        }
        if (k0 + FS_KC < n) fetch(k0 + FS_KC);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < FS_KC; kk += 4) {
            const uint32_t kr = kk + (lane >> 4), c = lane & 15;
            const double a0 = sa[kr][wi + c], a1 = sa[kr][wi + 16 + c];
            const double b0 = sb[kr][wj + c], b1 = sb[kr][wj + 16 + c];
            acc[0][0] = fs_mfma(a0, b0, acc[0][0]);
            acc[0][1] = fs_mfma(a0, b1, acc[0][1]);
            acc[1][0] = fs_mfma(a1, b0, acc[1][0]);
            acc[1][1] = fs_mfma(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }

#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t row = i0 + wi + 16 * p + (lane >> 4) + 4 * r, col = j0 + wj + 16 * q + (lane & 15);
                if (row < D && col < D) outer[(size_t)row * D + col] += acc[p][q][r];
            }
    if (diag) {                                               // (uniform over the block; the K loop ended in a barrier)
        sa[sr][sc] = csum;
        __syncthreads();
        if (tid < FS_TILE && i0 + tid < D) sum[i0 + tid] += ((sa[0][tid] + sa[1][tid]) + sa[2][tid]) + sa[3][tid];
    }
}

extern "C" int ssdnerf_feature_moments_accumulate(const float* x, uint32_t n, uint32_t D, double* sum, double* outer, void* stream) {
    SSD_REQUIRE(sum && outer, "feature_moments_accumulate: null accumulator");
    SSD_REQUIRE(D > 0 && D <= (1u << 20), "feature_moments_accumulate: feature dimension %u is outside [1, 2^20]", D);
    if (n == 0) return SSDNERF_OK;
    SSD_REQUIRE(x, "feature_moments_accumulate: null feature pointer");
    const uint32_t T = (D + FS_TILE - 1) / FS_TILE;
    hipLaunchKernelGGL(k_feature_moments, dim3(T * (T + 1) / 2), dim3(FS_THREADS), 0, (hipStream_t)stream, x, n, D, T, sum, outer);
    SSD_CHECK_LAUNCH("feature_moments_accumulate");
    return SSDNERF_OK;
}

// ------------------------------------------------------------------------------------------------ (b) KID subset sums
// Blocks of one subset (blockIdx.y), in this order: the T (T + 1) / 2 upper tiles of xx, the same of yy, the T^2 tiles of xy, T = ceil(m / 64).
// A[row i][k] = (row idx_a[i] of store a)[k], B[k][col j] = (row idx_b[j] of store b)[k].  An off-diagonal tile of xx / yy stands for its mirror image too
// (x 2, exact); position i == j is left out of xx / yy whatever rows the two positions hold.
__host__ __device__ static inline uint32_t ks_blocks(uint32_t T) { return T * (T + 1) + T * T; }

__global__ void __launch_bounds__(FS_THREADS) k_kid_tiles(const float* __restrict__ fake, const float* __restrict__ real, const int64_t* __restrict__ idx_f,
                                                          const int64_t* __restrict__ idx_r, uint32_t m, uint32_t D, uint32_t T, double* __restrict__ partial) {
    __shared__ double sa[FS_TILE][KS_LD], sb[FS_TILE][KS_LD];
    __shared__ double red[FS_THREADS / 64];
    const uint32_t tri = T * (T + 1) / 2;
    uint32_t t = blockIdx.x, kind, ti, tj;
    if (t < 2 * tri) {
        kind = t >= tri ? 1u : 0u;
        fs_tri_tile(t - kind * tri, T, ti, tj);
    } else {
        kind = 2;
        t -= 2 * tri;
        ti = t / T;
        tj = t - ti * T;
    }
    const float* __restrict__ A = kind == 1 ? real : fake;
    const float* __restrict__ B = kind == 0 ? fake : real;
    const int64_t* __restrict__ ia = (kind == 1 ? idx_r : idx_f) + (size_t)blockIdx.y * m;
    const int64_t* __restrict__ ib = (kind == 0 ? idx_f : idx_r) + (size_t)blockIdx.y * m;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t i0 = ti * FS_TILE, j0 = tj * FS_TILE;
    const uint32_t wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    const uint32_t sr = tid >> 5, sc = tid & 31;              // staging: value e of this thread is tile row sr + 8 e, k offset sc of the step

    const float* ra[FS_PER_THREAD];
    const float* rb[FS_PER_THREAD];                           // the gathered rows this thread stages (null: past the subset, staged as zeros)
#pragma unroll
    for (int e = 0; e < FS_PER_THREAD; ++e) {
        const uint32_t r = sr + 8 * e;
        ra[e] = i0 + r < m ? A + (size_t)ia[i0 + r] * D : nullptr;
        rb[e] = j0 + r < m ? B + (size_t)ib[j0 + r] * D : nullptr;
    }
    fs_d4 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = fs_d4{0.0, 0.0, 0.0, 0.0};
    float pa[FS_PER_THREAD], pb[FS_PER_THREAD];
    auto fetch = [&](uint32_t k0) {
        const bool in_k = k0 + sc < D;
#pragma unroll
        for (int e = 0; e < FS_PER_THREAD; ++e) {
            pa[e] = (ra[e] && in_k) ? ra[e][k0 + sc] : 0.f;
            pb[e] = (rb[e] && in_k) ? rb[e][k0 + sc] : 0.f;
        }
    };
    fetch(0);
    for (uint32_t k0 = 0; k0 < D; k0 += FS_KC) {
#pragma unroll
        for (int e = 0; e < FS_PER_THREAD; ++e) {
            sa[sr + 8 * e][sc] = (double)pa[e];
            sb[sr + 8 * e][sc] = (double)pb[e];
        }
        if (k0 + FS_KC < D) fetch(k0 + FS_KC);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < FS_KC; kk += 4) {
            const uint32_t kc = kk + (lane >> 4), r = lane & 15;
            const double a0 = sa[wi + r][kc], a1 = sa[wi + 16 + r][kc];
            const double b0 = sb[wj + r][kc], b1 = sb[wj + 16 + r][kc];
            acc[0][0] = fs_mfma(a0, b0, acc[0][0]);
            acc[0][1] = fs_mfma(a0, b1, acc[0][1]);
            acc[1][0] = fs_mfma(a1, b0, acc[1][0]);
            acc[1][1] = fs_mfma(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }

    // (dot / D + 1)^3 of the positions this lane holds, summed in registers
    const double Dd = (double)D;
    double part = 0.0;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t gi = i0 + wi + 16 * p + (lane >> 4) + 4 * r, gj = j0 + wj + 16 * q + (lane & 15);
                const double v = acc[p][q][r] / Dd + 1.0;
                const double c = (v * v) * v;
                const bool counted = gi < m && gj < m && (kind == 2 || gi != gj);
                part += counted ? c : 0.0;
            }
    if (kind != 2 && ti != tj) part *= 2.0;
    // fixed-order reduction: butterfly within each wave, then the waves in index order
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) part += __shfl_xor(part, s);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (tid == 0) partial[(size_t)blockIdx.y * ks_blocks(T) + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one block per subset, wave k adds the partial sums of kind k (xx, yy, xy): lane l takes blocks l, l + 64, ... in order, then a butterfly
__global__ void __launch_bounds__(192) k_kid_finish(const double* __restrict__ partial, uint32_t T, double* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63, kind = threadIdx.x >> 6;
    const uint32_t tri = T * (T + 1) / 2;
    const uint32_t lo = kind * tri, cnt = kind == 2 ? T * T : tri;
    const double* p = partial + (size_t)blockIdx.x * ks_blocks(T) + lo;
    double s = 0.0;
    for (uint32_t i = lane; i < cnt; i += 64) s += p[i];
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k);
    if (lane == 0) out[(size_t)blockIdx.x * 3 + kind] = s;
}

extern "C" size_t ssdnerf_kid_subset_sums_workspace(uint32_t num_subsets, uint32_t m) {
    const uint32_t T = (m + FS_TILE - 1) / FS_TILE;
    return (size_t)num_subsets * ks_blocks(T) * sizeof(double);
}

extern "C" int ssdnerf_kid_subset_sums(const float* fake, const float* real, const int64_t* idx_fake, const int64_t* idx_real, uint32_t num_subsets, uint32_t m,
                                       uint32_t D, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    SSD_REQUIRE(fake && real && idx_fake && idx_real && out && workspace, "kid_subset_sums: null pointer");
    SSD_REQUIRE(num_subsets > 0 && num_subsets <= 65535, "kid_subset_sums: %u subsets are outside [1, 65535]", num_subsets);
    SSD_REQUIRE(m >= 2 && m <= (1u << 20), "kid_subset_sums: subset size %u is outside [2, 2^20]", m);
    SSD_REQUIRE(D > 0, "kid_subset_sums: feature dimension 0");
    SSD_REQUIRE(((uintptr_t)workspace & 7) == 0, "kid_subset_sums: the workspace must be 8-byte aligned");
    if (workspace_bytes < ssdnerf_kid_subset_sums_workspace(num_subsets, m))
        return ssdnerf_fail(SSDNERF_E_WORKSPACE, "kid_subset_sums: workspace of %zu bytes, %zu needed", workspace_bytes,
                            ssdnerf_kid_subset_sums_workspace(num_subsets, m));
    const uint32_t T = (m + FS_TILE - 1) / FS_TILE;
    hipLaunchKernelGGL(k_kid_tiles, dim3(ks_blocks(T), num_subsets), dim3(FS_THREADS), 0, (hipStream_t)stream, fake, real, idx_fake, idx_real, m, D, T,
                       (double*)workspace);
    SSD_CHECK_LAUNCH("kid_subset_sums (tiles)");
    hipLaunchKernelGGL(k_kid_finish, dim3(num_subsets), dim3(192), 0, (hipStream_t)stream, (const double*)workspace, T, out);
    SSD_CHECK_LAUNCH("kid_subset_sums (finish)");
    return SSDNERF_OK;
}
