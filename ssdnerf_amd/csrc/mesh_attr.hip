// ssdnerf_amd/csrc/mesh_attr.hip -- surface attributes at the vertices of an extracted mesh.
//
// The reference's `save_mesh` (lib/models/autodecoders/base_nerf.py:172-182) writes the bare marching-cubes geometry.  The radiance field knows
// more at every surface vertex: the density gradient, whose direction is the exact surface normal of the iso-surface, and a colour.  One lane per
// vertex, next to the decode the fused path already has (decode_core.h: same gather, same weights as wave-uniform scalar operands):
//
//   p       = fma(v, scale, b_min)                       index coordinates of marching_cubes.hip -> world (these go to the file)
//   f, J    = the 18 bilinear features (ssd_gather18's arithmetic, the fraction more exactly: ma_grid_coord) and their derivatives in the two
//             coordinates each plane reads:
//             df/du = (W/2) [wy0 (t01 - t00) + wy1 (t11 - t10)],  df/dv = (H/2) [wx0 (t10 - t00) + wx1 (t11 - t01)]  (texels are subtracted FIRST:
//             neighbouring texels of a smooth plane nearly cancel, and the error bound of tests/_mesh_attr_ref.py is written on the differences),
//             exactly 0 on an axis whose unnormalised coordinate was clipped -- ATen's grid_sample backward for padding_mode='border', which counts
//             the borders themselves (ix <= 0, ix >= W - 1) as clipped
//   sigma   = exp(b_s + sum_i w_s[i] silu(h_i)),  D_k = sum_i w_s[i] silu'(h_i) W1[i][k],  silu'(h) = s (1 + h (1 - s)), s = sigmoid(h)
//   grad    = sigma J^T D,   n = -grad / |grad|  (density falls towards the outside: the orientation of mesh.py's triangle winding);  grad == 0 -> n = 0
//   colour  = the decoder's rgb at p for the view direction d = -n, i.e. seen head-on from outside (d = (0, 0, 1) where n = 0): ssd_mlp<1>, which
//             recomputes the 64 hidden units -- 1.2 k FMAs a vertex on 10^4 - 10^5 vertices
//
// No LDS, no matrix cores, no atomics: a lane's results depend on its own vertex only, so two calls return the same bits.  Plain vector stores.
#include "decode_core.h"

namespace {

constexpr unsigned MA_TPB = 256;

struct MeshMap { float b_min[3], scale[3]; };

// ssd_grid_coord's cell and ATen's clip rule (clip_coordinates_set_grad), with the bilinear FRACTION formed in one rounding.  The unnormalised
// coordinate ix = ((u + 1) W - 1) / 2 is an fp32 number of magnitude up to W: its own spacing (7.6e-6 at ix = 100) moves the sample point by up to
// 4e-6 texel units, and on a steep plane (a silhouette edge two texels wide) that alone is 2e-5 of sigma and 500 u A of the gradient -- ATen's fp32
// grid_sample carries the same error (tests/_mesh_attr_ref.py).  The cell index needs ix only to the integer; the fraction is
// fma(u, W/2, (W-1)/2 - floor(ix)), exact up to one rounding BELOW 1.  Where the two disagree about the cell (ix within its spacing of an integer) the
// cell follows the fraction.
SSD_DEV void ma_grid_coord(float u, float size_f, uint32_t size, uint32_t& i0, uint32_t& i1, float& w0, float& w1, float& dscale) {
    const float raw = ((u + 1.0f) * size_f - 1.0f) * 0.5f;
    const bool moves = raw > 0.0f && raw < size_f - 1.0f;
    dscale = moves ? size_f * 0.5f : 0.0f;
    const float ix = fminf(size_f - 1.0f, fmaxf(raw, 0.0f));
    float fl = floorf(ix);
    float w = ix - fl;                                                   // clipped: 0 on either border
    if (moves) {
        w = ssd_fma(u, size_f * 0.5f, (size_f - 1.0f) * 0.5f - fl);      // (W-1)/2 - fl is exact: half-integers below 2^23
        if (w < 0.0f && fl > 0.0f) { fl -= 1.0f; w += 1.0f; }
        else if (w >= 1.0f && fl < size_f - 1.0f) { fl += 1.0f; w -= 1.0f; }
        w = fminf(fmaxf(w, 0.0f), 1.0f);
    }
    i0 = (uint32_t)fl;                                                   // 0 <= fl <= size - 1 on every path
    i1 = min(i0 + 1u, size - 1u);                                        // the out-of-range neighbour only ever carries weight 0
    w1 = w;
    w0 = 1.0f - w;
}

// f by ssd_gather18's four-term chain (weights from ma_grid_coord), fu / fv its derivatives in the plane's width / height coordinate
template <typename PT>
SSD_DEV void ma_gather18_jac(const PT* __restrict__ planes, const PlaneGeom& g, float x, float y, float z, float f[18], float fu[18], float fv[18]) {
    const float us[3] = {x, x, y};
    const float vs[3] = {y, z, z};
    const uint64_t plane_stride = (uint64_t)g.Hp * g.Wp * 8;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        uint32_t x0, x1, y0, y1;
        float wx0, wx1, wy0, wy1, su, sv;
        ma_grid_coord(us[p], g.Wf, g.Wp, x0, x1, wx0, wx1, su);
        ma_grid_coord(vs[p], g.Hf, g.Hp, y0, y1, wy0, wy1, sv);
        const PT* base = planes + p * plane_stride;
        float t00[6], t01[6], t10[6], t11[6];
        Texel<PT>::load6(base + ((uint64_t)y0 * g.Wp + x0) * 8, t00);
        Texel<PT>::load6(base + ((uint64_t)y0 * g.Wp + x1) * 8, t01);
        Texel<PT>::load6(base + ((uint64_t)y1 * g.Wp + x0) * 8, t10);
        Texel<PT>::load6(base + ((uint64_t)y1 * g.Wp + x1) * 8, t11);
        const float w00 = wx0 * wy0, w01 = wx1 * wy0, w10 = wx0 * wy1, w11 = wx1 * wy1;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            float r = t00[c] * w00;
            r = ssd_fma(t01[c], w01, r);
            r = ssd_fma(t10[c], w10, r);
            r = ssd_fma(t11[c], w11, r);
            f[c * 3 + p] = r;
            fu[c * 3 + p] = su * ssd_fma(wy1, t11[c] - t10[c], wy0 * (t01[c] - t00[c]));
            fv[c * 3 + p] = sv * ssd_fma(wx1, t11[c] - t01[c], wx0 * (t10[c] - t00[c]));
        }
    }
}

template <typename PT>
__global__ void __launch_bounds__(MA_TPB) k_mesh_vertex_attributes(const PT* __restrict__ planes, PlaneGeom g, const float* __restrict__ P,
                                                                   const float* __restrict__ verts_idx, uint32_t V, MeshMap m, float sat,
                                                                   float* __restrict__ xyz, float* __restrict__ sigma_out, float* __restrict__ grad_sigma,
                                                                   float* __restrict__ normals, float* __restrict__ colors, uint8_t* __restrict__ colors_u8) {
    const uint32_t i = blockIdx.x * MA_TPB + threadIdx.x;
    if (i >= V) return;
    const uint64_t o = 3ull * i;
    const float px = ssd_fma(verts_idx[o], m.scale[0], m.b_min[0]);
    const float py = ssd_fma(verts_idx[o + 1], m.scale[1], m.b_min[1]);
    const float pz = ssd_fma(verts_idx[o + 2], m.scale[2], m.b_min[2]);
    xyz[o] = px; xyz[o + 1] = py; xyz[o + 2] = pz;

    float f[18], fu[18], fv[18];
    ma_gather18_jac<PT>(planes, g, px, py, pz, f, fu, fv);

    // density and D = d log(sigma) / d f in one pass over the hidden units (ssd_mlp<0>'s arithmetic for sigma)
    float D[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) D[k] = 0.0f;
    float sa = P[MLP_OFF_TAIL + 0];
#pragma unroll 4
    for (int j = 0; j < 64; ++j) {
        const float* __restrict__ rec = P + j * 24;
        float h = rec[18];
#pragma unroll
        for (int k = 0; k < 18; ++k) h = ssd_fma(rec[k], f[k], h);
        const float e = __builtin_amdgcn_exp2f(h * -1.4426950408889634f);
        const float s = __builtin_amdgcn_rcpf(1.0f + e);                 // one exp2 + one rcp serve silu and silu'
        sa = ssd_fma(rec[19], h * s, sa);
        const float a = rec[19] * (s * ssd_fma(h, 1.0f - s, 1.0f));
#pragma unroll
        for (int k = 0; k < 18; ++k) D[k] = ssd_fma(a, rec[k], D[k]);
    }
    const float sigma = ssd_exp(sa);
    sigma_out[i] = sigma;

    // J^T D: plane p contributes through its width coordinate (x, x, y) and its height coordinate (y, z, z)
    float gu[3], gv[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        float a = 0.0f, b = 0.0f;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            a = ssd_fma(D[c * 3 + p], fu[c * 3 + p], a);
            b = ssd_fma(D[c * 3 + p], fv[c * 3 + p], b);
        }
        gu[p] = a; gv[p] = b;
    }
    const float gx = sigma * (gu[0] + gu[1]);
    const float gy = sigma * (gv[0] + gu[2]);
    const float gz = sigma * (gv[1] + gv[2]);
    if (grad_sigma) { grad_sigma[o] = gx; grad_sigma[o + 1] = gy; grad_sigma[o + 2] = gz; }

    // n = -grad / |grad|, scaled by the largest component first so that the squares neither overflow nor vanish
    const float big = fmaxf(fabsf(gx), fmaxf(fabsf(gy), fabsf(gz)));
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (big > 0.0f && big < INFINITY) {
        const float qx = gx / big, qy = gy / big, qz = gz / big;
        const float len = sqrtf(ssd_fma(qx, qx, ssd_fma(qy, qy, qz * qz)));
        nx = -(qx / len); ny = -(qy / len); nz = -(qz / len);
    }
    normals[o] = nx; normals[o + 1] = ny; normals[o + 2] = nz;

    // colour seen head-on from outside: view direction d = -n
    const bool flat = nx == 0.0f && ny == 0.0f && nz == 0.0f;
    float sh[16];
    shb::eval<4, false>(flat ? 0.0f : -nx, flat ? 0.0f : -ny, flat ? 1.0f : -nz, sh, nullptr, nullptr, nullptr);
    float s2, cr, cg, cb;
    ssd_mlp<1>(P, f, sh, nullptr, sat, s2, cr, cg, cb);
    colors[o] = cr; colors[o + 1] = cg; colors[o + 2] = cb;
    if (colors_u8) { colors_u8[o] = ssd_quant_u8(cr); colors_u8[o + 1] = ssd_quant_u8(cg); colors_u8[o + 2] = ssd_quant_u8(cb); }
}

}  // namespace

extern "C" int ssdnerf_mesh_vertex_attributes(const void* planes, int planes_dtype, uint32_t Hp, uint32_t Wp, const float* mlp_params,
                                              const float* verts_idx, uint32_t V, const float* b_min, const float* scale, float sigmoid_saturation,
                                              float* xyz, float* sigma, float* grad_sigma, float* normals, float* colors, uint8_t* colors_u8, void* stream) {
    if (V == 0) return SSDNERF_OK;  // an empty surface: nothing to do (pointers may be null)
    SSD_REQUIRE(planes && mlp_params && verts_idx && b_min && scale && xyz && sigma && normals && colors, "mesh_vertex_attributes: null pointer");
    SSD_REQUIRE(planes_dtype == 0 || planes_dtype == 1, "mesh_vertex_attributes: unsupported plane dtype");
    SSD_REQUIRE(Hp >= 1 && Wp >= 1, "mesh_vertex_attributes: empty plane");
    SSD_REQUIRE(V < (1u << 30), "mesh_vertex_attributes: more than 2^30 vertices");
    const PlaneGeom g = ssd_plane_geom(Hp, Wp);
    MeshMap m;                                                           // b_min / scale are HOST arrays of three floats
    for (int a = 0; a < 3; ++a) { m.b_min[a] = b_min[a]; m.scale[a] = scale[a]; }
    dim3 gr(ssd_blocks(V, MA_TPB)), b(MA_TPB);
    hipStream_t s = (hipStream_t)stream;
    if (planes_dtype == 0)
        hipLaunchKernelGGL((k_mesh_vertex_attributes<float>), gr, b, 0, s, (const float*)planes, g, mlp_params, verts_idx, V, m, sigmoid_saturation, xyz, sigma,
                           grad_sigma, normals, colors, colors_u8);
    else
        hipLaunchKernelGGL((k_mesh_vertex_attributes<__half>), gr, b, 0, s, (const __half*)planes, g, mlp_params, verts_idx, V, m, sigmoid_saturation, xyz,
                           sigma, grad_sigma, normals, colors, colors_u8);
    SSD_CHECK_LAUNCH("mesh_vertex_attributes");
    return SSDNERF_OK;
}
