"""float64 reference of the mesh-attribute kernel (csrc/mesh_attr.hip) and the per-component error bound of its density gradient, shared by
tests/test_mesh_export_cpu.py (the reference is right; the bound holds for an fp32 evaluation and rejects wrong gradients) and
tests/test_mesh_export_gpu.py (the kernel meets it).

The reference is the decode restated in ``torch.float64`` -- ``grid_sample(bilinear, border, align_corners=False)``, ``F.linear``, SiLU, ``exp``, the
degree-4 SH basis from the formulas of csrc/sh_basis.h -- from the exact fp32 (or fp16, upcast) values the kernel reads; the gradient of sigma is
``torch.autograd.grad``'s.  Nothing here needs a GPU or the oracle's C library.

Bound (form as tests/_fp64_bounds.py: c * sqrt(K) * u * magnitudes): for each component a of grad sigma

    |g_a - ref_a| <= c sqrt(K) u A_a,   u = 2^-24, K = 64 * 18, c = C_BOUND = 8,
    A_a = sigma * sum_k (sum_i |w_s[i] silu'(h_i) W1[i][k]|) * |J|_ka,

|J|_ka the gather's Jacobian with the texel DIFFERENCES taken by magnitude: (W/2) [wy0 |t01 - t00| + wy1 |t11 - t10|] for the plane's width
coordinate, (H/2) [wx0 |t10 - t00| + wx1 |t11 - t01|] for its height coordinate, 0 where feature k does not read axis a or the axis is clipped.
Why c = 8: the gradient is a sum of K = 1152 products w_s[i] silu'(h_i) W1[i][k] J_ka accumulated in fp32, whose rounding errors add like a random
walk (sqrt(K) u A, ``conv_gamma``'s argument); each product carries four roundings of its own and silu' the ~2 ulp of the hardware exp2 / rcp; and
sigma's relative error (~ sqrt(64) u |sum w_s silu(h)| ~ 6e-6 on the synthetic scene) multiplies every component, which A / |g| ~ 3 on a surface
absorbs.

A has no term for the rounding of the POSITION, and whether an fp32 evaluation meets c = 8 depends on how it forms the bilinear fraction.  ATen's
ix = ((u + 1) W - 1) / 2 is an fp32 number of magnitude up to W, so ix - floor(ix) is off by up to the spacing of ix (4e-6 texel units): the gradient
is evaluated that far from the point, an error of (second difference of the texels) x 4e-6 next to a bound built from first differences.  On the
object's iso-surface the planes are smooth on that scale; points off the surface fall on the silhouette edges of the planes (a tanh step two texels
wide).  The kernel forms the fraction in one rounding below 1 (``_coord``), which is what "an fp32 evaluation of the same expression" means here.
Measured on the CPU (tests/test_mesh_export_cpu.py prints the figures; fp32 and fp16 planes), worst err / (u A) against c sqrt(K) = 272:

    surface 96^3                     explicit fp32, kernel's fraction  72 - 79  fp32 ``torch.autograd`` (ATen's fraction) 148 - 167 (64^3 - 128^3: 148 - 195)
    20 000 random points, 5 seeds    explicit fp32, kernel's fraction  58 - 62  fp32 ``torch.autograd`` 350 - 570 (6 - 12 of 60 000 components above 272)

so c = 8 stands for the kernel on both sets, with the constant NOT re-derived; ATen's fp32 figure on random points is recorded by the CPU test and held
to 4 c only (``C_ATEN_RANDOM`` = 32, the next power of two above 570 / sqrt(K) = 16.8): it says what the kernel's fraction buys, it is not a bound on
the kernel.  The wrong gradients of test 2 are off by 10^5 u A at the median."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
C_BOUND = 8
K_TERMS = 64 * 18
C_ATEN_RANDOM = 32        # fp32 ATen autograd on points off the surface (recorded; not the kernel's bound): see the module docstring
GAMMA = C_BOUND * math.sqrt(K_TERMS) * U32            # 272 u
GAMMA_ATEN_RANDOM = C_ATEN_RANDOM * math.sqrt(K_TERMS) * U32   # 1086 u
PLANE_AXES = ((0, 1), (0, 2), (1, 2))                 # plane p reads (width coordinate, height coordinate): xy, xz, yz
EXCLUDE_TEXEL_UNITS = 1e-3


def params64(sd):
    """the decoder's state dict -> float64 tensors by short names"""
    g = lambda k: sd[k].detach().cpu().double()
    return dict(W1=g("base_net.0.weight"), b1=g("base_net.0.bias"), ws=g("density_net.0.weight")[0], bs=g("density_net.0.bias")[0],
                Wd=g("dir_net.0.weight"), bd=g("dir_net.0.bias"), Wc=g("color_net.0.weight"), bc=g("color_net.0.bias"))


def planes64(code, plane_dtype=torch.float32):
    """the (3, 6, H, W) code as the kernel reads it (``pack_triplanes`` rounds to the plane dtype), in float64"""
    return code.detach().cpu().to(plane_dtype).double()


def _silu(h):
    return h * torch.sigmoid(h)


def _dsilu(h):
    s = torch.sigmoid(h)
    return s * (1 + h * (1 - s))


def features(code, pts, align_corners=False):
    """(N, 18) features through ``grid_sample`` in the dtype of ``code``; index c * 3 + plane"""
    n = pts.shape[0]
    grid = torch.stack([pts[:, list(ax)] for ax in PLANE_AXES], dim=0)[:, None]          # (3, 1, N, 2): x on the width axis
    pc = F.grid_sample(code, grid, mode="bilinear", padding_mode="border", align_corners=align_corners)   # (3, C, 1, N)
    return pc.squeeze(2).permute(2, 1, 0).reshape(n, -1)


def sigma_and_grad(P, code, pts):
    """(sigma (N), grad sigma (N, 3), hidden pre-activations h (N, 64), features (N, 18)) by autograd, in the dtype of the inputs"""
    x = pts.detach().clone().requires_grad_(True)
    f = features(code, x)
    h = F.linear(f, P["W1"], P["b1"])
    sigma = torch.exp(_silu(h) @ P["ws"] + P["bs"])
    (g,) = torch.autograd.grad(sigma.sum(), x)
    return sigma.detach(), g.detach(), h.detach(), f.detach()


def sh16(d):
    """degree-4 real SH basis (16 values) of directions d (N, 3) as csrc/sh_basis.h states it: Y[l*l + l + m] = c(l, m) Q(l, |m|; z) (m >= 0 ? A_|m| :
    B_|m|), A_m + i B_m = (x + i y)^m, Q(l, m) = d^m P_l / dz^m, c(l, m) = (-1)^m (m ? sqrt 2 : 1) sqrt((2l + 1) / (4 pi) (l - |m|)! / (l + |m|)!)"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    C = 4
    A, B = [torch.ones_like(x)], [torch.zeros_like(x)]
    for m in range(1, C + 1):
        A.append(x * A[m - 1] - y * B[m - 1])
        B.append(x * B[m - 1] + y * A[m - 1])
    Q = [[torch.zeros_like(x) for _ in range(C + 1)] for _ in range(C)]
    for m in range(C):
        dfact = 1.0
        for k in range(2 * m - 1, 1, -2):
            dfact *= k
        Q[m][m] = torch.full_like(x, dfact)
        if m + 1 < C:
            Q[m + 1][m] = (2 * m + 1) * z * Q[m][m]
        for l in range(m + 2, C):
            Q[l][m] = ((2 * l - 1) * z * Q[l - 1][m] - (l + m - 1) * Q[l - 2][m]) / (l - m)
    out = []
    for l in range(C):
        for m in range(-l, l + 1):
            am = abs(m)
            c = (-1.0) ** am * (math.sqrt(2.0) if am else 1.0) * math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - am) / math.factorial(l + am))
            out.append(c * Q[l][am] * (A[am] if m >= 0 else B[am]))
    return torch.stack(out, dim=1)


def colors(P, code, pts, dirs, sat):
    """the decoder's rgb (N, 3) at ``pts`` for view directions ``dirs``, with the saturation affine"""
    f = features(code, pts)
    h = F.linear(f, P["W1"], P["b1"])
    hd = F.linear(sh16(dirs), P["Wd"], P["bd"])
    rgb = torch.sigmoid(F.linear(_silu(h + hd), P["Wc"], P["bc"]))
    return rgb * (1 + 2 * sat) - sat


def view_dirs(normals):
    """the kernel's rule: d = -n, and (0, 0, 1) where n = 0"""
    d = -normals
    flat = (normals == 0).all(dim=1)
    d[flat] = torch.tensor([0.0, 0.0, 1.0], dtype=d.dtype)
    return d


def quantize_u8(c):
    return torch.round(c.clamp(0, 1) * 255)


# ------------------------------------------------------------------------------------------------ the gather written out (Jacobian, bound, wrong variants)
def _coord(u, size, align_corners=False, aten_order=False):
    """unnormalised coordinate -> (i0, i1, w0, w1, moves): ``moves`` False where ATen's border rule clips (ix <= 0 or ix >= size - 1).  In fp32 the
    fraction is formed as the kernel forms it, fma(u, size/2, (size-1)/2 - floor(ix)) -- one rounding below 1 (emulated through float64, where the
    product and the sum are exact) -- unless ``aten_order`` asks for ATen's ix - floor(ix)."""
    ix = (u + 1) / 2 * (size - 1) if align_corners else ((u + 1) * size - 1) / 2
    moves = (ix > 0) & (ix < size - 1)
    ix = ix.clamp(0, size - 1)
    fl = torch.floor(ix)
    w1 = ix - fl
    if u.dtype == torch.float32 and not align_corners and not aten_order:
        w = (u.double() * (size / 2) + ((size - 1) / 2 - fl.double())).float()
        down, up = (w < 0) & (fl > 0), (w >= 1) & (fl < size - 1)
        fl = fl - down.to(fl.dtype) + up.to(fl.dtype)
        w = (w + down.to(w.dtype) - up.to(w.dtype)).clamp(0, 1)
        w1 = torch.where(moves, w, w1)
    i0 = fl.long()
    i1 = (i0 + 1).clamp(max=size - 1)
    return i0, i1, 1 - w1, w1, moves


def gather_jacobian(code, pts, variant=None):
    """(f (N, 18), J (N, 18, 3), |J| (N, 18, 3)) from the formulas of csrc/mesh_attr.hip in the dtype of ``code``; ``variant`` names one deliberate
    mistake: 'no_half_size', 'align_corners', 'clipped_moves', 'missing_plane'; 'aten_order' is no mistake: ATen's fraction instead of the kernel's"""
    n = pts.shape[0]
    H, W = code.shape[-2:]
    ac = variant == "align_corners"
    f = code.new_zeros(n, 18)
    J = code.new_zeros(n, 18, 3)
    Jabs = code.new_zeros(n, 18, 3)
    ks = torch.arange(6) * 3
    for p, (au, av) in enumerate(PLANE_AXES):
        x0, x1, wx0, wx1, mu = _coord(pts[:, au], W, ac, variant == "aten_order")
        y0, y1, wy0, wy1, mv = _coord(pts[:, av], H, ac, variant == "aten_order")
        t = lambda yy, xx: code[p][:, yy, xx].T                                           # (N, 6)
        t00, t01, t10, t11 = t(y0, x0), t(y0, x1), t(y1, x0), t(y1, x1)
        col = lambda w: w[:, None]
        f[:, ks + p] = t00 * col(wx0 * wy0) + t01 * col(wx1 * wy0) + t10 * col(wx0 * wy1) + t11 * col(wx1 * wy1)
        su, sv = ((W - 1) / 2, (H - 1) / 2) if ac else (W / 2, H / 2)
        if variant == "no_half_size":
            su = sv = 1.0
        if variant == "clipped_moves":
            mu, mv = torch.ones_like(mu), torch.ones_like(mv)
        su, sv = su * mu.to(code.dtype), sv * mv.to(code.dtype)
        if variant == "missing_plane" and p == 2:
            continue
        J[:, ks + p, au] = col(su) * (col(wy0) * (t01 - t00) + col(wy1) * (t11 - t10))
        J[:, ks + p, av] = col(sv) * (col(wx0) * (t10 - t00) + col(wx1) * (t11 - t01))
        Jabs[:, ks + p, au] = col(su) * (col(wy0) * (t01 - t00).abs() + col(wy1) * (t11 - t10).abs())
        Jabs[:, ks + p, av] = col(sv) * (col(wx0) * (t10 - t00).abs() + col(wx1) * (t11 - t01).abs())
    return f, J, Jabs


def explicit_grad(P, code, pts, variant=None):
    """(sigma, grad sigma) from the kernel's formulas (steps 2 - 4 of its header) in the dtype of the inputs; ``variant`` as ``gather_jacobian``, or
    'sigmoid_for_dsilu'"""
    f, J, _ = gather_jacobian(code, pts, variant)
    h = F.linear(f, P["W1"], P["b1"])
    sigma = torch.exp(_silu(h) @ P["ws"] + P["bs"])
    ds = torch.sigmoid(h) if variant == "sigmoid_for_dsilu" else _dsilu(h)
    D = (ds * P["ws"]) @ P["W1"]                                                          # (N, 18)
    return sigma, sigma[:, None] * torch.einsum("nk,nka->na", D, J)


def bound_magnitude(P, code, pts):
    """A (N, 3) of the module docstring, in float64"""
    f, _, Jabs = gather_jacobian(code, pts)
    h = F.linear(f, P["W1"], P["b1"])
    sigma = torch.exp(_silu(h) @ P["ws"] + P["bs"])
    M = (_dsilu(h) * P["ws"]).abs() @ P["W1"].abs()                                       # sum_i |w_s[i] silu'(h_i) W1[i][k]|
    return sigma[:, None] * torch.einsum("nk,nka->na", M, Jabs)


def grad_bound(P, code, pts, gamma=GAMMA):
    """e (N, 3): the allowed |g_a - ref_a|"""
    return gamma * bound_magnitude(P, code, pts)


def worst_ratio(got, ref, A, keep):
    """(worst |got - ref| / (u A) over the kept points, number of kept components); a component with A == 0 must be exactly right (ratio inf if not)"""
    err = (got.double() - ref).abs()[keep]
    a = (U32 * A)[keep]
    r = torch.where(a > 0, err / a.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return (float(r.max()) if r.numel() else 0.0), int(r.numel())


def excluded(pts, size):
    """(N) bool: a coordinate within 1e-3 texel units of a texel centre line (an integer unnormalised coordinate inside the plane): the bilinear
    gradient jumps there, and fp32 and float64 may stand on different sides"""
    ix = ((pts.double() + 1) * size - 1) / 2
    near = ((ix - torch.round(ix)).abs() < EXCLUDE_TEXEL_UNITS) & (ix > -EXCLUDE_TEXEL_UNITS) & (ix < size - 1 + EXCLUDE_TEXEL_UNITS)
    return near.any(dim=1)


def clipped_axes(pts, size):
    """(N, 3) bool: the axes on which the border rule clips (gradient component exactly 0)"""
    ix = ((pts + 1) * size - 1) / 2
    return ~((ix > 0) & (ix < size - 1))


# ------------------------------------------------------------------------------------------------ test inputs
def fma_world(verts_idx, b_min, scale):
    """fma(v, scale, b_min) per fp32 element, exactly: the product of two fp32 values is exact in float64, the sum is formed in the 64-bit
    significand of x86 long double (exact for lattice coordinates: |v| >= 2^-9 next to |b_min| ~ 1), one rounding to fp32"""
    v = np.asarray(verts_idx, np.float32).astype(np.float64)
    prod = (v * np.asarray(scale, np.float32).astype(np.float64)[None, :]).astype(np.longdouble)
    return (prod + np.asarray(b_min, np.float32).astype(np.longdouble)[None, :]).astype(np.float32)


def density_volume(P, code, res, b_min=-1.1, b_max=1.1, chunk=1 << 18):
    """sigma on the res^3 lattice of ``extract_density_volume`` (0 outside the AABB [-1, 1]^3), float64 on the CPU; lattice positions rounded to fp32
    like the product's"""
    lin = torch.linspace(b_min, b_max, res, dtype=torch.float32).double()
    xx, yy, zz = torch.meshgrid(lin, lin, lin, indexing="ij")
    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], dim=-1)
    out = []
    with torch.no_grad():
        for c in pts.split(chunk):
            s = torch.exp(_silu(F.linear(features(code, c), P["W1"], P["b1"])) @ P["ws"] + P["bs"])
            out.append(s.masked_fill((c.abs() > 1).any(dim=1), 0))
    return torch.cat(out).reshape(res, res, res)


def crossing_vertices(volume, iso):
    """the vertices marching cubes puts on a volume, vectorised and in no particular order: one per lattice edge whose ends lie on different sides
    of ``iso``, linearly interpolated; (V, 3) float32 index coordinates"""
    vol = np.asarray(volume, np.float32)
    out = []
    for axis in range(3):
        a = np.take(vol, np.arange(vol.shape[axis] - 1), axis=axis)
        b = np.take(vol, np.arange(1, vol.shape[axis]), axis=axis)
        idx = np.argwhere((a > iso) != (b > iso))
        av, bv = a[tuple(idx.T)], b[tuple(idx.T)]
        p = idx.astype(np.float32)
        p[:, axis] += (np.float32(iso) - av) / (bv - av)
        out.append(p)
    return np.concatenate(out, axis=0)


def random_points(n, seed, corner=100, lim=1.15):
    """n points uniform in [-lim, lim]^3 (fp32), the first ``corner`` at (1, -1, 1): clipped on every axis"""
    g = torch.Generator().manual_seed(seed)
    pts = ((torch.rand(n, 3, generator=g, dtype=torch.float64) * 2 - 1) * lim).float()
    pts[:corner] = torch.tensor([1.0, -1.0, 1.0])
    return pts
