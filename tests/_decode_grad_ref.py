"""float64 reference of the decode gradient -- ``ssdnerf_point_decode_backward`` (csrc/decode_bwd.hip): ``k_decode_bwd_feat`` (or the opt-in
``k_decode_bwd_feat_mfma``), ``k_decode_bwd_bin_owned``, ``k_decode_bwd_sum`` -- with error bounds derived from the kernels' arithmetic, and the seeded
case families of tests/test_decode_grad_bounds_cpu.py (the bounds accept fp32 evaluations of the same arithmetic and reject subtly wrong ones) and
tests/test_decode_grad_fp64_gpu.py (the kernels meet them).  Built on tests/_render_ref.py: its gather, SH, activations, the forward's carried
pre-activation bounds (``decode_terms``), ``GUARD``, ``check_le`` and house style -- every input is the exact value the kernel read, upcast; a bound is a
first-order forward error analysis ``c u (sum of the magnitudes the fp32 evaluation rounds)``, u = 2^-24, carried from stage to stage (the VALU class's fma chains
by the partial sums of the kernel's own order, ``chain_rounding``: the worst-case-sum form could not tell the matrix-core first stage from the VALU one); second-order
remainders are added explicitly; each derivation stands next to its term; no constant is fitted to a GPU run.

The pipeline is split at its one linear seam, the workspace (``ssdnerf_point_decode_backward_layout``):
  * per sample (``decode_grad_ref``): d loss / d feature of one sample, the arithmetic of ``ssdb_mlp_backward`` (csrc/decode_bwd_math.h), against what
    the first stage stored in ``gfeat``;
  * per texel, reduction only (``scatter_ref``): the float64 scatter of the kernel's OWN ``pos`` and ``gfeat``, which are exact data there, so the bound
    holds nothing but the roundings of the weights, the products and the additions: a lost or doubled contribution stands out however small its weight;
  * per texel, end to end (``scatter_e2e_ref``): from the sample positions, with the per-sample bound and the coordinate uncertainty folded in.

Nothing here needs a GPU."""
import functools
from types import SimpleNamespace

import numpy as np

import _render_ref as RR
from _render_ref import C_EXP, C_X, GUARD, K_OUT, ORDER, U32  # noqa: F401  (re-exported for the two test modules)

# ------------------------------------------------------------------------------------------------ constants, each from its derivation
CLAMP_LO, CLAMP_HI = float(np.float32(1e-6)), 1e6      # TruncExp.backward's clamp as ssdb_mlp_backward holds it: the fp32 constants 1e-6f and 1e6f (the latter exact)
K_DC = 3.0       # MFMA class: dc = fma(dz2, w2, fma(dz1, w1, dz0 w0)): a product and two fmas, every partial sum at most sum |terms|: (K + 1) u sum |terms| with K = 2
K_TEXEL = 2.0    # per texel: (n_t + K + K_TEXEL) u sum |gf w| (``scatter_ref``)
# MFMA class (k_decode_bwd_feat_mfma).  An operand is split into a bf16 PAIR, both roundings to nearest (``db_split_pair``).  bf16 has 8 significand bits: for x in
# [2^e, 2^(e+1)) its spacing is 2^(e-7), so hi = bf16(x) errs by |x - hi| <= 2^(e-8) <= 2^-8 |x|; x - hi is exact in fp32 and lies below 2^(e-8) (or is that power of
# two, which bf16 holds), where the spacing is <= 2^(e-16): lo = bf16(x - hi) errs by <= 2^(e-17).  So x = hi + lo + r with |r| <= 2^-17 |x| (the kernel's own
# "to 2^-17"; ``pair_residual`` evaluates it), |lo| <= 2^-8 |x| (1 + 2^-8), |hi| <= (1 + 2^-8) |x|.  ``db_mfma3`` keeps hi hi + hi lo + lo hi (bf16 x bf16 products are
# exact in the fp32 accumulator); of a b = (hi_a + lo_a + r_a)(hi_b + lo_b + r_b) it drops lo_a lo_b (<= 2^-16 |a b|), r_a b (<= 2^-17 |a b|) and (hi_a + lo_a) r_b
# (<= 2^-17 |a b|): 2^-15 |a b| = 512 u |a b| per term, taken with the factor (1 + 2^-6) for the higher orders.  This is NOT the forward's three-way truncation split
# (``RR.SPLIT``).
PAIR = 2.0 ** 9 * (1.0 + 2.0 ** -6)
# Accumulation: a v_mfma_f32_32x32x16_bf16 is taken as 16 sequential fp32 additions onto its accumulator (the forward's model), every partial sum at most sum |terms|.
#   h:  two k steps (features 16, 17 and the bias row; features 0 - 15) of three MFMAs each, all six onto one accumulator: 96 roundings
#   d:  one k step, three MFMAs: 48 roundings of sum |Wd SH|; then fl(D + bd) and fl(h + .): u (sum |Wd SH| + |bd|) and u |h + d|  -> "dir" = 48 + PAIR + 1, the last
#       term being ``decode_terms``' own u |h + d|
#   heads: every lane sums its 32 hidden units by 32 fmas onto 0, the two lane halves are added, then the bias: 32 + 2 roundings of fp32 weights (no split)
#   gf: four k steps of three MFMAs onto one accumulator: 192 roundings, both operands (W1^T and dPRE) split
MFMA_LAYERS = {"base": 6 * 16 + PAIR, "dir": 3 * 16 + PAIR + 1.0, "out": 32 + 2}
K_GF_MFMA = 12 * 16 + PAIR


# ------------------------------------------------------------------------------------------------ per sample
def chain_rounding(terms, start):
    """the roundings of a sequential fma chain acc = fma(a_j, b_j, acc) from ``start``, in the kernel's order along the last axis of ``terms`` (= a_j b_j): every fma
    rounds its own result once, so the first-order error is at most u sum_j |p_j| over the partial sums p_j = start + t_1 + ... + t_j -- the sharpest worst-case form,
    and never more than the (K + 1) u (|start| + sum |terms|) it replaces.  (A chain from 0 starts with a plain rounded product: the same expression.)  The VALU
    kernels' order is fixed, so the reference can form the partial sums; where a large bias cancels against the sum this is several times smaller."""
    return U32 * np.abs(np.asarray(start)[..., None] + np.cumsum(terms, -1)).sum(-1)


def valu_terms(P, code, xyz, dirs, sat, density_only=False):
    """``RR.decode_terms`` for the VALU class with every layer's (K + 1) u sum |terms| replaced by ``chain_rounding`` in ``ssdb_mlp_backward``'s order (h: the bias, then
    features 0 .. 17; d: the bias, then SH 0 .. 15; sa, z: the bias, then hidden units 0 .. 63), everything else as there.  The worst-case-sum form cannot tell the
    matrix-core first stage from the VALU one on the coherent family (measured 0.26 of it); this form is what the control is held to, and with it every VALU check."""
    p = RR.unpack_params(P)
    f, Bf = RR.gather18(code, xyz)
    h = f @ p.W1.T + p.b1
    Bh = Bf @ np.abs(p.W1).T + chain_rounding(f[:, None, :] * p.W1[None], p.b1[None])
    s, Bs = RR.silu_terms(h, Bh)
    sa = s @ p.ws + p.bs
    Bsa = Bs @ np.abs(p.ws) + chain_rounding(s * p.ws, np.full(len(s), p.bs))
    assert float(Bsa.max(initial=0.0)) < GUARD, ("first order does not hold: density pre-activation bound", float(Bsa.max()))
    out = SimpleNamespace(p=p, f=f, B_f=Bf, h=h, B_h=Bh, sa=sa, B_sa=Bsa)
    if density_only:
        return out
    sh, Bsh = RR.sh4(dirs)
    d = sh @ p.Wd.T + p.bd
    hc = h + d
    Bhc = Bh + Bsh @ np.abs(p.Wd).T + chain_rounding(sh[:, None, :] * p.Wd[None], p.bd[None]) + U32 * np.abs(hc)
    c, Bc = RR.silu_terms(hc, Bhc)
    z = c @ p.Wc.T + p.bc
    Bz = Bc @ np.abs(p.Wc).T + np.stack([chain_rounding(c * p.Wc[j], np.full(len(c), p.bc[j])) for j in range(3)], 1)
    out.__dict__.update(sh=sh, B_sh=Bsh, hc=hc, B_hc=Bhc, z=z, B_z=Bz)
    return out


def dsilu_terms(h, Bh):
    """(silu'(h), bound) for silu'(u) = s (1 + u (1 - s)), s = sigmoid(u), as the kernels form it: sg = ssdb_sigmoid(h); sg * fma(h, 1 - sg, 1).
      carried:  |silu''| = |s (1 - s) (2 + u (1 - 2 s))| <= 1/2 for every u (its maximum, at 0), so the exact function moves by at most Bh / 2: a Lipschitz bound,
                sound for any Bh, no remainder to add
      own:      with h exact, the sigmoid errs by e_s = ``_sigmoid_rounding``; d/ds [s (1 + h (1 - s))] = 1 + h (1 - 2 s) and the second-order term is -h e_s^2;
                fl(1 - sg) rounds once, u (1 - s), scaled by |s h|; the fma rounds once, u |1 + h (1 - s)|, scaled by s: u |silu'|; the product once more: u |silu'|
      The own roundings happen at the kernel's h, not the reference's: each of their magnitudes (s, 1 - s, |h|, |silu'|) is 1-Lipschitz in h or better, five of them in
      products with factors <= 1 + |h|: an extra 8 u Bh (1 + |h|), below 7 % of the own terms while Bh < GUARD."""
    assert float(Bh.max(initial=0.0)) < GUARD, ("first order does not hold: pre-activation bound", float(Bh.max()))
    s = RR._sig(h)
    D = s * (1.0 + h * (1.0 - s))
    es = RR._sigmoid_rounding(h, s)
    own = np.abs(1.0 + h * (1.0 - 2.0 * s)) * es + np.abs(h) * es * es + U32 * (np.abs(s * h) * (1.0 - s) + 2.0 * np.abs(D))
    return D, 0.5 * Bh + own + 8.0 * U32 * Bh * (1.0 + np.abs(h))


def decode_grad_terms(P, code, xyz, dirs, sat, g_sigma, g_rgb, mfma=False, density_only=False, mutate=None):
    """``decode_grad_ref`` with its intermediates, as a namespace.  ``mutate="silu-term"``: the control of the CPU module -- silu' of hidden unit 0 of the
    density branch WITHOUT its u (1 - s) term (the value only; the bounds are the honest ones)."""
    t = RR.decode_terms(P, code, xyz, dirs, sat, MFMA_LAYERS, density_only) if mfma else valu_terms(P, code, xyz, dirs, sat, density_only)
    p, N = t.p, len(t.sa)
    gs = np.zeros(N) if g_sigma is None else RR._np64(g_sigma).reshape(-1)
    # density head: e = exp2(fl(sa log2e)) as the forward's sigma (relative: B_sa (1 + B_sa) carried, |sa| u for the scaled argument, C_EXP u for the exp2 unit).  The
    # clamp is 1-Lipschitz in e; its response to an e anywhere in [e - B_e, e + B_e] is evaluated exactly, so no sample is excluded at a knee and none past it is loose
    e = np.exp(t.sa)
    Be = e * (t.B_sa * (1.0 + t.B_sa) + (np.abs(t.sa) + C_EXP) * U32)
    E = np.clip(e, CLAMP_LO, CLAMP_HI)
    BE = np.maximum(np.abs(np.clip(e + Be, CLAMP_LO, CLAMP_HI) - E), np.abs(np.clip(e - Be, CLAMP_LO, CLAMP_HI) - E))
    dsa = gs * E                                                             # fl(g_sigma E): one rounding
    Bdsa = np.abs(gs) * BE + U32 * np.abs(dsa)
    D, BD = dsilu_terms(t.h, t.B_h)
    if mutate == "silu-term":
        D = D.copy()
        D[:, 0] = RR._sig(t.h[:, 0])
    # a_i = fl(fl(dsa w_i) silu'(h_i)): two roundings; the carried errors of both factors and their product
    a = dsa[:, None] * p.ws * D
    Ba = np.abs(p.ws * D) * Bdsa[:, None] + np.abs(dsa[:, None] * p.ws) * BD + np.abs(p.ws) * Bdsa[:, None] * BD + 2.0 * U32 * np.abs(a)
    dh, Bdh = a, Ba
    out = SimpleNamespace(fwd=t, e=e, E=E, dsa=dsa, B_dsa=Bdsa)
    if not density_only:
        gc = RR._np64(g_rgb).reshape(-1, 3)
        k = 1.0 + 2.0 * float(np.float32(sat))                             # k = fma(sat, 2, 1): one rounding (the kernel's sat is the fp32 value)
        s3, Bs3 = RR.sigmoid_terms(t.z, t.B_z)
        # fl(s fl(1 - s)): (s + d)(1 - s - d) = s (1 - s) + d (1 - 2 s) - d^2; the subtraction and the product round once each
        q = s3 * (1.0 - s3)
        Bq = np.abs(1.0 - 2.0 * s3) * Bs3 + Bs3 * Bs3 + 2.0 * U32 * q
        dz = gc * k * q                                                      # fl(fl(g k) q): k's rounding and two products
        Bdz = np.abs(gc) * k * Bq + 3.0 * U32 * np.abs(dz)
        dc = dz @ p.Wc                                                       # [N, 64]
        if mfma:
            Bdc = Bdz @ np.abs(p.Wc) + K_DC * U32 * (np.abs(dz) @ np.abs(p.Wc))
        else:                                                                # dz0 w0, then fma(dz1, w1, .), then fma(dz2, w2, .)
            Bdc = Bdz @ np.abs(p.Wc) + chain_rounding(dz[:, None, :] * p.Wc.T[None], np.zeros((1, 1)))
        Du, BDu = dsilu_terms(t.hc, t.B_hc)
        dh = dc * Du + a                                                     # fma(dc, silu'(u), a): one rounding
        Bdh = np.abs(Du) * Bdc + np.abs(dc) * BDu + Bdc * BDu + Ba + U32 * np.abs(dh)
        out.__dict__.update(dz=dz, B_dz=Bdz)
    gf = dh @ p.W1
    if mfma:
        Bgf = Bdh @ np.abs(p.W1) + K_GF_MFMA * U32 * (np.abs(dh) @ np.abs(p.W1))
    else:                                                                    # gf[k] = fma(dh_i, W1_ik, gf[k]) over hidden units 0 .. 63, from 0
        Bgf = Bdh @ np.abs(p.W1) + chain_rounding(dh[:, None, :] * p.W1.T[None], np.zeros((1, 1)))
    out.__dict__.update(dh=dh, B_dh=Bdh, gf=gf, B_gf=Bgf)
    return out


def decode_grad_ref(P, code, xyz, dirs, sat, g_sigma, g_rgb, mfma=False, density_only=False):
    """(gf [N, 18], B_gf [N, 18]), float64: d loss / d f of ``ssdb_mlp_backward`` on ``ssd_gather18``'s features (f[c * 3 + p]) for upstream gradients
    g_sigma [N] (or None) and g_rgb [N, 3] (None with ``density_only``), with the forward's notation (``RR.decode_terms``):
        dsa = g_sigma clamp(exp(sa), 1e-6, 1e6);  dz_j = g_rgb,j (1 + 2 sat) s_j (1 - s_j), s_j = sigmoid(z_j);
        dh_i = dsa w_sigma,i silu'(h_i) + (sum_j dz_j Wc_ji) silu'(h_i + d_i);  gf_k = sum_i dh_i W1_ik.
    ``mfma``: the bounds of k_decode_bwd_feat_mfma's arithmetic class (``MFMA_LAYERS``, ``K_GF_MFMA``) instead of the VALU kernel's.  ``code`` (3, 6, H, W):
    for fp16 planes the fp16-rounded values."""
    t = decode_grad_terms(P, code, xyz, dirs, sat, g_sigma, g_rgb, mfma, density_only)
    return t.gf, t.B_gf


# ------------------------------------------------------------------------------------------------ per texel: the reduction alone
def corners64(ix, size):
    """``ssdb_corners`` in float64 on fp32 coordinates: (i0, i1, w0, w1); w1 = ix - floor(ix) is exact in fp32 too, w0 = (floor + 1) - ix is what fp32 rounds once"""
    ix = np.asarray(ix, np.float64)
    fl = np.floor(ix)
    i0 = fl.astype(np.int64)
    return i0, np.minimum(i0 + 1, size - 1), (fl + 1.0) - ix, ix - fl


def contributions(pos, H, W):
    """the four corners of every sample: (texel index y W + x [4, n], weight [4, n]) in ``ssdb_scatter18``'s order"""
    x0, x1, wx0, wx1 = corners64(pos[:, 0], W)
    y0, y1, wy0, wy1 = corners64(pos[:, 1], H)
    return np.stack([y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1]), np.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1])


def scatter_ref(pos, gfeat, H, W, K):
    """(ref [6, H, W], bound [6, H, W], n_t [H, W]) of ONE scene and plane from the first stage's compacted fp32 ``pos`` [n, 2] and ``gfeat`` [n, 6], exact data here:
    ref = float64 sum of gf[c] (wx wy) over the four corners of every sample.  Bound per texel and channel: (n_t + K + K_TEXEL) u sum |gf w|, n_t = contributions of
    non-zero weight (a zero weight adds +-0 exactly).  It covers, per contribution, the rounding of wx0 or wy0 (either or both: the two-rounding corner is the reason the
    constant is not smaller), of the weight product and of gf w, and ANY order of the n_t additions -- run sums over 16-lane rows, elections, K partial images
    (an empty one adds 0 exactly) and the final sum over them: n_t contributions are joined by n_t - 1 rounded additions however they are grouped.  A texel no sample
    touches has bound 0: it must be exactly 0."""
    idx, w = contributions(pos, H, W)
    g = np.asarray(gfeat, np.float64)
    ref, mag = np.zeros((6, H * W)), np.zeros((6, H * W))
    n_t = np.zeros(H * W)
    for q in range(4):
        n_t += np.bincount(idx[q][w[q] != 0], minlength=H * W)
        for c in range(6):
            ref[c] += np.bincount(idx[q], weights=g[:, c] * w[q], minlength=H * W)
            mag[c] += np.bincount(idx[q], weights=np.abs(g[:, c]) * w[q], minlength=H * W)
    return ref.reshape(6, H, W), ((n_t + K + K_TEXEL) * U32 * mag).reshape(6, H, W), n_t.reshape(H, W)


def workspace_scatter_ref(counters, offsets, pos, gfeat, S, H, W, K):
    """(ref, bound) [S, 3, 6, H, W] of a whole backward from its workspace: counters [S], offsets [S + 1], pos [3, total, 2], gfeat [3, total, 6]"""
    ref, bnd = np.zeros((S, 3, 6, H, W)), np.zeros((S, 3, 6, H, W))
    for s in range(S):
        sl = slice(int(offsets[s]), int(offsets[s]) + int(counters[s]))
        for p in range(3):
            ref[s, p], bnd[s, p], _ = scatter_ref(pos[p, sl], gfeat[p, sl], H, W, K)
    return ref, bnd


# ------------------------------------------------------------------------------------------------ per texel: end to end
def _stencil(ix, size, dix):
    """four taps i0 - 1 .. i0 + 2 of the float64 coordinate (indices clipped to the plane): weights (0, w0, w1, 0) and their uncertainty.  The kernel's coordinate
    differs by at most dix = C_X u size texels, which moves w0 and w1 by dix each.  Within dix of a cell border the kernel's floor may be the neighbour's: its footprint
    then reaches one texel further -- i0 - 1 when the fraction is <= dix, i0 + 2 when it is >= 1 - dix -- with a weight of at most dix there, counted in that texel."""
    i0 = np.minimum(np.floor(ix).astype(np.int64), size - 1)
    fr = ix - i0
    idx = np.clip(np.stack([i0 - 1, i0, i0 + 1, i0 + 2]), 0, size - 1)
    w = np.stack([np.zeros_like(fr), 1.0 - fr, fr, np.zeros_like(fr)])
    dw = np.stack([np.where(fr <= dix, dix, 0.0), np.full_like(fr, dix), np.full_like(fr, dix), np.where(fr >= 1.0 - dix, dix, 0.0)])
    return idx, w, dw


def scatter_e2e_ref(xyz, gf, Bgf, H, W, K):
    """(ref [3, 6, H, W], bound) of ONE scene from its sample positions [n, 3] (fp32 values) and the per-sample reference gf, B_gf [n, 18] (zero rows: samples without
    an upstream gradient).  ref = float64 scatter with the float64 weights of the float64 coordinates.  Bound per texel and channel:
        sum (w + dw) B_gf  +  sum |gf| dw  +  (n_t + K + K_TEXEL) u sum |gf| (w + dw),
    dw = wx dwy + dwx wy + dwx dwy the uncertainty of a corner's weight (``_stencil``: a sample near a cell border is counted in both texels), n_t counting every tap of
    non-zero weight or uncertainty.  No sample and no texel is excluded."""
    xyz = RR._np64(xyz).reshape(-1, 3)
    dix, diy = C_X * U32 * W, C_X * U32 * H
    ref, bnd = np.zeros((3, 6, H * W)), np.zeros((3, 6, H * W))
    live = np.abs(gf).sum(1) > 0
    for p, (a, b) in enumerate(ORDER):
        xi, xw, xd = _stencil(RR._coord(xyz[live, a], W), W, dix)
        yi, yw, yd = _stencil(RR._coord(xyz[live, b], H), H, diy)
        lin, mag, n_t = np.zeros((6, H * W)), np.zeros((6, H * W)), np.zeros(H * W)
        for ty in range(4):
            for tx in range(4):
                w = xw[tx] * yw[ty]
                dw = xw[tx] * yd[ty] + xd[tx] * yw[ty] + xd[tx] * yd[ty]
                on = (w + dw) > 0
                if not on.any():
                    continue
                idx = (yi[ty] * W + xi[tx])[on]
                n_t += np.bincount(idx, minlength=H * W)
                for c in range(6):
                    g, B = gf[live, c * 3 + p][on], Bgf[live, c * 3 + p][on]
                    ref[p, c] += np.bincount(idx, weights=g * w[on], minlength=H * W)
                    lin[c] += np.bincount(idx, weights=(w + dw)[on] * B + np.abs(g) * dw[on], minlength=H * W)
                    mag[c] += np.bincount(idx, weights=np.abs(g) * (w + dw)[on], minlength=H * W)
        bnd[p] = lin + (n_t + K + K_TEXEL) * U32 * mag
    return ref.reshape(3, 6, H, W), bnd.reshape(3, 6, H, W)


# ------------------------------------------------------------------------------------------------ seeded case families
BORDER = 2.0 ** -8       # no generated coordinate lies this close (in texels) to a cell border, unless it is exact in fp32: the fp32 floor is the float64 floor
PLANES = {"square": (128, 128), "ragged": (40, 72), "odd": (33, 31)}


def _texel_coords(xyz, H, W):
    """the float64 coordinates the three planes use: ix [3, n] (along W), iy [3, n] (along H)"""
    x = RR._np64(xyz)
    return (np.stack([RR._coord(x[:, a], W) for a, _ in ORDER]), np.stack([RR._coord(x[:, b], H) for _, b in ORDER]))


def sample_keys(xyz, H, W):
    """[3, n] uint32: (floor(iy) << 16) | floor(ix) per plane, from float64"""
    ix, iy = _texel_coords(xyz, H, W)
    return ((np.floor(iy).astype(np.int64) << 16) | np.floor(ix).astype(np.int64)).astype(np.uint32)


def _unique_points(rng, n, H, W):
    """``n`` fp32 points whose key pairs of planes 0 and 1 are unique and whose every coordinate is either exact (a clamped coordinate; a texel centre of a
    128-texel axis) or at least BORDER away from a cell border.  One in twelve has a coordinate outside the box (up to 1.3: clamped to the border texel); on 128 x 128
    planes one in sixteen sits exactly on texel centres (u = (2 i + 1) / 128 - 1: ix = i without a rounding, weights 1, 0, 0, 0)."""
    out, seen = [], set()
    while len(out) < n:
        m = 2 * (n - len(out)) + 64
        xyz = rng.uniform(-1.0, 1.0, (m, 3))
        kind = rng.integers(0, 48, m)
        out_axis = rng.integers(0, 3, m)
        clamp = kind < 4
        xyz[clamp, out_axis[clamp]] = (rng.uniform(1.01, 1.3, m) * rng.choice([-1.0, 1.0], m))[clamp]
        centre = (kind >= 4) & (kind < 7) & (H == 128) & (W == 128)
        xyz[centre] = (2.0 * rng.integers(0, 128, (m, 3))[centre] + 1.0) / 128.0 - 1.0
        xyz = xyz.astype(np.float32)
        ix, iy = _texel_coords(xyz, H, W)
        co = np.concatenate([ix, iy])                                        # [6, m]
        fr = co - np.floor(co)
        exact = (np.abs(RR._np64(xyz)) > 1.0).T[[0, 0, 1, 1, 2, 2]] | centre[None]
        ok = (((fr >= BORDER) & (fr <= 1.0 - BORDER)) | exact).all(0)
        keys = sample_keys(xyz, H, W)
        for i in np.flatnonzero(ok):
            kp = (int(keys[0, i]), int(keys[1, i]))
            if kp not in seen and len(out) < n:
                seen.add(kp)
                out.append(xyz[i])
    return np.stack(out)


def _dirs(rng, n):
    d = rng.normal(size=(n, 3))
    if n >= 3:
        d[:3] = np.eye(3)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def pair_residual(x):
    """x - hi - lo of ``db_split_pair`` (csrc/decode_bwd.hip): hi = bf16(x), lo = bf16(x - hi), both rounded to nearest even, for fp32 values"""
    def bf16(v):
        b = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
        return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    x = np.asarray(x, np.float32)
    hi = bf16(x)
    return (x - hi) - bf16(x - hi)


def knee_params(code, xyz):
    """``base_params`` with the density head scaled and centred so that, over the case's own samples, the 0.6 % and 99.4 % quantiles of the density pre-activation sit at
    -+13.9: it crosses both knees of the clamp, exp(sa) = 1e-6 and 1e6 at sa = -+13.8, on that share of the samples (asserted by the CPU module), and no further, which
    keeps the matrix-core class's propagated bounds under ``GUARD``"""
    sd = RR.base_params()
    sa = np.concatenate([RR.decode_terms(RR.pack_params(sd), c, x, None, RR.SAT, False, True).sa for c, x in zip(code, xyz) if len(x)])
    lo, hi = np.quantile(sa, [0.006, 0.994])
    k = 27.8 / (hi - lo)
    sd["density_net.0.weight"] = sd["density_net.0.weight"] * float(k)
    sd["density_net.0.bias"] = (sd["density_net.0.bias"] - float(0.5 * (lo + hi))) * float(k)
    return sd


# name: (planes, fp16, parameters, scene sizes, zero upstream gradients)
SAMPLE_FAMILIES = {
    "square-fp32": ("square", False, "base", (3001,), None),
    "square-fp16-straddle": ("square", True, "base", (300, 0, 77, 1000), "third"),             # an empty scene; blocks that straddle two and three scenes; 30 % zeros
    "ragged-fp32-aligned": ("ragged", False, "base", (256, 256), None),                      # no block straddles
    "ragged-fp16-dead-scene": ("ragged", True, "base", (300, 0, 77, 1000), "scene2"),        # every sample of scene 2 without a gradient
    "coherent": ("square", False, "coherent", (3001,), None),                                # flat planes under ``coherent_params``: sum |terms| IS the value
    "knee": ("square", False, "knee", (3001, 400), "third"),                                  # (0.6 % of 2100 live samples past each knee)
}


@functools.lru_cache(maxsize=None)
def sample_case(name):
    """one seeded per-sample case: sd / P, code [S, 3, 6, H, W] fp32 (fp16-rounded for fp16 planes), fp16, xyz / dirs [total, 3], sizes, offsets [S + 1], g_sigma
    [total], g_rgb [total, 3] (fp32; all-zero rows where the family says so), sat"""
    planes, fp16, params, sizes, zeros = SAMPLE_FAMILIES[name]
    H, W = PLANES[planes]
    rng = np.random.default_rng(7000 + list(SAMPLE_FAMILIES).index(name))
    S, total = len(sizes), sum(sizes)
    if params == "coherent":
        # flat planes, all positive, on which the LAST feature (channel 5 of plane 2: f[17]) carries nearly all of every pre-activation.  The VALU chain then rounds
        # small partial sums until its last fma (``chain_rounding``: about u |h|), while the matrix-core form multiplies the bf16 pair of that one feature into all 64
        # hidden units: the pair's residual is one relative error common to every h_i, which the all-positive heads add up coherently.  The value is the one of a
        # fixed grid whose pair residual is largest (``pair_residual``; <= 2^-17 by the split's derivation): the family is sharp for the split, as flat-x8 is for the forward's
        code = np.broadcast_to(rng.uniform(0.01, 0.05, (S, 3, 6, 1, 1)), (S, 3, 6, H, W)).astype(np.float32).copy()
        grid = np.linspace(6.0, 10.0, 4001).astype(np.float32)
        code[:, 2, 5] = grid[np.argmax(np.abs(pair_residual(grid)) / grid)]
    elif params == "knee":                                                   # smooth planes (two waves across): the density pre-activation spreads over +-14 through
        yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")   # the features' range, not through their slope, which the coordinate term of B_f scales with
        fy, fx, ph = rng.uniform(-2, 2, (S, 3, 6, 1, 1)), rng.uniform(-2, 2, (S, 3, 6, 1, 1)), rng.uniform(0, 2 * np.pi, (S, 3, 6, 1, 1))
        code = np.sin(2 * np.pi * (fy * yy + fx * xx) + ph).astype(np.float32)
    else:
        code = (rng.normal(size=(S, 3, 6, H, W)) * 0.5).astype(np.float32)
    if fp16:
        code = code.astype(np.float16).astype(np.float32)
    xyz = [_unique_points(rng, n, H, W) if n else np.zeros((0, 3), np.float32) for n in sizes]
    sd = RR.coherent_params(code[0]) if params == "coherent" else knee_params(code, xyz) if params == "knee" else RR.base_params()
    g_sigma = (rng.normal(size=total) * (1e-3 if params == "coherent" else 0.1)).astype(np.float32)   # (coherent: exp(sa) = e^5.5; keeps both heads' shares comparable)
    g_rgb = rng.normal(size=(total, 3)).astype(np.float32)
    if params == "knee":                                                     # d sigma / d sa reaches 1e6: keep the products in range
        g_sigma = (g_sigma * 1e-3).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    dead = np.zeros(total, bool)
    if zeros == "third":
        dead = rng.random(total) < 0.3
    elif zeros == "scene2":
        dead[off[2]:off[3]] = True
        dead |= rng.random(total) < 0.1
    g_sigma[dead], g_rgb[dead] = 0.0, 0.0
    return SimpleNamespace(name=name, sd=sd, P=RR.pack_params(sd), code=np.ascontiguousarray(code), fp16=fp16, H=H, W=W, S=S, sizes=sizes, offsets=off,
                           xyz=np.concatenate(xyz), dirs=_dirs(rng, total), g_sigma=g_sigma, g_rgb=g_rgb, dead=dead, sat=RR.SAT)


@functools.lru_cache(maxsize=None)
def sample_reference(name, mfma, density_only):
    """(case, gf [total, 18], B_gf, active [total]): the float64 per-sample reference over every scene of the case; shared, read-only"""
    c = sample_case(name)
    gf, B = np.zeros((len(c.xyz), 18)), np.zeros((len(c.xyz), 18))
    for s in range(c.S):
        sl = slice(int(c.offsets[s]), int(c.offsets[s + 1]))
        if sl.stop > sl.start:
            gf[sl], B[sl] = decode_grad_ref(c.P, c.code[s], c.xyz[sl], c.dirs[sl], c.sat, c.g_sigma[sl], None if density_only else c.g_rgb[sl], mfma, density_only)
    active = (c.g_sigma != 0) if density_only else ((c.g_sigma != 0) | (c.g_rgb != 0).any(1))
    return c, gf, B, active


REDUCTION_KINDS = ("uniform", "one-point", "alternating", "runs", "quadrant", "borders", "two-scenes", "ray-bundle", "empty-split")
REDUCTION_CASES = tuple((k, p) for k in REDUCTION_KINDS for p in PLANES)


def _point_at(ix, size):
    """the normalised coordinate whose texel coordinate is ix (>= size - 1: beyond the last texel centre, clamped there exactly)"""
    return (2.0 * np.asarray(ix, np.float64) + 1.0) / size - 1.0


def _border_coords(size, rng):
    """texel coordinates with x0 = 15, 16, 31, 32, size - 2, size - 1 (those the plane has) at fractions 2^-6, 1/2 or 1 - 2^-6; size - 1 by the clamp (u = 1)"""
    i0 = sorted({v for v in (15, 16, 31, 32, size - 2, size - 1) if 0 <= v < size})
    return np.array([size - 0.5 if v == size - 1 else v + rng.choice([2.0 ** -6, 0.5, 1.0 - 2.0 ** -6]) for v in i0])


@functools.lru_cache(maxsize=None)
def reduction_case(kind, planes):
    """one seeded reduction case (the smallest shapes that exercise each mechanism of k_decode_bwd_bin_owned), as ``sample_case`` without zeros:
      uniform      3001 points of [-1.05, 1.05]^3
      one-point    2048 samples on one point: one run per row, one election winner per texel, n_t = 2048
      alternating  A, B, A, B ... over 2048 samples: no two neighbouring lanes agree, every lane goes to an election
      runs         1000 points, each 66 times in a row: runs straddle 16-lane rows, waves and 1024-key steps
      quadrant     4000 samples whose footprints lie inside the first 16 x 16 quadrant of every plane: that ring takes full 1024-key steps and wraps DBQ_CAP = 1152
      borders      footprints on every quadrant, tile and plane border: x0 and y0 in {15, 16, 31, 32, size - 2, size - 1} in all combinations on every plane, corner
                   weights down to 2^-12
      two-scenes   [66000, 2000] uniform samples: K >= 2 (asserted from the layout query); the second scene's splits are far shorter than the first's
      empty-split  [66000, 200]: the same, with a second scene of fewer than 256 samples -- a split's range is a multiple of 256 samples, so its second split is empty
      ray-bundle   64 axis-parallel rays of 128 samples: whole rays on one footprint of the plane they look down on"""
    H, W = PLANES[planes]
    rng = np.random.default_rng(9000 + 10 * REDUCTION_KINDS.index(kind) + list(PLANES).index(planes))
    sizes = None
    if kind == "uniform":
        xyz = rng.uniform(-1.05, 1.05, (3001, 3))
    elif kind == "one-point":
        xyz = np.repeat(rng.uniform(-0.9, 0.9, (1, 3)), 2048, 0)
    elif kind == "alternating":
        xyz = np.tile(rng.uniform(-0.9, 0.9, (2, 3)), (1024, 1))
    elif kind == "runs":
        xyz = np.repeat(rng.uniform(-1.0, 1.0, (1000, 3)), 66, 0)
    elif kind == "quadrant":
        # texel coordinates in [0.1, 14.9]: x0, y0 in 0 .. 14 on every plane.  x runs along W (planes 0, 1), z along H (planes 1, 2); y along H on plane 0 and
        # along W on plane 2: between the smaller axis's 0.1 and the larger axis's 14.9
        y = rng.uniform(_point_at(0.1, min(H, W)), _point_at(14.9, max(H, W)), 4000)
        xyz = np.stack([_point_at(rng.uniform(0.1, 14.9, 4000), W), y, _point_at(rng.uniform(0.1, 14.9, 4000), H)], 1)
    elif kind == "borders":
        xs, zs = _border_coords(W, rng), _border_coords(H, rng)
        ys = np.concatenate([_point_at(_border_coords(H, rng), H), _point_at(_border_coords(W, rng), W)])
        g = np.stack(np.meshgrid(_point_at(xs, W), ys, _point_at(zs, H), indexing="ij"), -1).reshape(-1, 3)
        xyz = g[rng.permutation(len(g))]
    elif kind in ("two-scenes", "empty-split"):
        sizes = (66000, 2000 if kind == "two-scenes" else 200)
        xyz = rng.uniform(-1.0, 1.0, (sum(sizes), 3))
    else:
        o = rng.uniform(-0.9, 0.9, (64, 1, 3))
        xyz = np.broadcast_to(o, (64, 128, 3)).copy()
        xyz[:, :, 2] = np.linspace(-1.0, 1.0, 128)[None]                    # along z: every ray on ONE footprint of the xy plane
        xyz = xyz.reshape(-1, 3)
    sizes = sizes or (len(xyz),)
    S, total = len(sizes), len(xyz)
    code = (rng.normal(size=(S, 3, 6, H, W)) * 0.5).astype(np.float32)
    sd = RR.base_params()
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return SimpleNamespace(name=f"{kind}/{planes}", kind=kind, sd=sd, P=RR.pack_params(sd), code=code, fp16=False, H=H, W=W, S=S, sizes=sizes, offsets=off,
                           xyz=xyz.astype(np.float32), dirs=_dirs(rng, total), g_sigma=(rng.normal(size=total) * 0.1).astype(np.float32),
                           g_rgb=rng.normal(size=(total, 3)).astype(np.float32), dead=np.zeros(total, bool), sat=RR.SAT)


def check_le(got, ref, bound):
    return RR.check_le(np.asarray(got, np.float64), ref, bound)
