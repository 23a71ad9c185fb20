"""float64 reference of the render path's arithmetic -- the bilinear triplane gather and the tiny MLP of csrc/decode_core.h (``ssd_grid_coord``,
``ssd_gather18``, ``ssd_mlp``; the same operation on the matrix cores in csrc/shade_mfma.hip) and the eval-branch composite of the fused render
kernels (render_fused.hip, render_queue.hip, shade_mfma.hip) -- with per-sample and per-ray error bounds derived from it, and the seeded case
families that tests/test_render_bounds_cpu.py (the bounds accept an fp32 emulation of each kernel and reject subtly wrong ones) and
tests/test_render_fp64_gpu.py (the kernels meet them) draw from.  House style of tests/_composite_ref.py, whose ``C_EXP``, ``alpha_terms`` and
composite recursion are reused: every input is the exact value the kernel read, upcast; a bound is a first-order forward error analysis of the
fp32 kernel, ``c * u * (sum of the magnitudes an fp32 evaluation of the same expression rounds)`` with u = 2^-24, carried from stage to stage
with magnitudes computed in float64; each derivation stands next to its term.  Where first order is not exact the second-order remainder is
added explicitly and a guard (``GUARD``) asserts that it is small.  No constant is fitted to what the kernels achieve; the measured worst
error / bound ratios are in profiles/render_bounds.json (written by ``python tests/test_render_fp64_gpu.py OUT.json``).

Two arithmetic classes:
  * VALU (``mfma=False``): ``k_point_decode`` and the "single" / "queue" render pipelines -- fp32 fmas in ssd_mlp's fixed order;
  * MFMA (``mfma=True``): the "queue_mfma" pipeline -- operands split into three bf16 terms, six products kept (see the constants below and ``decode_ref``).

Nothing here needs a GPU."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import _composite_ref as CR
from _composite_ref import C_EXP, MAX_UNDECIDED, THRESHOLDS, U32, f32_exact  # noqa: F401  (re-exported for the two test modules)

# ------------------------------------------------------------------------------------------------ constants, each from its derivation
C_X = 3.5        # ssd_grid_coord: ix = ((u + 1) W - 1) / 2 for |u| <= 1.  fl(u + 1) errs by <= u |u + 1| <= 2 u, which W / 2 scales to <= u W; the product
#                  rounds <= u (u + 1) W, halved: <= u W; the subtraction rounds <= u ((u + 1) W - 1), halved: <= u W (a contracted fma only drops one of the
#                  two); the halving is exact.  An ulp of the sample position itself, u |u| <= u, moves ix by <= u W / 2.  Sum: 3.5 u W texels.
C_CHAIN = 7.0    # bilinear chain: wx1 = ix - floor(ix) is exact, wx0 = fl((floor + 1) - ix) rounds once (<= u), the corner weight fl(wx wy) once more and
#                  carries both factors: <= 3 u relative; the chain is one product and three fmas, each rounding <= u times a partial sum that is at most
#                  sum |t w|: 4 u.  Together 7 u sum |t w|.
C_SH = 12.0      # shb::eval<4>: (x + iy)^m up to m = 3 is three levels of a product and an fma (6 roundings), Q(l, m; z) at most 4, the two final products 2;
#                  each rounding is <= u times the value of the same expression with every term replaced by its magnitude (``sh4`` evaluates that beside the value)
C_RCP = 2.0      # v_rcp_f32: 1 ulp = 2 u relative (the ISA's stated accuracy; C_EXP already is the exp2 unit's allowance)
# Layer sums: the worst-case (K + 1) u sum |terms| form (K fmas onto the bias, every partial sum at most the sum of magnitudes).  The lengths are 18, 16 and 64: the
# worst case is within a factor ~sqrt(K) of what random roundings give, and unlike a probabilistic bound it needs no exclusion rule.
K_BASE, K_DIR, K_OUT = 18 + 1, 16 + 1, 64 + 1
# MFMA class.  x = hi + mid + lo exactly (8 + 8 + 8 bits, truncations: every term has the sign of x); kept: the six products of weight >= 2^-16; dropped:
# mid lo, lo mid, lo lo, each <= 2^-24 |x w| (shade_mfma.hip, head) -> SPLIT u |x w|.  The weights enter as fl32(-log2(e) w) (SM_PRESCALE: one rounding, also of
# the folded column Wd'[:, 0] = fl32(-log2(e) (Wd[:, 0] SH_0 + bd)), formed in fp64) -> PRESCALE u |x w|; the output weights as fl32(-ln(2) w) -> one more rounding
# per term of the output layer.  Accumulation: a v_mfma_f32_32x32x16_bf16 is taken as 16 sequential fp32 additions onto its accumulator.  Products are issued
# smallest first: of the seven MFMAs of the base layer the last two (hi hi of features 0 - 15; the packed k-step of features 16, 17 and b1) add at full magnitude S,
# 32 roundings; the other five add terms of weight <= 2^-8: 5 x 16 x 2^-7 u S < u S.  The direction term accumulates in place on top of h: its last MFMA (hi hi) adds
# at the magnitude S + S_dir, 16 roundings, the other five < u (S + S_dir).
SPLIT, PRESCALE = 3.0, 1.0
# The output layer of the MFMA kernel: each lane half sums its 32 hidden units as two chains of 16 fmas, then three additions (the pair, the other half, the bias), on
# weights that carry the rescale rounding: 16 + 3 + 1.
K_BASE_MFMA, K_DIR_MFMA, K_OUT_MFMA = 2 * 16 + 1, 16 + 1, 16 + 3 + 1
GUARD = 2.0 ** -7    # every propagated pre-activation bound must stay below this.  The second-order remainders are ADDED below with their global constants
#                      (|silu''| <= 1/2, |sigmoid''| <= 1/10: Lagrange remainders B^2 / 4 and B^2 / 20; e^d - 1 <= d (1 + d) for d <= 1), so the bounds are sound for
#                      any B; the guard keeps those remainders below 1 % of the first-order terms, i.e. the bounds as sharp as the derivation says

ORDER = ((0, 1), (0, 2), (1, 2))     # planes (xy, xz, yz); the first coordinate runs along the width


def _np64(a):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ parameters
def pack_params(sd):
    """the packed parameter block (csrc/decode_core.h, ``decoders.pack_mlp_params``) of a reference-keyed state dict, as a float32 numpy array"""
    g = lambda k: np.asarray(sd[k].detach().cpu().numpy() if isinstance(sd[k], torch.Tensor) else sd[k], np.float32)
    rec = np.zeros((64, 24), np.float32)
    rec[:, :18], rec[:, 18], rec[:, 19] = g("base_net.0.weight"), g("base_net.0.bias"), g("density_net.0.weight")[0]
    rec[:, 20:23] = g("color_net.0.weight").T
    return np.concatenate([rec.reshape(-1), g("dir_net.0.weight").reshape(-1), g("dir_net.0.bias"), g("density_net.0.bias").reshape(-1), g("color_net.0.bias")])


def unpack_params(P):
    P = _np64(P)
    rec = P[:1536].reshape(64, 24)
    return SimpleNamespace(W1=rec[:, :18], b1=rec[:, 18], ws=rec[:, 19], Wc=rec[:, 20:23].T.copy(), Wd=P[1536:2560].reshape(64, 16), bd=P[2560:2624],
                           bs=P[2624], bc=P[2625:2628])


# ------------------------------------------------------------------------------------------------ SH4
@functools.lru_cache(maxsize=None)
def _sh_consts():
    """csrc/sh_basis.h's tables as the fp32 values the kernel folds (they are inputs: the reference evaluates the same polynomial exactly)"""
    f = math.factorial
    norm = {}
    for l in range(4):
        for m in range(-l, l + 1):
            am = abs(m)
            k = math.sqrt((2 * l + 1) / (4 * math.pi) * f(l - am) / f(l + am))
            norm[(l, m)] = float(np.float32((1.0 if am == 0 else math.sqrt(2.0)) * (-1.0 if am & 1 else 1.0) * k))
    return norm, [1.0, 1.0, 3.0, 15.0]


SH_0 = _sh_consts()[0][(0, 0)]


def sh4(d):
    """(SH4(d) [N, 16], bound [N, 16]) of fp32 directions: shb::eval<4, false> in float64, and C_SH u times the same expression on magnitudes"""
    d = _np64(d).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    one, zero = np.ones_like(x), np.zeros_like(x)
    A, B, Aa, Ba = [one], [zero], [one], [zero]
    for m in range(1, 4):
        A.append(x * A[m - 1] - y * B[m - 1]); B.append(x * B[m - 1] + y * A[m - 1])
        Aa.append(ax * Aa[m - 1] + ay * Ba[m - 1]); Ba.append(ax * Ba[m - 1] + ay * Aa[m - 1])
    norm, dfact = _sh_consts()
    Q, Qa = {}, {}
    for m in range(4):
        Q[(m, m)] = Qa[(m, m)] = dfact[m] * one
        if m + 1 < 4:
            Q[(m + 1, m)], Qa[(m + 1, m)] = (2 * m + 1) * z * Q[(m, m)], (2 * m + 1) * az * Qa[(m, m)]
        for l in range(m + 2, 4):
            inv = float(np.float32(1.0) / np.float32(l - m))
            Q[(l, m)] = ((2 * l - 1) * z * Q[(l - 1, m)] - (l + m - 1) * Q[(l - 2, m)]) * inv
            Qa[(l, m)] = ((2 * l - 1) * az * Qa[(l - 1, m)] + (l + m - 1) * Qa[(l - 2, m)]) * inv
    out, bnd = np.zeros((len(x), 16)), np.zeros((len(x), 16))
    for l in range(4):
        for m in range(-l, l + 1):
            am, i = abs(m), l * l + l + m
            out[:, i] = norm[(l, m)] * Q[(l, am)] * (A[am] if m >= 0 else B[am])
            bnd[:, i] = C_SH * U32 * abs(norm[(l, m)]) * Qa[(l, am)] * (Aa[am] if m >= 0 else Ba[am])
    bnd[:, 0] = 0.0                                                          # SH_0 = c(0, 0) * 1 * 1: exact
    return out, bnd


# ------------------------------------------------------------------------------------------------ gather
def _coord(u, size):
    return np.clip(((u + 1.0) * size - 1.0) * 0.5, 0.0, size - 1.0)        # align_corners=False, border clamp


def _foot(ix, size):
    i0 = np.minimum(np.floor(ix).astype(np.int64), size - 1)
    i1 = np.minimum(i0 + 1, size - 1)                                       # the clipped neighbour only ever carries weight 0
    w1 = ix - i0
    return i0, i1, 1.0 - w1, w1


def gather18(code, xyz, pos_unc=None):
    """(f [N, 18], B_f [N, 18]): f[c * 3 + p] = bilinear sample of channel c of plane p of ``code`` (3, 6, H, W; fp32, or fp16 values for fp16 planes).
      chain:       C_CHAIN u sum |t w|                                                                                         (C_CHAIN above)
      coordinates: each fractional coordinate is uncertain by C_X u size texels (C_X above); df/dix = wy0 (t01 - t00) + wy1 (t11 - t10) and likewise in y,
                   so the feature moves by at most that many texels times the absolute corner differences of the footprint.  A coordinate within its
                   uncertainty of a texel centre may fall into the neighbouring cell, whose slope is another: the slope is taken as the larger of the two
                   evaluated at ix -/+ the uncertainty.  The bilinear blend is continuous and the clamp 1-Lipschitz, so nothing else happens at cell or
                   plane borders.  Where the footprint's texels are equal the term is exactly 0.
      ``pos_unc`` [N, 3] (optional): an uncertainty of the sample position itself, per axis, in units of the position -- for a kernel that forms the
                   position and does not output it (tests/_density_ref.py).  ix = ((u + 1) size - 1) / 2 moves by size / 2 texels per unit: pos_unc size / 2
                   is added to the coordinate uncertainty.  None leaves every number as it was."""
    code, xyz = _np64(code), _np64(xyz).reshape(-1, 3)
    N, (H, W) = len(xyz), code.shape[2:]
    f, Bf = np.zeros((N, 18)), np.zeros((N, 18))
    dix, diy = C_X * U32 * W, C_X * U32 * H
    for p, (a, b) in enumerate(ORDER):
        pl = code[p]

        def tap(ix, iy):
            x0, x1, wx0, wx1 = _foot(ix, W)
            y0, y1, wy0, wy1 = _foot(iy, H)
            t = [pl[:, yy, xx].T for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]
            return t, (wx0[:, None], wx1[:, None], wy0[:, None], wy1[:, None])

        ix, iy = _coord(xyz[:, a], W), _coord(xyz[:, b], H)
        if pos_unc is None:
            dx, dy, dxc, dyc = dix, diy, dix, diy
        else:
            dx, dy = dix + 0.5 * W * _np64(pos_unc)[:, a], diy + 0.5 * H * _np64(pos_unc)[:, b]
            dxc, dyc = dx[:, None], dy[:, None]
        (t00, t01, t10, t11), (wx0, wx1, wy0, wy1) = tap(ix, iy)
        val = t00 * (wx0 * wy0) + t01 * (wx1 * wy0) + t10 * (wx0 * wy1) + t11 * (wx1 * wy1)
        mag = np.abs(t00) * (wx0 * wy0) + np.abs(t01) * (wx1 * wy0) + np.abs(t10) * (wx0 * wy1) + np.abs(t11) * (wx1 * wy1)

        def slope_x(ixs):
            (s00, s01, s10, s11), (_, _, vy0, vy1) = tap(np.clip(ixs, 0.0, W - 1.0), iy)
            return np.abs(vy0 * (s01 - s00) + vy1 * (s11 - s10))

        def slope_y(iys):
            (s00, s01, s10, s11), (vx0, vx1, _, _) = tap(ix, np.clip(iys, 0.0, H - 1.0))
            return np.abs(vx0 * (s10 - s00) + vx1 * (s11 - s01))

        cols = np.arange(6) * 3 + p
        f[:, cols] = val
        Bf[:, cols] = (C_CHAIN * U32 * mag + dxc * np.maximum(slope_x(ix - dx), slope_x(ix + dx))
                       + dyc * np.maximum(slope_y(iy - dy), slope_y(iy + dy)))
    return f, Bf


# ------------------------------------------------------------------------------------------------ activations
def _sig(h):
    return 0.5 * (1.0 + np.tanh(0.5 * h))


def _sigmoid_rounding(h, s):
    """the kernel's own error of sigmoid(h) = rcp(1 + exp2(-log2(e) h)), exact h: fl(h log2e) moves e = e^-h by |h| u relative and the exp2 unit is allowed
    C_EXP u (``_composite_ref.alpha_terms``' constant), which reach s = 1 / (1 + e) scaled by e / (1 + e) = 1 - s; the addition rounds once (u) and the
    reciprocal is allowed C_RCP u"""
    return s * U32 * ((1.0 - s) * (np.abs(h) + C_EXP) + 1.0 + C_RCP)


def silu_terms(h, Bh):
    """(silu(h), bound): the incoming error through the derivative silu' = s (1 + h (1 - s)), its second-order remainder |silu''| / 2 B^2 <= B^2 / 4, the
    sigmoid's own error times |h|, and the rounding of the product h * rcp"""
    assert float(Bh.max(initial=0.0)) < GUARD, ("first order does not hold: pre-activation bound", float(Bh.max()))
    s = _sig(h)
    v = h * s
    return v, np.abs(s * (1.0 + h * (1.0 - s))) * Bh + 0.25 * Bh * Bh + np.abs(h) * _sigmoid_rounding(h, s) + U32 * np.abs(v)


def sigmoid_terms(h, Bh):
    assert float(Bh.max(initial=0.0)) < GUARD, ("first order does not hold: pre-activation bound", float(Bh.max()))
    s = _sig(h)
    return s, s * (1.0 - s) * Bh + 0.05 * Bh * Bh + _sigmoid_rounding(h, s)


# ------------------------------------------------------------------------------------------------ per sample
def decode_terms(P, code, xyz, dirs, sat, mfma, density_only=False, pos_unc=None):
    """``ssd_mlp`` on ``ssd_gather18``'s features in float64, every quantity with its carried bound, as a namespace: the outputs sigma [N], B_sigma, rgb [N, 3], B_rgb
    (what ``decode_ref`` returns) and the features f, pre-activations h, h + d (``hc``), sa, z with B_f, B_h, B_hc, B_sa, B_z and the layer magnitudes S1, Sd, which
    the decode gradient's reference (tests/_decode_grad_ref.py) starts from.  ``mfma`` may also be a dict of another kernel's layer allowances (see below).
    ``pos_unc``: ``gather18``'s optional position uncertainty.
        h = W1 f + b1;  sigma = exp(w_sigma . silu(h) + b_sigma);  rgb = sigmoid(Wc silu(h + Wd SH4(d) + bd) + bc) (1 + 2 sat) - sat.
    Bounds, S_* = sum of the magnitudes of a layer's terms and its bias, B_* carried:
      h:       |W1| B_f + K_BASE u S_1                                        MFMA: (K_BASE_MFMA + SPLIT + PRESCALE) u S_1
      h_col:   VALU: d = Wd SH + bd by 16 fmas, then fl(h + d):  B_h + |Wd| B_SH + K_DIR u S_d + u |h + d|
               MFMA (accumulated in place on h): B_h + |Wd| B_SH + (SPLIT + PRESCALE) u S_d + K_DIR_MFMA u (S_1 + S_d)
      heads:   sum |w| B_silu + K_OUT u S_out                                  MFMA: K_OUT_MFMA (shorter chains, rescaled output weights)
      sigma:   relative: B_sa (1 + B_sa) carried, |sa| u for fl(sa log2e), C_EXP u for the exp2 unit
      rgb:     k = fl(1 + 2 sat) rounds once (u k sigmoid), the fma once (u |rgb|), the sigmoid's bound is scaled by k"""
    p = unpack_params(P)
    f, Bf = gather18(code, xyz, pos_unc)
    aW1 = np.abs(p.W1)
    h, S1 = f @ p.W1.T + p.b1, np.abs(f) @ aW1.T + np.abs(p.b1)
    own = mfma if isinstance(mfma, dict) else None      # another kernel's layer allowances {"base", "dir", "out"}, in the VALU class's shape (tests/_decode_grad_ref.py)
    Bh = Bf @ aW1.T + (own["base"] if own else (K_BASE_MFMA + SPLIT + PRESCALE) if mfma else K_BASE) * U32 * S1
    k_out = own["out"] if own else K_OUT_MFMA if mfma else K_OUT
    s, Bs = silu_terms(h, Bh)
    sa = s @ p.ws + p.bs
    Bsa = Bs @ np.abs(p.ws) + k_out * U32 * (np.abs(s) @ np.abs(p.ws) + abs(p.bs))
    assert float(Bsa.max(initial=0.0)) < GUARD, ("first order does not hold: density pre-activation bound", float(Bsa.max()))
    sigma = np.exp(sa)
    Bsigma = sigma * (Bsa * (1.0 + Bsa) + (np.abs(sa) + C_EXP) * U32)
    out = SimpleNamespace(p=p, f=f, B_f=Bf, h=h, B_h=Bh, S1=S1, sa=sa, B_sa=Bsa, sigma=sigma, B_sigma=Bsigma, rgb=None, B_rgb=None)
    if density_only:
        return out
    sh, Bsh = sh4(dirs)
    aWd = np.abs(p.Wd)
    d, Sd = sh @ p.Wd.T + p.bd, np.abs(sh) @ aWd.T + np.abs(p.bd)
    hc = h + d
    if own:
        Bhc = Bh + Bsh @ aWd.T + own["dir"] * U32 * Sd + U32 * np.abs(hc)
    elif mfma:
        Bhc = Bh + Bsh @ aWd.T + (SPLIT + PRESCALE) * U32 * Sd + K_DIR_MFMA * U32 * (S1 + Sd)
    else:
        Bhc = Bh + Bsh @ aWd.T + K_DIR * U32 * Sd + U32 * np.abs(hc)
    c, Bc = silu_terms(hc, Bhc)
    aWc = np.abs(p.Wc)
    pc = c @ p.Wc.T + p.bc
    Bpc = Bc @ aWc.T + k_out * U32 * (np.abs(c) @ aWc.T + np.abs(p.bc))
    sg, Bsg = sigmoid_terms(pc, Bpc)
    k = 1.0 + 2.0 * sat
    rgb = sg * k - sat
    out.__dict__.update(sh=sh, B_sh=Bsh, Sd=Sd, hc=hc, B_hc=Bhc, z=pc, B_z=Bpc, rgb=rgb, B_rgb=k * Bsg + U32 * (k * sg + np.abs(rgb)))
    return out


def decode_ref(P, code, xyz, dirs, sat, mfma, density_only=False):
    """(sigma [N], B_sigma [N], rgb [N, 3], B_rgb [N, 3]) of ``decode_terms``"""
    t = decode_terms(P, code, xyz, dirs, sat, mfma, density_only)
    return t.sigma, t.B_sigma, t.rgb, t.B_rgb


def folded_column_ref(P):
    """(Wd'[:, 0], bound): the direction layer's folded, prescaled first column -log2(e) (Wd[:, 0] SH_0 + bd) as the MFMA kernel's prologue forms it in
    fp64 (shade_mfma.hip), and the ONE rounding to fp32 it is allowed: u |value|.  A kernel's outputs do not show this operand on its own -- the term is
    one of 17 of a pre-activation whose other roundings any sound bound admits too -- so only an emulation's operand can be held to it."""
    p = unpack_params(P)
    v = (p.Wd[:, 0] * SH_0 + p.bd) * -1.4426950408889634074
    return v, U32 * np.abs(v)


# ------------------------------------------------------------------------------------------------ per ray
def composite_ref(sig, Bsig, rgb, Brgb, dt, t, T_thresh, bg, late=False):
    """the eval branch's composite of the fused kernels in float64, per ray over [N, L] sample arrays (a slot with dt == 0 ends the ray).  Restated from
    shade_mfma.hip / render_queue.hip / render_fused.hip:  alpha = 1 - exp(-sigma dt);  T = 1 - ws is read BEFORE the sample;  w = alpha T;  ws += w;
    depth = fma(w, t, depth);  colour = fma(w, rgb, colour);  the sample is counted;  THEN the ray ends if T < T_thresh (the transmittance in front of
    the sample it just added -- ``_composite_ref.composite_rays_ref``'s branch, with nothing incoming).  image = colour + bg (1 - ws).

    Bounds have two parts.  (1) The compositing roundings, by ``composite_rays_ref``'s recursion with exact sigma / rgb:
          B_T = B_ws + u T;  B_w = da T + (a + da) B_T + u w;  B_ws += B_w + u ws;  B_r += B_w |c| + u sum |w c|   (da, dq: ``alpha_terms``)
    (2) The decode bounds of each sample through the absolute float64 sensitivities of the composite.  With T_k the transmittance in front of sample k,
    T_{k+1} = T_k - w_k and R_k = sum_{i > k} w_i c_i:  d ws / d sigma_k = dt_k T_end;  d colour / d sigma_k = dt_k (T_{k+1} c_k - R_k);
    d colour / d c_k = w_k;  depth as colour with t for c;  d T_k / d sigma_i = -dt_i T_k (i < k).  First order holds while G = sum dt B_sigma over a
    ray is small (every output is a sum of terms exp(-sum x) c, which a perturbation of the sigmas moves by at most e^G - 1 <= G (1 + 2 G) relative): asserted < 2^-4, and part (2) is inflated by 1 + 2 G.  The blend fl(fl(bg fl(1 - ws)) + colour) adds |bg| (B_ws + u |1 - ws|) +
    u |bg (1 - ws)| + u |image|; a ray without samples gets bg exactly.

    ``undecided``: at some termination test |T_k - T_thresh| <= B_T,k (both parts).  ``late=True`` ends a ray only where the test is decided: the
    other alternative, whose count is the upper end of an undecided ray's range.
    Returns a namespace of float64 / int64 arrays: image, depth, weights_sum, B_*, count, undecided, first_undecided (count at the first undecided test)."""
    sig, Bsig, dt, t = (_np64(v) for v in (sig, Bsig, dt, t))
    rgb, Brgb = _np64(rgb), _np64(Brgb)
    N, L = dt.shape
    thr, bgv = f32_exact(T_thresh), f32_exact(bg)
    x = sig * dt
    a, q, da, dq = (v.numpy() for v in CR.alpha_terms(torch.from_numpy(x)))
    z = lambda *s: np.zeros(s)
    ws, Bws, dep, Bd, md, c3, Bc3, mc3, G = z(N), z(N), z(N), z(N), z(N), z(N, 3), z(N, 3), z(N, 3), z(N)
    run, undec = np.ones(N, bool), np.zeros(N, bool)
    cnt, first = np.zeros(N, np.int64), np.full(N, -1, np.int64)
    W, TP, comp = z(N, L), z(N, L), np.zeros((N, L), bool)
    for k in range(L):
        run &= dt[:, k] != 0
        act = run.copy()
        T = 1.0 - ws
        BT = Bws + U32 * np.abs(T)
        BTall = BT + T * G * (1.0 + 2.0 * G)
        w = a[:, k] * T
        Bw = da[:, k] * T + (a[:, k] + da[:, k]) * BT + U32 * w
        wsn = ws + w
        ck, tk = rgb[:, k], t[:, k]
        mdn, mc3n = md + np.abs(w * tk), mc3 + np.abs(w[:, None] * ck)
        a3 = act[:, None]
        Bws = np.where(act, Bws + Bw + U32 * wsn, Bws)
        Bd, Bc3 = np.where(act, Bd + Bw * np.abs(tk) + U32 * mdn, Bd), np.where(a3, Bc3 + Bw[:, None] * np.abs(ck) + U32 * mc3n, Bc3)
        ws, dep, c3 = np.where(act, wsn, ws), np.where(act, dep + w * tk, dep), np.where(a3, c3 + w[:, None] * ck, c3)
        md, mc3 = np.where(act, mdn, md), np.where(a3, mc3n, mc3)
        W[:, k], TP[:, k], comp[:, k] = np.where(act, w, 0.0), T, act
        G = G + np.where(act, dt[:, k] * Bsig[:, k], 0.0)
        cnt += act
        und = act & (np.abs(T - thr) <= BTall)
        first = np.where(und & (first < 0), cnt, first)
        undec |= und
        run &= ~(act & ((T - thr < -BTall) if late else (T < thr)))
    assert float(G.max(initial=0.0)) < 2.0 ** -4, ("first order does not hold: sum dt B_sigma over a ray", float(G.max()))
    infl = (1.0 + 2.0 * G)
    Tn = TP - W                                                              # T_{k+1}
    Tend = 1.0 - ws
    sB = np.where(comp, dt * Bsig, 0.0)
    wc, wt = W[..., None] * rgb, W * t
    Rc = wc.sum(1, keepdims=True) - np.cumsum(wc, 1)                        # sum over i > k
    Rt = wt.sum(1, keepdims=True) - np.cumsum(wt, 1)
    D_ws = Tend * sB.sum(1)
    D_d = (np.abs(Tn * t - Rt) * sB).sum(1)
    D_c = (np.abs(Tn[..., None] * rgb - Rc) * sB[..., None] + W[..., None] * Brgb).sum(1)
    Bws, Bd, Bc3 = Bws + infl * D_ws, Bd + infl * D_d, Bc3 + infl[:, None] * D_c
    one = 1.0 - ws
    image = c3 + bgv * one[:, None]
    Bimg = Bc3 + (abs(bgv) * (Bws + U32 * np.abs(one)) + U32 * np.abs(bgv * one))[:, None] + U32 * np.abs(image)
    Bimg = np.where((cnt > 0)[:, None], Bimg, 0.0)
    return SimpleNamespace(image=image, depth=dep, weights_sum=ws, B_image=Bimg, B_depth=Bd, B_weights_sum=Bws, count=cnt, undecided=undec,
                           first_undecided=first)


def march(case):
    """the CPU oracle's march of every ray of ``case`` over the whole ray (n_step = max_steps): positions, directions, (dt, t) as [N, 256, .] fp32 arrays.
    The Part-1 HIP ops are bit-exact with this oracle and the fused kernels are specified to march by the same arithmetic; C_X holds an ulp of position."""
    import oracle
    o = oracle.ops()
    N, ms = len(case.rays_o), case.max_steps
    b = case.bound
    nears, fars = o.near_far_from_aabb(case.rays_o, case.rays_d, np.array([-b, -b, -b, b, b, b], np.float32), case.min_near)
    xyzs, dirs, deltas = o.march_rays(N, ms, np.arange(N, dtype=np.int32), nears.copy(), case.rays_o, case.rays_d, b, case.bits, 1, case.grid, nears, fars,
                                      dt_gamma=case.dt_gamma, max_steps=ms)
    return xyzs[:N * ms].reshape(N, ms, 3), dirs[:N * ms].reshape(N, ms, 3), deltas[:N * ms].reshape(N, ms, 2), nears, fars


def render_ref(case, mfma, marched=None):
    """float64 render of ``case`` with per-ray bounds of the given arithmetic class (``composite_ref``'s namespace, plus ``count_hi``: the sample count of
    the other alternative of an undecided ray, ``n_marched``: occupied samples along the whole ray, ``hits_box``)"""
    xyzs, dirs, deltas, nears, fars = march(case) if marched is None else marched
    valid = deltas[..., 0] != 0
    L = max(int(valid.sum(1).max(initial=0)), 1)
    valid, N = valid[:, :L], len(valid)
    sig, Bsig, rgb, Brgb = np.zeros((N, L)), np.zeros((N, L)), np.zeros((N, L, 3)), np.zeros((N, L, 3))
    if valid.any():
        s, bs, c, bc = decode_ref(case.P, case.code, xyzs[:, :L][valid], dirs[:, :L][valid], case.sat, mfma)
        sig[valid], Bsig[valid], rgb[valid], Brgb[valid] = s, bs, c, bc
    dt, t = deltas[:, :L, 0].astype(np.float64), deltas[:, :L, 1].astype(np.float64)
    ref = composite_ref(sig, Bsig, rgb, Brgb, dt, t, case.T_thresh, case.bg)
    ref.count_hi = composite_ref(sig, Bsig, rgb, Brgb, dt, t, case.T_thresh, case.bg, late=True).count if ref.undecided.any() else ref.count
    ref.n_marched, ref.hits_box = valid.sum(1), np.isfinite(nears) & (nears < fars)
    ref.samples = SimpleNamespace(valid=valid, sigma=sig, B_sigma=Bsig, rgb=rgb, B_rgb=Brgb)
    return ref


def check_le(got, ref, bound, mask=None):
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v))
    return CR.check_le(got, t(ref), t(bound), t(mask))


def ray_failures(got, ref):
    """{output: (elements outside their bound, worst error / bound)} of a dict of render outputs (image [N, 3], depth, weights_sum, sample_counts [N]).
    Floats of decided rays against their bounds; "counts": decided rays whose sample count is not the reference's, plus undecided rays whose count lies
    outside the range of the two alternatives; "sane": rays, undecided ones included, with an output that is not finite."""
    dec = ~ref.undecided
    res = {k: check_le(got[k], getattr(ref, k), getattr(ref, "B_" + k), dec) for k in ("image", "depth", "weights_sum")}
    cnt = np.asarray(got["sample_counts"]).astype(np.int64).reshape(-1)
    lo = np.where(ref.undecided, np.minimum(ref.count, ref.first_undecided), ref.count)
    hi = np.where(ref.undecided, np.maximum(ref.count, ref.count_hi), ref.count)
    res["counts"] = (int(((cnt < lo) | (cnt > hi)).sum()), 0.0)
    res["sane"] = (sum(int((~np.isfinite(_np64(got[k]))).sum()) for k in ("image", "depth", "weights_sum")), 0.0)
    return res


def n_failures(res) -> int:
    return sum(v[0] for v in res.values())


# ------------------------------------------------------------------------------------------------ seeded case families
RAY_COUNTS = (1, 63, 257, 4097)      # one ray; under a 64-entry queue slice; one past a 256-lane block; two 2048-ray cull blocks and one ray
DT_GAMMAS = (0.0, 0.0038095)
SAT = 0.001


def base_params(b_sigma=0.0, scale=1.0):
    """``synthetic.make_decoder_params`` with the density head's bias moved, and dir_net / color_net scaled as
    test_direction_term_with_large_decoder_weights does (its dir_net bias included)"""
    from ssdnerf_amd import synthetic as S
    sd = {k: v.clone() for k, v in S.make_decoder_params().items()}
    sd["density_net.0.bias"] = sd["density_net.0.bias"] + b_sigma
    if scale != 1.0:
        sd["dir_net.0.weight"] = sd["dir_net.0.weight"] * scale
        sd["dir_net.0.bias"] = torch.linspace(-0.5, 0.5, 64) * scale
        sd["color_net.0.weight"] = sd["color_net.0.weight"] * scale
    return sd


def coherent_params(code, scale=1.0, sa_target=5.5):
    """the flat family's decoder: ``base_params`` with every weight replaced by its magnitude and b1 = 0, on features that are all positive.  Every term of
    every layer then has one sign, so sum |terms| IS the pre-activation: the worst-case form of the layer bounds is attained by any systematic error -- a
    dropped or truncated split product, a missing row -- instead of being averaged away over 18 and then 64 random signs, and a rounding-class error
    still is not.  The density bias puts the (position-independent) density pre-activation at ``sa_target`` (sigma dt = 3.3 per sample: the transmittance falls in steps of e^-3.3, 1.3e-3 and then 4.9e-5, far from either threshold); the colour bias
    centres the colour pre-activations over 256 directions, so that the sigmoid is not saturated for most rays."""
    sd = base_params(0.0, scale)
    for k in ("base_net.0.weight", "density_net.0.weight", "dir_net.0.weight", "color_net.0.weight"):
        sd[k] = sd[k].abs()
    sd["base_net.0.bias"] = torch.zeros(64)
    p = unpack_params(pack_params(sd))
    f = _np64(code)[:, :, 0, 0].T.reshape(-1)                               # f[c * 3 + p]
    h = p.W1 @ f
    s = h * _sig(h)
    sd["density_net.0.bias"] = torch.tensor([np.float32(sa_target - s @ p.ws)])
    d = np.random.default_rng(5).normal(size=(256, 3))
    sh, _ = sh4((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    hc = h + sh @ p.Wd.T + p.bd
    sd["color_net.0.bias"] = torch.from_numpy((-(hc * _sig(hc)) @ p.Wc.T).mean(0).astype(np.float32))
    return sd


def make_rays(rng, n, special=False):
    """``n`` rays (fp32 origins, fp32 unit directions): origins on a shell of radius 2.2 - 3 around the box, seven in ten aimed at the inner
    [-0.45, 0.45]^3 (where the smooth scene's object is), the others at a point of [-1.3, 1.3]^3 (some of these miss the box); the first ray always aims at the centre.  ``special``: from ray 1 on, rays that start inside the box, rays that graze a
    face just inside it (coordinate bound (1 - 2^-12): the gather clamps to the border texel and the neighbour is the clipped one at weight 0) and
    axis-parallel rays (a direction component exactly 0)."""
    o = rng.normal(size=(n, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(2.2, 3.0, (n, 1))
    tgt = np.where(rng.random((n, 1)) < 0.7, rng.uniform(-0.45, 0.45, (n, 3)), rng.uniform(-1.3, 1.3, (n, 3)))
    tgt[0] = rng.uniform(-0.3, 0.3, 3)
    d = tgt - o
    if special and n >= 16:
        e = 1.0 - 2.0 ** -12
        extra_o = [(0.31, -0.22, 2.5), (2.5, 0.11, 0.37), (-0.4, -2.5, 0.05), (-2.5, 0.3, e), (0.2, -2.5, -e), (e, 0.1, 2.5), (-2.5, e, -e)]
        extra_d = [(0, 0, -1), (-1, 0, 0), (0, 1, 0), (1, 0.05, 0), (0.03, 1, 0), (0, 0.02, -1), (1, 0, 0)]
        k = len(extra_o)
        o[1:1 + k], d[1:1 + k] = np.array(extra_o), np.array(extra_d, np.float64)
        m = min(n - 1 - k, max(4, n // 8))
        o[1 + k:1 + k + m] = rng.uniform(-0.7, 0.7, (m, 3))                 # inside the box
        d[1 + k:1 + k + m] = rng.normal(size=(m, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def _aim_distance(o, d):
    """the parameter at which a ray aimed at the inner half of the box is closest to the origin (inside the inner half, hence inside the box)"""
    return float(-(o.astype(np.float64) @ d.astype(np.float64)))


def _random_bits(rng, grid, p):
    return np.packbits((rng.random(grid ** 3) < p).astype(np.uint8), bitorder="little")     # (morton-ordered index space: any pattern is a valid field)


@functools.lru_cache(maxsize=None)
def _smooth_scene(b_sigma):
    """``synthetic.make_triplane`` and the bitfield the oracle derives from its own density (one jittered pass, threshold 0.1), with the decoder whose
    density bias is moved by ``b_sigma`` AFTER the field was derived: the occupied cells stay those of the object"""
    from oracle import render as R
    from ssdnerf_amd import synthetic as S
    code = S.make_triplane()
    jit = [torch.rand(64 ** 3, 3, generator=torch.Generator().manual_seed(7)).numpy()]
    _, bits, _ = R.get_density(S.make_decoder_params(), code, jit, density_thresh=0.1)
    return code.numpy(), np.ascontiguousarray(bits)


FAMILIES = {
    # name: (scene, b_sigma, weight scale, dt_gamma, T_thresh, bg, fp16 planes, ray counts)
    "flat": ("flat", 0.0, 1.0, 0.0, 1e-4, 1.0, False, RAY_COUNTS),
    "flat-x8": ("flat", 0.0, 8.0, 0.0, 1e-4, 1.0, False, (257, 4097)),
    "smooth": ("smooth", -2.0, 1.0, DT_GAMMAS[0], 1e-4, 1.0, False, (1, 257)),
    "smooth-cone": ("smooth", -2.0, 1.0, DT_GAMMAS[1], 1e-4, 1.0, False, (257,)),
    "smooth-fp16": ("smooth", -2.0, 1.0, DT_GAMMAS[0], 1e-4, 1.0, True, (257,)),
    "smooth-cone-fp16": ("smooth", -2.0, 1.0, DT_GAMMAS[1], 1e-4, 1.0, True, (63,)),
    "rough": ("rough", 7.0, 1.0, 0.0, 1e-4, 1.0, False, (1, 257)),
    "opaque-1e-4": ("smooth", 3.0, 1.0, 0.0, THRESHOLDS[0], 1.0, False, (1, 63)),
    "opaque-1e-2": ("smooth", 3.0, 1.0, 0.0, THRESHOLDS[1], 1.0, False, (257,)),
    "thin-bg1": ("smooth", -14.0, 1.0, 0.0, 1e-4, 1.0, False, (257,)),
    "thin-bg0.3": ("smooth", -14.0, 1.0, 0.0, 1e-4, 0.3, False, (1, 257)),
}
CASES = tuple((f, n) for f, v in FAMILIES.items() for n in v[7])


@functools.lru_cache(maxsize=None)
def case(family, n_rays):
    """one seeded case: a namespace with the state dict ``sd`` and its packed block ``P``, ``code`` (3, 6, H, W) fp32 (already fp16-rounded when
    ``fp16``), ``bits`` (uint8, grid^3 / 8), grid, bound, max_steps, min_near, dt_gamma, T_thresh, bg, sat, rays_o / rays_d [N, 3] fp32.
      flat:   every plane channel a positive constant over 128 x 128 (features do not depend on position: the coordinate term is exactly 0) under
              ``coherent_params``; 64^3 grid with isolated occupied cells (p = 0.01): a ray takes a few samples; hot-path geometry
      smooth: synthetic.make_triplane with its density-derived bitfield, 64^3, 128 x 128, bound 1, 256 steps: the specialised kernel forms
      rough:  randn / 2 planes of 40 x 72, 32^3 grid, random bitfield at p = 0.3: the generic forms; rays that graze faces, start inside, run along axes
      smooth runs with the density head's bias at -2: opacities around 0.6 and no ray near the T_thresh cut (with fp32 sums the test T = 1 - ws carries
              an absolute error of ~u per sample, 1 % of T_thresh = 1e-4 after 20 samples: of rays that approach 1e-4 gradually, 2 - 3 % are undecided, which is
              a property of the kernels' arithmetic and more than the cap allows; measured here: 8 of 257 at bias 0)
      (rough: bias +7, opacities around 0.2.)  opaque / thin: the smooth scene with that bias at +3 (the cut falls after ~6 samples, in steps of e^-3 and more) / -14 (weights ~1e-6)"""
    scene, b_sigma, scale, dt_gamma, thr, bg, fp16, _ = FAMILIES[family]
    rng = np.random.default_rng(1000 * list(FAMILIES).index(family) + n_rays)
    if scene == "flat":
        code = np.broadcast_to(rng.uniform(0.2, 1.5, (3, 6, 1, 1)), (3, 6, 128, 128)).astype(np.float32)
        grid, bits = 64, _random_bits(rng, 64, 0.01)
    elif scene == "smooth":
        grid = 64
        code, bits = _smooth_scene(0.0)
    else:
        code = (rng.normal(size=(3, 6, 40, 72)) * 0.5).astype(np.float32)
        grid, bits = 32, _random_bits(rng, 32, 0.3)
    if fp16:
        code = code.astype(np.float16).astype(np.float32)
    sd = coherent_params(code, scale) if scene == "flat" else base_params(b_sigma, scale)
    o, d = make_rays(rng, n_rays, special=scene == "rough")
    if scene != "smooth":                                                   # the cell around the first ray's target is occupied: a one-ray case takes samples
        import oracle
        tgt = o[0].astype(np.float64) + d[0].astype(np.float64) * _aim_distance(o[0], d[0])
        cell = np.clip(np.floor((tgt + 1.0) * 0.5 * grid), 0, grid - 1).astype(np.int32)
        m = int(oracle.ops().morton3D(cell[None])[0])
        bits = bits.copy()
        bits[m >> 3] |= np.uint8(1 << (m & 7))
    return SimpleNamespace(family=family, sd=sd, P=pack_params(sd), code=np.ascontiguousarray(code), fp16=fp16, bits=bits, grid=grid, bound=1.0, max_steps=256,
                           min_near=0.2, dt_gamma=dt_gamma, T_thresh=thr, bg=bg, sat=SAT, rays_o=o, rays_d=d)


@functools.lru_cache(maxsize=None)
def reference(family, n_rays, mfma):
    """(case, float64 reference with the bounds of the arithmetic class); computed once per process and shared (treat both as read-only)"""
    c = case(family, n_rays)
    return c, render_ref(c, mfma, _marched(family, n_rays))


@functools.lru_cache(maxsize=None)
def _marched(family, n_rays):
    return march(case(family, n_rays))


# ------------------------------------------------------------------------------------------------ point decode cases
POINT_CASES = (("square-fp32", (128, 128), False), ("square-fp16", (128, 128), True), ("ragged-fp32", (40, 72), False), ("ragged-fp16", (40, 72), True))


@functools.lru_cache(maxsize=None)
def point_case(name, n=3001):
    """``n`` points for ``point_decode``: the eight corners (+-1, +-1, +-1), the origin, points outside the box (up to 1.3: border clamp), points on texel
    centres and cell borders of the plane, the rest uniform; unit directions, the first three along the axes"""
    _, (H, W), fp16 = next(c for c in POINT_CASES if c[0] == name)
    rng = np.random.default_rng(50 + [c[0] for c in POINT_CASES].index(name))
    if (H, W) == (128, 128):
        from ssdnerf_amd import synthetic as S
        code = S.make_triplane().numpy()
    else:
        code = (rng.normal(size=(3, 6, H, W)) * 0.5).astype(np.float32)
    if fp16:
        code = code.astype(np.float16).astype(np.float32)
    xyz = rng.uniform(-1.0, 1.0, (n, 3))
    xyz[:8] = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    xyz[8] = 0.0
    xyz[9:200] = rng.uniform(-1.3, 1.3, (191, 3))
    xyz[200:300] = (2.0 * rng.integers(0, W, (100, 3)) + 1.0) / W - 1.0     # texel centres along the width: ix is an integer
    xyz[300:400] = 2.0 * rng.integers(0, H + 1, (100, 3)) / H - 1.0          # cell borders along the height
    d = rng.normal(size=(n, 3))
    d[:3] = np.eye(3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    sd = base_params()
    return SimpleNamespace(name=name, sd=sd, P=pack_params(sd), code=np.ascontiguousarray(code), fp16=fp16, xyz=xyz.astype(np.float32), dirs=d.astype(np.float32),
                           sat=SAT)


@functools.lru_cache(maxsize=None)
def point_reference(name):
    c = point_case(name)
    return c, decode_ref(c.P, c.code, c.xyz, c.dirs, c.sat, mfma=False)
