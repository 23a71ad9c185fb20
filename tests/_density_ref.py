"""float64 reference of the density-grid refresh -- ``k_density_update`` (csrc/decode.hip), ``k_packbits<., DEV_THRESH>`` (csrc/raymarching_ops.hip)
and the glue between them (ssdnerf_amd/density.py) -- with the bounds a correct refresh meets, numpy float32 emulations of both kernels, a list of
subtly wrong variants (``MUTANTS``) and the seeded cases that tests/test_density_bounds_cpu.py (the checks accept the emulations and reject every
mutant) and tests/test_density_fp64_gpu.py (the kernels meet them) draw from.  House style of tests/_render_ref.py: every input is the exact value
the kernel read, upcast; every bound is a forward error analysis with its derivation next to the term; nothing is fitted to what the kernels achieve.

The refresh, per scene s and cell n of the H^3 grid (n -> (cx, cy, cz) x-major, H a power of two):
    xyz   = (c - centre) cell + (jitter[n] (2 half_cell) - half_cell)          (no jitter: the first term alone)
    sigma = ssd_mlp<0>(ssd_gather18(planes[s], xyz))                            (``decode_terms(.., mfma=False, density_only=True)``)
    g     = grid[s, morton(cx, cy, cz)];   valid = g >= 0 and sigma is not NaN
    g'    = max(rt(fl32(g decay)), rt(min(sigma, MAX))) where valid, else g     (rt: round to nearest even into the grid dtype, MAX its largest value)
    mean  = sum max(g', 0) / (S H^3)                                            (fp32, one atomic per block of 2048 cells)
    thr   = min(mean, density_thresh), mean rounded to fp16 first for fp16 grids;   bit = g' > thr, little-endian within a byte.

What is held to what:
  cells      a valid cell must lie in [max(dec, rt(min(sigma - B, MAX))), max(dec, rt(min(sigma + B, MAX)))], dec = rt(fl32(g decay)) reproduced exactly
             and B ``decode_terms``' bound with the position uncertainty below: rounding is monotone, so this interval is exactly the set of values a
             kernel whose sigma lies within B can store -- no tolerance is added.  Every other cell must keep its bits.
  position   the kernel's position is no output.  centre, cell, half_cell are the fp32 values the C wrapper forms; c - centre (a half-integer below
             2^10) and 2 half_cell are exact.  With p = (c - centre) cell, q = jitter 2 half_cell, t = q - half_cell: the product rounds <= u |p|, the
             jitter product <= u |q|, the subtraction <= u |t|, the addition <= u |xyz|; an fma contraction of either pair only drops one of them.  Each
             rounding acts on a computed value that carries the earlier ones: <= u^2 (|p| + 2 |q| + |t|) more, below 2 u times the first-order sum;
             (1 + 3 u) covers it and the third order.  Without jitter: u |p|.  ``gather18(pos_unc=)`` turns it into texels.
  mean       over the kernel's OWN output grid g' (so the check is independent of the cells' check), float64 sum of max(g', 0) over all S H^3 cells.
             All terms are non-negative: every partial sum is at most the total, so each fp32 addition errs by at most u times the (computed) total.
             A block adds 8 values per lane in sequence, 6 levels of the wave reduction, 4 wave sums: K_BLOCK = 18 roundings on the block's share;
             inv_count = fl32(1 / (S H^3)) and the product with it: K_SCALE = 2; the atomics add the blocks' shares in any order, one rounding each,
             at most u times the running total: n_blocks.  Compounded exactly: B_mean = mean ((1 + u)^(18 + 2 + n_blocks) - 1), whatever the order --
             the threshold of a refresh is reproducible to rounding, not to the bit.  A block whose total exceeds FLT_MAX (fp32 grids holding FLT_MAX)
             overflows in any order: the mean must then be +inf; a case may not have a total near FLT_MAX (``mean_ref`` refuses it).
  threshold  fp32 grids: in min(mean -+ B_mean, density_thresh); fp16 grids: in min(rt16(mean -+ B_mean), density_thresh) (rt16 is monotone).
  bitfield   equal to g' > (the threshold the refresh returned), bit for bit: the threshold is observable, so no cell is excluded or allowed to flip.
  NaN        a cell whose footprint (the four texels ``ssd_gather18`` loads per plane, weight 0 included: 0 NaN = NaN) holds a NaN texel is not valid.
             The footprint is taken at the reference position -+ its uncertainty; a case in which the two disagree for a cell is refused.

Nothing here needs a GPU."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import _render_ref as RR
from _render_ref import GUARD, U32  # noqa: F401  (re-exported for the two test modules)

F = np.float32
_f64 = lambda a: np.asarray(a, np.float64)
FLT_MAX, HALF_MAX = float(np.finfo(np.float32).max), 65504.0
TPB, CHUNKS = 256, 8
BLOCK = TPB * CHUNKS                 # cells per block of k_density_update
K_BLOCK, K_SCALE = 8 + 6 + 4, 2      # (derivations: the module docstring)
THRESH = 0.01                        # density_thresh of every case (the configs' value)
BOUND = 1.0


# ------------------------------------------------------------------------------------------------ cells, Morton order, rounding
def _spread3(v):
    v, out = np.asarray(v, np.int64), 0
    for i in range(10):
        out = out | (((v >> i) & 1) << (3 * i))
    return out


def morton(cx, cy, cz):
    return _spread3(cx) | (_spread3(cy) << 1) | (_spread3(cz) << 2)


def cell_coords(H):
    n = np.arange(H ** 3, dtype=np.int64)
    return n // (H * H), (n // H) % H, n % H


@functools.lru_cache(maxsize=None)
def morton_of_cell(H):
    """Morton index of cell n (x-major)"""
    return morton(*cell_coords(H))


def grid_np(g16):
    return np.float16 if g16 else np.float32


def rt(x, g16):
    """round to nearest even into the grid dtype, as float64 (numpy converts float64 to either directly: one rounding)"""
    with np.errstate(over="ignore"):
        return _f64(x).astype(grid_np(g16)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ seeded cases
# family: (shift of the density head's bias, weight of the shape pathway's hidden unit in the density head; ``make_decoder_params``: 3)
#   object    +3 puts the field outside the object (3e-4 e^3 = 6e-3, varying smoothly) around density_thresh = 0.01: about four bits in ten are set and the
#             pattern depends on every cell, not on the few cells inside the object
#   sat / overflow   the steeper pathway lifts the inside of the object (silu(4) = 3.93 times the weight) past 65504 / FLT_MAX while the outside stays
#             below density_thresh, so that the bitfield is not all ones
FAMILIES = {"object": (3.0, 3.0), "sparse": (-8.0, 3.0), "sat": (0.0, 6.0), "overflow": (0.0, 30.0), "nan": (3.0, 3.0), "empty": (-120.0, 3.0)}
CASES = {
    # name: (H, S, (Hp, Wp), fp16 planes, fp16 grid, decay, old grid, family)
    "h8-object": (8, 1, (12, 20), False, False, 1.0, "zeros", "object"),
    "h8-object-fp16": (8, 1, (12, 20), True, True, 0.9, "prev", "object"),
    "h8-empty": (8, 1, (12, 20), False, True, 1.0, "zeros", "empty"),
    "h16-object-128": (16, 1, (128, 128), False, True, 0.9, "prev", "object"),
    "h16-sparse-neg": (16, 1, (128, 128), True, False, 0.5, "neg", "sparse"),
    "h16-object-neg-fp16": (16, 1, (12, 20), True, True, 0.5, "neg", "object"),
    "h16-sat-fp16": (16, 1, (12, 20), False, True, 0.9, "prev", "sat"),
    "h16-overflow": (16, 1, (12, 20), False, False, 1.0, "zeros", "overflow"),
    "h16-sat-fp32": (16, 1, (12, 20), True, False, 0.9, "prev", "sat"),
    "h16-nan": (16, 1, (12, 20), False, False, 0.9, "prev", "nan"),
    "h32-s3-sparse": (32, 3, (12, 20), False, True, 0.9, "prev", "sparse"),
    "h32-s2-object": (32, 2, (12, 20), True, False, 1.0, "zeros", "object"),
}
NAN_TEXEL = (0, 2, 6, 11)            # (plane, channel, row, column) of the "nan" family's texel


def _scene_code(seed, plane):
    """``synthetic.make_triplane`` (``_render_ref._smooth_scene``'s object), resampled to ``plane`` by nearest neighbour where that is not 128 x 128: a
    small, non-square plane whose texel-to-texel slopes are steep (the silhouette channel jumps from -2 to 2) and whose border texels are reached"""
    from ssdnerf_amd import synthetic as S
    code = S.make_triplane(seed)
    if tuple(plane) != tuple(code.shape[2:]):
        code = torch.nn.functional.interpolate(code, size=tuple(plane), mode="nearest")
    return code.numpy().astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """one seeded case: H, S, code [S, 3, 6, Hp, Wp] fp32 (fp16 values for fp16 planes), state dict ``sd`` and packed block ``P``, ``jitter`` [H^3, 3] fp32
    in [0, 1), ``decay``, ``old`` [S, H^3] in the grid dtype and Morton order, ``thresh``, ``bound``.
      families   object: mean > density_thresh;  sparse: mean < density_thresh;  sat: the object's inside exceeds 65504;  overflow: it exceeds FLT_MAX;
                 nan: the object with one NaN texel;  empty: every density underflows to 0 (the all-empty control: threshold 0, no bit set)
      old grids  zeros (the first step of get_density);  prev: what a refresh with another jitter leaves, rt(min(sigma, MAX));  neg: the same times a
                 per-cell factor in [1/4, 4] (so that decay 0.5 meets both branches), a fifth of the cells -1
    ``"<name>@<i>"`` is step i of ``get_density`` on that case's scene: its own jitter, decay 1.0, and a zero grid unless the caller passes the old one."""
    if "@" in name:
        base, step = name.split("@")
        b = case(base)
        jit = np.random.default_rng(9000 + int(step)).random((b.H ** 3, 3), dtype=np.float32)
        return SimpleNamespace(**{**b.__dict__, "name": name, "jitter": jit, "decay": 1.0, "old_kind": "zeros", "old": np.zeros_like(b.old)})
    H, S, plane, p16, g16, decay, old_kind, family = CASES[name]
    rng = np.random.default_rng(7000 + list(CASES).index(name))
    code = np.stack([_scene_code(2021 + s, plane) for s in range(S)])
    if family == "nan":
        code[(0,) + NAN_TEXEL] = np.nan
    if p16:
        code = code.astype(np.float16).astype(np.float32)
    sd = RR.base_params(FAMILIES[family][0])
    sd["density_net.0.weight"][0, 0] = FAMILIES[family][1]
    c = SimpleNamespace(name=name, H=H, S=S, p16=p16, g16=g16, decay=decay, family=family, old_kind=old_kind, code=np.ascontiguousarray(code), sd=sd,
                        P=RR.pack_params(sd), jitter=rng.random((H ** 3, 3), dtype=np.float32), thresh=THRESH, bound=BOUND)
    old = np.zeros((S, H ** 3), grid_np(g16))
    if old_kind != "zeros":
        prev = rng.random((H ** 3, 3), dtype=np.float32)
        sig = np.stack([_decode(c, s, *positions(c, prev))[0] for s in range(S)])
        if old_kind == "neg":
            sig = sig * np.exp2(rng.uniform(-2.0, 2.0, sig.shape))
        v = np.minimum(sig, HALF_MAX if g16 else FLT_MAX).astype(grid_np(g16))
        if old_kind == "neg":
            v[rng.random(v.shape) < 0.2] = -1.0
        old[:, morton_of_cell(H)] = v
    c.old = old
    return c


# ------------------------------------------------------------------------------------------------ the float64 reference
def positions(c, jitter):
    """(xyz [H^3, 3], B_pos [H^3, 3]) in float64, cells x-major; ``jitter``: [H^3, 3] fp32 or None (derivation: the module docstring)"""
    H = c.H
    centre, cell, half_cell = float(F((H - 1) / 2.0)), float(F(2.0 * c.bound / H)), float(F(c.bound / H))     # as the C wrapper forms them from doubles
    p = (np.stack(cell_coords(H), 1).astype(np.float64) - centre) * cell
    if jitter is None:
        return p, U32 * np.abs(p)
    q = _f64(jitter) * (2.0 * half_cell)
    t = q - half_cell
    xyz = p + t
    return xyz, U32 * (np.abs(p) + np.abs(q) + np.abs(t) + np.abs(xyz)) * (1.0 + 3.0 * U32)


def _clean(code):
    return np.where(np.isnan(code), 0.0, code)


def _decode(c, s, xyz, Bpos):
    t = RR.decode_terms(c.P, _clean(c.code[s]), xyz, None, RR.SAT, mfma=False, density_only=True, pos_unc=Bpos)
    return t.sigma, t.B_sigma


def nan_footprint(c, s, xyz, Bpos):
    """(touched at every position within the uncertainty, touched at some) per cell: does the footprint of any plane hold a NaN texel"""
    code = c.code[s]
    every, some = np.zeros(len(xyz), bool), np.zeros(len(xyz), bool)
    if not np.isnan(code).any():
        return every, some
    Hp, Wp = code.shape[2:]
    for p, (a, b) in enumerate(RR.ORDER):
        bad = np.isnan(code[p]).any(0)
        if not bad.any():
            continue
        ix, iy = RR._coord(xyz[:, a], Wp), RR._coord(xyz[:, b], Hp)
        dx, dy = RR.C_X * U32 * Wp + 0.5 * Wp * Bpos[:, a], RR.C_X * U32 * Hp + 0.5 * Hp * Bpos[:, b]
        hit = []
        for sx in (-1.0, 1.0):
            for sy in (-1.0, 1.0):
                x0, x1, _, _ = RR._foot(np.clip(ix + sx * dx, 0.0, Wp - 1.0), Wp)
                y0, y1, _, _ = RR._foot(np.clip(iy + sy * dy, 0.0, Hp - 1.0), Hp)
                hit.append(bad[y0, x0] | bad[y0, x1] | bad[y1, x0] | bad[y1, x1])
        every |= np.logical_and.reduce(hit)
        some |= np.logical_or.reduce(hit)
    return every, some


def reference(name, use_jitter=True, old=None):
    """the reference of case ``name`` (with its jitter, or the jitter-free form), optionally on another old grid ``old`` [S, H^3]: a namespace of
    [S, H^3] arrays in Morton order -- ``valid``, ``dec``, ``lo`` <= cell <= ``hi`` (float64 values of the grid dtype), and ``sigma``, ``B`` (float64),
    ``fresh_lo`` / ``fresh_hi`` (the fresh value's own interval).  The decode is computed once per (case, jitter form) and shared."""
    c = case(name)
    sig, B, nan = _fresh(name, use_jitter)
    old = c.old if old is None else old
    assert old.dtype == grid_np(c.g16) and old.shape == (c.S, c.H ** 3)
    MAX = HALF_MAX if c.g16 else FLT_MAX
    old32 = old.astype(F)
    with np.errstate(invalid="ignore"):
        dec = rt(old32 * F(c.decay), c.g16)                                # one fp32 product, then the grid rounding: exact
    flo, fhi = rt(np.minimum(sig - B, MAX), c.g16), rt(np.minimum(sig + B, MAX), c.g16)
    valid = (old32 >= 0) & ~nan
    return SimpleNamespace(valid=valid, old=old, dec=dec, lo=np.maximum(dec, flo), hi=np.maximum(dec, fhi), sigma=sig, B=B, fresh_lo=flo, fresh_hi=fhi, nan=nan)


@functools.lru_cache(maxsize=None)
def _fresh(name, use_jitter):
    c = case(name)
    xyz, Bpos = positions(c, c.jitter if use_jitter else None)
    m = morton_of_cell(c.H)
    sig, B, nan = np.zeros((c.S, c.H ** 3)), np.zeros((c.S, c.H ** 3)), np.zeros((c.S, c.H ** 3), bool)
    for s in range(c.S):
        sig[s, m], B[s, m] = _decode(c, s, xyz, Bpos)
        every, some = nan_footprint(c, s, xyz, Bpos)
        assert not (some & ~every).any(), "a cell's footprint holds the NaN texel at one end of its position uncertainty only: choose another seed"
        nan[s, m] = every
    return sig, B, nan


# ------------------------------------------------------------------------------------------------ the checks
def _bits_of(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def check_cells(ref, got):
    """{"cells": (valid cells outside their interval, worst |cell - centre| / half-width), "untouched": (other cells whose bits changed, 0)}; a valid
    cell whose interval is one value has ratio 0 where it equals it"""
    assert got.dtype == ref.old.dtype and got.shape == ref.old.shape
    g = got.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inside = (g >= ref.lo) & (g <= ref.hi)                              # (a NaN is outside)
        half, mid = (ref.hi - ref.lo) * 0.5, ref.lo + (ref.hi - ref.lo) * 0.5
        ratio = np.where(half > 0, np.abs(g - mid) / np.where(half > 0, half, 1.0), np.where(g == ref.lo, 0.0, np.inf))
    bad = ref.valid & ~inside
    worst = float(np.where(ref.valid & inside, ratio, 0.0).max(initial=0.0)) if not bad.any() else float("inf")
    return dict(cells=(int(bad.sum()), worst), untouched=(int((~ref.valid & (_bits_of(got) != _bits_of(ref.old))).sum()), 0.0))


def n_blocks(c):
    return c.S * (-(-c.H ** 3 // BLOCK))


def mean_ref(c, got):
    """(mean, B_mean) of the kernel's own output grid ``got`` [S, H^3]; (inf, 0) where a block's sum overflows fp32 in any order"""
    v = np.maximum(got.astype(np.float64), 0.0)
    v = np.where(np.isnan(v), 0.0, v)                                       # fmaxf(NaN, 0) = 0
    H3 = c.H ** 3
    k = K_BLOCK + K_SCALE + n_blocks(c)
    grow = math.expm1(k * math.log1p(U32))
    per_block = np.zeros((c.S, -(-H3 // BLOCK) * BLOCK))
    per_block[:, :H3] = v[:, morton_of_cell(c.H)]
    tot = per_block.reshape(c.S, -1, BLOCK).sum(-1)
    over = tot * (1.0 - K_BLOCK * U32) > FLT_MAX * (1.0 + U32)
    if over.any():
        return float("inf"), 0.0
    mean = float(v.sum() / (c.S * H3))
    assert float(tot.max()) * (1.0 + grow) < FLT_MAX and mean * (1.0 + grow) < FLT_MAX, "a sum near FLT_MAX: the case does not decide whether it overflows"
    return mean, mean * grow


def check_mean(c, got_grid, got_mean):
    mean, B = mean_ref(c, got_grid)
    got_mean = float(got_mean)
    if math.isinf(mean) or B == 0.0:
        ok = got_mean == mean
        return dict(mean=(int(not ok), 0.0 if ok else float("inf")))
    err = abs(got_mean - mean)
    return dict(mean=(int(not err <= B), err / B))


def thresh_interval(c, got_grid):
    """[lo, hi] of the threshold a refresh may return for its own output grid"""
    mean, B = mean_ref(c, got_grid)
    lo, hi = mean - B, mean + B
    if c.g16:
        lo, hi = float(rt(lo, True)), float(rt(hi, True))                  # ``mean.half().float()``
    t = float(F(c.thresh))
    return min(lo, t), min(hi, t)


def check_thresh(c, got_grid, thr):
    lo, hi = thresh_interval(c, got_grid)
    return dict(thresh=(int(not lo <= float(thr) <= hi), 0.0))


def expected_bits(got_grid, thr):
    with np.errstate(invalid="ignore"):
        return np.packbits(got_grid.astype(F) > F(thr), axis=1, bitorder="little")


def check_bits(got_grid, thr, bits):
    exp = expected_bits(got_grid, thr)
    assert bits.shape == exp.shape and bits.dtype == np.uint8
    return dict(bits=(int(np.unpackbits(bits ^ exp).sum()), 0.0))


def check_refresh(c, ref, out):
    """every check on a whole refresh ``out``: grid [S, H^3], mean (fp32, as the kernel left it; None: not taken), thr (the threshold used and
    returned), bits [S, H^3 / 8]"""
    res = check_cells(ref, out.grid)
    if out.mean is not None:
        res.update(check_mean(c, out.grid, out.mean))
        res.update(check_thresh(c, out.grid, out.thr))
        res.update(check_bits(out.grid, out.thr, out.bits))
    return res


def n_failures(res):
    return sum(v[0] for v in res.values())


# ------------------------------------------------------------------------------------------------ fp32 emulations of the two kernels and the glue
LOG2E = F(1.4426950408889634)
MUTANTS = {
    # what is wrong: the case on which a check must fail
    "decay-unrounded": "h8-object-fp16",        # the decayed value not rounded to the grid dtype before the max (rounding is monotone: the stored cell is the same, the mean is not)
    "decay-fused": "h8-object-fp16",            # the exact product rounded once, straight to fp16 (what v_fma_mixlo_f16 gives): other than rt16(fl32(.)) for one fp16 value in 23 at decay 0.9
    "decay-after-max": "h8-object-fp16",        # max(old, fresh) decay
    "jitter-half": "h8-object",                 # jitter scaled by half_cell: half a cell of bias
    "tail-chunk": "h8-object",                  # the last chunk of a partly filled block dropped
    "mean-one-scene": "h32-s3-sparse",          # the mean over scene 0 alone
    "mean-neg": "h16-object-neg-fp16",          # a -1 cell counted as -1
    "mean-no-fp16-round": "h32-s3-sparse",      # the fp16 rounding of the mean skipped
    "packbits-ge": "h8-empty",                  # >= for >
    "no-saturation": "h16-sat-fp16",            # the clamp at the dtype's largest value missing
    "no-saturation-fp32": "h16-overflow",
    "centre": "h8-object",                      # centre = H / 2
    "z-major": "h16-object-128",                # cell n taken z-major (the jitter row then belongs to another cell)
    "morton-swap": "h16-object-128",            # Morton index of (cz, cy, cx)
    "thresh-max": "h8-object",                  # max for min in the threshold
    "nan-fmin": "h16-nan",                      # NaN tested after fminf(sigma, MAX), which returns MAX for a NaN
}
_POSITION_MUTANTS = ("jitter-half", "centre", "z-major")


def fma(a, b, c):
    return (_f64(a) * _f64(b) + _f64(c)).astype(F)                          # (24-bit factors: the float64 product is exact, the sum rounds twice only in ties)


def _exp2(x):
    return np.exp2(_f64(x)).astype(F)


def _rcp(x):
    return (1.0 / _f64(x)).astype(F)


def _emu_coord(u, size):
    sf = F(size)
    ix = ((u + F(1)) * sf - F(1)) * F(0.5)
    ix = np.minimum(sf - F(1), np.maximum(ix, F(0)))
    fl = np.floor(ix)
    i0 = fl.astype(np.int64)
    return i0, np.minimum(i0 + 1, size - 1), ((fl + F(1)) - ix).astype(F), (ix - fl).astype(F)


def emu_sigma(P, code, xyz):
    """``ssd_gather18`` and ``ssd_mlp<0>`` in fp32, in their order (correctly rounded exp2 / reciprocal where the kernel uses the hardware units: the
    emulation stands for the arithmetic class, not for the kernel's bits)"""
    code, xyz = np.asarray(code, F), np.asarray(xyz, F)
    Hp, Wp = code.shape[2:]
    f = np.zeros((len(xyz), 18), F)
    for p, (a, b) in enumerate(RR.ORDER):
        x0, x1, wx0, wx1 = _emu_coord(xyz[:, a], Wp)
        y0, y1, wy0, wy1 = _emu_coord(xyz[:, b], Hp)
        pl = code[p]
        w00, w01, w10, w11 = (wx0 * wy0)[:, None], (wx1 * wy0)[:, None], (wx0 * wy1)[:, None], (wx1 * wy1)[:, None]
        f[:, np.arange(6) * 3 + p] = fma(pl[:, y1, x1].T, w11, fma(pl[:, y1, x0].T, w10, fma(pl[:, y0, x1].T, w01, pl[:, y0, x0].T * w00)))
    p = RR.unpack_params(P)
    W1, b1, ws = np.asarray(p.W1, F), np.asarray(p.b1, F), np.asarray(p.ws, F)
    h = np.broadcast_to(b1, (len(xyz), 64)).astype(F)
    for k in range(18):
        h = fma(W1[None, :, k], f[:, k, None], h)
    s = h * _rcp(F(1) + _exp2(h * -LOG2E))
    sa = np.full(len(xyz), F(p.bs), F)
    for i in range(64):
        sa = fma(ws[i], s[:, i], sa)
    return _exp2(sa * LOG2E)


def _emu_cells(c, mut):
    n = np.arange(c.H ** 3, dtype=np.int64)
    if mut == "z-major":
        return n % c.H, (n // c.H) % c.H, n // (c.H * c.H)
    return cell_coords(c.H)


@functools.lru_cache(maxsize=None)
def _emu_fresh(name, contract, use_jitter, mut):
    """sigma [S, H^3] fp32 per cell n, by the straightforward form of the position or the fma-contracted one"""
    c = case(name)
    H = c.H
    centre = F(H / 2.0) if mut == "centre" else F((H - 1) / 2.0)
    cell, half_cell = F(2.0 * c.bound / H), F(c.bound / H)
    d = np.stack(_emu_cells(c, mut), 1).astype(F) - centre
    if not use_jitter:
        xyz = d * cell
    else:
        scale = half_cell if mut == "jitter-half" else F(2) * half_cell
        xyz = fma(d, cell, fma(c.jitter, scale, -half_cell)) if contract else d * cell + (c.jitter * scale - half_cell)
    with np.errstate(all="ignore"):
        return np.stack([emu_sigma(c.P, c.code[s], xyz) for s in range(c.S)])


def _emu_mean(contrib, c, mut, reverse):
    """the block reduction and the atomics of k_density_update on contrib [S, H^3] (fp32, cells x-major); ``reverse``: the atomics in the opposite order"""
    H3 = c.H ** 3
    nb = -(-H3 // BLOCK)
    x = np.zeros((c.S, nb * BLOCK), F)
    x[:, :H3] = contrib
    x = x.reshape(c.S, nb, CHUNKS, TPB)
    with np.errstate(over="ignore", invalid="ignore"):
        lane = np.zeros((c.S, nb, TPB), F)
        for ch in range(CHUNKS):
            lane = lane + x[:, :, ch]
        w = lane.reshape(c.S, nb, TPB // 64, 64).copy()
        for off in (32, 16, 8, 4, 2, 1):
            w[..., :off] = w[..., :off] + w[..., off:2 * off]
        t = np.zeros((c.S, nb), F)
        for i in range(TPB // 64):
            t = t + w[..., i, 0]
        inv = F(1.0 / H3) if mut == "mean-one-scene" else F(1.0 / (float(c.S) * float(H3)))
        part = (t * inv)[:1] if mut == "mean-one-scene" else t * inv
        mean = F(0)
        for v in (part.reshape(-1)[::-1] if reverse else part.reshape(-1)):
            mean = F(mean + v)
    return mean


def emulate(name, contract=False, use_jitter=True, want_mean=True, mut=None, old=None):
    """one refresh of case ``name`` by the emulation: a namespace (grid, mean, thr, bits) as ``check_refresh`` takes it.  ``contract``: the fma-contracted
    position and the atomics in the opposite order; ``mut``: one of ``MUTANTS``"""
    c = case(name)
    g16, gd = c.g16, grid_np(c.g16)
    MAX = F(HALF_MAX if g16 else FLT_MAX)
    sig = _emu_fresh(name, contract, use_jitter, mut if mut in _POSITION_MUTANTS else None)
    cx, cy, cz = _emu_cells(c, mut)
    idx = morton(cz, cy, cx) if mut == "morton-swap" else morton(cx, cy, cz)
    old = c.old if old is None else old
    grid = old.copy()
    contrib = np.zeros((c.S, c.H ** 3), F)
    rnd = lambda v: v.astype(gd).astype(F)
    skip = np.zeros(c.H ** 3, bool)
    if mut == "tail-chunk" and c.H ** 3 % BLOCK:
        skip[c.H ** 3 - TPB:] = True
    with np.errstate(all="ignore"):
        for s in range(c.S):
            o = old[s, idx].astype(F)
            fresh = rnd(sig[s] if mut in ("no-saturation", "no-saturation-fp32") else np.fmin(sig[s], MAX))      # fminf: a NaN gives MAX
            valid = (o >= 0) & (fresh >= 0) & ~skip
            if mut != "nan-fmin":
                valid &= ~np.isnan(sig[s])
            if mut == "decay-after-max":
                out = np.maximum(o, fresh) * F(c.decay)
            elif mut == "decay-unrounded":
                out = np.maximum(o * F(c.decay), fresh)
            elif mut == "decay-fused":
                out = np.maximum((_f64(o) * float(F(c.decay))).astype(gd).astype(F), fresh)
            else:
                out = np.maximum(rnd(o * F(c.decay)), fresh)
            out = np.where(valid, out, o)
            grid[s, idx[valid]] = out[valid].astype(gd)
            contrib[s] = np.where(skip, F(0), out if mut == "mean-neg" else np.fmax(out, F(0)))
        if not want_mean:
            return SimpleNamespace(grid=grid, mean=None, thr=None, bits=None)
        mean = _emu_mean(contrib, c, mut, reverse=contract)
        m = mean if (not g16 or mut == "mean-no-fp16-round") else F(np.float16(mean))
        thr = np.maximum(m, F(c.thresh)) if mut == "thresh-max" else np.fmin(m, F(c.thresh))
        gf = grid.astype(F)
        bits = np.packbits((gf >= thr) if mut == "packbits-ge" else (gf > thr), axis=1, bitorder="little")
    return SimpleNamespace(grid=grid, mean=mean, thr=F(thr), bits=bits)
