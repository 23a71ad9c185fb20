"""The bounds of tests/_decode_grad_ref.py hold and have teeth (no GPU).
  * per sample: the gcc build of the kernels' arithmetic header (csrc/decode_bwd_math.h through tests/host/decode_bwd_host.c; correctly rounded exp2 and division where
    the device has its hardware units: it stands for the arithmetic class, not for the kernel's bits) lies inside ``B_gf`` on every sample of every per-sample family,
    colour and density-only, with every propagated pre-activation bound under ``GUARD``; silu' without its u (1 - s) term on ONE hidden unit leaves the bound;
  * per texel: a numpy fp32 evaluation of the reduction (fp32 weights, products and additions) of the first stage's ``pos`` and ``gfeat`` lies inside the reduction
    bound on every texel of every reduction family in three orders of the additions (sample order, reversed, a seeded shuffle split into partial sums), and four
    perturbations of it -- a dropped smallest-weight contribution, a doubled one, a run that misses its last lane, a sample lost behind the ring's wrap -- do not;
  * end to end: the same evaluation from the sample positions lies inside the end-to-end bound."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _decode_grad_ref as G
import _render_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@functools.lru_cache(maxsize=None)
def host():
    so = os.path.join(tempfile.mkdtemp(prefix="decode_grad_host"), "decode_bwd_host.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "host", "decode_bwd_host.c"), "-o", so, "-lm"],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.decode_bwd_gf.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def first_stage(c, density_only=False):
    """(gf [total, 18], pos [3, total, 2]) fp32 of the host build, in sample order (no compaction: samples without a gradient give exact zeros)"""
    total = len(c.xyz)
    gf, pos = np.zeros((total, 18), F), np.zeros((3, total, 2), F)
    sh = None if density_only else np.ascontiguousarray(RR.sh4(c.dirs)[0].astype(F))     # (the float64 SH rounded once: within the SH bound of every component)
    for s in range(c.S):
        a, b = int(c.offsets[s]), int(c.offsets[s + 1])
        if a == b:
            continue
        planes = np.zeros((3, c.H, c.W, 8), F)
        planes[..., :6] = c.code[s].transpose(0, 2, 3, 1)
        g, ps = np.zeros((b - a, 18), F), np.zeros((3, b - a, 2), F)
        grgb = None if density_only else np.ascontiguousarray(c.g_rgb[a:b])
        host().decode_bwd_gf(_p(planes), ctypes.c_uint32(c.H), ctypes.c_uint32(c.W), _p(np.ascontiguousarray(c.P, F)), _p(np.ascontiguousarray(c.xyz[a:b])),
                             _p(None if sh is None else np.ascontiguousarray(sh[a:b])), ctypes.c_uint32(b - a), ctypes.c_float(c.sat),
                             _p(np.ascontiguousarray(c.g_sigma[a:b])), _p(grgb), _p(g), _p(ps))
        gf[a:b], pos[:, a:b] = g, ps
    return gf, pos


# ------------------------------------------------------------------------------------------------ per sample
@pytest.mark.parametrize("density_only", [False, True], ids=["colour", "density-only"])
@pytest.mark.parametrize("name", list(G.SAMPLE_FAMILIES))
def test_host_build_meets_the_per_sample_bound(name, density_only):
    c, gf, B, active = G.sample_reference(name, False, density_only)
    got, pos = first_stage(c, density_only)
    bad, worst = G.check_le(got, gf, B)
    print(name, density_only, "worst ratio", round(worst, 3))
    assert bad == 0, (bad, worst)
    assert not np.abs(got[~active]).any() and active.any()
    # the stored coordinate is within C_X u size texels of the float64 coordinate
    ix, iy = G._texel_coords(c.xyz, c.H, c.W)
    assert float(np.abs(pos[..., 0] - ix).max()) <= G.C_X * G.U32 * c.W and float(np.abs(pos[..., 1] - iy).max()) <= G.C_X * G.U32 * c.H
    assert np.array_equal(((np.floor(pos[..., 1]).astype(np.int64) << 16) | np.floor(pos[..., 0]).astype(np.int64)).astype(np.uint32), G.sample_keys(c.xyz, c.H, c.W))


@pytest.mark.parametrize("name", list(G.SAMPLE_FAMILIES))
def test_propagated_bounds_stay_under_the_guard_and_identification_is_unique(name):
    c = G.sample_case(name)
    keys = G.sample_keys(c.xyz, c.H, c.W)
    for s in range(c.S):
        a, b = int(c.offsets[s]), int(c.offsets[s + 1])
        if a == b:
            continue
        assert len(set(zip(keys[0, a:b].tolist(), keys[1, a:b].tolist()))) == b - a <= 3001
        for mfma in (False, True):
            t = G.decode_grad_terms(c.P, c.code[s], c.xyz[a:b], c.dirs[a:b], c.sat, c.g_sigma[a:b], c.g_rgb[a:b], mfma).fwd
            assert max(float(v.max()) for v in (t.B_h, t.B_hc, t.B_sa, t.B_z)) < G.GUARD


def test_knee_family_crosses_both_knees_of_the_clamp():
    c = G.sample_case("knee")
    t = G.decode_grad_terms(c.P, c.code[0], c.xyz[:c.sizes[0]], None, c.sat, c.g_sigma[:c.sizes[0]], None, False, True)
    live = c.g_sigma[:c.sizes[0]] != 0
    lo, hi = (t.e < G.CLAMP_LO) & live, (t.e > G.CLAMP_HI) & live
    inside = (t.e > 1e-3) & (t.e < 1e3) & live
    print("below", int(lo.sum()), "above", int(hi.sum()), "inside", int(inside.sum()))
    assert lo.sum() >= 10 and hi.sum() >= 10 and inside.sum() >= 100
    # past a knee the gradient is the clamp's constant: the bound there is a rounding, not exp's
    assert float((t.B_dsa[hi] / np.abs(t.dsa[hi])).max()) <= 2 * G.U32


def test_silu_derivative_without_its_second_term_on_one_unit_leaves_the_bound():
    c, gf, B, _ = G.sample_reference("square-fp32", False, False)
    wrong = G.decode_grad_terms(c.P, c.code[0], c.xyz, c.dirs, c.sat, c.g_sigma, c.g_rgb, False, False, mutate="silu-term").gf
    bad, worst = G.check_le(wrong, gf, B)
    print("samples x features outside", bad, "worst ratio", round(worst, 1))
    assert bad >= 1 and worst > 1.0


# ------------------------------------------------------------------------------------------------ per texel: the reduction
def corners32(ix, size):
    fl = np.floor(ix)
    i0 = fl.astype(np.int64)
    return i0, np.minimum(i0 + 1, size - 1), ((fl + F(1)) - ix).astype(F), (ix - fl).astype(F)


def contributions32(pos, gfeat, H, W):
    """(texel index [4, n], value [4, n, 6]) fp32: the products of k_decode_bwd_bin_owned / ssdb_scatter18"""
    x0, x1, wx0, wx1 = corners32(pos[:, 0], W)
    y0, y1, wy0, wy1 = corners32(pos[:, 1], H)
    idx = np.stack([y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1])
    w = np.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1]).astype(F)
    return idx, (gfeat[None] * w[..., None]).astype(F), w


def reduce32(idx, val, H, W, order, splits=1):
    """fp32 additions of the contributions of the samples in ``order``, split into ``splits`` partial images that are summed at the end: [6, H, W]"""
    parts = np.zeros((splits, H * W, 6), F)
    for k, chunk in enumerate(np.array_split(order, splits)):
        np.add.at(parts[k], idx[:, chunk].T.reshape(-1), val[:, chunk].transpose(1, 0, 2).reshape(-1, 6))
    out = np.zeros((H * W, 6), F)
    for k in range(splits):
        out = (out + parts[k]).astype(F)
    return out.T.reshape(6, H, W)


@functools.lru_cache(maxsize=None)
def reduction_inputs(kind, planes):
    c = G.reduction_case(kind, planes)
    gf, pos = first_stage(c)
    gfeat = np.ascontiguousarray(gf.reshape(-1, 6, 3).transpose(2, 0, 1))   # [3, total, 6]: gfeat[p][j][c] = gf[j][c * 3 + p]
    return c, pos, gfeat


SPLITS = 4


@pytest.mark.parametrize("kind,planes", G.REDUCTION_CASES)
def test_fp32_reduction_in_any_order_meets_the_reduction_bound(kind, planes):
    c, pos, gfeat = reduction_inputs(kind, planes)
    worst = 0.0
    for s in range(c.S):
        a, b = int(c.offsets[s]), int(c.offsets[s + 1])
        for p in range(3):
            idx, val, _ = contributions32(pos[p, a:b], gfeat[p, a:b], c.H, c.W)
            n = b - a
            for order, splits in ((np.arange(n), 1), (np.arange(n)[::-1], 1), (np.random.default_rng(3).permutation(n), SPLITS)):
                ref, bnd, n_t = G.scatter_ref(pos[p, a:b], gfeat[p, a:b], c.H, c.W, splits)
                got = reduce32(idx, val, c.H, c.W, order, splits)
                bad, r = G.check_le(got, ref, bnd)
                assert bad == 0, (kind, planes, s, p, splits, bad, r)
                assert not got[:, n_t == 0].any()
                worst = max(worst, r)
    print(kind, planes, "worst ratio", round(worst, 3))


def _perturbed(kind, planes, pick):
    """texels outside the reduction bound, per plane, after ``pick(idx, val, w)`` has altered the fp32 contributions (sample order, one image)"""
    c, pos, gfeat = reduction_inputs(kind, planes)
    out = []
    for p in range(3):
        idx, val, w = contributions32(pos[p], gfeat[p], c.H, c.W)
        ref, bnd, _ = G.scatter_ref(pos[p], gfeat[p], c.H, c.W, 1)
        assert G.check_le(reduce32(idx, val, c.H, c.W, np.arange(len(pos[p]))), ref, bnd)[0] == 0
        idx, val = pick(idx.copy(), val.copy(), w)
        out.append(G.check_le(reduce32(idx, val, c.H, c.W, np.arange(idx.shape[1])), ref, bnd)[0])
    return out


def _smallest(w):
    q, i = np.unravel_index(np.argmin(np.where(w > 0, w, np.inf)), w.shape)
    return int(q), int(i)


@pytest.mark.parametrize("planes", list(G.PLANES))
def test_a_dropped_smallest_weight_contribution_leaves_the_bound(planes):
    def pick(idx, val, w):
        q, i = _smallest(w)
        assert 0 < w[q, i] <= 2.0 ** -11                                    # a corner of weight 2^-6 x 2^-6 (or 2^-6 x 1/2) at a border footprint
        val[q, i] = 0
        return idx, val
    bad = _perturbed("borders", planes, pick)
    print(planes, bad)
    assert min(bad) >= 1


@pytest.mark.parametrize("planes", list(G.PLANES))
def test_a_doubled_smallest_weight_contribution_leaves_the_bound(planes):
    def pick(idx, val, w):
        q, i = _smallest(w)
        val[q, i] = val[q, i] * F(2)
        return idx, val
    assert min(_perturbed("borders", planes, pick)) >= 1


@pytest.mark.parametrize("planes", list(G.PLANES))
def test_a_run_that_misses_its_last_lane_leaves_the_bound(planes):
    def pick(idx, val, w):
        val[:, 66 * 500 + 65] = 0                                            # the 66th sample of run 500
        return idx, val
    assert min(_perturbed("runs", planes, pick)) >= 1


@pytest.mark.parametrize("planes", list(G.PLANES))
def test_a_sample_lost_behind_the_ring_wrap_leaves_the_bound(planes):
    def pick(idx, val, w):
        val[:, 1152 + 100] = 0                                               # a slot of the second lap of a 1152-slot ring
        return idx, val
    assert min(_perturbed("quadrant", planes, pick)) >= 1


def test_quadrant_family_stays_inside_one_quadrant_and_borders_family_reaches_every_border():
    for planes, (H, W) in G.PLANES.items():
        _, pos, _ = reduction_inputs("quadrant", planes)
        assert float(pos.max()) < 15.0 and len(pos[0]) == 4000
        _, pos, _ = reduction_inputs("borders", planes)
        for p in range(3):
            x0, y0 = np.floor(pos[p, :, 0]).astype(int), np.floor(pos[p, :, 1]).astype(int)
            want = {(x, y) for x in (15, 16, 31, 32, W - 2, W - 1) if x < W for y in (15, 16, 31, 32, H - 2, H - 1) if y < H}
            assert want <= set(zip(x0.tolist(), y0.tolist())), (planes, p)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("name", [n for n, v in G.SAMPLE_FAMILIES.items() if len(v[3]) > 1])
def test_host_first_stage_and_fp32_reduction_meet_the_end_to_end_bound(name):
    c, gf, B, _ = G.sample_reference(name, False, False)
    got_gf, pos = first_stage(c)
    gfeat = np.ascontiguousarray(got_gf.reshape(-1, 6, 3).transpose(2, 0, 1))
    worst = 0.0
    for s in range(c.S):
        a, b = int(c.offsets[s]), int(c.offsets[s + 1])
        ref, bnd = G.scatter_e2e_ref(c.xyz[a:b], gf[a:b], B[a:b], c.H, c.W, 1)
        got = np.zeros((3, 6, c.H, c.W), F)
        for p in range(3):
            if b > a:
                idx, val, _ = contributions32(pos[p, a:b], gfeat[p, a:b], c.H, c.W)
                got[p] = reduce32(idx, val, c.H, c.W, np.arange(b - a))
        bad, r = G.check_le(got, ref, bnd)
        assert bad == 0, (name, s, bad, r)
        worst = max(worst, r)
    print(name, "worst ratio", round(worst, 3))
