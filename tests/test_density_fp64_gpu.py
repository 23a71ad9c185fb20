"""The density-grid refresh -- ``k_density_update`` (csrc/decode.hip), ``k_packbits<., DEV_THRESH>`` (csrc/raymarching_ops.hip) and the glue of
ssdnerf_amd/density.py -- against the float64 reference and the checks of tests/_density_ref.py, on the seeded cases that
tests/test_density_bounds_cpu.py proves the checks on, at three levels: the C ABI (also without a mean and without jitter),
``density.update_density_grid`` (with the threshold it returns) and ``density.get_density`` (every step against the previous step's own grid).
Every valid cell must lie in its interval, every other cell keep its bits, the mean lie within its bound of the float64 mean of the kernel's own
grid, and the bitfield equal ``grid > threshold`` bit for bit.  A grid size that is not a power of two is refused at both entry points, with the
grid and the bitfield untouched.  Oracle parity stays in tests/test_render_gpu.py.

``python tests/test_density_fp64_gpu.py OUT.json`` runs every case through the C ABI and writes the worst error / bound ratios
(profiles/density_bounds.json is such a run)."""
import functools
import json
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _density_ref as DR

pytestmark = pytest.mark.gpu
NAMES = tuple(DR.CASES)
STEPS_CASE = "h16-object-neg-fp16"       # get_density: H = 16, fp16 planes, fp16 grid


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def planes_of(name):
    from ssdnerf_amd.decoders import pack_triplanes
    c = DR.case(name)
    return pack_triplanes(cu(c.code), torch.float16 if c.p16 else torch.float32)


@functools.lru_cache(maxsize=None)
def decoder_of(family):
    """a decoder that holds the family's state dict; the packed block the kernel reads must be the one the reference upcasts"""
    from ssdnerf_amd.decoders import TriPlaneDecoder
    c = DR.case(next(n for n in NAMES if DR.CASES[n][7] == family))
    dec = TriPlaneDecoder(base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], dir_layers=[16, 64], max_steps=256)
    dec.load_state_dict(c.sd, strict=False)
    dec = dec.cuda().eval()
    assert dec.bound == c.bound and np.array_equal(dec.packed_params().cpu().numpy().view(np.uint32), c.P.view(np.uint32))
    return dec


def run_cabi(name, use_jitter=True, want_mean=True):
    """``ssdnerf_density_grid_update`` + ``ssdnerf_packbits_dev_thresh`` as the glue calls them; the mean is returned as the kernel left it"""
    from ssdnerf_amd import _cabi as C
    c = DR.case(name)
    planes, P = planes_of(name), cu(c.P)
    grid, bits = cu(c.old), torch.zeros(c.S, c.H ** 3 // 8, dtype=torch.uint8).cuda()
    jitter = cu(c.jitter) if use_jitter else None
    mean = torch.zeros(1, dtype=torch.float32).cuda() if want_mean else None
    _, _, hp, wp, _ = planes.shape
    C.check(C.lib().ssdnerf_density_grid_update(C.ptr(planes), C.dtype_code(planes), C.u32(hp), C.u32(wp), C.ptr(P), C.u32(c.S), C.u32(c.H), C.f32(c.bound),
                                                C.ptr(jitter), C.f32(c.decay), C.ptr(grid), C.dtype_code(grid), C.ptr(mean), C.stream()), "density_grid_update")
    if not want_mean:
        torch.cuda.synchronize()
        return SimpleNamespace(grid=grid.cpu().numpy(), mean=None, thr=None, bits=None)
    m = mean.half().float() if c.g16 else mean
    C.check(C.lib().ssdnerf_packbits_dev_thresh(C.ptr(grid), C.dtype_code(grid), C.u32(c.S * c.H ** 3 // 8), C.ptr(m), C.f32(c.thresh), C.ptr(bits),
                                                C.stream()), "packbits_dev_thresh")
    torch.cuda.synchronize()
    thr = np.fmin(m.cpu().numpy()[0], np.float32(c.thresh))
    return SimpleNamespace(grid=grid.cpu().numpy(), mean=mean.cpu().numpy()[0], thr=thr, bits=bits.cpu().numpy())


def run_api(name, old=None):
    from ssdnerf_amd.density import update_density_grid
    c = DR.case(name)
    grid, bits = cu(c.old if old is None else old), torch.zeros(c.S, c.H ** 3 // 8, dtype=torch.uint8).cuda()
    thr = update_density_grid(decoder_of(c.family), cu(c.code), grid, bits, density_thresh=c.thresh, decay=c.decay, jitter=cu(c.jitter), planes=planes_of(name))
    assert thr.dtype == torch.float32 and thr.dim() == 0
    return SimpleNamespace(grid=grid.cpu().numpy(), thr=thr.cpu().numpy()[()], bits=bits.cpu().numpy())


def api_failures(c, ref, out):
    res = DR.check_cells(ref, out.grid)
    res.update(DR.check_thresh(c, out.grid, out.thr))
    res.update(DR.check_bits(out.grid, out.thr, out.bits))
    return res


def show(tag, res):
    print(tag, {k: (v[0], round(v[1], 4)) for k, v in res.items()})


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("name", NAMES)
def test_the_kernels_meet_every_check(name):
    c = DR.case(name)
    res = DR.check_refresh(c, DR.reference(name), run_cabi(name))
    show(name, res)
    assert DR.n_failures(res) == 0, res


@pytest.mark.parametrize("name", ["h8-object", "h16-object-128", "h16-nan", "h32-s3-sparse"])
def test_the_kernels_meet_every_check_without_a_mean_and_without_jitter(name):
    c = DR.case(name)
    res = DR.check_refresh(c, DR.reference(name), run_cabi(name, want_mean=False))
    show(name + " no mean", res)
    assert set(res) == {"cells", "untouched"} and DR.n_failures(res) == 0, res
    res = DR.check_refresh(c, DR.reference(name, use_jitter=False), run_cabi(name, use_jitter=False))
    show(name + " no jitter", res)
    assert DR.n_failures(res) == 0, res


# ------------------------------------------------------------------------------------------------ update_density_grid
@pytest.mark.parametrize("name", NAMES)
def test_update_density_grid_meets_every_check_and_repeats_its_grid(name):
    c, ref = DR.case(name), DR.reference(name)
    a, b = run_api(name), run_api(name)
    for out in (a, b):
        res = api_failures(c, ref, out)
        show(name, res)
        assert DR.n_failures(res) == 0, res
    assert np.array_equal(DR._bits_of(a.grid), DR._bits_of(b.grid))         # (the thresholds may differ within the mean's bound: the atomics' order)


# ------------------------------------------------------------------------------------------------ get_density
def test_get_density_meets_the_checks_at_every_step(monkeypatch):
    """8 steps from zeros with injected jitters: each step's grid against the reference on the previous step's own grid as the exact old one; the final
    bitfield against the final grid and the threshold interval of its mean (which must decide every bit)"""
    from ssdnerf_amd import density
    steps = 8
    cases = [DR.case(f"{STEPS_CASE}@{i}") for i in range(steps)]
    c0 = cases[0]
    grids, inner = [], density.update_density_grid

    def recording(decoder, code, grid, bits, **kw):
        out = inner(decoder, code, grid, bits, **kw)
        grids.append(grid.cpu().numpy().copy())
        return out

    monkeypatch.setattr(density, "update_density_grid", recording)
    grid, bits = density.get_density(decoder_of(c0.family), cu(c0.code), grid_size=c0.H, density_thresh=c0.thresh, density_step=steps,
                                     jitters=[cu(c.jitter) for c in cases], grid_dtype=torch.float16)
    assert len(grids) == steps and np.array_equal(DR._bits_of(grid.cpu().numpy()), DR._bits_of(grids[-1]))
    old = np.zeros_like(c0.old)
    for i, c in enumerate(cases):
        res = DR.check_cells(DR.reference(c.name, old=old), grids[i])
        show(c.name, res)
        assert DR.n_failures(res) == 0, (i, res)
        old = grids[i]
    assert int((grids[-1] != grids[0]).sum()) >= 100                         # (later steps did raise cells)
    lo, hi = DR.thresh_interval(cases[-1], grids[-1])
    exp = DR.expected_bits(grids[-1], lo)
    assert np.array_equal(exp, DR.expected_bits(grids[-1], hi)) and np.array_equal(bits.cpu().numpy(), exp)
    assert 0.01 <= float(np.unpackbits(exp).mean()) <= 0.99


# ------------------------------------------------------------------------------------------------ the guard
@pytest.mark.parametrize("grid_size", [12, 24, 1])
@pytest.mark.parametrize("g16", [False, True], ids=["fp32", "fp16"])
def test_a_grid_size_that_is_no_power_of_two_is_refused_without_a_launch(grid_size, g16):
    """cell (cx, cy, cz) is written at its Morton index: 3647 at most for H = 12, whose grid has 1728 cells.  The library returns its error before
    any launch; the buffers are sized for the largest index such a launch could reach all the same, and keep their sentinels"""
    from ssdnerf_amd import _cabi as C
    c = DR.case("h8-object")
    planes, P = planes_of("h8-object"), cu(c.P)
    cells = 32 ** 3
    grid = torch.full((cells,), 7.0, dtype=torch.float16 if g16 else torch.float32).cuda()
    bits = torch.full((cells // 8,), 0xA5, dtype=torch.uint8).cuda()
    mean = torch.full((1,), 3.0).cuda()
    _, _, hp, wp, _ = planes.shape
    status = C.lib().ssdnerf_density_grid_update(C.ptr(planes), C.dtype_code(planes), C.u32(hp), C.u32(wp), C.ptr(P), C.u32(1), C.u32(grid_size), C.f32(1.0),
                                                 C.ptr(None), C.f32(0.9), C.ptr(grid), C.dtype_code(grid), C.ptr(mean), C.stream())
    torch.cuda.synchronize()
    assert status != 0 and b"power of two" in C.lib().ssdnerf_last_error()
    with pytest.raises(RuntimeError, match="power of two"):
        C.check(status, "density_grid_update")
    assert bool((grid == 7.0).all()) and bool((bits == 0xA5).all()) and float(mean[0]) == 3.0


def test_update_density_grid_refuses_such_a_grid_before_it_allocates_or_launches():
    from ssdnerf_amd.density import update_density_grid
    c = DR.case("h8-object")
    grid, bits = torch.full((1, 12 ** 3), 7.0).cuda(), torch.full((1, 12 ** 3 // 8), 0xA5, dtype=torch.uint8).cuda()
    dec, code, planes = decoder_of(c.family), cu(c.code), planes_of("h8-object")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="power of two"):
        update_density_grid(dec, code, grid, bits, jitter=None, planes=planes)      # (jitter=None: a guard that came late would have drawn one)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and bool((grid == 7.0).all()) and bool((bits == 0xA5).all())


# ------------------------------------------------------------------------------------------------ the measured ratios
def measure():
    worst = {}
    for name in NAMES:
        c = DR.case(name)
        res = DR.check_refresh(c, DR.reference(name), run_cabi(name))
        assert DR.n_failures(res) == 0, (name, res)
        worst[name] = dict(cell_vs_half_width=round(res["cells"][1], 4), mean_vs_bound=round(res["mean"][1], 4))
    return worst


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    worst = measure()
    out = dict(what="worst |cell - centre of its interval| / half-width and |mean - fp64 mean of the kernel's grid| / B_mean per seeded case of "
                    "tests/test_density_fp64_gpu.py, through the C ABI (an fp16 cell's interval is one or two adjacent fp16 values: its ratio is 0 or 1)",
               device=torch.cuda.get_device_name(0), worst_ratio=worst)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
