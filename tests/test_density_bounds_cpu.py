"""The checks of tests/_density_ref.py have teeth (no GPU): the numpy float32 emulations of the density-grid refresh -- the straightforward form of the
cell position with the atomics in block order, and the fma-contracted form with the atomics in the opposite order -- meet every check on every seeded
case, with and without jitter; each subtly wrong variant (``MUTANTS``) fails at least one check on the case named next to it; and the cases are what
they claim, so that tests/test_density_fp64_gpu.py cannot pass by exercising nothing.  The conditions on the cases are met by the reference and the
emulation alone."""
import numpy as np
import pytest

import _density_ref as DR

NAMES = tuple(DR.CASES)


@pytest.mark.parametrize("contract", [False, True], ids=["plain", "contracted"])
@pytest.mark.parametrize("name", NAMES)
def test_faithful_emulations_meet_every_check(name, contract):
    c, ref = DR.case(name), DR.reference(name)
    res = DR.check_refresh(c, ref, DR.emulate(name, contract))
    print(name, contract, {k: round(v[1], 4) for k, v in res.items()})
    assert DR.n_failures(res) == 0, res


@pytest.mark.parametrize("name", ["h8-object", "h16-object-128", "h16-nan"])
def test_the_jitter_free_form_and_the_form_without_a_mean_meet_the_checks(name):
    c = DR.case(name)
    for contract in (False, True):
        res = DR.check_refresh(c, DR.reference(name, use_jitter=False), DR.emulate(name, contract, use_jitter=False))
        assert DR.n_failures(res) == 0, res
    res = DR.check_refresh(c, DR.reference(name), DR.emulate(name, want_mean=False))
    assert set(res) == {"cells", "untouched"} and DR.n_failures(res) == 0, res


@pytest.mark.parametrize("mut", list(DR.MUTANTS))
def test_each_mutant_fails_a_check(mut):
    name = DR.MUTANTS[mut]
    c, ref = DR.case(name), DR.reference(name)
    res = DR.check_refresh(c, ref, DR.emulate(name, mut=mut))
    print(mut, name, res)
    assert DR.n_failures(res) >= 1, res
    assert DR.n_failures(DR.check_refresh(c, ref, DR.emulate(name))) == 0          # (and not because the case fails anyway)


def test_a_chain_of_refreshes_on_their_own_outputs_meets_the_checks():
    """the chain ``get_density`` runs: each step's own jitter, decay 1.0, the emulation's previous output as the exact old grid"""
    old = None
    for i in range(3):
        name = f"h16-object-neg-fp16@{i}"
        out = DR.emulate(name, contract=bool(i & 1), old=old)
        res = DR.check_refresh(DR.case(name), DR.reference(name, old=old), out)
        assert DR.n_failures(res) == 0, (i, res)
        assert i == 0 or int((out.grid != old).sum()) >= 100
        old = out.grid


# ------------------------------------------------------------------------------------------------ the cases are what they claim
def test_the_guard_holds_and_the_case_table_covers_what_it_names():
    for name in NAMES:
        DR.reference(name)                                                   # ``decode_terms`` asserts GUARD on every pre-activation bound
    v = list(DR.CASES.values())
    assert {x[0] for x in v} == {8, 16, 32} and {(x[0], x[1]) for x in v} >= {(32, 3), (32, 2)}
    assert {(x[3], x[4]) for x in v} == {(False, False), (False, True), (True, False), (True, True)}
    assert {x[5] for x in v} == {1.0, 0.9, 0.5} and {x[6] for x in v} == {"zeros", "prev", "neg"} and {x[7] for x in v} == set(DR.FAMILIES)
    assert (128, 128) in {x[2] for x in v} and any(x[2][0] != x[2][1] and max(x[2]) <= 20 for x in v)
    assert 8 ** 3 % DR.BLOCK != 0 and 16 ** 3 == 2 * DR.BLOCK               # one partly filled block; two full ones
    assert set(DR.MUTANTS.values()) <= set(NAMES)


def test_both_sides_of_the_threshold_occur_and_the_bit_shares_are_not_trivial():
    sides = set()
    for name in NAMES:
        c, out = DR.case(name), DR.emulate(name)
        mean, B = DR.mean_ref(c, out.grid)
        t = float(np.float32(c.thresh))
        assert not (mean - B <= t <= mean + B), (name, "the mean is within its bound of density_thresh")
        sides.add(mean < t)
        assert (mean < t) == (c.family in ("sparse", "empty")), (name, mean)
        share = float(np.unpackbits(out.bits).mean())
        if c.family == "empty":
            assert share == 0.0 and mean == 0.0 and float(out.thr) == 0.0 and not out.grid.any()
        else:
            assert 0.01 <= share <= 0.99, (name, share)
    assert sides == {False, True}


def test_the_old_grids_meet_both_branches_of_the_max():
    for name in NAMES:
        c, ref = DR.case(name), DR.reference(name)
        if c.old_kind == "zeros":
            assert not c.old.any()
            continue
        n = int(ref.valid.sum())
        decayed, fresh = int((ref.valid & (ref.dec > ref.fresh_hi)).sum()), int((ref.valid & (ref.fresh_lo > ref.dec)).sum())
        print(name, n, decayed / n, fresh / n)
        assert decayed >= 0.05 * n and fresh >= 0.05 * n, (name, n, decayed, fresh)
        if c.old_kind == "neg":
            assert 0.1 * c.old.size <= int((c.old == -1).sum()) <= 0.3 * c.old.size


def test_the_saturating_cases_saturate_and_the_nan_case_splits():
    g = DR.emulate("h16-sat-fp16").grid
    assert g.dtype == np.float16 and int((g == 65504).sum()) >= 10 and np.isfinite(g).all()
    g = DR.emulate("h16-overflow").grid
    assert g.dtype == np.float32 and int((g == np.finfo(np.float32).max).sum()) >= 10 and np.isfinite(g).all()
    assert DR.mean_ref(DR.case("h16-overflow"), g) == (float("inf"), 0.0) and np.isinf(DR.emulate("h16-overflow").mean)
    g = DR.emulate("h16-sat-fp32").grid
    assert g.dtype == np.float32 and float(g.max()) > 65504
    c, ref = DR.case("h16-nan"), DR.reference("h16-nan")
    assert int(np.isnan(c.code).sum()) == 1
    out = DR.emulate("h16-nan")
    changed = DR._bits_of(out.grid) != DR._bits_of(c.old)
    assert int(ref.nan.sum()) >= 10 and not (ref.nan & changed).any() and int((~ref.nan & changed).sum()) >= 100
    assert int((ref.nan & (c.old >= 0)).sum()) >= 10                         # (the NaN alone keeps these cells, not a negative old value)


@pytest.mark.parametrize("cells", [12 ** 3, 10 ** 3, 3 ** 3, 100, 1])
def test_update_density_grid_refuses_a_grid_that_is_no_power_of_two_cube(cells):
    """a cell is written at its Morton index, which is below H^3 only for a power of two (H = 12: up to 3647 of 1728): the entry point raises before
    it looks at the decoder, allocates or launches -- so this runs without a GPU"""
    import torch
    from ssdnerf_amd.density import update_density_grid
    grid, bits = torch.full((1, cells), 7.0), torch.full((1, max(cells // 8, 1)), 0xA5, dtype=torch.uint8)
    with pytest.raises(ValueError, match="power of two"):
        update_density_grid(None, None, grid, bits)
    assert bool((grid == 7.0).all()) and bool((bits == 0xA5).all())
