"""Training ray batches whose pixel numbers are made on the device (csrc/keyed_perm.h; ``ssdnerf_perm_indices`` / ``ssdnerf_sample_rays_perm_u8``,
csrc/scene_store.hip; ``StoredViews.sample_permuted``; ``fitting.RayBatcher(index_source='device')``; ``cfg['ray_index_source']``).
The permutation's reference is the numpy restatement of the header's comment (tests/_perm_ref.py), bit for bit; the fused sampler's reference is the
existing ``ssdnerf_sample_rays_u8`` fed the indices, under ``torch.equal``.  The cases are those of tests/test_ray_sample_gpu.py (its synthetic stores
and its smallest stage-1 model), built by that module's helpers.  Every test fails without the feature: the symbols and the options are missing."""
import numpy as np
import pytest
import torch

import _perm_ref as KP
import test_ray_sample_gpu as RS
from ssdnerf_amd import _cabi as C
from ssdnerf_amd.fitting import RayBatcher

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -7.25
WALK = (3, 2, 6, 8)                                                      # S, V, h, w: P = 96 in a domain of 256 -- the walk is exercised
EXACT = (2, 1, 4, 4)                                                     # P = 16 = its own domain: no walk
SEED = 0xC0FFEE1234567


def _spans(P, R):
    return [(start, min(R, P - start)) for start in range(0, P, R)]


def _indices(S, P, start, R, seed, draw, status=False):
    out = torch.full((S * R + 2,), -5, dtype=torch.int64, device="cuda")                                  # one guard element either side
    st = C.lib().ssdnerf_perm_indices(C.ptr(out[1:]), S, P, start, R, seed, draw, C.stream())
    if status:
        return st, out
    C.check(st, "perm_indices")
    assert int(out[0]) == -5 and int(out[-1]) == -5, "written outside out"
    return out[1:-1].view(S, R)


def _fused(case, seed, draw, start, R, outs):
    return C.lib().ssdnerf_sample_rays_perm_u8(C.ptr(case["store"]), case["N"], case["h"], case["w"], C.ptr(case["table"]), C.ptr(case["c2w"]),
                                               C.ptr(case["intr"]), case["S"], case["V"], seed, draw, start, R, *outs, C.stream())


# ------------------------------------------------------------------------------------------------ the permutation
@pytest.mark.parametrize("S,P,R", [(3, 96, 20), (2, 16, 5), (2, 16, 16), (2, 1, 1), (1, 4097, 300)])
def test_perm_indices_equal_the_restatement_bit_for_bit(S, P, R):
    for seed, draw in ((SEED, 0), (2 ** 64 - 1, 3)):
        whole = []
        for start, count in _spans(P, R):
            got = _indices(S, P, start, count, seed, draw).cpu().numpy()
            assert np.array_equal(got, KP.perm_indices(seed, S, draw, P, start, count)), (start, count, seed, draw)
            whole.append(got)
        assert np.array_equal(np.sort(np.concatenate(whole, axis=1), axis=1), np.tile(np.arange(P), (S, 1)))


def test_perm_indices_of_a_training_scene_are_a_permutation():
    S, P = 2, 819200                                                      # 50 views of 128 x 128: 3200 blocks per scene
    got = _indices(S, P, 0, P, SEED, 0)
    assert torch.equal(got.sort(dim=1).values, torch.arange(P, device="cuda").expand(S, P))
    assert not torch.equal(got[0], got[1])
    for start in (0, P - 4096):
        assert np.array_equal(got[:, start:start + 4096].cpu().numpy(), KP.perm_indices(SEED, S, 0, P, start, 4096))


# ------------------------------------------------------------------------------------------------ the fused sampler
@pytest.mark.parametrize("shape,R", [(WALK, 20), (EXACT, 5), (EXACT, 16), ((2, 2, 128, 128), 4096 + 37)])
def test_fused_sampler_equals_sample_rays_u8_fed_the_indices(shape, R):
    case = RS._case(*shape)
    S, P = case["S"], case["P"]
    inputs = [case["big"], case["table"], case["c2w"], case["intr"]]
    before = [t.clone() for t in inputs]
    spans = _spans(P, R)
    for draw, (start, count) in [(0, s) for s in (spans if P < 1000 else [spans[0], spans[-1]])] + [(2, spans[0])]:
        inds = _indices(S, P, start, count, SEED, draw)
        want = [torch.empty((S, count, 3), device="cuda") for _ in range(3)]
        C.check(RS._call(case, inds, count, [C.ptr(t) for t in want]), "sample_rays_u8")
        padded = [torch.full((2 * GUARD + S * count * 3,), SENTINEL, device="cuda") for _ in range(3)]
        C.check(_fused(case, SEED, draw, start, count, [C.ptr(p[GUARD:]) for p in padded]), "sample_rays_perm_u8")
        torch.cuda.synchronize()
        for name, p, e in zip(("rays_o", "rays_d", "target"), padded, want):
            assert bool((p[:GUARD] == SENTINEL).all()) and bool((p[GUARD + S * count * 3:] == SENTINEL).all()), ("written outside", name)
            assert torch.equal(p[GUARD:GUARD + S * count * 3].view(S, count, 3), e), (name, draw, start, count)
            assert not bool(torch.isnan(e).any())
    for t, b in zip(inputs, before):
        assert torch.equal(t, b), "an input was written"


def test_sample_permuted_is_the_fused_launch():
    case = RS._case(*WALK)
    views, _ = RS._handle(case)
    got = views.sample_permuted(SEED, 1, 80, 16)
    want = views.sample(_indices(case["S"], case["P"], 80, 16, SEED, 1))
    assert all(tuple(g.shape) == (3, 16, 3) and torch.equal(g, e) for g, e in zip(got, want))
    assert (views.sample_launches, views.dense_calls) == (2, 0)
    for bad in (dict(start=90, count=7), dict(start=0, count=0), dict(start=-1, count=4), dict(seed=2 ** 64), dict(draw=2 ** 32)):
        with pytest.raises(ValueError):
            views.sample_permuted(**dict(dict(seed=SEED, draw=0, start=0, count=4), **bad))


# ------------------------------------------------------------------------------------------------ RayBatcher
def _pixel_ids(case):
    """(S, P) int64: a number per pixel recovered from a batch's bits -- the position of each (ray, colour) row in the dense arrays"""
    return torch.cat(case["dense"], dim=2)                                                                # (S, P, 9)


def _visited(case, batch):
    """the pixel numbers of a batch, found by matching its nine floats against the dense arrays (rays of different pixels differ in direction)"""
    rows = torch.cat(batch, dim=2)                                                                        # (S, R, 9)
    table = _pixel_ids(case)
    match = (rows[:, :, None, :6] == table[:, None, :, :6]).all(dim=3)                                    # (S, R, P)
    assert bool((match.sum(dim=2) == 1).all())
    found = match.int().argmax(dim=2)
    assert torch.equal(torch.gather(table, 1, found[:, :, None].expand(-1, -1, 9)), rows)
    return found


@pytest.mark.parametrize("shape,R", [(WALK, 20), (EXACT, 5)])
def test_fixed_batcher_visits_every_pixel_once_per_epoch_and_cycles(shape, R):
    case = RS._case(*shape)
    dense, stored, views = RS._conditionings(case)
    S, P = case["S"], case["P"]
    a, b = RayBatcher(dense, R, fixed=True, index_source="device", seed=SEED), RayBatcher(stored, R, fixed=True, index_source="device", seed=SEED)
    n = len(_spans(P, R))
    assert a.n_chunks == b.n_chunks == n and a.chunks is None and b.chunks is None
    seen = []
    for k, (start, count) in enumerate(_spans(P, R)):
        from_dense, from_store = a.batch(k), b.batch(k)
        assert all(tuple(t.shape) == (S, count, 3) for t in from_store)
        assert RS._triples_equal(from_dense, from_store), k                                               # the same pixels from either conditioning
        assert RS._triples_equal(b.batch(k + n), from_store) and RS._triples_equal(a.batch(k + 2 * n), from_store), k
        found = _visited(case, from_store)
        assert np.array_equal(found.cpu().numpy(), KP.perm_indices(SEED, S, 0, P, start, count)) and torch.equal(found, b.indices(k))
        seen.append(found)
    assert torch.equal(torch.cat(seen, dim=1).sort(dim=1).values, torch.arange(P, device="cuda").expand(S, P))
    assert views.dense_calls == 0 and views.sample_launches == 2 * n
    other = RayBatcher(stored, R, fixed=True, index_source="device", seed=SEED + 1)
    assert not RS._triples_equal(other.batch(0), b.batch(0))


def test_fresh_takes_have_no_duplicates_differ_and_reproduce():
    case = RS._case(*WALK)
    dense, stored, views = RS._conditionings(case)
    S, P, R = case["S"], case["P"], 20
    torch.manual_seed(11)
    a, b = RayBatcher(stored, R, fixed=False, index_source="device"), RayBatcher(dense, R, fixed=False, index_source="device", seed=SEED)
    torch.manual_seed(11)
    again = RayBatcher(stored, R, fixed=False, index_source="device")
    assert again.seed == a.seed and 0 <= a.seed < 2 ** 64 and b.seed == SEED
    takes = [a.take(None) for _ in range(3)]
    for n, take in enumerate(takes):
        found = _visited(case, take)
        assert np.array_equal(found.cpu().numpy(), KP.perm_indices(a.seed, S, n, P, 0, R))                  # take n: the head of draw n
        assert all(len(set(row)) == R for row in found.cpu().tolist())
        assert RS._triples_equal(again.batch(n), take)                                                    # the same seed: the same takes
    assert not RS._triples_equal(takes[0], takes[1]) and not RS._triples_equal(takes[1], takes[2])
    stored_b = RayBatcher(stored, R, fixed=False, index_source="device", seed=SEED)
    assert RS._triples_equal(b.take(None), stored_b.take(None)) and RS._triples_equal(b.take(None), stored_b.take(None))
    assert views.dense_calls == 0


def test_small_views_are_returned_whole_and_in_order():
    case = RS._case(*EXACT)
    dense, stored, views = RS._conditionings(case)
    for R in (16, 4096):
        for fixed in (True, False):
            a, b = RayBatcher(dense, R, fixed=fixed, index_source="device", seed=1), RayBatcher(stored, R, fixed=fixed, index_source="device", seed=1)
            assert b.indices(0) is None
            assert RS._triples_equal(a.batch(2), a.flat) and RS._triples_equal(b.batch(2), a.flat) and RS._triples_equal(b.take(None), a.flat)


# ------------------------------------------------------------------------------------------------ end to end
# the loader batch of tests/golden/srn_tiny has 4 conditioning views of 8 x 8 per scene: 256 pixels.  96 rays per step leave something to draw
# (chunks of 96, 96 and 64); the 256 of test_ray_sample_gpu.py would take every pixel in order and draw nothing in either mode
TRAIN_CFG = dict(RS.TRAIN_CFG, n_inverse_rays=96, n_decoder_rays=96)
TEST_CFG = dict(RS.TEST_CFG, n_inverse_rays=96)


class _Counts:
    def __init__(self, monkeypatch):
        self.n = dict(randperm=0, ssdnerf_perm_indices=0, ssdnerf_sample_rays_perm_u8=0, ssdnerf_sample_rays_u8=0)
        lib = C.lib()
        for name in list(self.n)[1:]:
            monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)))
        monkeypatch.setattr(torch, "randperm", self._wrap("randperm", torch.randperm))

    def _wrap(self, name, fn):
        def counted(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return counted


def _train_once(batch, train_cfg):
    import test_tv_loss_gpu as TV
    torch.manual_seed(0)
    m = TV._stage1_model(train_cfg=train_cfg, test_cfg=dict(TEST_CFG)).train()
    opt = dict(decoder=torch.optim.Adam(m.decoder.parameters(), lr=1e-3))
    init = m.get_init_code_(len(batch["scene_id"]), device="cuda").detach().clone()
    torch.manual_seed(1)
    out = m.train_step(batch, opt)
    torch.cuda.synchronize()
    codes = torch.stack([m.cache[i]["param"]["code_"].float() for i in batch["scene_id"]])
    return codes - init.to(codes.device), codes, {k: torch.as_tensor(v).detach().float().cpu() for k, v in out["log_vars"].items()}


def test_stage1_train_step_draws_its_rays_on_the_device(monkeypatch):
    monkeypatch.chdir(RS.GOLDEN)
    dense, stored = RS._batches()
    views = stored["cond_imgs"]
    assert views.shape[1:4].numel() > TRAIN_CFG["n_inverse_rays"]
    steps = TRAIN_CFG["extra_scene_step"] + 1
    counts = _Counts(monkeypatch)
    moved, codes, logs = _train_once(stored, dict(TRAIN_CFG, ray_index_source="device"))
    assert counts.n == dict(randperm=0, ssdnerf_perm_indices=0, ssdnerf_sample_rays_perm_u8=steps, ssdnerf_sample_rays_u8=0), counts.n
    assert views.dense_calls == 0 and views.sample_launches == steps
    assert all(bool(torch.isfinite(v).all()) for v in logs.values()), logs
    # the codes moved: three Adam steps of lr 1e-2, far above the rounding of a cache that may hold them as fp16 (2^-11 relative)
    assert bool(torch.isfinite(codes).all()) and float(moved.abs().max()) > 5e-3, float(moved.abs().max())
    # a dense batch in device mode: the indices come from ssdnerf_perm_indices, still no randperm
    counts.n = dict.fromkeys(counts.n, 0)
    _, codes_dense, logs_dense = _train_once(dense, dict(TRAIN_CFG, ray_index_source="device"))
    assert counts.n == dict(randperm=0, ssdnerf_perm_indices=steps, ssdnerf_sample_rays_perm_u8=0, ssdnerf_sample_rays_u8=0), counts.n
    assert all(bool(torch.isfinite(v).all()) for v in logs_dense.values())
    # the default configuration: the host draw, neither new entry point
    counts.n = dict.fromkeys(counts.n, 0)
    _train_once(RS._batches()[1], dict(TRAIN_CFG))
    assert counts.n["randperm"] > 0 and counts.n["ssdnerf_sample_rays_u8"] == steps, counts.n
    assert counts.n["ssdnerf_perm_indices"] == 0 and counts.n["ssdnerf_sample_rays_perm_u8"] == 0, counts.n
    with pytest.raises(ValueError, match="ray_index_source"):
        _train_once(stored, dict(TRAIN_CFG, ray_index_source="gpu"))


def test_inversion_and_guidance_read_the_key_from_the_test_cfg(monkeypatch):
    import test_tv_loss_gpu as TV
    from ssdnerf_amd.fitting import Conditioning, GuidanceObjective
    monkeypatch.chdir(RS.GOLDEN)
    _, stored = RS._batches()
    views = stored["cond_imgs"]
    cfg = dict(TEST_CFG, ray_index_source="device")
    m = TV._stage1_model(train_cfg=dict(TRAIN_CFG), test_cfg=cfg).eval()
    counts = _Counts(monkeypatch)
    torch.manual_seed(2)
    lv = m.val_step(stored)["log_vars"]
    assert np.isfinite(lv["test_psnr"]) and np.isfinite(lv["train_psnr"]), lv
    assert counts.n["randperm"] == 0 and counts.n["ssdnerf_sample_rays_perm_u8"] == cfg["n_inverse_steps"] == views.sample_launches, counts.n
    objective = GuidanceObjective(m, m.decoder, Conditioning.from_batch(stored, 0.5), cfg)
    assert objective.batcher.index_source == "device" and counts.n["randperm"] == 0
    assert GuidanceObjective(m, m.decoder, Conditioning.from_batch(stored, 0.5), dict(TEST_CFG)).batcher.index_source == "host"
    assert counts.n["randperm"] == 2


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_invalid_and_launch_nothing():
    case = RS._case(*WALK)
    S, P, R = case["S"], case["P"], 8
    null = C.ctypes.c_void_p(0)
    lib = C.lib()
    out = torch.full((S * R + 1,), -5, dtype=torch.int64, device="cuda")

    def refuse_indices(match, ptr=None, S=S, P=P, start=0, R=R):
        with pytest.raises(RuntimeError, match=match):
            C.check(lib.ssdnerf_perm_indices(C.ptr(out) if ptr is None else ptr, S, P, start, R, SEED, 0, C.stream()), "perm_indices")

    refuse_indices("null pointer", ptr=null)
    refuse_indices("must be positive", S=0)
    refuse_indices("must be positive", R=0)
    refuse_indices("must be positive", P=0)
    refuse_indices("below 2\\^32", P=2 ** 32)
    refuse_indices("leave", start=P - R + 1)
    refuse_indices("leave", start=P + 1)
    refuse_indices("leave", start=2 ** 64 - 4)                                                            # start + R wraps in 64 bits
    refuse_indices("8-byte aligned", ptr=C.ctypes.c_void_p(out.data_ptr() + 4))
    outs = [torch.full((S * R * 3 + 1,), SENTINEL, device="cuda") for _ in range(3)]

    def refuse_fused(match, case=case, start=0, R=R, at=None, value=None):
        ptrs = [C.ptr(o) for o in outs]
        if at is not None:
            ptrs[at] = value
        with pytest.raises(RuntimeError, match=match):
            C.check(_fused(case, SEED, 0, start, R, ptrs), "sample_rays_perm_u8")

    for at in range(3):
        refuse_fused("null output", at=at, value=null)
    for key in ("store", "table", "c2w", "intr"):
        refuse_fused("null input", case=dict(case, **{key: None}))
    refuse_fused("must be positive", case=dict(case, S=0))
    refuse_fused("must be positive", R=0)
    refuse_fused("no pixels", case=dict(case, V=0))
    refuse_fused("no pixels", case=dict(case, h=0))
    refuse_fused("2\\^32 pixels", case=dict(case, h=2 ** 16, w=2 ** 15))                                  # V h w = 2^32
    refuse_fused("leave", start=P - R + 1)
    refuse_fused("4-byte aligned", at=2, value=C.ctypes.c_void_p(outs[2].data_ptr() + 2))
    torch.cuda.synchronize()
    assert bool((out == -5).all()) and all(bool((o == SENTINEL).all()) for o in outs)
    C.check(lib.ssdnerf_perm_indices(C.ptr(out), S, P, P - R, R, SEED, 0, C.stream()), "perm_indices")       # the last admissible start is fine
    C.check(_fused(case, SEED, 0, P - R, R, [C.ptr(o) for o in outs]), "sample_rays_perm_u8")
    torch.cuda.synchronize()
    assert bool((out[:-1] >= 0).all()) and int(out[-1]) == -5
    assert bool((outs[0][:-1] != SENTINEL).all()) and float(outs[0][-1]) == SENTINEL
