"""The device-resident scene cache on the MI355X: the two kernels of csrc/scene_cache.hip through the C ABI (store then load at odd sizes, slot
orders, alignments, with sentinels everywhere, against torch's ``_clamp_to(x, dtype).to(dtype)`` bit for bit; the exhaustive input set of the CPU
test through the store kernel), ``MultiSceneNeRF(cache_store='device')`` against the host cache where nothing is rendered (bit-equal leaves,
moments, grids, exports and files), and training steps on it."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import _cache_ref as R

pytestmark = pytest.mark.gpu

SENT = 0xA5
N_SLOTS = 40


# ---------------------------------------------------------------------------------------------- 1. the kernels through the C ABI
def _padded(nbytes, offset=0):
    """(whole, payload): a uint8 buffer full of sentinels and the ``nbytes`` of it that start ``offset`` bytes past a 16-byte boundary"""
    whole = torch.full((64 + nbytes + 64,), SENT, dtype=torch.uint8, device="cuda")
    start = 32 + (-whole.data_ptr()) % 16 + offset
    payload = whole[start:start + nbytes]
    assert payload.data_ptr() % 16 == offset % 16
    return whole, payload


def _only_sentinels_outside(whole, payload):
    rest = whole.clone()
    start = payload.data_ptr() - whole.data_ptr()
    rest[start:start + payload.numel()] = SENT
    return bool((rest == SENT).all())


def _values(S, numel, seed, payload_nans):
    """fp32 (S, numel): magnitudes from 1e-9 to 1e6 with the values the clamp and the rounding turn on sprinkled in"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, numel, generator=g) * 10.0 ** torch.randint(-9, 7, (S, numel), generator=g).float()
    special = torch.tensor([float("inf"), -float("inf"), float("nan"), 65520.0, -70000.0, 1e-10, -0.0, 2.0 ** -25, 2.0 ** -24, 3.4e38, 65519.9, 1e-40])
    flat = x.view(-1)
    where = torch.randperm(flat.numel(), generator=g)[:special.numel()]
    flat[where] = special[:where.numel()]
    if payload_nans and flat.numel() > 2:                    # NaNs with a payload and a signalling one: an fp32 store has to keep their bits
        flat.view(torch.int32)[where[:2]] = torch.tensor([0x7FC12345, -8388607], dtype=torch.int32)
    return x


def _same16(got, want, dtype):
    """16-bit patterns (int16 CPU tensors) equal, NaN compared by isnan"""
    R.assert_same_bits(got.reshape(-1).numpy().view(np.uint16), want.reshape(-1).numpy().view(np.uint16), dtype, str(dtype))


class _Case:
    """one store of N_SLOTS slots and one batch of S rows, every array inside its own sentinel padding"""

    def __init__(self, numel, grid_bytes, bits_bytes, S, half, offset, seed):
        from ssdnerf_amd import _cabi as C
        self.C, self.lib = C, C.lib()
        self.numel, self.gb, self.bb, self.S, self.half = numel, grid_bytes, bits_bytes, S, half
        self.esz = 2 if half else 4
        g = torch.Generator().manual_seed(seed)
        self.slots = torch.randperm(N_SLOTS, generator=g)[:S].tolist()          # non-monotonic
        self.rows = torch.randperm(S, generator=g).tolist()
        self.has_state = [int(k % 3 != 1) for k in range(S)]
        self.store = [_padded(N_SLOTS * w) for w in (numel * self.esz, numel * self.esz, numel * self.esz, grid_bytes, bits_bytes)]
        self.desc = C.CacheStore(*[p.data_ptr() for _, p in self.store], N_SLOTS, numel, grid_bytes, bits_bytes, 1 if half else 0, 2 if half else 0)
        self.widths = (numel * 4, numel * 4, numel * 4, grid_bytes, bits_bytes)
        self.offset = offset

    def batch(self):
        return [_padded(self.S * w, self.offset) for w in self.widths]

    def table(self, rows=None):
        tab = (self.C.CacheRow * self.S)()
        for e, slot, row, hs in zip(tab, self.slots, rows or self.rows, self.has_state):
            e.slot, e.row, e.has_state = slot, row, hs
        return tab

    def call(self, store, bufs, rows=None):
        fn = self.lib.ssdnerf_cache_store_multi if store else self.lib.ssdnerf_cache_load_multi
        self.C.check(fn(self.desc, self.table(rows), self.S, *[p.data_ptr() for _, p in bufs], self.C.stream()), "cache kernel")
        torch.cuda.synchronize()

    def store_rows(self, k, which):
        """the bytes of slot ``k`` in store array ``which`` (0 code, 1 exp_avg, 2 exp_avg_sq, 3 grid, 4 bits), on the CPU"""
        w = (self.numel * self.esz,) * 3 + (self.gb, self.bb)
        return self.store[which][1][k * w[which]:(k + 1) * w[which]].cpu()


def _check_store_then_load(numel, grid_bytes, bits_bytes, S, half, offset, seed):
    from ssdnerf_amd.scene_cache import _clamp_to
    c = _Case(numel, grid_bytes, bits_bytes, S, half, offset, seed)
    g = torch.Generator().manual_seed(seed + 1)
    src = [_values(S, numel, seed + 2 + j, payload_nans=not half) for j in range(3)]
    src += [torch.randint(0, 256, (S, grid_bytes), dtype=torch.uint8, generator=g), torch.randint(0, 256, (S, bits_bytes), dtype=torch.uint8, generator=g)]
    bufs = c.batch()
    for (_, payload), t in zip(bufs, src):
        payload.copy_(t.reshape(-1).view(torch.uint8).cuda())
    before = [payload.clone() for _, payload in bufs]
    c.call(True, bufs)
    # ---- the store: named slots hold the converted rows, everything else its sentinels, the batch is only read
    for (whole, payload), b in zip(bufs, before):
        assert torch.equal(payload, b) and _only_sentinels_outside(whole, payload)
    for whole, payload in c.store:
        assert _only_sentinels_outside(whole, payload)
    named = dict(zip(c.slots, zip(c.rows, c.has_state)))
    dts = (torch.float16, torch.bfloat16, torch.bfloat16) if half else (torch.float32,) * 3
    for k in range(N_SLOTS):
        for which in range(5):
            got = c.store_rows(k, which)
            written = k in named and (which in (0, 3, 4) or named[k][1])
            if not written:
                assert bool((got == SENT).all()), (k, which)
                continue
            row = named[k][0]
            if which >= 3:
                assert torch.equal(got, src[which][row])
            elif half:
                _same16(got.view(torch.int16), _clamp_to(src[which][row], dts[which]).to(dts[which]).view(torch.int16), dts[which])
            else:
                assert torch.equal(got.view(torch.int32), src[which][row].view(torch.int32))                 # a bit copy: Inf and NaN payloads kept
    # ---- a second store into a second, identical store: the same bytes
    c2 = _Case(numel, grid_bytes, bits_bytes, S, half, offset, seed)
    c2.call(True, bufs)
    for (_, a), (_, b) in zip(c.store, c2.store):
        assert torch.equal(a, b)
    # ---- the load, into other rows than the store came from
    stored = [payload.clone() for _, payload in c.store]
    rows2 = c.rows[1:] + c.rows[:1]
    out = c.batch()
    c.call(False, out, rows2)
    for (whole, payload), s in zip(c.store, stored):
        assert torch.equal(payload, s)
    for whole, payload in out:
        assert _only_sentinels_outside(whole, payload)
    for slot, row, hs in zip(c.slots, rows2, c.has_state):
        for which in range(5):
            w = c.widths[which]
            got = out[which][1][row * w:(row + 1) * w].cpu()
            if which in (1, 2) and not hs:
                assert bool((got == SENT).all()), (slot, row, which)
                continue
            kept = c.store_rows(slot, which)
            if which >= 3 or not half:
                assert torch.equal(got, kept)
                continue
            want = kept.view(dts[which]).float()
            nan = want.isnan()
            assert torch.equal(got.view(torch.float32).isnan(), nan)
            assert torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan])                    # the stored value, widened exactly
    out2 = c.batch()
    c.call(False, out2, rows2)
    for (_, a), (_, b) in zip(out, out2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("offset", [4, 0])
@pytest.mark.parametrize("S", [1, 3, 32])
@pytest.mark.parametrize("half", [False, True])
def test_store_then_load_through_the_c_abi(half, S, offset):
    """offset 4: batch buffers that are only 4-byte aligned (every access element by element); offset 0: 16-byte groups wherever a row allows"""
    seed = 0
    for numel in (1, 3, 7, 8, 9, 210, 2051):
        # every numel with every grid size; the bitfield sizes rotate through them (each of the three meets each numel at S = 1 + 3 + 32)
        for j, grid_bytes in enumerate((2, 1026, 8192)):
            bits_bytes = (1, 65, 512)[(j + S + numel) % 3]
            seed += 10
            _check_store_then_load(numel, grid_bytes, bits_bytes, S, half, offset, seed)


@pytest.mark.parametrize("half", [False, True])
def test_every_grid_and_bitfield_size_pair_and_rows_of_several_chunks(half):
    for grid_bytes in (2, 1026, 8192):
        for bits_bytes in (1, 65, 512):
            _check_store_then_load(9, grid_bytes, bits_bytes, 3, half, 4, 1000 + grid_bytes + bits_bytes)
    # more than one block per segment (csrc/scene_cache.hip: SC_ELEMS = 4096 elements, SC_BYTES = 16384 bytes), aligned and not
    _check_store_then_load(2 * 4096 + 5, 2 * 16384 + 16, 16384 + 1, 3, half, 0, 2000)
    _check_store_then_load(4096 + 8, 16384 + 2, 16384 + 16, 2, half, 4, 2001)


def test_the_exhaustive_input_set_through_the_store_kernel():
    """the input set of tests/test_scene_cache_cpu.py (every 16-bit pattern, every tie, its neighbours, the specials) once through the store kernel:
    the same expected bits as the gcc build of the header"""
    from ssdnerf_amd import _cabi as C
    lib = C.lib()
    for dtype, which in ((torch.float16, 0), (torch.bfloat16, 1)):
        x = R.inputs(dtype)
        want = R.expected(x, dtype)
        numel = x.size
        dev = torch.from_numpy(x.view(np.int32).copy()).cuda()
        for shift in (0, 1):                                  # 16-byte groups, and (one element in) the element-wise path
            src = torch.zeros(numel + 4, dtype=torch.int32, device="cuda")
            src[shift:shift + numel] = dev
            arrays = [torch.zeros(2 * numel, dtype=torch.int16, device="cuda") for _ in range(3)]
            grid, bits = torch.zeros(2, 2, dtype=torch.uint8, device="cuda"), torch.zeros(2, 1, dtype=torch.uint8, device="cuda")
            desc = C.CacheStore(*[a.data_ptr() for a in arrays], grid.data_ptr(), bits.data_ptr(), 2, numel, 2, 1, 1, 2)
            tab = (C.CacheRow * 1)()
            tab[0].slot, tab[0].row, tab[0].has_state = 0, 0, 1
            p = src.data_ptr() + 4 * shift
            assert p % 16 == 4 * shift and all(a.data_ptr() % 16 == 0 for a in arrays)
            C.check(lib.ssdnerf_cache_store_multi(desc, tab, 1, p, p, p, grid.data_ptr(), bits.data_ptr(), C.stream()), "cache_store_multi")
            torch.cuda.synchronize()
            got = arrays[which][:numel].cpu().numpy().view(np.uint16)
            R.assert_same_bits(got, want, dtype, f"store kernel, {dtype}, shift {shift}")
            assert not bool(arrays[which][numel:].any())      # slot 1 was not named


# ---------------------------------------------------------------------------------------------- 2. the model against the host cache
CODE_SIZE, GRID, CACHE = (3, 2, 5, 7), 16, 5


def _model(store, half, cache_size=CACHE, writers=0, **train_cfg):
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd.registry import MODELS
    torch.manual_seed(0)
    m = MODELS.build(dict(type="MultiSceneNeRF", code_size=CODE_SIZE, code_activation=dict(type="TanhCode", scale=2), grid_size=GRID,
                          decoder=dict(type="TriPlaneDecoder", base_layers=[6, 64], density_layers=[64, 1], color_layers=[64, 3], dir_layers=[16, 64]),
                          cache_size=cache_size, cache_16bit=half, cache_store=store, num_file_writers=writers,
                          train_cfg=dict(optimizer=dict(type="Adam", lr=0.01), **train_cfg)))
    return m.cuda()


def _hand_made(m, ids, seed, step=7.0, with_state=True):
    """(leaves, optimizers, grid, bits): a caller's own tensors -- no rows of anything"""
    g = torch.Generator().manual_seed(seed)
    leaves, n = [], len(ids)
    for k in range(n):
        x = torch.randn(CODE_SIZE, generator=g) * (1e5 if k == 1 else 1.0)          # (one scene beyond fp16's range: the clamp)
        # (Inf only where the store is 16-bit: the host path's FIRST save of a scene clamps an fp32 code to +-FLT_MAX -- out_dict_to clamps whatever
        #  the dtype -- while its later saves, and the device store always, copy fp32 bits as they are)
        x.view(-1)[:3] = torch.tensor([float("inf") if m.cache_16bit else 3e38, -1e-9, 65519.9])
        leaves.append(x.cuda().requires_grad_(True))
    opts = m.build_optimizer(leaves, m.train_cfg)
    if with_state:
        for leaf, opt in zip(leaves, opts):
            opt.state[leaf] = dict(step=torch.tensor(step), exp_avg=(torch.randn(CODE_SIZE, generator=g) * 1e-3).cuda(),
                                   exp_avg_sq=(torch.rand(CODE_SIZE, generator=g) * 1e-6).cuda())
    grid = torch.rand(n, GRID ** 3, generator=g).half().cuda()
    bits = torch.randint(0, 256, (n, GRID ** 3 // 8), dtype=torch.uint8, generator=g).cuda()
    return leaves, opts, grid, bits


def _same(a, b, path="entry"):
    """two cache entries / files equal: keys, types, and tensors by dtype, shape and bits"""
    assert type(a) is type(b), (path, type(a), type(b))
    if isinstance(a, dict):
        assert list(a) == list(b), (path, list(a), list(b))
        for k in a:
            _same(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{k}]")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, (path, a.dtype, b.dtype, a.shape, b.shape, a.device, b.device)
        raw = lambda t: t.contiguous().view(-1).view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)
        assert torch.equal(raw(a), raw(b)), path
    else:
        assert a == b, (path, a, b)


def _same_loaded(a, b):
    """two load_cache results equal bit for bit, optimizer states included"""
    (la, oa, ga, ba), (lb, ob, gb, bb) = a, b
    assert len(la) == len(lb)
    for x, y, p, q in zip(la, lb, oa, ob):
        assert x.requires_grad and y.requires_grad and x.is_leaf and y.is_leaf and x.shape == y.shape == CODE_SIZE
        assert torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32))
        sp, sq = p.state[x] if x in p.state else {}, q.state[y] if y in q.state else {}
        assert set(sp) == set(sq)
        for key in sp:
            assert sp[key].dtype == sq[key].dtype == torch.float32 and sp[key].device == sq[key].device, key
            assert torch.equal(sp[key].reshape(-1).view(torch.int32), sq[key].reshape(-1).view(torch.int32)), key
    assert ga.dtype == gb.dtype == torch.float16 and torch.equal(ga.view(torch.int16), gb.view(torch.int16))
    assert ba.dtype == bb.dtype == torch.uint8 and torch.equal(ba, bb)


@pytest.mark.parametrize("writers", [0, 2])
@pytest.mark.parametrize("half", [False, True])
def test_device_cache_equals_the_host_cache_where_nothing_is_rendered(tmp_path, half, writers):
    ids, names = [3, 0, 4, 1, 2], ["s3", "s0", "s4", "s1", "s2"]
    dirs = {store: str(tmp_path / store) for store in ("host", "device")}
    models = {store: _model(store, half, writers=writers, save_dir=dirs[store]) for store in ("host", "device")}
    loaded = {}
    for store, m in models.items():
        m.save_cache(*_hand_made(m, ids, seed=11), ids, names)
        if writers:
            m.file_writers.flush()
        loaded[store] = m.load_cache(dict(scene_id=ids, scene_name=names))
    mh, md = models["host"], models["device"]
    assert md.cache.launches == 2 and md.cache.host_copies == 5                  # one store, one load; the five files
    _same_loaded(loaded["host"], loaded["device"])
    step = loaded["device"][1][0].state[loaded["device"][0][0]]["step"]
    assert float(step) == 7.0 and step.device.type == "cpu" and step.dtype == torch.float32 and step.dim() == 0
    want_dtypes = (torch.float16, torch.bfloat16) if half else (torch.float32, torch.float32)
    for sid in ids:
        e = md.cache[sid]
        _same(mh.cache[sid], e, f"cache[{sid}]")
        assert (e["param"]["code_"].dtype, e["optimizer"]["state"][0]["exp_avg"].dtype) == want_dtypes
        e["param"]["code_"].zero_()                                               # an export is a copy: the cache does not see this
        assert bool(md.cache[sid]["param"]["code_"].abs().max() > 0)
    assert md.cache.host_copies == 5 + 2 * len(ids)
    assert sorted(os.listdir(dirs["device"])) == sorted(os.listdir(dirs["host"])) == sorted(n + ".pth" for n in names)
    for n in names:
        _same(torch.load(os.path.join(dirs["host"], n + ".pth"), map_location="cpu"), torch.load(os.path.join(dirs["device"], n + ".pth"), map_location="cpu"), n)
    # ---- the files seed a fresh device cache
    m2 = _model("device", half, cache_load_from=dirs["device"])
    again = m2.load_cache(dict(scene_id=ids, scene_name=names))
    assert m2.cache_loaded and m2.cache.host_copies == 5
    _same_loaded(loaded["device"], again)
    for sid in ids:
        _same(md.cache[sid], m2.cache[sid], f"reloaded cache[{sid}]")


def test_files_of_another_dtype_are_converted_by_the_store_rule_and_activated_codes_are_inverted(tmp_path):
    from ssdnerf_amd.scene_cache import _clamp_to
    ids, names = [0, 1, 2, 3, 4], ["a", "b", "c", "d", "e"]
    src = _model("host", False, save_dir=str(tmp_path / "fp32"))
    leaves, opts, grid, bits = _hand_made(src, ids, seed=21)
    src.save_cache(leaves, opts, grid, bits, ids, names)
    m = _model("device", True, cache_load_from=str(tmp_path / "fp32"))
    m.load_cache(dict(scene_id=[2], scene_name=["c"]))
    for k, sid in enumerate(ids):
        e = m.cache[sid]
        assert torch.equal(e["param"]["code_"].view(torch.int16), _clamp_to(leaves[k].detach().cpu(), torch.float16).half().view(torch.int16))
        want = _clamp_to(opts[k].state[leaves[k]]["exp_avg_sq"].cpu(), torch.bfloat16).bfloat16()
        assert torch.equal(e["optimizer"]["state"][0]["exp_avg_sq"].view(torch.int16), want.view(torch.int16))
        assert float(e["optimizer"]["state"][0]["step"]) == 7.0 and e["scene_name"] == names[k]
    # test-time files hold the activated code only
    os.makedirs(tmp_path / "eval")
    code = torch.tanh(0.5 * torch.randn(5, *CODE_SIZE, generator=torch.Generator().manual_seed(3))) * 2     # (|x| < 3: atanh is well conditioned)
    for k, n in enumerate(names):
        torch.save(dict(scene_name=n, param=dict(code=code[k], density_grid=grid[k].cpu(), density_bitfield=bits[k].cpu())), str(tmp_path / "eval" / (n + ".pth")))
    m3 = _model("device", False, cache_load_from=str(tmp_path / "eval"))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got, o3, g3, b3 = m3.load_cache(dict(scene_id=[4, 1], scene_name=["e", "b"]))
    assert any("on-the-fly inversion" in str(x.message) for x in w)
    assert torch.allclose(torch.tanh(got[0].detach().cpu()) * 2, code[4], atol=1e-5) and torch.equal(g3[1].cpu(), grid[1].cpu())
    assert len(o3[0].state) == 0 and m3.cache[4]["param"]["code_"].dtype == torch.float32 and "optimizer" not in m3.cache[4]


@pytest.mark.parametrize("half", [False, True])
def test_fresh_slots_draw_from_the_same_stream_and_mix_with_present_ones(half):
    mh, md = _model("host", half), _model("device", half)
    out = {}
    for m in (mh, md):
        torch.manual_seed(5)
        out[m] = m.load_cache(dict(scene_id=[2, 0], scene_name=["s2", "s0"]))
    _same_loaded(out[mh], out[md])
    assert float(out[md][0][0].detach().abs().max()) > 0 and md.cache.launches == 0          # nothing present: nothing to launch
    for m in (mh, md):
        m.save_cache(*_hand_made(m, [3, 1], seed=31), [3, 1], ["s3", "s1"])
        torch.manual_seed(6)
        out[m] = m.load_cache(dict(scene_id=[0, 3, 2, 1, 4], scene_name=["s0", "s3", "s2", "s1", "s4"]))
    _same_loaded(out[mh], out[md])
    assert md.cache.launches == 2                                                 # the store, and ONE load for the two present scenes
    leaves, opts = out[md][0], out[md][1]
    assert len(opts[0].state) == 0 and float(opts[1].state[leaves[1]]["step"]) == 7.0 and md.cache[0] is None and md.cache[3] is not None
    # scenes saved without optimizer state (nothing has stepped yet) come back without one
    for m in (mh, md):
        m.save_cache(*_hand_made(m, [4], seed=32, with_state=False), [4], ["s4"])
        out[m] = m.load_cache(dict(scene_id=[4, 1], scene_name=["s4", "s1"]))
    _same_loaded(out[mh], out[md])
    _same(mh.cache[4], md.cache[4])
    assert len(out[md][1][0].state) == 0 and len(out[md][1][1].state) == 1


def test_a_batch_of_33_scenes_takes_two_launches_each_way():
    md, mh = _model("device", True, cache_size=40), _model("host", True, cache_size=40)
    ids = [(7 * k) % 40 for k in range(33)]
    names = [f"s{sid}" for sid in ids]
    out = {}
    for m in (mh, md):
        count = md.cache.launches
        m.save_cache(*_hand_made(m, ids, seed=41), ids, names)
        if m is md:
            assert md.cache.launches == count + 2
        out[m] = m.load_cache(dict(scene_id=ids, scene_name=names))
        if m is md:
            assert md.cache.launches == count + 4
    _same_loaded(out[mh], out[md])
    # rows of the batch buffers go back without a gather, still in two launches
    leaves, opts, grid, bits = out[md]
    md.save_cache(leaves, opts, grid, bits, ids, names)
    assert md.cache.launches == count + 6
    _same(mh.cache[ids[32]], md.cache[ids[32]])


def test_the_last_occurrence_of_a_duplicated_scene_wins_and_other_optimizers_are_refused():
    mh, md = _model("host", False), _model("device", False)
    ids, names = [2, 4, 2], ["s2", "s4", "s2"]
    for m in (mh, md):
        leaves, opts, grid, bits = _hand_made(m, ids, seed=51)
        m.save_cache(leaves, opts, grid, bits, ids, names)
    assert md.cache.launches == 1
    assert torch.equal(md.cache[2]["param"]["code_"], leaves[2].detach().cpu()) and not torch.equal(leaves[0], leaves[2])
    assert torch.equal(md.cache[2]["param"]["density_grid"], grid[2].cpu())
    for sid in (2, 4):
        _same(mh.cache[sid], md.cache[sid])
    loaded = md.load_cache(dict(scene_id=ids, scene_name=names))                  # a slot may be read twice
    assert torch.equal(loaded[0][0].detach(), loaded[0][2].detach()) and torch.equal(loaded[0][2].detach(), leaves[2].detach())
    leaf = torch.zeros(CODE_SIZE, device="cuda", requires_grad=True)
    sgd = torch.optim.SGD([leaf], lr=0.1, momentum=0.9)
    leaf.grad = torch.ones_like(leaf)
    sgd.step()
    with pytest.raises(TypeError, match="Adam"):
        md.save_cache([leaf], [sgd], grid[:1], bits[:1], [1], ["s1"])
    assert md.cache[1] is None


# ---------------------------------------------------------------------------------------------- 3. training on the device cache
def _stage1_model(kind, **train_cfg):
    import test_tv_loss_gpu as TV
    from ssdnerf_amd import synthetic as S
    from ssdnerf_amd.registry import MODELS
    cfg = dict(dt_gamma_scale=0.5, density_thresh=0.1, extra_scene_step=3, n_inverse_rays=2 ** 12, n_decoder_rays=2 ** 12, loss_coef=0.1 / (64 * 64),
               optimizer=dict(type=kind, lr=1e-2, weight_decay=0.), **train_cfg)
    m = MODELS.build(dict(type="MultiSceneNeRF", code_size=(3, 6, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64,
                          decoder=TV.DEC, decoder_use_ema=True, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
                          reg_loss=dict(type="TVLoss", power=1.5, loss_weight=1.0), cache_size=4, cache_store="device", init_from_mean=True, train_cfg=cfg))
    m.decoder.load_state_dict(S.make_decoder_params(), strict=False)
    m.decoder_ema.load_state_dict(S.make_decoder_params(), strict=False)
    with torch.no_grad():
        m.init_code.copy_(S.make_triplane(80))
    return m.cuda().train()


@pytest.mark.parametrize("kind", ["HIPAdam", "Adam"])
def test_two_stage1_train_steps_on_the_device_cache(tmp_path, kind):
    import test_tv_loss_gpu as TV
    from ssdnerf_amd.models import _torch_factory
    m = _stage1_model(kind)
    imgs, poses, intr = TV._views([51, 52], [30, 150])
    data = dict(scene_id=[0, 2], scene_name=["s0", "s2"], cond_imgs=imgs, cond_poses=poses, cond_intrinsics=intr)
    cls, kw = _torch_factory(torch.optim, dict(type=kind, lr=1e-3))
    opt = dict(decoder=cls(m.decoder.parameters(), **kw))
    torch.manual_seed(1)
    cache = m.cache
    codes = []
    for k in (1, 2):
        copies, launches = cache.host_copies, cache.launches
        out = m.train_step(data, opt)
        assert cache.host_copies == copies                                        # no host round trip inside the step
        assert cache.launches == launches + (1 if k == 1 else 2)                  # (the first step finds nothing to load)
        assert bool(torch.isfinite(out["log_vars"]["loss"])) and out["num_samples"] == 2
        for sid in (0, 2):
            slot = cache.slot_of[sid]
            assert cache.present[slot] and cache.has_state[slot] and float(cache.step[slot]) == 4.0 * k
        codes.append(torch.stack([cache[sid]["param"]["code_"] for sid in (0, 2)]))
        assert cache[1] is None and cache[3] is None
    assert bool(torch.isfinite(codes[1]).all()) and float(codes[0].abs().max()) > 0 and not torch.equal(codes[0], codes[1])
    assert float(cache[2]["optimizer"]["state"][0]["step"]) == 8.0
    # with save_dir the step exports its batch: one host copy per scene
    m.train_cfg["save_dir"] = str(tmp_path / "cache")
    copies = cache.host_copies
    m.train_step(data, opt)
    assert cache.host_copies == copies + 2 and sorted(os.listdir(tmp_path / "cache")) == ["s0.pth", "s2.pth"]
    saved = torch.load(str(tmp_path / "cache" / "s2.pth"), map_location="cpu")
    _same(saved, cache[2], "s2.pth")
    assert float(saved["optimizer"]["state"][0]["step"]) == 12.0


@pytest.mark.parametrize("code_optimizer", [dict(type="SGD", lr=200.0), dict(type="Adam", lr=5e-3)])
def test_one_diffusion_nerf_train_step_on_the_device_cache(code_optimizer):
    """the model dict of test_diffusion_gpu.py::test_diffusion_nerf_train_step_matches_oracle (its SGD code optimizer, which keeps no state, and Adam)"""
    import ssdnerf_amd  # noqa: F401
    import test_diffusion_gpu as TD
    from ssdnerf_amd import synthetic as S
    from ssdnerf_amd.registry import MODELS
    hw = 64
    m = MODELS.build(dict(
        type="DiffusionNeRF", code_size=(3, 6, 128, 128), code_reshape=(18, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64,
        diffusion=dict(type="GaussianDiffusion", num_timesteps=1000, betas_cfg=dict(type="linear"),
                       denoising=dict(type="DenoisingUnetMod", image_size=128, in_channels=18, base_channels=32, channels_cfg=[1, 1, 2],
                                      resblocks_per_downsample=1, dropout=0.0, use_scale_shift_norm=True, num_heads=4, attention_res=[32],
                                      norm_cfg=dict(type="GN", num_groups=8)),
                       timestep_sampler=dict(type="SNRWeightedTimeStepSampler", power=0.5),
                       ddpm_loss=dict(type="DDPMMSELossMod", rescale_mode="timestep_weight", data_info=dict(pred="v_t_pred", target="v_t"),
                                      weight_scale=4.0, scale_norm=True)),
        decoder=dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3],
                     use_dir_enc=True, dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001, max_steps=256),
        decoder_use_ema=True, freeze_decoder=False, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
        reg_loss=dict(type="RegLoss", power=2, loss_weight=3e-3), cache_size=4, cache_store="device",
        train_cfg=dict(dt_gamma_scale=0.5, density_thresh=0.1, extra_scene_step=1, n_inverse_rays=hw * hw, n_decoder_rays=hw * hw,
                       loss_coef=0.1 / (hw * hw), optimizer=code_optimizer)))
    TD._randomize(m.diffusion.denoising, 9)
    m.decoder.load_state_dict(S.make_decoder_params(), strict=False)
    m = m.cuda().train()
    code0_ = m.code_activation.inverse(S.make_triplane(37)).contiguous()
    m.get_init_code_ = lambda num_scenes, device=None: code0_.clone().to(device).requires_grad_(True)
    target = torch.rand(hw * hw, 3, generator=torch.Generator().manual_seed(41))
    data = dict(scene_id=[1], scene_name=["a"], cond_imgs=target.reshape(1, 1, hw, hw, 3).cuda(), cond_poses=S.spiral_poses()[[64]].cuda()[None],
                cond_intrinsics=S.cars_intrinsics(hw, hw).cuda()[None, None])
    opt = dict(diffusion=torch.optim.SGD(m.diffusion.parameters(), lr=1e-3), decoder=torch.optim.SGD(m.decoder.parameters(), lr=0.05))
    np.random.seed(13); torch.manual_seed(13)
    out = m.train_step(data, opt)
    cache = m.cache
    assert out["num_samples"] == 1 and cache.host_copies == 0 and cache.launches == 1
    e = cache[1]
    assert bool(torch.isfinite(e["param"]["code_"]).all()) and not torch.equal(e["param"]["code_"], code0_) and cache[0] is None
    assert bool(e["param"]["density_bitfield"].any())
    if code_optimizer["type"] == "Adam":
        assert float(e["optimizer"]["state"][0]["step"]) == 2.0 and e["optimizer"]["state"][0]["exp_avg"].dtype == torch.float32
    else:
        assert e["optimizer"]["state"] == {} and e["optimizer"]["param_groups"][0]["lr"] == 200.0
