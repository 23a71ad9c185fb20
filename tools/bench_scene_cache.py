"""The per-scene training cache on the host and on the device (``MultiSceneNeRF(cache_store='host' | 'device')``, ssdnerf_amd/scene_cache.py
``DeviceSceneCache``, csrc/scene_cache.hip), on the GPU.  The shape of the cars configs: 8 scenes per step out of a 64-slot
cache, codes of 3 x 6 x 128^2, grid 64^3, in fp32 and under ``cache_16bit``.

  (a) load_save       ``load_cache`` + ``save_cache`` of one batch, nothing in between, every slot filled and carrying Adam state; each step takes the
                      next 8 of the 64 scenes.  host: the dict of CPU tensors (pageable copies each way); device: one launch each way
  (b) kernel_alone    the two launches straight through the C ABI on prepared buffers, with the bytes they move and that traffic's share of
                      8 TB/s (the traffic is derived from the sizes, not measured)
  (c) train_step      ms per stage-1 ``MultiSceneNeRF.train_step`` (``extra_scene_step=15``, 2^12 rays, ``HIPAdam``; the model dict of
                      tools/bench_ray_sampler.py) in both modes, and ``torch.cuda.max_memory_allocated`` over one such step each

every path warmed up, windows alternated between the modes in one process, per call by HIP events and by the host clock over the same
synchronised window, median (min - max).  The host mode is the code as it was before the device cache existed.

Writes one JSON line to ``--out`` and prints it.   usage: python tools/bench_scene_cache.py [--windows 5] [--steps 8] [--train-steps 3] [--out profiles/scene_cache.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_ray_sampler as B  # noqa: E402  (the stage-1 model dict, the cameras and the window helpers)

S, SLOTS, CODE, GRID, V = 8, 64, (3, 6, 128, 128), 64, 8
PEAK_TBPS = 8.0


def _model(store, half, cache_size=SLOTS):
    from ssdnerf_amd import synthetic as SY
    from ssdnerf_amd.registry import MODELS
    torch.manual_seed(0)
    m = MODELS.build(dict(type="MultiSceneNeRF", code_size=CODE, code_activation=dict(type="TanhCode", scale=2), grid_size=GRID, decoder=B.DEC,
                          decoder_use_ema=True, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
                          reg_loss=dict(type="TVLoss", power=1.5, loss_weight=1.0), cache_size=cache_size, cache_16bit=half, cache_store=store,
                          init_from_mean=True, train_cfg=dict(B.TRAIN_CFG)))
    m.decoder.load_state_dict(SY.make_decoder_params(), strict=False)
    m.decoder_ema.load_state_dict(SY.make_decoder_params(), strict=False)
    with torch.no_grad():
        m.init_code.copy_(SY.make_triplane(80))
    return m.cuda().train()


def _fill(m):
    """every slot filled, with Adam state at step 7"""
    g = torch.Generator().manual_seed(1)
    for start in range(0, SLOTS, S):
        ids = list(range(start, start + S))
        leaves, opts, grid, bits = m.load_cache(dict(scene_id=ids, scene_name=[f"s{i}" for i in ids]))
        for leaf, opt in zip(leaves, opts):
            opt.state[leaf] = dict(step=torch.tensor(7.0), exp_avg=(torch.randn(CODE, generator=g) * 1e-3).cuda(),
                                   exp_avg_sq=(torch.rand(CODE, generator=g) * 1e-6).cuda())
        m.save_cache(leaves, opts, grid, bits, ids, [f"s{i}" for i in ids])


def _load_save(args):
    res = {}
    for half in (False, True):
        models = {store: _model(store, half) for store in ("host", "device")}
        turn = {store: 0 for store in models}
        for m in models.values():
            _fill(m)

        def step(store):
            m = models[store]
            ids = [(turn[store] * S + j) % SLOTS for j in range(S)]
            turn[store] += 1
            names = [f"s{i}" for i in ids]
            leaves, opts, grid, bits = m.load_cache(dict(scene_id=ids, scene_name=names))
            m.save_cache(leaves, opts, grid, bits, ids, names)

        got = B._alternate({store: (lambda store=store: step(store)) for store in models}, args.steps, args.windows, warmup=8)
        cache = models["device"].cache
        got["device"].update(launches_per_step=2, host_copies=cache.host_copies)
        res["cache_16bit" if half else "fp32"] = got
        res["kernel_alone_" + ("16bit" if half else "fp32")] = _kernels(models["device"], args)
        del models
        torch.cuda.empty_cache()
    return res


def _kernels(m, args):
    """(b) on the filled cache of ``m``: the launches alone"""
    from ssdnerf_amd import _cabi as C
    cache, lib = m.cache, C.lib()
    bufs = cache.batch_buffers(S)
    tab = (C.CacheRow * S)()
    for k, e in enumerate(tab):
        e.slot, e.row, e.has_state = (5 * k + 3) % SLOTS, k, 1
    call = (cache._desc, tab, S, *[C.ptr(b) for b in bufs], C.stream())
    C.check(lib.ssdnerf_cache_load_multi(*call), "cache_load_multi")
    C.check(lib.ssdnerf_cache_store_multi(*call), "cache_store_multi")
    got = B._alternate({"load": lambda: lib.ssdnerf_cache_load_multi(*call), "store": lambda: lib.ssdnerf_cache_store_multi(*call)}, 50, args.windows, warmup=3)
    numel = cache.numel
    stored = numel * (cache.code_.element_size() + 2 * cache.exp_avg.element_size()) + cache.grid_bytes + cache.bits_bytes
    batch = 3 * numel * 4 + cache.grid_bytes + cache.bits_bytes
    moved = S * (stored + batch)
    for name in ("load", "store"):
        us = got[name]["event_ms"]["median"] * 1e3
        got[name].update(mbytes_moved=round(moved / 1e6, 2), floor_us_at_8tbps=round(moved / (PEAK_TBPS * 1e6), 2),
                         share_of_8tbps=round(moved / (us * 1e-6) / (PEAK_TBPS * 1e12), 4) if us > 0 else None)
    got["bytes_per_scene"] = dict(store=stored, batch=batch)
    return got


def _batch():
    """8 synthetic scenes rendered from V cameras each: the dense conditioning batch of a training step"""
    from ssdnerf_amd import nerf, synthetic as SY
    from ssdnerf_amd.density import get_density
    dec = B._decoder()
    codes = torch.stack([SY.make_triplane(51 + s) for s in range(S)]).cuda()
    poses = SY.spiral_poses()[torch.linspace(0, 250, V).round().long()][None].expand(S, -1, -1, -1).contiguous().cuda()
    intr = SY.cars_intrinsics(B.H, B.W)[None, None].expand(S, V, -1).contiguous().cuda()
    with torch.no_grad():
        _, bits = get_density(dec, codes, GRID, density_thresh=0.1, density_step=4)
        image, _ = nerf.render(dec, codes, bits, B.H, B.W, intr, poses)
    ids = list(range(S))
    return dict(scene_id=ids, scene_name=[f"s{i}" for i in ids], cond_imgs=image.clamp(0, 1), cond_poses=poses, cond_intrinsics=intr)


def _train_steps(args):
    data = _batch()
    state = {}
    for store in ("host", "device"):
        m = _model(store, False)
        state[store] = (m, dict(decoder=torch.optim.Adam(m.decoder.parameters(), lr=1e-3)))

    def step(store):
        m, opt = state[store]
        state[store + "_loss"] = m.train_step(data, opt)["log_vars"]["loss"]

    res = B._alternate({store: (lambda store=store: step(store)) for store in ("host", "device")}, args.train_steps, args.windows, warmup=2)
    for store in ("host", "device"):                                    # the peak of one more step each, from the same resting state
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step(store)
        torch.cuda.synchronize()
        res[store].update(allocated_before_mbytes=round(before / 1e6, 1), max_allocated_mbytes=round(torch.cuda.max_memory_allocated() / 1e6, 1),
                          last_loss=float(state[store + "_loss"]))
    res["device"].update(host_copies=state["device"][0].cache.host_copies)
    med = {store: res[store]["event_ms"]["median"] for store in ("host", "device")}
    spread = max(res[store]["event_ms"]["max"] - res[store]["event_ms"]["min"] for store in ("host", "device"))
    res["difference_ms"] = round(med["host"] - med["device"], 4)
    res["spread_between_windows_ms"] = round(spread, 4)
    res["difference_exceeds_spread"] = bool(abs(med["host"] - med["device"]) > spread)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8, help="load+save steps per window (8 steps visit all 64 slots)")
    ap.add_argument("--train-steps", type=int, default=3, help="training steps per window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_cache.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_cache: needs the GPU (no HIP device visible)")
    if args.windows < 4:
        raise SystemExit("bench_scene_cache: at least four windows per mode")
    res = dict(tool="bench_scene_cache", device=torch.cuda.get_device_name(0), windows=args.windows, scenes=S, slots=SLOTS, code_size=list(CODE), grid_size=GRID,
               extra_scene_step=B.TRAIN_CFG["extra_scene_step"], rays_per_scene=B.R)
    res["load_save"] = _load_save(args)
    res["train_step"] = _train_steps(args)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
