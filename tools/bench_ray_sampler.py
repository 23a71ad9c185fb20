"""Ray batches for training, from the fp32 batch and straight from the uint8 image store (ssdnerf_amd/datasets.py ``StoredViews``,
csrc/scene_store.hip ``ssdnerf_sample_rays_u8``), on the GPU.  The training batch of the cars configs: 8 scenes x 50 views
of 128 x 128, R = 4096 rays per scene and step.

  (a) dense_prepare     what a dense batch costs before its first ray: ``SceneStore.gather`` + ``nerf.get_cam_rays`` (3 x 78.6 MB written)
  (b) dense_take        one ``RayBatcher.take(None)`` on the dense batch (``fixed=False``: the index draw and three indexed gathers);
      dense_take_given  the same with the indices given (what ``fixed=True`` does per step)
  (c) stored_take       one ``take(None)`` on the stored batch (the index draw and ONE launch);  stored_take_given: with the indices given
  (d) index_draw        the draw alone: eight ``torch.randperm(819 200)[:R]`` and a stack
  (f) kernel_alone      the launch straight through the C ABI on prepared indices and outputs
  (e) train_step        ms per ``MultiSceneNeRF.train_step`` (stage-1 model, ``extra_scene_step=15``, 2^12 rays, ``HIPAdam``) on a batch from
                        ``build_dataloader(..., cond_imgs='dense')`` and from ``cond_imgs='stored'``, the batch assembly inside the timed region, and
                        ``torch.cuda.max_memory_allocated`` over one such step each (views rendered from eight synthetic scenes, written as an SRN tree)

every path warmed up, windows alternated between the paths, per call by HIP events and by the host clock over the same synchronised window, median
(min - max).  ``bit_equal`` says whether the stored and the dense ray batches of this run had the same bits.  ``--dense-only`` times what exists
without the feature -- (a), (b), (d) and the dense half of (e) -- so the same file can be run in a checkout of an earlier commit.

Writes one JSON line to ``--out`` and prints it.   usage: python tools/bench_ray_sampler.py [--windows 7] [--steps 50] [--train-steps 2] [--modes dense,stored] [--out profiles/ray_sampler.json]"""
import argparse
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, V, H, W, R = 8, 50, 128, 128, 4096
DEC = dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[6 * 3, 64], density_layers=[64, 1], color_layers=[64, 3], use_dir_enc=True,
           dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001, max_steps=256)
TRAIN_CFG = dict(dt_gamma_scale=0.5, density_thresh=0.1, extra_scene_step=15, n_inverse_rays=R, n_decoder_rays=R, loss_coef=0.1 / (H * W),
                 optimizer=dict(type="HIPAdam", lr=1e-2, weight_decay=0.))


def _window(fn, steps):
    """(HIP-event ms per call, host wall ms per call) of ``steps`` calls between two synchronisations"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, (time.perf_counter() - t0) * 1e3 / steps


def _spread(vals):
    return dict(median=round(statistics.median(vals), 5), min=round(min(vals), 5), max=round(max(vals), 5))


def _alternate(fns, steps, windows, warmup):
    """{name: {event_ms, wall_ms}}: ``windows`` windows per path, taken in turn, ``steps`` calls per window"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    got = {name: ([], []) for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            ev, wall = _window(fn, steps)
            got[name][0].append(ev)
            got[name][1].append(wall)
    return {name: dict(event_ms=_spread(ev), wall_ms=_spread(wall), calls_per_window=steps) for name, (ev, wall) in got.items()}


def _triples_equal(a, b):
    return all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _cameras():
    from ssdnerf_amd import synthetic as SY
    poses = SY.spiral_poses()[torch.linspace(0, 250, V).round().long()]
    return poses[None].expand(S, -1, -1, -1).contiguous().cuda(), SY.cars_intrinsics(H, W)[None, None].expand(S, V, -1).contiguous().cuda()


def _ray_batches(args, dense_only):
    """(a) - (d), (f) on a store of random bytes"""
    from ssdnerf_amd import _cabi as C
    from ssdnerf_amd import datasets as D
    from ssdnerf_amd.fitting import Conditioning, RayBatcher
    pixels = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (S * V, H, W, 3), dtype=np.uint8))
    store = D.SceneStore(pixels)
    poses, intr = _cameras()
    table = np.arange(S * V, dtype=np.int64).reshape(S, V)
    P = V * H * W

    def dense_prepare():
        images = store.gather(table.reshape(-1)).view(S, V, H, W, 3)
        return Conditioning.from_batch(dict(cond_imgs=images, cond_poses=poses, cond_intrinsics=intr), 0.5)

    def draw():
        return torch.stack([torch.randperm(P, device="cuda")[:R] for _ in range(S)], dim=0)

    dense = RayBatcher(dense_prepare(), R, fixed=False)
    given = draw()
    fns = {"dense_prepare": dense_prepare, "dense_take": lambda: dense.take(None), "dense_take_given": lambda: dense.take(given), "index_draw": draw}
    res = {}
    if not dense_only:
        views = D.StoredViews(store, table, poses, intr)
        stored = RayBatcher(Conditioning.from_batch(dict(cond_imgs=views, cond_poses=poses, cond_intrinsics=intr), 0.5), R, fixed=False)
        outs = [torch.empty((S, R, 3), device="cuda") for _ in range(3)]
        call = (C.ptr(store.pixels), store.num_images, H, W, C.ptr(views.view_image_dev), C.ptr(views.poses), C.ptr(views.intrinsics), S, V, C.ptr(given), R,
                C.ptr(outs[0]), C.ptr(outs[1]), C.ptr(outs[2]), C.stream())
        lib = C.lib()
        C.check(lib.ssdnerf_sample_rays_u8(*call), "sample_rays_u8")
        want = dense.take(given)
        equal = _triples_equal(outs, want) and _triples_equal(stored.take(given), want)
        torch.manual_seed(3)
        a = dense.take(None)
        torch.manual_seed(3)
        equal = equal and _triples_equal(stored.take(None), a)
        res["bit_equal"] = bool(equal)
        fns.update(stored_take=lambda: stored.take(None), stored_take_given=lambda: stored.take(given),
                   kernel_alone=lambda: lib.ssdnerf_sample_rays_u8(*call))
    res.update(_alternate(fns, args.steps, args.windows, warmup=3))
    res.update(dense_prepare_mbytes_written=round(3 * S * P * 12 / 1e6, 1), kernel_mbytes_moved=round(S * R * (8 + 3 + 36) / 1e6, 2))
    return res


# ---------------------------------------------------------------------------------------------- (e): a stage-1 training step on loader batches
def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def _write_png(path, img):
    """an 8-bit RGB PNG, filter type 0 on every row"""
    h, w, _ = img.shape
    raw = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * 3)], axis=1).tobytes()
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(raw, 1)) + _chunk(b"IEND", b""))


def _decoder():
    from ssdnerf_amd import synthetic as SY
    from ssdnerf_amd.decoders import TriPlaneDecoder
    dec = TriPlaneDecoder(**{k: v for k, v in DEC.items() if k != "type"})
    dec.load_state_dict(SY.make_decoder_params(), strict=False)
    return dec.cuda().eval()


def _write_tree(root):
    """eight synthetic scenes rendered from the V cameras, as an SRN folder tree"""
    from ssdnerf_amd import nerf, synthetic as SY
    from ssdnerf_amd.density import get_density
    dec = _decoder()
    codes = torch.stack([SY.make_triplane(51 + s) for s in range(S)]).cuda()
    poses, intr = _cameras()
    with torch.no_grad():
        _, bits = get_density(dec, codes, 64, density_thresh=0.1, density_step=4)
        image, _ = nerf.render(dec, codes, bits, H, W, intr, poses)
    image = torch.round(image.clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()
    f0 = float(intr[0, 0, 0])
    for s in range(S):
        scene = os.path.join(root, "%04d" % s)
        os.makedirs(os.path.join(scene, "rgb"))
        os.makedirs(os.path.join(scene, "pose"))
        with open(os.path.join(scene, "intrinsics.txt"), "w") as f:
            f.write("%r %r %r 0.\n0. 0. 0.\n1.\n%d %d\n" % (f0, W / 2, H / 2, H, W))
        for v in range(V):
            _write_png(os.path.join(scene, "rgb", "%06d.png" % v), image[s, v])
            with open(os.path.join(scene, "pose", "%06d.txt" % v), "w") as f:
                f.write(" ".join(repr(float(x)) for x in poses[s, v].reshape(-1).tolist()) + "\n")


def _model():
    from ssdnerf_amd import synthetic as SY
    from ssdnerf_amd.registry import MODELS
    torch.manual_seed(0)
    m = MODELS.build(dict(type="MultiSceneNeRF", code_size=(3, 6, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64,
                          decoder=DEC, decoder_use_ema=True, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
                          reg_loss=dict(type="TVLoss", power=1.5, loss_weight=1.0), cache_size=S, init_from_mean=True, train_cfg=dict(TRAIN_CFG)))
    m.decoder.load_state_dict(SY.make_decoder_params(), strict=False)
    m.decoder_ema.load_state_dict(SY.make_decoder_params(), strict=False)
    with torch.no_grad():
        m.init_code.copy_(SY.make_triplane(80))
    m = m.cuda().train()
    return m, dict(decoder=torch.optim.Adam(m.decoder.parameters(), lr=1e-3))


def _train_steps(args, dense_only):
    from ssdnerf_amd import datasets as D
    tmp = tempfile.mkdtemp(prefix="bench_ray_sampler_")
    try:
        _write_tree(os.path.join(tmp, "cars"))
        ds = D.ShapeNetSRN(os.path.join(tmp, "cars"), radius=1.0)       # (radius 1: the poses are written in the scene's own units)
        modes = ["dense"] if dense_only else args.modes.split(",")
        loaders = {mode: (D.build_dataloader(ds, S) if mode == "dense" else D.build_dataloader(ds, S, cond_imgs=mode)) for mode in modes}
        for loader in loaders.values():
            loader.scene_store                                           # the store is built outside the timed region: once per run, not per batch
    finally:
        shutil.rmtree(tmp)
    ids = list(range(S))
    state = {}
    for mode in modes:
        m, opt = _model()
        state[mode] = (m, opt, loaders[mode])

    def step(mode):
        m, opt, loader = state[mode]
        out = m.train_step(loader.batch(ids), opt)
        state[mode + "_loss"] = out["log_vars"]["loss"]

    res = _alternate({mode: (lambda mode=mode: step(mode)) for mode in modes}, args.train_steps, args.windows, warmup=2)
    res = {"train_step_" + k: v for k, v in res.items()}
    for mode in modes:                                                   # the peak of one more step each, from the same resting state
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step(mode)
        torch.cuda.synchronize()
        res["train_step_" + mode].update(allocated_before_mbytes=round(before / 1e6, 1), max_allocated_mbytes=round(torch.cuda.max_memory_allocated() / 1e6, 1),
                                        last_loss=float(state[mode + "_loss"]))
    if "stored" in modes:
        views = state["stored"][2].batch(ids)["cond_imgs"]
        res["stored_batch_dense_calls"] = views.dense_calls
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="calls per window of the ray-batch paths")
    ap.add_argument("--train-steps", type=int, default=2, help="training steps per window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--modes", default="dense,stored", help="the loaders of (e), alternated in this order: dense, stored or both")
    ap.add_argument("--dense-only", action="store_true", help="only what exists without StoredViews (for a checkout of an earlier commit)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_sampler.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ray_sampler: needs the GPU (no HIP device visible)")
    res = dict(tool="bench_ray_sampler", device=torch.cuda.get_device_name(0), windows=args.windows, scenes=S, views=V, image=[H, W, 3], rays_per_scene=R,
               extra_scene_step=TRAIN_CFG["extra_scene_step"], dense_only=args.dense_only, train_step_modes="dense" if args.dense_only else args.modes)
    res["ray_batches"] = _ray_batches(args, args.dense_only)
    res["train_step"] = _train_steps(args, args.dense_only)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
