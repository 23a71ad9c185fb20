"""Training ray batches with their pixel numbers drawn on the host (``torch.randperm``, the default) against made on the device (the keyed
permutation of csrc/keyed_perm.h: ``ssdnerf_perm_indices`` / ``ssdnerf_sample_rays_perm_u8``, ``fitting.RayBatcher(index_source='device')``;
DESIGN.md section 23), on the GPU.  The training batch of the cars configs: 8 scenes x 50 views of 128 x 128, R = 4096 rays per scene and step.
The yardstick is the host mode IN THE SAME PROCESS, which is the unchanged path; windows of the modes alternate.

  fresh_*      one ``RayBatcher(fixed=False).take(None)``: a freshly drawn ray batch (what ``loss_decoder`` pays per step), on the stored and on the
               dense conditioning, host and device indices
  fixed_*      ``RayBatcher(fixed=True)`` built and its first batch taken (what ``CodeFitter`` pays when it is built, once per training step: the
               host mode permutes all 819 200 pixels of every scene), the same four
  launch_*     the bare launches through the C ABI: ``ssdnerf_perm_indices``, ``ssdnerf_sample_rays_perm_u8``, and ``ssdnerf_sample_rays_u8`` on
               prepared indices for comparison
  feistel      the mean number of passes through the network per index (tests/_perm_ref.py on the host): over all 819 200 positions of a scene,
               and over the R leading positions of the 8 scenes
  train_step   ms per ``MultiSceneNeRF.train_step`` (stage-1 model, ``extra_scene_step=15``, ``HIPAdam``) on stored loader batches, the batch
               assembly inside the timed region, with ``train_cfg['ray_index_source']`` 'host' and 'device'

per call by HIP events and by the host clock over the same synchronised window, median (min - max) over the windows.  ``speedup`` entries are
ratios of medians with ``exceeds_spread``: whether the slower mode's fastest window is still slower than the faster mode's slowest one.

Writes one JSON line to ``--out`` and prints it.   usage: python tools/bench_ray_perm.py [--windows 7] [--steps 50] [--train-steps 2] [--out profiles/ray_perm.json]"""
import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_ray_sampler as B  # noqa: E402  (the workload, the window timer and the stage-1 model of the section-18 benchmark)

S, V, H, W, R = B.S, B.V, B.H, B.W, B.R
SEED = 0x5EED0123456789


def _compare(res, host, device):
    """host / device by the medians of the HIP-event times, and whether the gap is larger than the spread between windows"""
    h, d = res[host]["event_ms"], res[device]["event_ms"]
    slow, fast = (h, d) if h["median"] >= d["median"] else (d, h)
    return dict(host=host, device=device, speedup=round(h["median"] / d["median"], 3), exceeds_spread=bool(slow["min"] > fast["max"]),
                wall_speedup=round(res[host]["wall_ms"]["median"] / res[device]["wall_ms"]["median"], 3))


def _ray_batches(args):
    from ssdnerf_amd import _cabi as C
    from ssdnerf_amd import datasets as D
    from ssdnerf_amd.fitting import Conditioning, RayBatcher
    pixels = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (S * V, H, W, 3), dtype=np.uint8))
    store = D.SceneStore(pixels)
    poses, intr = B._cameras()
    table = np.arange(S * V, dtype=np.int64).reshape(S, V)
    P = V * H * W
    views = D.StoredViews(store, table, poses, intr)
    images = store.gather(table.reshape(-1)).view(S, V, H, W, 3)
    conds = dict(stored=Conditioning.from_batch(dict(cond_imgs=views, cond_poses=poses, cond_intrinsics=intr), 0.5),
                 dense=Conditioning.from_batch(dict(cond_imgs=images, cond_poses=poses, cond_intrinsics=intr), 0.5))
    fns = {}
    for kind, cond in conds.items():
        for source in ("host", "device"):
            fresh = RayBatcher(cond, R, fixed=False, index_source=source, seed=SEED if source == "device" else None)
            fns[f"fresh_{kind}_{source}"] = lambda fresh=fresh: fresh.take(None)
            fns[f"fixed_{kind}_{source}"] = lambda cond=cond, source=source: RayBatcher(cond, R, fixed=True, index_source=source).batch(0)
    lib = C.lib()
    inds = torch.empty((S, R), dtype=torch.int64, device="cuda")
    outs = [torch.empty((S, R, 3), device="cuda") for _ in range(3)]
    head = (C.ptr(store.pixels), store.num_images, H, W, C.ptr(views.view_image_dev), C.ptr(views.poses), C.ptr(views.intrinsics), S, V)
    tail = (C.ptr(outs[0]), C.ptr(outs[1]), C.ptr(outs[2]), C.stream())
    fns["launch_perm_indices"] = lambda: lib.ssdnerf_perm_indices(C.ptr(inds), S, P, 0, R, SEED, 0, C.stream())
    fns["launch_sample_rays_perm_u8"] = lambda: lib.ssdnerf_sample_rays_perm_u8(*head, SEED, 0, 0, R, *tail)
    fns["launch_sample_rays_u8"] = lambda: lib.ssdnerf_sample_rays_u8(*head, C.ptr(inds), R, *tail)
    # the two device routes give the same bits: fused against indices + the existing sampler, and the dense against the stored conditioning
    C.check(fns["launch_perm_indices"](), "perm_indices")
    C.check(fns["launch_sample_rays_u8"](), "sample_rays_u8")
    want = [o.clone() for o in outs]
    C.check(fns["launch_sample_rays_perm_u8"](), "sample_rays_perm_u8")
    a, b = (RayBatcher(conds[k], R, fixed=True, index_source="device", seed=SEED) for k in ("stored", "dense"))
    res = dict(bit_equal=bool(B._triples_equal(outs, want) and B._triples_equal(a.batch(3), b.batch(3))))
    res.update(B._alternate(fns, args.steps, args.windows, warmup=3))
    res["compare"] = [_compare(res, f"{what}_{kind}_host", f"{what}_{kind}_device") for what in ("fresh", "fixed") for kind in ("stored", "dense")]
    return res


def _feistel():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _perm_ref as KP
    P = V * H * W
    whole = KP.walk(KP.round_keys(SEED, 0, 0), P, np.arange(P, dtype=np.uint32))[1]
    heads = np.stack([KP.walk(KP.round_keys(SEED, s, 0), P, np.arange(R, dtype=np.uint32))[1] for s in range(S)])
    return dict(rounds=KP.ROUNDS, domain=4 ** KP.half_bits(P), pixels=P, bound=round(4 ** KP.half_bits(P) / P, 4),
                mean_passes_all_positions=round(float(whole.mean()), 4), max_passes_all_positions=int(whole.max()),
                mean_passes_training_batch=round(float(heads.mean()), 4), max_passes_training_batch=int(heads.max()))


def _train_steps(args):
    from ssdnerf_amd import datasets as D
    tmp = tempfile.mkdtemp(prefix="bench_ray_perm_")
    try:
        B._write_tree(os.path.join(tmp, "cars"))
        ds = D.ShapeNetSRN(os.path.join(tmp, "cars"), radius=1.0)
        loader = D.build_dataloader(ds, S, cond_imgs="stored")
        loader.scene_store                                               # built outside the timed region
    finally:
        shutil.rmtree(tmp)
    ids, state = list(range(S)), {}
    for source in ("host", "device"):
        m, opt = B._model()
        m.train_cfg["ray_index_source"] = source
        state[source] = (m, opt)

    def step(source):
        m, opt = state[source]
        state[source + "_loss"] = m.train_step(loader.batch(ids), opt)["log_vars"]["loss"]

    res = B._alternate({source: (lambda source=source: step(source)) for source in ("host", "device")}, args.train_steps, args.windows, warmup=2)
    out = {"train_step_" + k: dict(v, last_loss=float(state[k + "_loss"])) for k, v in res.items()}
    out["compare"] = _compare(res, "host", "device")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="calls per window of the ray-batch paths")
    ap.add_argument("--train-steps", type=int, default=2, help="training steps per window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_perm.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ray_perm: needs the GPU (no HIP device visible)")
    res = dict(tool="bench_ray_perm", device=torch.cuda.get_device_name(0), windows=args.windows, scenes=S, views=V, image=[H, W, 3], rays_per_scene=R,
               extra_scene_step=B.TRAIN_CFG["extra_scene_step"])
    res["feistel"] = _feistel()
    res["ray_batches"] = _ray_batches(args)
    res["train_step"] = _train_steps(args)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
