"""Assembling a batch of views from the image store (ssdnerf_amd/datasets.py, csrc/scene_store.hip), on the GPU:

  * the training batch, 8 scenes x 50 views of 128 x 128 (19.7 MB of uint8 in, 78.6 MB of fp32 out), and the evaluation batch, 8 x 250, by
      device_store       ``SceneStore.gather`` from the device-resident store (index upload and output allocation included)
      kernel_alone       the same launch straight through the C ABI on a prepared index and output (its event time is the kernel's)
      kernel_alone_NAME  the same from a side build of the library (``--alt-lib NAME=PATH``; e.g. scene_store.hip with -DGV_PLAIN_STORES or -DGV_LOAD16), when given
      host_store         ``SceneStore.gather`` from the pinned host store, copies included
      eager              the eager restatement on the same GPU, ``store[idx].float() / 255``
      reference_host     the reference-shaped host path: numpy ``astype(float32) / 255`` of the same images and a pageable upload
    per call by HIP events and by the host clock over the same synchronised window, every path warmed up, windows alternated between the
    paths, median (min - max); the bytes the launch moves (1 in + 4 out per element) and their share of 8 TB/s;
  * the seconds to build the store of a synthetic tree of 64 scenes x 50 views of 128 x 128 from PNG files and from the pixel cache.

Prints one JSON line.   usage: python tools/bench_dataset.py [--steps 50] [--windows 7] [--alt-lib NAME=PATH ...] > profiles/dataset.json"""
import argparse
import ctypes
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

HBM_BYTES_PER_S = 8.0e12
H = W = 128
SCENES, VIEWS = 64, 50


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
    """{name: {event_ms, wall_ms}}: ``windows`` windows per path, taken in turn; ``steps[name]`` calls per window"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    got = {name: ([], []) for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            ev, wall = _window(fn, steps[name])
            got[name][0].append(ev)
            got[name][1].append(wall)
    return {name: dict(event_ms=_spread(ev), wall_ms=_spread(wall), calls_per_window=steps[name]) for name, (ev, wall) in got.items()}


def _batch(pixels_np, dev, host, scenes, views, steps, windows, alt_libs):
    from ssdnerf_amd import _cabi as C
    g = np.random.default_rng(scenes * views)
    starts = g.integers(0, pixels_np.shape[0] - views, scenes)
    idx = np.concatenate([np.arange(s, s + views) for s in starts])
    n, image_bytes = len(idx), H * W * 3
    idx_dev = torch.from_numpy(idx).cuda()
    index = idx_dev.to(torch.int32)
    out = torch.empty((n, H, W, 3), device="cuda")
    lib, stream = C.lib(), C.stream()
    args = (C.ptr(dev.pixels), image_bytes, dev.num_images, C.ptr(index), n, C.ptr(out), stream)
    C.check(lib.ssdnerf_gather_views_u8(*args), "gather_views_u8")
    want = torch.from_numpy(pixels_np[idx].astype(np.float32) / 255).cuda()
    assert torch.equal(out, want) and torch.equal(dev.gather(idx), want) and torch.equal(host.gather(idx), want)
    eager_identical = bool(torch.equal(dev.pixels[idx_dev].float() / 255, want))

    fns = {"device_store": lambda: dev.gather(idx), "kernel_alone": lambda: lib.ssdnerf_gather_views_u8(*args)}
    for name, path in alt_libs.items():
        alt = ctypes.CDLL(path)
        alt.ssdnerf_gather_views_u8.argtypes = lib.ssdnerf_gather_views_u8.argtypes
        out.zero_()
        C.check(alt.ssdnerf_gather_views_u8(*args), f"gather_views_u8 ({name} build)")
        assert torch.equal(out, want), name
        fns["kernel_alone_" + name] = (lambda alt=alt: alt.ssdnerf_gather_views_u8(*args))
    fns["host_store"] = lambda: host.gather(idx)
    fns["eager"] = lambda: dev.pixels[idx_dev].float() / 255
    fns["reference_host"] = lambda: torch.from_numpy(pixels_np[idx].astype(np.float32) / 255).cuda()
    slow = max(2, steps // 25)
    res = _alternate(fns, {k: (slow if k == "reference_host" else steps) for k in fns}, windows, warmup=3)
    nbytes = 5 * n * image_bytes
    floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
    res.update(eager_bit_identical=eager_identical, scenes=scenes, views=views, images=n, mbytes_in=round(n * image_bytes / 1e6, 2), mbytes_out=round(4 * n * image_bytes / 1e6, 2),
               min_ms_at_8tbps=round(floor_ms, 5), kernel_share_of_8tbps=round(floor_ms / res["kernel_alone"]["event_ms"]["median"], 3),
               kernel_tbytes_per_s=round(nbytes / res["kernel_alone"]["event_ms"]["median"] / 1e9, 3))
    for name in alt_libs:
        res[f"kernel_{name}_share_of_8tbps"] = round(floor_ms / res["kernel_alone_" + name]["event_ms"]["median"], 3)
    return res


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def _write_png(path, img):
    """an 8-bit RGB PNG, filter type 0 on every row"""
    h, w, _ = img.shape
    raw = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * 3)], axis=1).tobytes()
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(raw, 1)) + _chunk(b"IEND", b""))


def _write_tree(root):
    g = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    for s in range(SCENES):
        scene = os.path.join(root, "%04d" % s)
        os.makedirs(os.path.join(scene, "rgb"))
        os.makedirs(os.path.join(scene, "pose"))
        with open(os.path.join(scene, "intrinsics.txt"), "w") as f:
            f.write("131.25 64. 64. 0.\n0. 0. 0.\n1.\n%d %d\n" % (H, W))
        for v in range(VIEWS):
            img = np.full((H, W, 3), 255, np.uint8)                        # a blob on white, like a rendered car: PNG compresses it well
            blob = (yy - 64) ** 2 + (xx - 64 - v) ** 2 < (20 + s % 17) ** 2
            img[blob] = g.integers(0, 256, (int(blob.sum()), 3), dtype=np.uint8)
            _write_png(os.path.join(scene, "rgb", "%06d.png" % v), img)
            with open(os.path.join(scene, "pose", "%06d.txt" % v), "w") as f:
                f.write(" ".join(["1 0 0 0", "0 1 0 0", "0 0 1 1.3", "0 0 0 1"]) + "\n")


def _build_store(tmp):
    from ssdnerf_amd import datasets as D
    tree, cache = os.path.join(tmp, "cars"), os.path.join(tmp, "pixels.npy")
    _write_tree(tree)
    ds = D.ShapeNetSRN(tree, pixel_cache_path=cache)

    def build():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store = D.SceneStore(ds)
        torch.cuda.synchronize()
        return store, time.perf_counter() - t0
    store, from_png = build()
    _, from_cache = build()
    pixels = store.pixels.cpu().numpy()
    return pixels, dict(scenes=SCENES, views=VIEWS, images=SCENES * VIEWS, decoder="Pillow" if D._have_pil() else "built-in", decode_threads=D.DECODE_THREADS,
                        png_mbytes=round(sum(os.path.getsize(p) for p in ds.image_paths) / 1e6, 2), store_mbytes=round(pixels.nbytes / 1e6, 2),
                        seconds_from_png=round(from_png, 3), seconds_from_pixel_cache=round(from_cache, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--alt-lib", action="append", default=[], metavar="NAME=PATH",
                    help="a side build of the library to time beside the shipped one, e.g. plain=.variants/plain/libssdnerf_hip.so (scene_store.hip compiled with "
                         "-DGV_PLAIN_STORES by `python -m ssdnerf_amd.build --variant plain --source scene_store.hip -- -DGV_PLAIN_STORES`; -DGV_LOAD16 is the "
                         "other switch)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dataset: needs the GPU (no HIP device visible)")
    from ssdnerf_amd import datasets as D
    alt_libs = dict(a.split("=", 1) for a in args.alt_lib)
    res = dict(tool="bench_dataset", device=torch.cuda.get_device_name(0), windows=args.windows, image=[H, W, 3])
    tmp = tempfile.mkdtemp(prefix="bench_dataset_")
    try:
        pixels, res["build_store"] = _build_store(tmp)
    finally:
        shutil.rmtree(tmp)
    dev, host = D.SceneStore(pixels, store="device"), D.SceneStore(pixels, store="host")
    res["train_batch"] = _batch(pixels, dev, host, 8, 50, args.steps, args.windows, alt_libs)
    res["eval_batch"] = _batch(pixels, dev, host, 8, 250, max(4, args.steps // 4), args.windows, alt_libs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
