"""Writing the test views of one evaluation batch and the code planes of its scenes as PNG files (ssdnerf_amd/viz.py, csrc/png_rows.hip): 8 scenes x 251
views of 128 x 128 beside their ground truth, and the 8 scenes' (3, 6, 128, 128) codes.  Windows alternate in one process between

  * ``write_views`` / ``write_code_planes``: the whole call by the host clock (it ends with every file closed), and its three stages one after the
    other -- the launch (to a device synchronise), the device-to-host copy through pinned memory, deflate + write on the thread pool;
  * ``filter_launch`` / ``plane_launch``: the kernels alone through the C ABI, by HIP events: the bytes the algorithm needs (every operand byte read
    once, every output byte written once) over that time, and their share of 8 TB/s;
  * ``reference_shaped``: what the reference does, restated: quantise and concatenate with torch, ``.cpu().numpy()``, one ``plt.imsave`` per image
    (Pillow's ``Image.save`` where matplotlib does not import; absent where neither does).

Also: the files' total bytes with the adaptive filter choice and with filter type 0 throughout (same deflate level), and the share of each filter
type among the rows.  Files go to a scratch directory that is removed at the end.  Writes one JSON line.
usage: python tools/bench_viz.py [--out profiles/viz.json] [--windows 3]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
PNG_OVERHEAD = 8 + 25 + 12 + 12                          # signature, IHDR, IDAT's and IEND's framing


def _spread(vals):
    return dict(median=round(statistics.median(vals), 4), min=round(min(vals), 4), max=round(max(vals), 4))


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _events(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _saver():
    """(name, save(path, array, **kw)) of the reference-shaped path, or (None, None)"""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        return "matplotlib.pyplot.imsave", lambda path, arr, **kw: plt.imsave(path, arr, **kw)
    except Exception:                                                    # noqa: BLE001
        pass
    try:
        from PIL import Image
        return "PIL.Image.save", lambda path, arr, **kw: Image.fromarray(arr).save(path) if arr.ndim == 3 else None
    except Exception:                                                    # noqa: BLE001
        return None, None


def _deflated_bytes(rows, level):
    """total file bytes of the (n, h, 1 + L) streams at this deflate level"""
    with ThreadPoolExecutor(max_workers=16) as pool:
        return sum(pool.map(lambda r: len(zlib.compress(r, level)) + PNG_OVERHEAD, rows))


def _staged(viz, run_launch, width, height, level, folder, names):
    """the three stages of a write, one after the other -> (launch_ms, copy_ms, compress_write_ms)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = run_launch()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    host = viz._to_host(rows)
    t2 = time.perf_counter()
    viz._write_all([os.path.join(folder, n) for n in names], host, width, height, level)
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (time.perf_counter() - t2) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viz.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--views", type=int, default=251)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--level", type=int, default=6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_viz: needs the GPU (no HIP device visible)")
    from ssdnerf_amd import _cabi as C, synthetic as S, viz
    Sn, V, hw = args.scenes, args.views, args.size
    # the views: smooth shapes with noise at k / 255 (what val_step hands over) beside a noisier ground truth off that grid
    g = torch.Generator(device="cuda").manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(hw, device="cuda"), torch.arange(hw, device="cuda"), indexing="ij")
    phase = torch.rand(Sn, V, 1, 1, 3, device="cuda", generator=g) * 6.28
    smooth = 0.5 + 0.4 * torch.sin(0.06 * xx[None, None, :, :, None] + 0.045 * yy[None, None, :, :, None] + phase)
    disc = (((xx - hw / 2) ** 2 + (yy - hw / 2) ** 2) < (hw / 3) ** 2)[None, None, :, :, None]
    clean = torch.where(disc, smooth, torch.ones_like(smooth))                       # an object on the white background of the cars renders
    pred = torch.round((clean + 0.01 * torch.randn(clean.shape, device="cuda", generator=g)).clamp(0, 1) * 255) / 255
    target = (clean + 0.02 * torch.randn(clean.shape, device="cuda", generator=g) * disc).clamp(0, 1)
    del smooth, clean, phase
    names = ["scene_%04d" % s for s in range(Sn)]
    paths = [["rgb/%06d.png" % v for v in range(V)] for _ in range(Sn)]
    metrics = dict(psnr=torch.rand(Sn, V, device="cuda") * 10 + 20, ssim=torch.rand(Sn, V, device="cuda"))
    code = torch.stack([S.make_triplane(60 + s) for s in range(Sn)]).cuda()
    folder = tempfile.mkdtemp(prefix="bench_viz_")
    saver_name, save = _saver()
    lib = C.lib()
    n = Sn * V
    flat_p, flat_t = pred.view(n, hw, hw, 3), target.view(n, hw, hw, 3)
    rows_buf = torch.empty((n, hw, 1 + 6 * hw), dtype=torch.uint8, device="cuda")
    rgb_buf = torch.empty((Sn, 3 * code.size(3), code.size(2) * code.size(4), 3), dtype=torch.uint8, device="cuda")
    table = torch.from_numpy(viz.viridis_table().copy()).cuda()

    def filter_launch():
        lib.ssdnerf_png_filter_rows(C.ptr(flat_p), 0, C.ptr(flat_t), 0, n, hw, hw, C.ptr(rows_buf), C.stream())

    def plane_launch():
        lib.ssdnerf_code_plane_rgb(C.ptr(code), C.ptr(table), Sn, code.size(2), code.size(3), code.size(4), -1.0, 1.0, 0, C.ptr(rgb_buf), C.stream())

    def write_views():
        viz.write_views(os.path.join(folder, "ours"), names, pred, target, img_paths=paths, metrics=metrics, level=args.level)

    def write_planes():
        viz.write_code_planes(os.path.join(folder, "ours"), code, names, level=args.level)

    def reference_views():
        out = torch.round(pred * 255).to(torch.uint8).cpu().numpy()
        real = (target * 255).to(torch.uint8).cpu().numpy()
        out = np.concatenate([real, out], axis=-2)
        os.makedirs(os.path.join(folder, "ref"), exist_ok=True)
        for s in range(Sn):
            for v in range(V):
                save(os.path.join(folder, "ref", "scene_%s_%06d.png" % (names[s], v)), out[s][v])

    def reference_planes():
        sheet = code.cpu().numpy()[..., ::-1, :].transpose(0, 1, 3, 2, 4).reshape(Sn, 3 * code.size(3), code.size(2) * code.size(4))
        os.makedirs(os.path.join(folder, "ref"), exist_ok=True)
        for s in range(Sn):
            save(os.path.join(folder, "ref", "scene_%s.png" % names[s]), sheet[s], vmin=-1, vmax=1)

    try:
        for fn in (filter_launch, plane_launch, write_views, write_planes):          # warm-up: code objects, pinned allocation, the pool's first threads
            fn()
        torch.cuda.synchronize()
        got = {k: [] for k in ("views_call", "views_launch", "views_copy", "views_compress_write", "filter_launch_event", "views_reference",
                               "planes_call", "planes_launch", "planes_copy", "planes_compress_write", "plane_launch_event", "planes_reference")}
        view_names = ["v%05d.png" % i for i in range(n)]
        for _ in range(args.windows):
            got["views_call"].append(_wall(write_views))
            a, b, c = _staged(viz, lambda: viz.filter_rows(flat_p, flat_t), 2 * hw, hw, args.level, os.path.join(folder, "ours"), view_names)
            got["views_launch"].append(a); got["views_copy"].append(b); got["views_compress_write"].append(c)
            got["filter_launch_event"].append(_events(filter_launch, 20))
            got["planes_call"].append(_wall(write_planes))
            a, b, c = _staged(viz, lambda: viz.filter_rows(viz.code_plane_rgb(code)), rgb_buf.size(2), rgb_buf.size(1), args.level,
                              os.path.join(folder, "ours"), ["p%d.png" % i for i in range(Sn)])
            got["planes_launch"].append(a); got["planes_copy"].append(b); got["planes_compress_write"].append(c)
            got["plane_launch_event"].append(_events(plane_launch, 20))
            if save is not None:
                got["views_reference"].append(_wall(reference_views))
                if saver_name.startswith("matplotlib"):
                    got["planes_reference"].append(_wall(reference_planes))
        res = dict(tool="bench_viz", device=torch.cuda.get_device_name(0), windows=args.windows, deflate_level=args.level, writer_threads=viz.MAX_WRITERS,
                   workload=f"{Sn} scenes x {V} views of {hw} x {hw} beside their ground truth (fp32 operands); code planes of {Sn} scenes {tuple(code.shape[1:])}",
                   files=dict(views=n, planes=Sn), reference_shaped_saver=saver_name)
        res.update({k + "_ms": _spread(v) for k, v in got.items() if v})
        # bytes the kernels need, over their event time
        view_bytes = flat_p.numel() * 4 + flat_t.numel() * 4 + rows_buf.numel()
        plane_bytes = code.numel() * 4 + rgb_buf.numel()
        for key, nbytes, ev in (("filter_launch", view_bytes, "filter_launch_event"), ("plane_launch", plane_bytes, "plane_launch_event")):
            ms = statistics.median(got[ev])
            res[key] = dict(mbytes_needed=round(nbytes / 1e6, 2), min_ms_at_8tbps=round(nbytes / HBM_BYTES_PER_S * 1e3, 5),
                            tbytes_per_s=round(nbytes / (ms * 1e-3) / 1e12, 3), share_of_8tbps=round(nbytes / HBM_BYTES_PER_S * 1e3 / ms, 3))
        # file sizes: the adaptive choice against filter type 0 throughout
        for key, rows in (("views", viz.filter_rows(flat_p, flat_t)), ("planes", viz.filter_rows(viz.code_plane_rgb(code)))):
            host = np.ascontiguousarray(viz._to_host(rows))
            kinds = np.bincount(host[..., 0].reshape(-1), minlength=5)
            # type 0 throughout: the scanlines themselves behind a zero byte, recomputed with torch from the operands as the reference-shaped path does
            if key == "views":
                raw = torch.cat([(flat_t * 255).to(torch.uint8), torch.round(flat_p * 255).to(torch.uint8)], dim=2).reshape(n, hw, -1).cpu()
            else:
                raw = viz.code_plane_rgb(code).reshape(Sn, rgb_buf.size(1), -1).cpu()
            zero = torch.cat([torch.zeros(raw.shape[:2] + (1,), dtype=torch.uint8), raw], dim=2).numpy()
            res[key + "_file_bytes"] = dict(adaptive=_deflated_bytes(host, args.level), filter_type_0=_deflated_bytes(zero, args.level),
                                            raw_scanline_bytes=int(raw.numel()),
                                            rows_per_filter_type={str(t): int(c) for t, c in enumerate(kinds)})
        line = json.dumps(res)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        print(line)
    finally:
        shutil.rmtree(folder, ignore_errors=True)


if __name__ == "__main__":
    main()
