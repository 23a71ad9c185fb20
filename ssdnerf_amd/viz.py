"""Test views and code planes as PNG files (the reference's ``viz_dir``: eval_and_viz, base_nerf.py:576-608; decoder.visualize,
triplane_decoder.py:186-194).  DESIGN.md section 21.

The GPU does what is per pixel and per row -- quantising, the [target | prediction] layout, the colour map of the code planes and PNG's adaptive row
filtering (csrc/png_rows.hip) -- in one launch per call; the filtered rows come to the host in one copy through pinned memory, and a pool of at most 16
threads deflates them with the standard library's ``zlib`` (which releases the GIL) and writes the files.  Nothing is compressed on the GPU.  CPU
tensors take a numpy path that gives the same bytes.

Every byte of a file is defined by the rules ``filter_rows`` / ``code_plane_rgb`` / ``png_bytes`` state; the files are 8-bit RGB (matplotlib's
``imsave`` writes RGBA with alpha 255 -- the decoded RGB is the same).  Nothing here imports matplotlib: viridis (CC0) ships as ``viridis_u8.hex``.
"""
from __future__ import annotations

import bisect
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

MAX_WRITERS = 16                      # the pool's cap; never sized by os.cpu_count()
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"
_VIRIDIS: Optional[np.ndarray] = None
_VIRIDIS_DEV: dict = {}


def viridis_table() -> np.ndarray:
    """matplotlib's viridis as (256, 3) uint8 (``cmap(np.arange(256), bytes=True)[:, :3]``), read once from the 256 ``RRGGBB`` lines of viridis_u8.hex"""
    global _VIRIDIS
    if _VIRIDIS is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "viridis_u8.hex")) as f:
            rows = [bytes.fromhex(line.strip()) for line in f if line.strip()]
        table = np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 3)
        if table.shape != (256, 3):
            raise RuntimeError(f"viridis_u8.hex: 256 lines of RRGGBB expected, got {table.shape}")
        _VIRIDIS = table
    return _VIRIDIS


# ---------------------------------------------------------------------------------------------- bytes of the operands
def _check_images(t, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.size(3) != 3 or t.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{what} must be a float32 or uint8 tensor (N, h, w, 3), got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if t.numel() == 0:
        raise ValueError(f"{what} is empty: {tuple(t.shape)}")


def _bytes_numpy(x: np.ndarray, target: bool) -> np.ndarray:
    """the byte rules of ``filter_rows`` in numpy (fp32 arithmetic, one rounding per operation as on the device)"""
    if x.dtype == np.uint8:
        return x
    with np.errstate(invalid="ignore"):
        v = np.where(np.isnan(x), np.float32(0), x).astype(np.float32)
        v = np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)
        return (v if target else np.rint(v)).astype(np.uint8)


def _filter_numpy(lines: np.ndarray) -> np.ndarray:
    """(N, h, L) uint8 scanlines -> (N, h, 1 + L): the five PNG filters per row, lowest sum of min(r, 256 - r), ties to the lowest type"""
    n, h, L = lines.shape
    x = lines.astype(np.int16)
    b = np.zeros_like(x)
    b[:, 1:] = x[:, :-1]
    a, c = np.zeros_like(x), np.zeros_like(x)
    a[..., 3:], c[..., 3:] = x[..., :-3], b[..., :-3]
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth], axis=0) & 255           # (5, N, h, L)
    score = np.minimum(cand, 256 - cand).astype(np.int64).sum(axis=-1)                          # (5, N, h)
    kind = np.argmin(score, axis=0)                                                             # the first minimum: the lowest type
    out = np.empty((n, h, 1 + L), np.uint8)
    out[..., 0] = kind
    out[..., 1:] = np.take_along_axis(cand, kind[None, ..., None], axis=0)[0]
    return out


def filter_rows(pred: torch.Tensor, target: Optional[torch.Tensor] = None) -> torch.Tensor:
    """N images -> N streams of filtered scanlines, ready for deflate: uint8 (N, h, 1 + 3 W) on ``pred``'s device, W = w without a target and 2 w
    with one (target on the left, prediction on the right, as the reference concatenates on axis -2).

    ``pred``, ``target``: (N, h, w, 3), each float32 or uint8.  Bytes of a float32 ``pred``: ``rint(clamp(x, 0, 1) * 255)``, ties to even (the
    quantisation of ``nerf.quantize_u8``; k / 255 gives k).  Bytes of a float32 ``target``: ``(uint8)(clamp(t, 0, 1) * 255)``, truncated as the
    reference's ``.to(torch.uint8)`` (the clamp is ours: that conversion is undefined outside [0, 255]).  uint8 operands are taken as they are.
    **NaN becomes 0 in both operands** (our definition).  Filtering as the PNG specification has it for 8-bit RGB (bpp = 3): a = the byte 3 to the
    left (0 in the first pixel; the seam is not special), b = the byte above (0 in row 0), c = above-left; per row None, Sub, Up, Average
    (``floor((a + b) / 2)``) and Paeth (ties a, b, c) are scored by ``sum(min(r, 256 - r))`` over the filtered bytes; the lowest score wins, a tie goes
    to the lowest filter number; the row is ``[type, filtered bytes]``.  The choice changes the file size, never the pixels.

    GPU tensors: one launch of ``ssdnerf_png_filter_rows``.  CPU tensors: numpy, the same bytes."""
    _check_images(pred, "filter_rows: pred")
    if target is not None:
        _check_images(target, "filter_rows: target")
        if target.shape != pred.shape or target.device != pred.device:
            raise ValueError(f"filter_rows: target {tuple(target.shape)} on {target.device} does not match pred {tuple(pred.shape)} on {pred.device}")
    n, h, w, _ = pred.shape
    width = w if target is None else 2 * w
    if not pred.is_cuda:
        line = _bytes_numpy(pred.detach().contiguous().numpy(), False).reshape(n, h, 3 * w)
        if target is not None:
            line = np.concatenate([_bytes_numpy(target.detach().contiguous().numpy(), True).reshape(n, h, 3 * w), line], axis=-1)
        return torch.from_numpy(_filter_numpy(line))
    from . import _cabi as C
    pred = pred.detach().contiguous()
    target = None if target is None else target.detach().contiguous()
    with torch.cuda.device(pred.device):
        out = torch.empty((n, h, 1 + 3 * width), dtype=torch.uint8, device=pred.device)
        C.check(C.lib().ssdnerf_png_filter_rows(C.ptr(pred), int(pred.dtype == torch.uint8), C.ptr(target),
                                                int(target is not None and target.dtype == torch.uint8), n, h, w, C.ptr(out), C.stream()), "png_filter_rows")
    return out


def code_plane_rgb(code: torch.Tensor, code_range: Sequence[float] = (-1, 1), flip_z: bool = False) -> torch.Tensor:
    """Triplane codes (S, 3, C, h, w) float32 -> the reference's plane sheet as uint8 RGB (S, 3 h, C w, 3): rows reversed within each plane unless
    ``flip_z``, then ``(S, 3, C, h, w) -> (S, 3, h, C, w) -> (S, 3 h, C w)``, then matplotlib's mapping of a float32 array through viridis:
    ``t = (x - vmin) / (vmax - vmin)`` in fp32, NaN -> (0, 0, 0), t < 0 -> entry 0, t >= 1 -> entry 255, else entry ``floor(t * 256)``.
    GPU tensors: one launch of ``ssdnerf_code_plane_rgb``; CPU tensors: numpy, the same bytes."""
    if not isinstance(code, torch.Tensor) or code.dim() != 5 or code.size(1) != 3 or code.numel() == 0:
        raise ValueError(f"code_plane_rgb: code must be (S, 3, C, h, w), got {tuple(getattr(code, 'shape', ()))}")
    vmin, vmax = float(code_range[0]), float(code_range[1])
    code = code.detach().to(torch.float32).contiguous()
    S, _, Cn, h, w = code.shape
    table = viridis_table()
    if not code.is_cuda:
        x = code.numpy()
        if not flip_z:
            x = x[..., ::-1, :]
        x = x.transpose(0, 1, 3, 2, 4).reshape(S, 3 * h, Cn * w)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            t = (x - np.float32(vmin)) / (np.float32(vmax) - np.float32(vmin))
            entry = np.where(t < 0, 0, np.where(t >= 1, 255, np.floor(np.where(np.isfinite(t), t, 0) * np.float32(256)))).astype(np.int64)
        rgb = table[entry]
        rgb[np.isnan(t)] = 0
        return torch.from_numpy(np.ascontiguousarray(rgb))
    from . import _cabi as C
    key = (code.device.type, code.device.index)
    if key not in _VIRIDIS_DEV:
        _VIRIDIS_DEV[key] = torch.from_numpy(table.copy()).to(code.device)
    with torch.cuda.device(code.device):
        out = torch.empty((S, 3 * h, Cn * w, 3), dtype=torch.uint8, device=code.device)
        C.check(C.lib().ssdnerf_code_plane_rgb(C.ptr(code), C.ptr(_VIRIDIS_DEV[key]), S, Cn, h, w, vmin, vmax, int(bool(flip_z)), C.ptr(out), C.stream()),
                "code_plane_rgb")
    return out


# ---------------------------------------------------------------------------------------------- the file
def _chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def png_bytes(rows, width: int, height: int, level: int = 6) -> bytes:
    """One PNG file: the signature, ``IHDR`` (8-bit, colour type 2, no interlace), one ``IDAT`` holding ``zlib.compress(rows, level)`` and ``IEND``;
    CRCs from ``zlib.crc32``.  ``rows``: the ``height * (1 + 3 * width)`` bytes of ``filter_rows`` for one image (bytes, a uint8 array or tensor)."""
    if isinstance(rows, torch.Tensor):
        rows = rows.detach().cpu().contiguous().numpy()
    data = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1) if isinstance(rows, np.ndarray) else np.frombuffer(rows, np.uint8)
    if len(data) != height * (1 + 3 * width):
        raise ValueError(f"png_bytes: {len(data)} bytes of rows, {height} x (1 + 3 x {width}) expected")
    return b"".join([_PNG_MAGIC, _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)), _chunk(b"IDAT", zlib.compress(data, level)),
                     _chunk(b"IEND", b"")])


def _to_host(rows: torch.Tensor) -> np.ndarray:
    """the whole stream buffer on the host: one device-to-host copy through pinned memory"""
    if not rows.is_cuda:
        return rows.numpy()
    host = torch.empty(rows.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(rows, non_blocking=True)
    torch.cuda.current_stream(rows.device).synchronize()
    return host.numpy()


def _write_all(paths: List[str], rows: np.ndarray, width: int, height: int, level: int) -> None:
    """deflate and write every stream on at most MAX_WRITERS threads; returns when every file is closed"""
    def one(i: int) -> None:
        data = png_bytes(rows[i], width, height, level)
        with open(paths[i], "wb") as f:
            f.write(data)
    if len(paths) == 1:
        one(0)
        return
    with ThreadPoolExecutor(max_workers=min(MAX_WRITERS, len(paths))) as pool:
        list(pool.map(one, range(len(paths))))                          # (list: re-raises a worker's exception)


def _flat_images(t, S: int, V: int, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() != 5 or tuple(t.shape[:2]) != (S, V):
        raise ValueError(f"write_views: {what} must be ({S}, {V}, h, w, 3), got {tuple(getattr(t, 'shape', ()))}")
    return t.reshape(S * V, *t.shape[2:])


def write_views(viz_dir: str, scene_names: Sequence[str], pred: torch.Tensor, target: Optional[torch.Tensor] = None, img_paths=None, metrics=None,
                level: int = 6) -> List[str]:
    """The test views of a batch as PNG files under ``viz_dir`` -> their paths, scene by scene.  ``pred`` (and ``target``, which then stands on the
    left of every file): (S, V, h, w, 3), float32 or uint8, by the byte rules of ``filter_rows``.

    File names are the reference's: without ``img_paths`` ``scene_<name>_{:03d}.png`` by view number; with ``img_paths`` (S lists of V paths) and
    ``metrics`` (a dict of (S, V) tensors ``psnr``, ``ssim`` and optionally ``lpips``: ``extra['test_metrics']`` of ``val_step``)
    ``scene_<name>_<stem>_psnr{:02.1f}_ssim{:.2f}_lpips{:.3f}.png`` -- a missing LPIPS formats as ``nan`` -- after every file matching
    ``scene_<name>_<stem>*.png`` has been removed (the name is matched literally, never as a pattern).

    One launch, one device-to-host copy of all streams through pinned memory, one copy for all scores; then at most 16 threads deflate (``level``)
    and write.  Returns when every file is closed."""
    if not isinstance(pred, torch.Tensor) or pred.dim() != 5:
        raise ValueError(f"write_views: pred must be (S, V, h, w, 3), got {tuple(getattr(pred, 'shape', ()))}")
    S, V, h, w, _ = pred.shape
    scene_names = list(scene_names)
    if len(scene_names) != S:
        raise ValueError(f"write_views: {len(scene_names)} scene names for {S} scenes")
    rows = filter_rows(_flat_images(pred, S, V, "pred"), None if target is None else _flat_images(target, S, V, "target"))
    os.makedirs(viz_dir, exist_ok=True)
    paths = []
    if img_paths is None:
        paths = [os.path.join(viz_dir, "scene_" + name + "_{:03d}.png".format(v)) for name in scene_names for v in range(V)]
    else:
        if metrics is None or "psnr" not in metrics or "ssim" not in metrics:
            raise ValueError("write_views: img_paths name the files after the views' scores, so metrics with 'psnr' and 'ssim' are needed")
        if len(img_paths) != S or any(len(p) != V for p in img_paths):
            raise ValueError(f"write_views: img_paths must be {S} lists of {V} paths")
        keys = ["psnr", "ssim"] + (["lpips"] if metrics.get("lpips") is not None else [])
        table = torch.stack([torch.as_tensor(metrics[k]).detach().to(torch.float32).reshape(S, V) for k in keys], dim=0).cpu().tolist()   # one copy
        # what the reference removes with glob(base + '*.png') per view, from ONE directory listing: a view's stale files are the sorted names
        # from `base` on that start with it (a literal prefix: nothing in a scene name is a pattern)
        present = sorted(f for f in os.listdir(viz_dir) if f.endswith(".png") and not f.startswith("."))
        for s, name in enumerate(scene_names):
            for v in range(V):
                base = "scene_" + name + "_" + os.path.splitext(os.path.basename(img_paths[s][v]))[0]
                i = bisect.bisect_left(present, base)
                while i < len(present) and present[i].startswith(base):
                    if os.path.exists(os.path.join(viz_dir, present[i])):            # (one view's base may be a prefix of another's)
                        os.remove(os.path.join(viz_dir, present[i]))
                    i += 1
                lpips = table[2][s][v] if len(keys) == 3 else float("nan")
                paths.append(os.path.join(viz_dir, base + "_psnr{:02.1f}_ssim{:.2f}_lpips{:.3f}.png".format(table[0][s][v], table[1][s][v], lpips)))
    _write_all(paths, _to_host(rows), w if target is None else 2 * w, h, level)
    return paths


def write_code_planes(viz_dir: str, code: torch.Tensor, scene_names: Sequence[str], code_range: Sequence[float] = (-1, 1), flip_z: bool = False,
                      level: int = 6) -> List[str]:
    """``scene_<name>.png`` per scene: the three code planes of ``code`` (S, 3, C, h, w) as one viridis image of 3 h rows and C w columns
    (``code_plane_rgb``), filtered and written like the views."""
    scene_names = list(scene_names)
    if len(scene_names) != code.size(0):
        raise ValueError(f"write_code_planes: {len(scene_names)} scene names for {code.size(0)} scenes")
    rgb = code_plane_rgb(code, code_range, flip_z)
    rows = filter_rows(rgb)
    os.makedirs(viz_dir, exist_ok=True)
    paths = [os.path.join(viz_dir, "scene_" + name + ".png") for name in scene_names]
    _write_all(paths, _to_host(rows), rgb.size(2), rgb.size(1), level)
    return paths
