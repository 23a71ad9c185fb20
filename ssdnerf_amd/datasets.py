"""The reference's dataset (lib/datasets/shapenet_srn.py) and its loader, on a device-resident image store.

Four layers:

``ShapeNetSRN``   reads a folder tree in the SRN layout (``<prefix>/<scene>/{intrinsics.txt, rgb/*.png, pose/*.txt}``) with the reference's
                  constructor keywords and defaults; ``ds[i]`` is the reference's per-scene dict with CPU tensors (no GPU, no library).
``SceneStore``    every pixel of a dataset as ONE uint8 tensor (num_images, h, w, 3) -- on the GPU (``store='device'``) or in pinned host
                  memory (``store='host'``) -- and ``gather(image_indices)``: the fp32 views of a batch from one launch of
                  ``ssdnerf_gather_views_u8`` (csrc/scene_store.hip), bit-identical to the reference's ``img.astype(np.float32) / 255``.
``StoredViews``   the conditioning views of a batch left IN the store (``build_dataloader(..., cond_imgs='stored')``): ``sample(inds)`` gives the
                  rays and target colours of sampled pixels from one launch of ``ssdnerf_sample_rays_u8``, ``dense()`` the arrays themselves.
``SceneLoader``   an in-process iterable of batch dicts with exactly the keys ``train_step`` / ``val_step`` / ``evaluate_3d`` read, in the
                  reference's scene order (``parallel.shard_scenes`` for evaluation, lib/datasets/samplers/distributed_sampler.py for
                  training).  No worker processes and no per-iteration host traffic beyond a few hundred index bytes.

There is no fallback: a ``SceneStore`` without a HIP device raises."""
from __future__ import annotations

import hashlib
import json
import math
import os
import pickle
import random
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import parallel
from .registry import DATASETS

DECODE_THREADS = 16          # PNG decoders in flight at most (never sized by os.cpu_count(): a shared machine shows all of its CPUs)
_UPLOAD_CHUNK = 1 << 28      # bytes per host -> device copy while a store is filled


# ---------------------------------------------------------------------------------------------- scene folders
def load_intrinsics(path: str) -> Tuple[float, float, float, float, int, int]:
    """``intrinsics.txt``: line 1 ``f cx cy _``, line 4 ``height width`` -> (fx, fy, cx, cy, h, w) with fx = fy = f"""
    with open(path, "r") as f:
        lines = [f.readline() for _ in range(4)]
    focal, cx, cy, _ = map(float, lines[0].split())
    height, width = map(int, lines[3].split())
    return focal, focal, cx, cy, height, width


def load_pose(path: str) -> torch.Tensor:
    """a camera-to-world matrix: 16 numbers read as float32, (4, 4)"""
    with open(path, "r") as f:
        values = np.array(f.read().split(), dtype=np.float32)
    if values.size != 16:
        raise ValueError(f"{path}: {values.size} numbers, a pose has 16")
    return torch.from_numpy(values.reshape(4, 4))


# ---------------------------------------------------------------------------------------------- PNG
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def decode_png(data: bytes, name: str = "<bytes>") -> np.ndarray:
    """The built-in reader: 8-bit, non-interlaced, colour type 2 (RGB) or 6 (RGBA, alpha dropped without compositing) -> (h, w, 3) uint8,
    all five row filters, on the standard library's zlib.  Anything else raises ``ValueError`` naming the file."""
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f"{name}: not a PNG file")
    pos, header, idat = 8, None, []
    while pos + 8 <= len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + length]
        if len(body) != length:
            raise ValueError(f"{name}: truncated {kind!r} chunk")
        pos += 12 + length
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if header is None:
        raise ValueError(f"{name}: no IHDR chunk")
    w, h, depth, colour, compression, filtering, interlace = header
    if depth != 8 or colour not in (2, 6) or interlace != 0 or compression != 0 or filtering != 0:
        raise ValueError(f"{name}: the built-in PNG reader takes 8-bit non-interlaced RGB / RGBA only, this file has bit depth {depth}, colour type "
                         f"{colour}, interlace {interlace} (install Pillow for anything else)")
    bpp = 3 if colour == 2 else 4
    stride = w * bpp
    try:
        raw = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise ValueError(f"{name}: {e}") from e
    if len(raw) != h * (stride + 1):
        raise ValueError(f"{name}: {len(raw)} bytes of image data, {h} rows of {stride} + 1 expected")
    rows = np.frombuffer(raw, np.uint8).reshape(h, stride + 1)
    out = np.empty((h, stride), np.uint8)
    zero = np.zeros(stride, np.uint8)
    for y in range(h):
        kind, line = int(rows[y, 0]), rows[y, 1:]
        up = out[y - 1] if y else zero
        if kind == 0:
            out[y] = line
        elif kind == 1:                                                 # Sub: a running sum per channel, modulo 256
            out[y] = np.cumsum(line.reshape(w, bpp), axis=0, dtype=np.uint8).reshape(stride)
        elif kind == 2:                                                 # Up
            out[y] = line + up
        elif kind in (3, 4):                                            # Average / Paeth: each byte needs its left neighbour's RESULT
            cur, above, src = bytearray(stride), up.tolist(), line.tolist()
            for i in range(stride):
                a = cur[i - bpp] if i >= bpp else 0
                b = above[i]
                if kind == 3:
                    pred = (a + b) >> 1
                else:
                    c = above[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[i] = (src[i] + pred) & 0xFF
            out[y] = np.frombuffer(bytes(cur), np.uint8)
        else:
            raise ValueError(f"{name}: row {y} has filter type {kind}")
    return np.ascontiguousarray(out.reshape(h, w, bpp)[:, :, :3])


_PIL_FOUND: Optional[bool] = None


def _have_pil() -> bool:
    """whether Pillow imports: found out once (a failed import searches the whole path, and a dataset has 123 000 images)"""
    global _PIL_FOUND
    if _PIL_FOUND is None:
        try:
            import PIL.Image  # noqa: F401
            _PIL_FOUND = True
        except Exception:                                                # noqa: BLE001
            _PIL_FOUND = False
    return _PIL_FOUND


def read_image(path: str) -> np.ndarray:
    """(h, w, 3) uint8 RGB, as ``mmcv.imread(path, channel_order='rgb')`` gives it: Pillow where it imports, the built-in reader otherwise"""
    if _have_pil():
        import PIL.Image
        with PIL.Image.open(path) as im:
            return np.asarray(im.convert("RGB"), dtype=np.uint8)
    with open(path, "rb") as f:
        return decode_png(f.read(), path)


def _paths_key(paths: Sequence[str]) -> str:
    return hashlib.sha256("\n".join(paths).encode()).hexdigest()


# ---------------------------------------------------------------------------------------------- dataset
def _normalise_pose(c2w: torch.Tensor, center: torch.Tensor, radius: torch.Tensor) -> torch.Tensor:
    """rotation kept, translation (t - center) / radius, last row 0 0 0 1 (float32 torch, as the reference forms it)"""
    c2w = torch.as_tensor(c2w, dtype=torch.float32)
    top = torch.cat([c2w[:3, :3], (c2w[:3, 3:] - center[:, None]) / radius[:, None]], dim=-1)
    return torch.cat([top, top.new_tensor([[0.0, 0.0, 0.0, 1.0]])], dim=-2)


@DATASETS.register_module()
class ShapeNetSRN(torch.utils.data.Dataset):
    """lib/datasets/shapenet_srn.py's ``ShapeNetSRN``: the same keywords, defaults, scene order, view selection and per-scene dict (plain values
    instead of mmcv ``DataContainer``s).  ``pixel_cache_path`` is new: see ``load_pixels``."""

    def __init__(self, data_prefix, code_dir=None, code_only=False, load_imgs=True, specific_observation_idcs=None, num_test_imgs=0,
                 random_test_imgs=False, scene_id_as_name=False, cache_path=None, test_pose_override=None, num_train_imgs=-1, load_cond_data=True,
                 load_test_data=True, max_num_scenes=-1, radius=0.5, test_mode=False, step=1, pixel_cache_path=None):
        super().__init__()
        self.data_prefix, self.code_dir, self.code_only, self.load_imgs = data_prefix, code_dir, code_only, load_imgs
        self.specific_observation_idcs, self.num_test_imgs, self.random_test_imgs = specific_observation_idcs, num_test_imgs, random_test_imgs
        self.scene_id_as_name, self.cache_path, self.test_pose_override = scene_id_as_name, cache_path, test_pose_override
        self.num_train_imgs, self.load_cond_data, self.load_test_data = num_train_imgs, load_cond_data, load_test_data
        self.max_num_scenes, self.step, self.test_mode, self.pixel_cache_path = max_num_scenes, step, test_mode, pixel_cache_path
        self.radius = torch.tensor([radius], dtype=torch.float32).expand(3)
        self.center = torch.zeros_like(self.radius)
        self.load_scenes()
        self.test_poses = self.test_intrinsics = None
        if test_pose_override is not None:
            pose_dir = os.path.join(test_pose_override, "pose")
            poses = [_normalise_pose(load_pose(os.path.join(pose_dir, name)), self.center, self.radius) for name in sorted(os.listdir(pose_dir))]
            self.test_poses = torch.stack(poses, dim=0)                                          # (n, 4, 4)
            fx, fy, cx, cy, _, _ = load_intrinsics(os.path.join(test_pose_override, "intrinsics.txt"))
            self.test_intrinsics = torch.tensor([fx, fy, cx, cy], dtype=torch.float32)[None].expand(self.test_poses.size(0), -1)

    # ------------------------------------------------------------------ the scene list
    def load_scenes(self) -> None:
        if self.cache_path is not None and os.path.exists(self.cache_path):
            with open(self.cache_path, "rb") as f:
                scenes = pickle.load(f)
        else:
            scenes = []
            for prefix in self.data_prefix if isinstance(self.data_prefix, list) else [self.data_prefix]:
                for name in os.listdir(prefix):
                    scene_dir = os.path.join(prefix, name)
                    if not os.path.isdir(scene_dir):
                        continue
                    image_dir = os.path.join(scene_dir, "rgb")
                    image_names = sorted(os.listdir(image_dir))
                    scenes.append(dict(
                        intrinsics=load_intrinsics(os.path.join(scene_dir, "intrinsics.txt")),
                        image_paths=[os.path.join(image_dir, n) for n in image_names],
                        poses=[load_pose(os.path.join(scene_dir, "pose/" + os.path.splitext(n)[0] + ".txt")) for n in image_names]))
            scenes = sorted(scenes, key=lambda s: s["image_paths"][0].split("/")[-3])
            if self.cache_path is not None:
                with open(self.cache_path, "wb") as f:
                    pickle.dump(scenes, f, protocol=2)                   # mmcv.dump's protocol: the reference reads this file too
        end = len(scenes)
        if self.max_num_scenes >= 0:
            end = min(end, self.max_num_scenes * self.step)
        self.scenes = scenes[:end:self.step]
        self.num_scenes = len(self.scenes)
        # flat image numbering over the scenes in order: image j of scene i is number image_offsets[i] + j (SceneStore, SceneLoader)
        counts = [len(s["image_paths"]) for s in self.scenes]
        self.image_offsets = [0] + np.cumsum(counts, dtype=np.int64).tolist()
        self.image_paths = [p for s in self.scenes for p in s["image_paths"]]
        flat = [_normalise_pose(p, self.center, self.radius) for s in self.scenes for p in s["poses"]]
        self.poses = torch.stack(flat, dim=0) if flat else torch.zeros(0, 4, 4)                  # (num_images, 4, 4), normalised
        self.intrinsics = torch.tensor([list(s["intrinsics"][:4]) for s in self.scenes], dtype=torch.float32).reshape(-1, 4)

    def __len__(self) -> int:
        return self.num_scenes

    def scene_name(self, scene_id: int) -> str:
        return self.scenes[scene_id]["image_paths"][0].split("/")[-3]

    def select_views(self, scene_id: int) -> Tuple[List[int], List[int]]:
        """(conditioning views, test views) of a scene; with ``random_test_imgs`` a fresh ``random.sample`` per call, as in the reference"""
        num_imgs = len(self.scenes[scene_id]["image_paths"])
        if self.specific_observation_idcs is None:
            num_train = self.num_train_imgs if self.num_train_imgs >= 0 else num_imgs - self.num_test_imgs
            if self.random_test_imgs:
                cond = random.sample(range(num_imgs), num_train)
            else:
                cond = np.round(np.linspace(0, num_imgs - 1, num_train)).astype(np.int64).tolist()
        else:
            cond = [int(i) for i in self.specific_observation_idcs]
        test = list(range(num_imgs))
        for i in cond:
            test.remove(i)
        return cond, test

    def scene_record(self, scene_id: int) -> Dict:
        """Everything of ``ds[scene_id]`` except the pixels, plus ``cond_ids`` / ``test_ids`` (the FLAT image numbers of the selected views): what ``__getitem__`` and ``SceneLoader`` share, so that both follow one statement of the reference's key rules."""
        scene_id = int(scene_id)
        name = self.scene_name(scene_id)
        rec = dict(scene_id=scene_id, scene_name="{:04d}".format(scene_id) if self.scene_id_as_name else name)
        if not self.code_only:
            paths, first = self.scenes[scene_id]["image_paths"], self.image_offsets[scene_id]
            cond, test = self.select_views(scene_id)
            for key, ids, wanted in (("cond", cond, self.load_cond_data), ("test", test, self.load_test_data)):
                if wanted and len(ids) > 0:
                    flat = [first + i for i in ids]
                    rec[key + "_poses"] = self.poses[flat]
                    rec[key + "_intrinsics"] = self.intrinsics[scene_id][None].expand(len(ids), -1)
                    rec[key + "_img_paths"] = [paths[i] for i in ids]
                    rec[key + "_ids"] = flat
        if self.code_dir is not None:
            code_file = os.path.join(self.code_dir, name + ".pth")
            if os.path.exists(code_file):
                rec["code"] = torch.load(code_file, map_location="cpu")
        if self.test_pose_override is not None:
            rec.update(test_poses=self.test_poses, test_intrinsics=self.test_intrinsics)
        return rec

    def __getitem__(self, scene_id: int) -> Dict:
        rec = self.scene_record(scene_id)
        for key in ("cond", "test"):
            ids = rec.pop(key + "_ids", None)
            if ids is not None and self.load_imgs:
                imgs = [torch.from_numpy(read_image(self.image_paths[i]).astype(np.float32) / 255) for i in ids]
                rec[key + "_imgs"] = torch.stack(imgs, dim=0)                                    # (n, h, w, 3)
        return rec

    # ------------------------------------------------------------------ all pixels
    def load_pixels(self) -> np.ndarray:
        """Every image of the dataset, decoded: (num_images, h, w, 3) uint8 in flat image order.  With ``pixel_cache_path`` the array is one
        ``.npy`` written after the first decode and memory-mapped afterwards; beside it ``<pixel_cache_path>.key.json`` holds a hash of the image
        path list, and a file whose key does not match this dataset's list (or whose shape does not) is rebuilt.  At most ``DECODE_THREADS``
        decoders run at a time.  Views of different sizes raise ``ValueError``."""
        paths = self.image_paths
        if not paths:
            raise ValueError("ShapeNetSRN.load_pixels: the dataset has no images")
        key = _paths_key(paths)
        cache = self.pixel_cache_path
        if cache is not None and os.path.exists(cache) and os.path.exists(cache + ".key.json"):
            try:
                with open(cache + ".key.json") as f:
                    meta = json.load(f)
                if meta.get("sha256") == key:
                    arr = np.load(cache, mmap_mode="r")
                    if arr.dtype == np.uint8 and arr.ndim == 4 and arr.shape[0] == len(paths) and arr.shape[3] == 3:
                        return arr
            except (OSError, ValueError):
                pass                                                     # unreadable: rebuild
        first = read_image(paths[0])
        shape = (len(paths),) + first.shape
        if cache is not None:
            tmp = cache + ".tmp.npy"
            arr = np.lib.format.open_memmap(tmp, mode="w+", dtype=np.uint8, shape=shape)
        else:
            arr = np.empty(shape, np.uint8)
        arr[0] = first

        def decode(i: int) -> None:
            img = read_image(paths[i])
            if img.shape != first.shape:
                raise ValueError(f"ShapeNetSRN: views of different sizes in one dataset: {paths[i]} is {img.shape[0]} x {img.shape[1]}, "
                                 f"{paths[0]} is {first.shape[0]} x {first.shape[1]}")
            arr[i] = img

        try:
            with ThreadPoolExecutor(max_workers=DECODE_THREADS) as pool:
                for _ in pool.map(decode, range(1, len(paths)), chunksize=1):
                    pass
        except BaseException:
            if cache is not None:
                del arr
                os.remove(tmp)
            raise
        if cache is None:
            return arr
        arr.flush()
        del arr
        os.replace(tmp, cache)
        with open(cache + ".key.json", "w") as f:
            json.dump(dict(sha256=key, num_images=len(paths), shape=list(shape)), f)
        return np.load(cache, mmap_mode="r")


# ---------------------------------------------------------------------------------------------- the image store
class SceneStore:
    """The pixels of a dataset as one uint8 tensor ``pixels`` (num_images, h, w, 3) and ``offsets`` (first image of every scene, one past the
    last at the end).  ``store='device'``: on the GPU.  ``store='host'``: in pinned host memory; ``gather`` then copies the batch's images --
    one ``non_blocking`` copy per run of consecutive indices -- into a device staging buffer and runs the same kernel on that.  The staging
    buffer is reused from call to call: an event recorded behind every kernel is waited for (on the device, not by the host) by the stream of
    the next call before its first copy, so a buffer is never overwritten under a kernel that still reads it, on whichever stream that ran.

    ``source``: a ``ShapeNetSRN`` (its ``load_pixels()`` and ``image_offsets``) or a uint8 array / tensor (num_images, h, w, 3)."""

    def __init__(self, source, store: str = "device", device=None, offsets: Optional[Sequence[int]] = None):
        if store not in ("device", "host"):
            raise ValueError(f"SceneStore: store must be 'device' or 'host', got {store!r}")
        if not torch.cuda.is_available():
            raise RuntimeError("SceneStore needs a HIP device (there is no CPU path; ShapeNetSRN's ds[i] is the host layer)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"SceneStore needs a HIP device, got {self.device} (there is no CPU path)")
        if isinstance(source, ShapeNetSRN):
            pixels, offsets = source.load_pixels(), source.image_offsets
        else:
            pixels = source
        if isinstance(pixels, torch.Tensor):
            if pixels.dtype != torch.uint8 or pixels.dim() != 4 or pixels.size(3) != 3:
                raise ValueError(f"SceneStore: pixels must be uint8 (num_images, h, w, 3), got {pixels.dtype} {tuple(pixels.shape)}")
        elif pixels.dtype != np.uint8 or pixels.ndim != 4 or pixels.shape[3] != 3:
            raise ValueError(f"SceneStore: pixels must be uint8 (num_images, h, w, 3), got {pixels.dtype} {tuple(pixels.shape)}")
        if pixels.shape[0] == 0 or pixels.shape[1] * pixels.shape[2] == 0:
            raise ValueError(f"SceneStore: an empty store {tuple(pixels.shape)}")
        self.store = store
        self.shape = tuple(int(v) for v in pixels.shape)
        self.num_images, self.image_bytes = self.shape[0], self.shape[1] * self.shape[2] * 3
        self.offsets = list(offsets) if offsets is not None else [0, self.num_images]
        target = dict(device=self.device) if store == "device" else dict(pin_memory=True)
        self.pixels = torch.empty(self.shape, dtype=torch.uint8, **target)
        step = max(1, _UPLOAD_CHUNK // self.image_bytes)
        for a in range(0, self.num_images, step):                        # in pieces: `pixels` may be a memory-mapped file of several GB
            part = pixels[a:a + step]
            part = part if isinstance(part, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(part))
            self.pixels[a:a + step].copy_(part)
        self._staging: Optional[torch.Tensor] = None
        self._staging_free: Optional[torch.cuda.Event] = None

    def _check_indices(self, image_indices, what: str = "SceneStore.gather") -> np.ndarray:
        if isinstance(image_indices, torch.Tensor):
            if image_indices.is_cuda:
                raise ValueError(f"{what}: the indices must be on the host (they are validated before they are uploaded)")
            image_indices = image_indices.numpy()
        idx = np.asarray(image_indices)
        if idx.ndim != 1 or idx.size == 0:
            raise ValueError(f"{what}: a non-empty 1-D list of image indices is needed, got shape {idx.shape}")
        if idx.dtype.kind not in "iu":
            raise ValueError(f"{what}: integer indices are needed, got {idx.dtype}")
        if int(idx.min()) < 0 or int(idx.max()) >= self.num_images:
            bad = idx[(idx < 0) | (idx >= self.num_images)][0]
            raise ValueError(f"{what}: image index {int(bad)} is outside [0, {self.num_images})")
        return idx.astype(np.int64)

    def gather(self, image_indices) -> torch.Tensor:
        """fp32 (len, h, w, 3) on the device: ``pixels[i].float() / 255`` for every i of the HOST list ``image_indices``, from one library call.
        An index outside [0, num_images) raises ``ValueError`` before anything is uploaded."""
        from . import _cabi as C
        idx = self._check_indices(image_indices)
        n = int(idx.size)
        with torch.cuda.device(self.device):
            out = torch.empty((n,) + self.shape[1:], dtype=torch.float32, device=self.device)
            if self.store == "device":
                src, num = self.pixels, self.num_images
                index = torch.from_numpy(idx.astype(np.int32)).to(self.device)
            else:
                stream = torch.cuda.current_stream()
                if self._staging_free is not None:
                    stream.wait_event(self._staging_free)                # the kernel of the previous call has read the buffer
                if self._staging is None or self._staging.size(0) < n:
                    self._staging = torch.empty((n,) + self.shape[1:], dtype=torch.uint8, device=self.device)
                a = 0
                while a < n:                                             # one copy per run of consecutive images
                    b = a + 1
                    while b < n and idx[b] == idx[b - 1] + 1:
                        b += 1
                    self._staging[a:b].copy_(self.pixels[int(idx[a]):int(idx[a]) + (b - a)], non_blocking=True)
                    a = b
                src, num = self._staging, n
                index = torch.arange(n, dtype=torch.int32, device=self.device)
            C.check(C.lib().ssdnerf_gather_views_u8(C.ptr(src), self.image_bytes, num, C.ptr(index), n, C.ptr(out), C.stream()), "gather_views_u8")
            if self.store == "host":
                self._staging_free = torch.cuda.Event()
                self._staging_free.record(stream)
        return out


class StoredViews:
    """The conditioning views of a batch, left where they are: ``store`` (a device ``SceneStore``), the (S, V) table ``view_image`` of store image
    numbers -- a HOST array, validated against the store before anything is uploaded -- and the views' cameras ``poses`` (S, V, 4, 4) /
    ``intrinsics`` (S, V, 4) on the store's device.  It stands where the fp32 ``cond_imgs`` (S, V, h, w, 3) of a batch stands (``shape``,
    ``size``, ``device``, ``dtype`` answer as that tensor would) and gives the fitting code what it reads from it:

    ``sample(inds)``  (rays_o, rays_d, target), each (S, R, 3): pixels ``inds`` (S, R) int64 on the device -- or every pixel, ``None`` -- with
                      their rays, from ONE launch of ``ssdnerf_sample_rays_u8`` (csrc/scene_store.hip), bit for bit what indexing the dense
                      arrays gives.  An index outside [0, V*h*w) gives a NaN ray.
    ``sample_permuted(seed, draw, start, count)``  the same three arrays for the pixels at positions start .. start + count - 1 of a keyed permutation
                      that the kernel evaluates itself (``ssdnerf_sample_rays_perm_u8``): no index tensor exists.
    ``dense()``       (images, rays_o, rays_d), each (S, V, h, w, 3): the arrays themselves, by ``SceneStore.gather`` and ``nerf.get_cam_rays``,
                      built on the first call and kept -- for consumers that need whole images.

    ``sample_launches`` counts the calls of ``sample`` and ``sample_permuted``; ``dense_calls`` the times the dense arrays were built (0 or 1)."""

    dtype = torch.float32

    def __init__(self, store: SceneStore, view_image, poses: torch.Tensor, intrinsics: torch.Tensor):
        if not isinstance(store, SceneStore) or store.store != "device":
            raise ValueError("StoredViews: a SceneStore with store='device' is needed (sampling from the pinned host store is not implemented)")
        if isinstance(view_image, torch.Tensor):
            if view_image.is_cuda:
                raise ValueError("StoredViews: view_image must be on the host (it is validated before it is uploaded)")
            view_image = view_image.numpy()
        table = np.asarray(view_image)
        if table.ndim != 2:
            raise ValueError(f"StoredViews: view_image must be (scenes, views), got shape {table.shape}")
        self.view_image = store._check_indices(table.reshape(-1), "StoredViews").reshape(table.shape)
        S, V = self.view_image.shape
        h, w = store.shape[1:3]
        if V * h * w >= 1 << 32:
            raise ValueError(f"StoredViews: {V} views of {h} x {w} are 2^32 pixels per scene or more")
        if tuple(poses.shape) != (S, V, 4, 4) or tuple(intrinsics.shape) != (S, V, 4):
            raise ValueError(f"StoredViews: poses {tuple(poses.shape)} / intrinsics {tuple(intrinsics.shape)} do not fit a ({S}, {V}) view table")
        self.store = store
        self.poses = poses.detach().to(device=store.device, dtype=torch.float32).contiguous()
        self.intrinsics = intrinsics.detach().to(device=store.device, dtype=torch.float32).contiguous()
        self.device = self.poses.device
        self.view_image_dev = torch.from_numpy(self.view_image.astype(np.int32)).to(self.device)
        self.shape = torch.Size((S, V, h, w, 3))
        self.sample_launches = self.dense_calls = 0
        self._dense: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None

    def size(self, dim: Optional[int] = None):
        return self.shape if dim is None else self.shape[dim]

    def sample(self, inds: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        from . import _cabi as C
        S, V, h, w, _ = self.shape
        if inds is None:
            R = V * h * w
        else:
            if inds.dtype != torch.int64 or inds.dim() != 2 or inds.size(0) != S or inds.device != self.poses.device:
                raise ValueError(f"StoredViews.sample: inds must be int64 ({S}, R) on {self.device}, got {inds.dtype} {tuple(inds.shape)} on {inds.device}")
            inds, R = inds.contiguous(), inds.size(1)
        with torch.cuda.device(self.device):
            rays_o, rays_d, target = (torch.empty((S, R, 3), dtype=torch.float32, device=self.device) for _ in range(3))
            C.check(C.lib().ssdnerf_sample_rays_u8(C.ptr(self.store.pixels), self.store.num_images, h, w, C.ptr(self.view_image_dev), C.ptr(self.poses),
                                                   C.ptr(self.intrinsics), S, V, C.ptr(inds), R, C.ptr(rays_o), C.ptr(rays_d), C.ptr(target),
                                                   C.stream()), "sample_rays_u8")
        self.sample_launches += 1
        return rays_o, rays_d, target

    def sample_permuted(self, seed: int, draw: int, start: int, count: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``sample`` without an index tensor: ray r of scene s is pixel pi(seed, s, draw, V*h*w)(start + r) of the keyed permutation of
        csrc/keyed_perm.h, r < ``count``, evaluated inside ONE launch of ``ssdnerf_sample_rays_perm_u8`` -- bit for bit what ``sample`` gives on the
        indices ``ssdnerf_perm_indices`` writes for the same arguments.  ``start + count`` may not pass V*h*w."""
        from . import _cabi as C
        S, V, h, w, _ = self.shape
        seed, draw, start, count = int(seed), int(draw), int(start), int(count)
        if not (0 <= seed < 1 << 64 and 0 <= draw < 1 << 32):
            raise ValueError(f"StoredViews.sample_permuted: seed must fit 64 bits and draw 32, got {seed} and {draw}")
        if not (start >= 0 and count > 0 and start + count <= V * h * w):
            raise ValueError(f"StoredViews.sample_permuted: positions [{start}, {start} + {count}) leave the {V * h * w} pixels of a scene")
        with torch.cuda.device(self.device):
            rays_o, rays_d, target = (torch.empty((S, count, 3), dtype=torch.float32, device=self.device) for _ in range(3))
            C.check(C.lib().ssdnerf_sample_rays_perm_u8(C.ptr(self.store.pixels), self.store.num_images, h, w, C.ptr(self.view_image_dev), C.ptr(self.poses),
                                                        C.ptr(self.intrinsics), S, V, seed, draw, start, count, C.ptr(rays_o), C.ptr(rays_d),
                                                        C.ptr(target), C.stream()), "sample_rays_perm_u8")
        self.sample_launches += 1
        return rays_o, rays_d, target

    def dense(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        if self._dense is None:
            from . import nerf
            images = self.store.gather(self.view_image.reshape(-1)).view(self.shape)
            rays_o, rays_d = nerf.get_cam_rays(self.poses, self.intrinsics, self.shape[2], self.shape[3])
            self._dense = (images, rays_o, rays_d)
            self.dense_calls += 1
        return self._dense


# ---------------------------------------------------------------------------------------------- the loader
def _wrap_pad(indices: List[int], length: int) -> List[int]:
    """the list padded to ``length`` with its own front (the sampler's `indices += indices[:total - len]`; repeated when one wrap is not enough)"""
    out = list(indices)
    while indices and len(out) < length:
        out += indices[:length - len(out)]
    return out


class SceneLoader:
    """Batches of a ``ShapeNetSRN`` for one rank, assembled in this process (``build_dataloader``).  ``scene_indices(epoch)`` is the host list of
    scene ids of an epoch, pure Python; iterating cuts it into batches of ``samples_per_gpu`` and fills each from the ``SceneStore``."""

    def __init__(self, dataset: ShapeNetSRN, samples_per_gpu: int, shuffle: bool = False, split_data: bool = False, seed: int = 0,
                 rank: Optional[int] = None, world_size: Optional[int] = None, store: str = "device", device=None, cond_imgs: str = "dense"):
        if samples_per_gpu < 1:
            raise ValueError(f"samples_per_gpu must be at least 1, got {samples_per_gpu}")
        if cond_imgs not in ("dense", "stored"):
            raise ValueError(f"cond_imgs must be 'dense' or 'stored', got {cond_imgs!r}")
        if cond_imgs == "stored" and store != "device":
            raise ValueError(f"cond_imgs='stored' samples rays from the device store; store={store!r} keeps the pixels in host memory")
        if rank is None or world_size is None:
            import torch.distributed as dist
            on = dist.is_available() and dist.is_initialized()
            rank = (dist.get_rank() if on else 0) if rank is None else rank
            world_size = (dist.get_world_size() if on else 1) if world_size is None else world_size
        if not 0 <= rank < world_size:
            raise ValueError(f"rank {rank} is outside [0, {world_size})")
        self.dataset, self.samples_per_gpu, self.shuffle, self.split_data, self.seed = dataset, int(samples_per_gpu), shuffle, split_data, seed
        self.rank, self.world_size, self.store_kind, self.device, self.cond_imgs = rank, world_size, store, device, cond_imgs
        self.epoch = 0
        self._store: Optional[SceneStore] = None
        self._dev: Optional[Dict[str, torch.Tensor]] = None

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def scene_indices(self, epoch: Optional[int] = None) -> List[int]:
        n, spg, ws = len(self.dataset), self.samples_per_gpu, self.world_size
        if not self.shuffle:
            return list(parallel.shard_scenes(n, self.rank, ws))
        g = torch.Generator()
        g.manual_seed(self.seed + (self.epoch if epoch is None else int(epoch)))
        if self.split_data and ws > 1:
            bounds = parallel.shard_bounds(n, ws)
            lo, hi = int(bounds[self.rank]), int(bounds[self.rank + 1])
            num_samples = max(math.ceil((int(bounds[r + 1]) - int(bounds[r])) / spg) for r in range(ws)) * spg
            return _wrap_pad((lo + torch.randperm(hi - lo, generator=g)).tolist(), num_samples)
        num_samples = math.ceil(n / ws / spg) * spg
        return _wrap_pad(torch.randperm(n, generator=g).tolist(), num_samples * ws)[self.rank:num_samples * ws:ws]

    def __len__(self) -> int:
        return math.ceil(len(self.scene_indices(0)) / self.samples_per_gpu)

    @property
    def scene_store(self) -> SceneStore:
        if self._store is None:
            self._store = SceneStore(self.dataset, store=self.store_kind, device=self.device)
        return self._store

    def _device_tables(self) -> Dict[str, torch.Tensor]:
        if self._dev is None:
            if not torch.cuda.is_available():
                raise RuntimeError("SceneLoader needs a HIP device to assemble batches (scene_indices() and the dataset's ds[i] need none)")
            ds = self.dataset
            device = torch.device("cuda", torch.cuda.current_device()) if self.device is None else torch.device(self.device)
            self._dev = dict(poses=ds.poses.to(device), intrinsics=ds.intrinsics.to(device))
            if ds.test_poses is not None:
                self._dev.update(test_poses=ds.test_poses.to(device), test_intrinsics=ds.test_intrinsics.contiguous().to(device))
        return self._dev

    def batch(self, scene_ids: Sequence[int]) -> Dict:
        """the batch dict of these scenes: lists for ``scene_id`` / ``scene_name`` / ``*_img_paths`` / ``code``, device tensors for the rest"""
        ds = self.dataset
        recs = [ds.scene_record(i) for i in scene_ids]
        out: Dict = dict(scene_id=[r["scene_id"] for r in recs], scene_name=[r["scene_name"] for r in recs])
        S = len(recs)
        for key in ("cond", "test"):
            have = [key + "_img_paths" in r for r in recs]
            if not any(have):
                continue
            counts = sorted({len(r.get(key + "_img_paths", ())) for r in recs})
            if len(counts) != 1:
                raise ValueError(f"SceneLoader: the scenes {list(scene_ids)} of one batch have different numbers of {key} views: {counts}")
            V, dev = counts[0], self._device_tables()
            flat = [i for r in recs for i in r[key + "_ids"]]
            where = torch.tensor(flat, dtype=torch.int64).to(dev["poses"].device)
            out[key + "_poses"] = dev["poses"][where].view(S, V, 4, 4)
            scene_where = torch.tensor(out["scene_id"], dtype=torch.int64).to(dev["poses"].device)
            out[key + "_intrinsics"] = dev["intrinsics"][scene_where][:, None].expand(S, V, 4).contiguous()
            out[key + "_img_paths"] = [r[key + "_img_paths"] for r in recs]
            if ds.load_imgs and key == "cond" and self.cond_imgs == "stored":       # the views stay in the store: no launch here
                out[key + "_imgs"] = StoredViews(self.scene_store, np.asarray(flat, dtype=np.int64).reshape(S, V), out[key + "_poses"],
                                                 out[key + "_intrinsics"])
            elif ds.load_imgs:
                out[key + "_imgs"] = self.scene_store.gather(flat).view(S, V, *self.scene_store.shape[1:])   # ONE launch per view group
        if all("code" in r for r in recs):
            out["code"] = [r["code"] for r in recs]
        if ds.test_pose_override is not None:
            dev = self._device_tables()
            n = dev["test_poses"].size(0)
            out["test_poses"] = dev["test_poses"][None].expand(S, n, 4, 4).contiguous()
            out["test_intrinsics"] = dev["test_intrinsics"][None].expand(S, n, 4).contiguous()
        return out

    def __iter__(self):
        order = self.scene_indices()
        for a in range(0, len(order), self.samples_per_gpu):
            yield self.batch(order[a:a + self.samples_per_gpu])


def build_dataset(cfg, default_args=None) -> ShapeNetSRN:
    """``mmgen.datasets.build_dataset``: pops ``type`` and builds from ``registry.DATASETS`` (``cfg.data.train`` / ``val_cond`` / ``val_uncond``)"""
    from .config import _plain
    return DATASETS.build(_plain(cfg), default_args)


def build_dataloader(dataset, samples_per_gpu, shuffle=False, split_data=False, seed=0, rank=None, world_size=None, store="device", device=None,
                     cond_imgs="dense") -> SceneLoader:
    """The loader of one rank.  ``shuffle=False`` (evaluation): this rank's ``parallel.shard_scenes`` range in order, ragged last batch, no padding.
    ``shuffle=True`` (training): the reference sampler's order (lib/datasets/samplers/distributed_sampler.py).
    ``cond_imgs='stored'``: the batches' ``cond_imgs`` is a ``StoredViews`` handle instead of the fp32 tensor."""
    return SceneLoader(dataset, samples_per_gpu, shuffle=shuffle, split_data=split_data, seed=seed, rank=rank, world_size=world_size, store=store,
                       device=device, cond_imgs=cond_imgs)
