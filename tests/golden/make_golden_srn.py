#!/usr/bin/env python
"""tests/golden/make_golden_srn.py -- the fixture of the dataset layer (ssdnerf_amd/datasets.py): a tiny folder tree in the SRN layout,
``srn_tiny/``, and what THE REFERENCE'S OWN ``ShapeNetSRN.parse_scene`` returns on it, ``srn_tiny.npz``, with a provenance note,
``srn_tiny_provenance.txt``.  Generated like make_golden_tv.py by executing the reference's Python in the build container (the fixture
travels, the reference does not).  Run from anywhere; the tree is addressed RELATIVE to this folder (``srn_tiny/cars``), so the recorded
image paths do not name a machine -- a test changes into this folder before it builds its dataset.

The tree (a few KB), written by the stdlib PNG writer below (``encode_png``):
    srn_tiny/cars/zeta_03, alpha_01, mid_02   created in this order, which is not the sorted one; 6, 6 and 4 views of 8 x 8
        intrinsics.txt                        f cx cy 0 / barycentre / scale / height width
        rgb/00000k.png                        RGB and RGBA files (alpha random: dropping it and compositing it differ); every row of a file
                                              has its own filter type, and every one of the five types occurs in every file
        pose/00000k.txt                       16 numbers, a camera on a sphere looking at the origin
    srn_tiny/spiral/{intrinsics.txt, pose/*.txt}   the ``test_pose_override`` folder, 3 poses

What runs for real (from the reference tree, unmodified): lib/datasets/shapenet_srn.py -- ``load_intrinsics``, ``load_pose``, ``ShapeNetSRN``
(``load_scenes``, ``parse_scene``).  What is substituted (not installable here): ``mmcv.imread(path, channel_order='rgb')`` by Pillow's
``Image.open(path).convert('RGB')``, ``mmcv.load`` / ``mmcv.dump`` by pickle, ``mmcv.parallel.DataContainer`` by a function that returns its
value, ``mmgen.datasets.builder.DATASETS`` by a registry that only records the class.

Fixture layout: ``sets_json`` maps a set's name to its constructor keywords (``SETS`` below: the keyword sets of the configs' ``train``,
``val_uncond`` and ``val_cond`` blocks with their view counts scaled to this tree, ``num_train_imgs=3``, ``random_test_imgs=True`` under
``random.seed(0)`` with the scenes parsed in order, ``code_only``); ``<set>/n`` is the number of scenes, ``<set>/<i>/__keys__`` the keys of
``parse_scene(i)`` and ``<set>/<i>/<key>`` each value (tensors as arrays, strings and path lists as unicode arrays).  ``pixels/<path>`` is
the (h, w, 3 or 4) uint8 array every PNG was written from.
"""
import importlib.util
import json
import os
import pickle
import random
import shutil
import struct
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("REF", "/root/reference")
TREE = "srn_tiny"
SCENES = [("zeta_03", 6), ("alpha_01", 6), ("mid_02", 4)]           # creation order
SIZE = 8
SETS = {
    "train": dict(),
    "val_uncond": dict(load_imgs=False, num_test_imgs=6, scene_id_as_name=True, step=2),
    "val_cond": dict(num_test_imgs=4, step=2),
    "val_cond_override": dict(specific_observation_idcs=[1], test_pose_override=TREE + "/spiral"),
    "num_train_3": dict(num_train_imgs=3),
    "random_test": dict(random_test_imgs=True, num_test_imgs=2),
    "code_only": dict(code_only=True),
}


# ---------------------------------------------------------------------------------------------- a PNG writer on zlib
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_row(kind, row, above, bpp):
    """one scanline (list of ints) under PNG filter ``kind`` (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth)"""
    out = []
    for i, x in enumerate(row):
        a = row[i - bpp] if i >= bpp else 0
        b = above[i]
        c = above[i - bpp] if i >= bpp else 0
        pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[kind]
        out.append((x - pred) & 0xFF)
    return out


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def encode_png(pixels, filters, bit_depth=8, interlace=0):
    """(h, w, 3 or 4) uint8 -> the bytes of a PNG whose row y uses filter type ``filters[y % len(filters)]``.  ``bit_depth`` / ``interlace``
    only set the header fields (for files a reader has to refuse)."""
    h, w, bpp = pixels.shape
    raw, above = bytearray(), [0] * (w * bpp)
    for y in range(h):
        row = pixels[y].reshape(-1).tolist()
        kind = filters[y % len(filters)]
        raw.append(kind)
        raw.extend(filter_row(kind, row, above, bpp))
        above = row
    header = struct.pack(">IIBBBBB", w, h, bit_depth, 2 if bpp == 3 else 6, 0, 0, interlace)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", header) + _chunk(b"IDAT", zlib.compress(bytes(raw), 9)) + _chunk(b"IEND", b"")


# ---------------------------------------------------------------------------------------------- the tree
def _look_at(eye):
    """camera-to-world with the camera at ``eye`` looking at the origin (z forward, y down: the SRN convention)"""
    z = -eye / np.linalg.norm(eye)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m


def _write_pose(path, m):
    with open(path, "w") as f:
        f.write(" ".join("%.9g" % v for v in m.reshape(-1)) + "\n")


def _write_intrinsics(path):
    with open(path, "w") as f:
        f.write("%.6f %.1f %.1f 0.\n0. 0. 0.\n1.\n%d %d\n" % (131.25 * SIZE / 128, SIZE / 2, SIZE / 2, SIZE, SIZE))


def write_tree(root):
    """writes ``root`` (removing an earlier one) and returns {relative png path: the pixels it was written from}"""
    if os.path.isdir(root):
        shutil.rmtree(root)
    g = np.random.default_rng(20240)
    pixels = {}
    n_img = 0
    for name, views in SCENES:
        scene = os.path.join(root, "cars", name)
        os.makedirs(os.path.join(scene, "rgb"))
        os.makedirs(os.path.join(scene, "pose"))
        _write_intrinsics(os.path.join(scene, "intrinsics.txt"))
        for k in range(views):
            bpp = 4 if n_img % 3 == 1 else 3
            yy, xx = np.mgrid[0:SIZE, 0:SIZE]
            smooth = (yy * 23 + xx * 11 + 40 * k)[..., None] + np.arange(bpp) * 50
            img = ((smooth + g.integers(0, 64, (SIZE, SIZE, bpp))) % 256).astype(np.uint8)
            if k == 0:
                img[0, 0, :3], img[-1, -1, :3] = 0, 255
            rel = "/".join([TREE, "cars", name, "rgb", "%06d.png" % k])
            with open(os.path.join(scene, "rgb", "%06d.png" % k), "wb") as f:
                f.write(encode_png(img, [(n_img + j) % 5 for j in range(5)]))
            pixels[rel] = img
            ang = 2 * np.pi * (k + 0.37 * n_img) / views
            eye = 1.3 * np.array([np.cos(ang) * np.cos(0.4), np.sin(ang) * np.cos(0.4), np.sin(0.4)])
            _write_pose(os.path.join(scene, "pose", "%06d.txt" % k), _look_at(eye))
            n_img += 1
    spiral = os.path.join(root, "spiral")
    os.makedirs(os.path.join(spiral, "pose"))
    _write_intrinsics(os.path.join(spiral, "intrinsics.txt"))
    for k in range(3):
        ang = 2 * np.pi * k / 3 + 0.2
        eye = 1.3 * np.array([np.cos(ang) * np.cos(0.6), np.sin(ang) * np.cos(0.6), np.sin(0.6)])
        _write_pose(os.path.join(spiral, "pose", "%06d.txt" % k), _look_at(eye))
    return pixels


# ---------------------------------------------------------------------------------------------- the reference, with mmcv / mmgen substituted
class _Registry:
    def __init__(self):
        self.module_dict = {}

    def register_module(self, name=None, module=None, force=False):
        def _register(cls):
            self.module_dict[name or cls.__name__] = cls
            return cls
        return _register if module is None else _register(module)


def _load_reference():
    import PIL.Image
    mods = {name: types.ModuleType(name) for name in ("mmcv", "mmcv.parallel", "mmgen", "mmgen.datasets", "mmgen.datasets.builder")}

    def imread(path, channel_order="bgr"):
        assert channel_order == "rgb"
        with PIL.Image.open(path) as im:
            return np.asarray(im.convert("RGB"), dtype=np.uint8)

    def load(path):
        with open(path, "rb") as f:
            return pickle.load(f)

    def dump(obj, path):
        with open(path, "wb") as f:
            pickle.dump(obj, f, protocol=2)

    mods["mmcv"].imread, mods["mmcv"].load, mods["mmcv"].dump = imread, load, dump
    mods["mmcv"].parallel = mods["mmcv.parallel"]
    mods["mmcv.parallel"].DataContainer = lambda value, **kwargs: value
    mods["mmgen.datasets.builder"].DATASETS = _Registry()
    sys.modules.update(mods)
    spec = importlib.util.spec_from_file_location("ref_shapenet_srn", os.path.join(REF, "lib", "datasets", "shapenet_srn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _record(arrays, prefix, result):
    import torch
    arrays[prefix + "/__keys__"] = np.array(sorted(result.keys()))
    for key, value in result.items():
        if isinstance(value, torch.Tensor):
            value = value.contiguous().numpy()
        arrays[prefix + "/" + key] = np.array(value)


def main():
    import PIL
    import torch
    assert os.path.isdir(REF), REF
    os.chdir(HERE)
    pixels = write_tree(TREE)
    ref = _load_reference()
    arrays = {"pixels/" + rel: img for rel, img in pixels.items()}
    for name, kwargs in SETS.items():
        random.seed(0)
        ds = ref.ShapeNetSRN(data_prefix=TREE + "/cars", **kwargs)
        arrays[name + "/n"] = np.int64(len(ds))
        for i in range(len(ds)):
            _record(arrays, "%s/%d" % (name, i), ds.parse_scene(i))
    arrays["sets_json"] = np.array(json.dumps(SETS))
    np.savez_compressed(os.path.join(HERE, "srn_tiny.npz"), **arrays)
    note = (f"srn_tiny/ and srn_tiny.npz: tests/golden/make_golden_srn.py (the reference's lib/datasets/shapenet_srn.py executed on the tree; mmcv.imread "
            f"substituted by Pillow's Image.open(path).convert('RGB'), mmcv.load / mmcv.dump by pickle, mmcv.parallel.DataContainer by a function that "
            f"returns its value, mmgen's DATASETS by a registry that only records the class); sets {', '.join(SETS)}; "
            f"torch {torch.__version__}, numpy {np.__version__}, Pillow {PIL.__version__}.\n")
    with open(os.path.join(HERE, "srn_tiny_provenance.txt"), "w") as f:
        f.write(note)
    print(note, end="")


if __name__ == "__main__":
    main()
