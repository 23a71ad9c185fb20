"""Minimal loader for the reference's mmcv-style python configs (``mmcv.Config.fromfile``; used at
tools/train.py:129 / tools/test.py of the reference): executes the file, resolves ``_base_`` inheritance with mmcv's
merge rules (child keys override recursively; ``_delete_=True`` replaces a dict), and exposes attribute access.
``build_model`` is what ``mmgen.models.build_model(cfg.model, train_cfg=..., test_cfg=...)`` does."""
from __future__ import annotations

import os
import runpy
from typing import Any, Dict

from .registry import METRICS, MODELS


class ConfigDict(dict):
    def __getattr__(self, name):
        try:
            v = self[name]
        except KeyError as e:
            raise AttributeError(name) from e
        return v

    def __setattr__(self, name, value):
        self[name] = value


def _wrap(v):
    if isinstance(v, dict):
        return ConfigDict({k: _wrap(x) for k, x in v.items()})
    if isinstance(v, list):
        return [_wrap(x) for x in v]
    if isinstance(v, tuple):
        return tuple(_wrap(x) for x in v)
    return v


def _merge(base: Dict[str, Any], child: Dict[str, Any]) -> Dict[str, Any]:
    out = dict(base)
    for k, v in child.items():
        if isinstance(v, dict) and isinstance(out.get(k), dict) and not v.get("_delete_", False):
            out[k] = _merge(out[k], v)
        else:
            if isinstance(v, dict):
                v = {kk: vv for kk, vv in v.items() if kk != "_delete_"}
            out[k] = v
    return out


def _load(path: str) -> Dict[str, Any]:
    path = os.path.abspath(path)
    ns = runpy.run_path(path)
    cfg = {k: v for k, v in ns.items() if not k.startswith("__") and not callable(v) and type(v).__name__ != "module"}
    base = cfg.pop("_base_", None)
    if base is not None:
        bases = base if isinstance(base, (list, tuple)) else [base]
        merged: Dict[str, Any] = {}
        for b in bases:
            merged = _merge(merged, _load(os.path.join(os.path.dirname(path), b)))
        cfg = _merge(merged, cfg)
    return cfg


class Config(ConfigDict):
    @staticmethod
    def fromfile(path: str) -> "Config":
        c = Config(_wrap(_load(path)))
        c["filename"] = os.path.abspath(path)
        return c

    def merge_from_dict(self, options: Dict[str, Any]) -> None:
        """``--cfg-options a.b.c=v`` semantics."""
        for key, value in options.items():
            d = self
            parts = key.split(".")
            for p in parts[:-1]:
                d = d.setdefault(p, ConfigDict())
            d[parts[-1]] = _wrap(value)


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_plain(x) for x in v]
    return v


def build_model(cfg: Config):
    import ssdnerf_amd.decoders, ssdnerf_amd.diffusion, ssdnerf_amd.models, ssdnerf_amd.unet  # noqa: F401  (populate the registries)
    return MODELS.build(_plain(cfg["model"]), default_args=dict(train_cfg=_plain(cfg.get("train_cfg", {})), test_cfg=_plain(cfg.get("test_cfg", {}))))


def build_metrics(cfg) -> list:
    """The metric objects of a config's ``evaluation`` block(s), as the reference's eval hook builds them (``build_metric`` over the ``metrics`` entry of
    every ``dict(type='GenerativeEvalHook3D', ...)``): ``cfg.evaluation`` is a dict or a list of dicts, each ``metrics`` a dict or a list of dicts
    (``dict(type='FIDKID', num_images=..., inception_pkl=..., inception_args=..., bgr2rgb=False)``).  Blocks without metrics contribute nothing."""
    import ssdnerf_amd.fidkid  # noqa: F401  (populate the registry)
    evaluation = cfg.get("evaluation") or []
    blocks = evaluation if isinstance(evaluation, (list, tuple)) else [evaluation]
    out = []
    for block in blocks:
        metrics = block.get("metrics") or []
        for m in metrics if isinstance(metrics, (list, tuple)) else [metrics]:
            out.append(METRICS.build(_plain(m)))
    return out


def build_dataset(cfg, default_args=None):
    """A ``data`` block's entry (``cfg.data.train`` / ``val_cond`` / ``val_uncond``: ``dict(type='ShapeNetSRN', ...)``) -> the dataset (datasets.py)"""
    from .datasets import build_dataset as build
    return build(cfg, default_args)


def build_dataloader(dataset, samples_per_gpu, **kwargs):
    """This rank's in-process loader of batch dicts over a device-resident image store (``datasets.build_dataloader``)"""
    from .datasets import build_dataloader as build
    return build(dataset, samples_per_gpu, **kwargs)
