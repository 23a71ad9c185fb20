#!/usr/bin/env python
"""tests/golden/make_golden_tv.py -- the golden fixture of the total-variation regulariser (csrc/tv_loss.hip, codes.TVLoss), generated like
make_golden.py by EXECUTING THE REFERENCE'S OWN PYTHON in the build container (the fixture travels, the reference does not).  Writes tv_loss.npz
and its provenance note, tv_loss_provenance.txt, next to this file.

What runs for real (from the reference tree, unmodified):
    lib/models/losses/tv_loss.py    tv_loss (diff / cat / stack / norm / pow / mean) and TVLoss, in float64, with PyTorch's autograd

What is substituted (not installable here): mmgen's ``MODULES`` registry and its ``weighted_loss`` decorator, restated from SURVEY.md Appendix A
as ``make_golden_recons.py`` restates ``reduce_loss``: ``loss_func(pred, target, **kwargs)`` then the reduction (no weight, no avg_factor), so
the mean reduction is pinned by this restatement, not by mmgen's own file.

Fixture layout, case k = 0 .. n_cases - 1:
    x_k           float32 (S, 3, C, h, w) code
    power_k, weight_k   TVLoss(power, loss_weight)
    means_k       float64 (S, 3, C) per-slice means of r^power (reduction='none')
    value_k       float64 () TVLoss(...)(x), mmgen's default reduction='mean'
    grad_k        float64 (S, 3, C, h, w) d value / d x by autograd
"""
import functools
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("REF", "/root/reference")


def _reduce_loss(loss, reduction):
    return {"none": lambda v: v, "mean": lambda v: v.mean(), "sum": lambda v: v.sum()}[reduction](loss)


def _weighted_loss(loss_func):
    @functools.wraps(loss_func)
    def wrapper(pred, target=None, weight=None, reduction="mean", avg_factor=None, **kwargs):
        assert weight is None and avg_factor is None
        return _reduce_loss(loss_func(pred, target, **kwargs), reduction)
    return wrapper


class _Registry:
    def __init__(self):
        self.module_dict = {}

    def register_module(self, name=None, module=None, force=False):
        def _register(cls):
            self.module_dict[name or cls.__name__] = cls
            return cls
        return _register if module is None else _register(module)


def _load_reference():
    mods = {name: types.ModuleType(name) for name in ("mmgen", "mmgen.models", "mmgen.models.builder", "mmgen.models.losses",
                                                      "mmgen.models.losses.utils")}
    mods["mmgen.models.builder"].MODULES = _Registry()
    mods["mmgen.models.losses.utils"].weighted_loss = _weighted_loss
    sys.modules.update(mods)
    spec = importlib.util.spec_from_file_location("ref_tv_loss", os.path.join(REF, "lib", "models", "losses", "tv_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cases():
    g = np.random.default_rng(2024)
    out = []
    out.append((g.standard_normal((2, 3, 4, 8, 8)).astype(np.float32), 1.5, 1.0))
    out.append((g.standard_normal((1, 3, 2, 7, 13)).astype(np.float32), 1.0, 1.0))
    out.append((g.standard_normal((1, 3, 2, 1, 17)).astype(np.float32), 2.0, 1.0))
    out.append((g.standard_normal((1, 3, 2, 17, 1)).astype(np.float32), 3.0, 1.0))
    out.append((g.standard_normal((1, 3, 1, 1, 1)).astype(np.float32), 1.5, 1.0))
    # piecewise constant: 3 x 3 blocks of one value each, so most differences are exactly zero
    blocks = g.integers(-4, 5, (2, 3, 2, 3, 2)).astype(np.float32) * 0.25
    out.append((blocks.repeat(3, axis=-2).repeat(3, axis=-1)[..., :9, :6].copy(), 1.5, 2.5))
    flat = np.full((1, 3, 2, 5, 5), 0.375, np.float32)
    flat[0, 1, 0, 2:, 3:] = -1.0                                        # a step in one slice; the other slices stay constant
    out.append((flat, 1.0, 1.0))
    out.append((g.uniform(-1, 1, (1, 3, 2, 6, 11)).astype(np.float32) * 1e-3, 3.0, 0.5))
    return out


def main():
    assert os.path.isdir(REF), REF
    ref = _load_reference()
    arrays = {}
    for k, (x, power, weight) in enumerate(_cases()):
        leaf = torch.from_numpy(x).double().requires_grad_(True)
        loss = ref.TVLoss(power=power, loss_weight=weight)
        value = loss(leaf)
        value.backward()
        means = ref.tv_loss(leaf.detach(), [-2, -1], power=power, reduction="none")
        assert torch.isfinite(leaf.grad).all(), k
        arrays.update({f"x_{k}": x, f"power_{k}": np.float64(power), f"weight_{k}": np.float64(weight), f"means_{k}": means.numpy(),
                       f"value_{k}": value.detach().numpy(), f"grad_{k}": leaf.grad.numpy()})
    arrays["n_cases"] = np.int64(len(_cases()))
    np.savez_compressed(os.path.join(HERE, "tv_loss.npz"), **arrays)
    note = (f"tv_loss.npz: tests/golden/make_golden_tv.py (the reference lib/models/losses/tv_loss.py executed in float64 with autograd; "
            f"mmgen weighted_loss restated, mean reduction); {len(_cases())} cases; torch {torch.__version__}, numpy {np.__version__}.\n")
    with open(os.path.join(HERE, "tv_loss_provenance.txt"), "w") as f:
        f.write(note)
    print(note, end="")


if __name__ == "__main__":
    main()
