"""``ExponentialMovingAverageHook``: the first custom hook of every training config of the reference

    dict(type='ExponentialMovingAverageHook', module_keys=('diffusion_ema', 'decoder_ema'), interp_mode='lerp', interval=1, start_iter=0,
         momentum_policy='rampup', momentum_cfg=dict(ema_kimg=4, ema_rampup=0.05, batch_size=16, eps=1e-8), priority='VERY_HIGH')

with the update of EVERY state-dict entry of EVERY module pair on a device in one HIP launch (csrc/ema.hip, arithmetic in csrc/ema_math.h).
``val_uncond``, ``val_step``, ``render`` and ``evaluate_3d`` all read ``diffusion_ema`` / ``decoder_ema``; without this hook after every
``train_step`` those stay at their initialisation.

The semantics are mmgen 0.7.2's (mmgen/core/hooks/ema_hook.py), restated from memory -- mmgen is not on disk here:
the source module of ``key`` is ``key[:-4]``; while ``iter < start_iter`` every EMA entry is a copy of its source entry; afterwards, every
``interval`` iterations, every entry of the source's ``state_dict()`` (parameters AND buffers) becomes

    ema <- src + (ema - src) * m         m = momentum if src.requires_grad else momentum_nontrainable (0.0: buffers and frozen weights are copied)

three eager fp32 operations per element, which is exactly what the kernel rounds (not ``torch.lerp``).

Routing: an fp32, contiguous, same-shape pair on one GPU is a row of that device's PLAN (a device-resident table of pointers, built once,
validated by ``ssdnerf_ema_plan_build``) and rides in the one launch; any other entry (another dtype, a CPU model, a non-contiguous tensor,
devices that differ) takes the eager formula per tensor.  Every call re-reads the live tensors' pointers, dtypes, shapes, devices and
``requires_grad`` on the host and rebuilds the plan when any of them differs from what the plan was built from (``.to()``, ``.half()``, a
``load_state_dict`` that reallocates, a swapped Parameter or submodule), so a launch never sees a stale pointer.  In steady state a call
is that host check, one library call and ``increment_version`` on the written tensors: no host synchronisation, no allocation, on the
current stream.  Entries added to or removed from a module after the first update are not noticed: call ``hook.reset()``."""
from __future__ import annotations

import ctypes
import warnings
from copy import deepcopy
from typing import Dict, List, Optional, Tuple

import torch

from . import _cabi as C
from .registry import HOOKS

launches = 0             # library calls so far (one per device and update)
plan_builds = 0          # device plans built so far (one per device whenever the tensors behind a hook changed)
eager_tensors = 0        # state-dict entries that took the per-tensor eager path so far


def rampup_momentum(iteration: int, ema_kimg: float = 10, ema_rampup: Optional[float] = 0.05, batch_size: int = 4, eps: float = 1e-8) -> float:
    """the ``rampup`` momentum policy (StyleGAN2-ADA's EMA ramp-up), in Python doubles: half-life ``ema_kimg`` thousand images, never more
    than ``ema_rampup`` times the images seen so far"""
    cur_nimg = (iteration + 1) * batch_size
    ema_nimg = ema_kimg * 1000
    if ema_rampup is not None:
        ema_nimg = min(ema_nimg, cur_nimg * ema_rampup)
    return 0.5 ** (batch_size / max(ema_nimg, eps))


def _entries(module: torch.nn.Module, prefix: str = ""):
    """(key, owner module, name, is_buffer) of every ``state_dict()`` entry, in its order"""
    for name, p in module._parameters.items():
        if p is not None:
            yield prefix + name, module, name, False
    for name, b in module._buffers.items():
        if b is not None and name not in module._non_persistent_buffers_set:
            yield prefix + name, module, name, True
    for cname, child in module._modules.items():
        if child is not None:
            yield from _entries(child, prefix + cname + ".")


def _links(module: torch.nn.Module, out: List) -> List:
    """(parent, child name, child) of every submodule: what must still hold for a cached walk to describe the module"""
    for cname, child in module._modules.items():
        out.append((module, cname, child))
        if child is not None:
            _links(child, out)
    return out


def _signature(s: torch.Tensor, e: torch.Tensor) -> Tuple:
    """everything about a pair that decides its route and its row"""
    return (s.data_ptr(), e.data_ptr(), s.requires_grad, s.dtype, e.dtype, s.shape, e.shape, s.device, e.device, s.is_contiguous(), e.is_contiguous())


def _eager(s: torch.Tensor, e: torch.Tensor, m: Optional[float]) -> None:
    """one entry by the reference's per-tensor formula (``m is None``: the copy before ``start_iter``); what ``load_state_dict`` did there
    -- a ``copy_`` into the EMA tensor, casting where the formula changed the dtype -- is the ``copy_`` here"""
    s = s.detach()
    if s.device != e.device:
        s = s.to(e.device)
    e.copy_(s if m is None else s + (e.detach() - s) * m)


@HOOKS.register_module()
class ExponentialMovingAverageHook:
    def __init__(self, module_keys, interp_mode="lerp", interp_cfg=None, interval=-1, start_iter=0, momentum_policy="fixed", momentum_cfg=None,
                 priority="NORMAL"):
        if not (isinstance(module_keys, str) or (isinstance(module_keys, (tuple, list)) and all(isinstance(k, str) for k in module_keys))):
            raise TypeError(f"module_keys must be a str or a tuple of str, got {module_keys!r}")
        self.module_keys = (module_keys,) if isinstance(module_keys, str) else tuple(module_keys)
        for k in self.module_keys:
            if not k.endswith("_ema") or len(k) == 4:
                raise ValueError(f'You should give keys that end with "_ema", got {k!r}')
        if interp_mode != "lerp":
            raise NotImplementedError(f"Currently, we do not support {interp_mode} for EMA (only 'lerp')")
        if momentum_policy not in ("fixed", "rampup"):
            raise NotImplementedError(f"Currently, we do not support {momentum_policy} for momentum_policy ('fixed' or 'rampup')")
        self.interp_mode, self.momentum_policy = interp_mode, momentum_policy
        self.interp_cfg = dict() if interp_cfg is None else deepcopy(dict(interp_cfg))
        unknown = set(self.interp_cfg) - {"momentum", "momentum_nontrainable"}
        if unknown:
            raise TypeError(f"lerp got unexpected interp_cfg keys {sorted(unknown)}")
        self.momentum_cfg = dict() if momentum_cfg is None else deepcopy(dict(momentum_cfg))
        if momentum_policy == "rampup":
            rampup_momentum(0, **self.momentum_cfg)                      # a bad momentum_cfg fails here, not at the first iteration
        self.interval, self.start_iter, self.priority = interval, start_iter, priority
        self.reset()

    # ------------------------------------------------------------------------------------------ schedule
    def acts_at(self, iteration: int) -> bool:
        """whether ``after_train_iter`` does anything at ``runner.iter == iteration``"""
        if iteration < self.start_iter:
            return True
        return self.interval > 0 and (iteration + 1 - self.start_iter) % self.interval == 0

    def momenta(self, iteration: int) -> Tuple[float, float]:
        """(momentum, momentum_nontrainable) of the update at ``iteration``"""
        cfg = dict(self.interp_cfg)
        if self.momentum_policy == "rampup":
            cfg["momentum"] = rampup_momentum(iteration, **self.momentum_cfg)
        return float(cfg.get("momentum", 0.999)), float(cfg.get("momentum_nontrainable", 0.0))

    # ------------------------------------------------------------------------------------------ runner interface
    @staticmethod
    def _model_of(runner):
        model = runner.model
        return model.module if hasattr(model, "module") else model

    def before_run(self, runner) -> None:
        model = self._model_of(runner)
        for k in self.module_keys:
            if not hasattr(model, k) and not hasattr(model, k[:-4]):
                raise RuntimeError(f"Cannot find both {k[:-4]} and {k} network for EMA hook.")
            if not hasattr(model, k):
                setattr(model, k, deepcopy(getattr(model, k[:-4])))
                warnings.warn(f"We do not suggest construct and initialize EMA model {k} in hook. You may explicitly define it by yourself.")

    def after_train_iter(self, runner) -> None:
        self.update(self._model_of(runner), runner.iter)

    # ------------------------------------------------------------------------------------------ the update
    def reset(self) -> None:
        """forget the cached walk of the modules and the device plans (rebuilt by the next update)"""
        self._model = None
        self._roots: List = []
        self._links: List = []
        self._pairs: List = []                                           # (key, src owner, ema owner, name, is_buffer)
        self._sig: Optional[List] = None
        self._plans: Dict[int, Tuple] = {}                               # device index -> (plan tensor, T, blocks, written tensors)
        self._eager_idx: List = []                                       # indices into _pairs: the entries of the eager path

    def _walk(self, model) -> None:
        self.reset()
        pairs, roots, links = [], [], []
        for k in self.module_keys:
            if not hasattr(model, k[:-4]):
                raise RuntimeError(f"Cannot find {k[:-4]} network for EMA hook.")
            if not hasattr(model, k):
                raise RuntimeError(f"Cannot find {k} network for EMA hook (before_run creates it).")
            src, ema = getattr(model, k[:-4]), getattr(model, k)
            roots.append((k, src, ema))
            _links(src, links)
            _links(ema, links)
            ema_entries = {key: (owner, name, is_buf) for key, owner, name, is_buf in _entries(ema)}
            for key, owner, name, is_buf in _entries(src):
                if key not in ema_entries:
                    raise KeyError(f"{k} has no state-dict entry {key!r} of {k[:-4]}")
                e_owner, e_name, e_buf = ema_entries[key]
                pairs.append((f"{k}.{key}", owner, "_buffers" if is_buf else "_parameters", name, e_owner, "_buffers" if e_buf else "_parameters", e_name))
        self._model, self._roots, self._links, self._pairs = model, roots, links, pairs

    def _live(self):
        """the live (source, EMA) tensors of every entry, or None when the module structure is no longer the one that was walked"""
        out = []
        try:
            for _, so, sd, sn, eo, ed, en in self._pairs:
                s, e = getattr(so, sd)[sn], getattr(eo, ed)[en]
                if s is None or e is None:
                    return None
                out.append((s, e))
        except KeyError:
            return None
        return out

    def _structure_holds(self, model) -> bool:
        if model is not self._model:
            return False
        for k, src, ema in self._roots:
            if getattr(model, k[:-4], None) is not src or getattr(model, k, None) is not ema:
                return False
        for parent, cname, child in self._links:
            if parent._modules.get(cname) is not child:
                return False
        return True

    def _build_plans(self, live, sig) -> None:
        global plan_builds
        lib = None
        rows: Dict[int, List] = {}
        self._eager_idx, self._plans = [], {}
        seen = set()
        for i, ((s, e), g) in enumerate(zip(live, sig)):
            if id(e) in seen:                                            # one tensor under two names (tied weights, a module used twice): once
                continue
            seen.add(id(e))
            if s.shape != e.shape:
                raise RuntimeError(f"size mismatch for {self._pairs[i][0]}: source {tuple(s.shape)}, EMA {tuple(e.shape)}")
            if s.numel() == 0:
                continue
            if (s.dtype == torch.float32 and e.dtype == torch.float32 and s.is_cuda and s.device == e.device and s.is_contiguous() and e.is_contiguous()
                    and s.layout == torch.strided and e.layout == torch.strided):
                rows.setdefault(s.device.index, []).append((s, e))
            else:
                self._eager_idx.append(i)
        for dev, pairs in rows.items():
            lib = lib or C.lib()
            table = (C.EmaRow * len(pairs))()
            for r, (s, e) in zip(table, pairs):
                r.src, r.dst, r.numel, r.trainable = s.data_ptr(), e.data_ptr(), s.numel(), int(s.requires_grad)
            blocks = ctypes.c_uint32(0)
            C.check(lib.ssdnerf_ema_plan_build(table, len(pairs), ctypes.byref(blocks)), "ema_plan_build")
            plan = torch.frombuffer(table, dtype=torch.uint8).to(torch.device("cuda", dev))      # a copy: `table` may go
            self._plans[dev] = (plan, len(pairs), int(blocks.value), [e for _, e in pairs])
            plan_builds += 1
        self._sig = sig

    def _current(self, model):
        """the live (source, EMA) tensors of every entry, with the plans made to describe them: the host-side validity check of every update
        (tools/bench_ema.py times it alone)"""
        live = self._live() if self._model is not None and self._structure_holds(model) else None
        if live is None:
            self._walk(model)
            live = self._live()
        sig = [_signature(s, e) for s, e in live]
        if sig != self._sig:
            self._build_plans(live, sig)
        return live

    @torch.no_grad()
    def update(self, model, iteration: int) -> bool:
        """what ``after_train_iter`` does at ``runner.iter == iteration`` on ``runner.model``; returns whether the schedule acted"""
        global launches, eager_tensors
        if not self.acts_at(iteration):
            return False
        live = self._current(model)
        if iteration < self.start_iter:
            for s, e in live:
                _eager(s, e, None)
            return True
        momentum, nontrainable = self.momenta(iteration)
        for dev, (plan, T, blocks, written) in self._plans.items():
            with torch.cuda.device(dev):
                C.check(C.lib().ssdnerf_ema_update_multi(plan.data_ptr(), T, blocks, momentum, nontrainable, C.stream()), "ema_update_multi")
            launches += 1
            # the kernel wrote through raw pointers: tell autograd, and everything keyed on ``_version`` (the decoder's packed parameter
            # block, unet_fast's packed weights), as mmgen's load_state_dict did
            torch.autograd.graph.increment_version(written)
        for i in self._eager_idx:
            s, e = live[i]
            _eager(s, e, momentum if s.requires_grad else nontrainable)
        eager_tensors += len(self._eager_idx)
        return True
