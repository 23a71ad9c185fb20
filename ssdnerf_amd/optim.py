"""``HIPAdam``: the reference's optimizer (``torch.optim.Adam``, amsgrad=False, maximize=False) with the step of EVERY parameter of EVERY
optimizer handed to ``step_all`` in one HIP launch (csrc/adam.hip, arithmetic in csrc/adam_math.h).

Stage-1 fitting holds one optimizer per scene code, because optimizer states are cached per scene; ``CodeFitter.step`` and
``MultiSceneNeRF._joint_step`` used to loop over them, a handful of library kernels per optimizer and iteration.  ``step_all`` gathers the
parameters of all of them -- and of the decoder's optimizer -- into the table of ``ssdnerf_adam_step_multi``: one launch for 8 scenes + decoder.

The state is exactly ``torch.optim.Adam``'s (``step``: 0-dim float32 CPU tensor; ``exp_avg`` / ``exp_avg_sq``: ``zeros_like(param)``, created at
the first step; the same ``param_groups`` keys), so ``scene_cache.optimizer_set_state`` / ``optimizer_state_to`` / ``optimizer_state_copy``, the
16-bit cache and torch's LR schedulers work on it unchanged.  There is no fallback: a parameter that is not a contiguous fp32 GPU tensor is refused.
Not thread-safe (``step_all`` collects the rows of the optimizers it steps in a module-level list)."""
from __future__ import annotations

import inspect
import math
from typing import Iterable, List, Optional

import torch

from . import _cabi as C

CAPACITY = 32            # tensors per library call (SSDNERF_ADAM_MAX_TENSORS, include/ssdnerf_hip.h); longer lists take several calls
launches = 0             # library calls so far (tests assert the batching with it)

_ADAM_DEFAULTS = {k: p.default for k, p in inspect.signature(torch.optim.Adam.__init__).parameters.items() if k not in ("self", "params")}
_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable", "fused", "decoupled_weight_decay")
_table = None            # the host table handed to the library: allocated once, refilled per call
_pending: Optional[List] = None


def _check_tensor(t, what: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"HIPAdam: {what} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32 or t.is_sparse:
        raise TypeError(f"HIPAdam: {what} must be a dense fp32 tensor, got {t.dtype}{' (sparse)' if t.is_sparse else ''}")
    if not t.is_cuda:
        raise ValueError(f"HIPAdam: {what} must be on the GPU, got {t.device} (there is no CPU path)")
    if not t.is_contiguous():
        raise ValueError(f"HIPAdam: {what} must be contiguous, got strides {tuple(t.stride())} for shape {tuple(t.shape)}")


class HIPAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, **torch_kwargs):
        unknown = set(torch_kwargs) - set(_ADAM_DEFAULTS)
        if unknown:
            raise TypeError(f"HIPAdam: unexpected arguments {sorted(unknown)}")
        for flag in _UNSUPPORTED:
            if torch_kwargs.get(flag):
                raise NotImplementedError(f"HIPAdam: {flag}=True is not implemented (torch.optim.Adam's default form only)")
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(_ADAM_DEFAULTS, **torch_kwargs)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        ps = param_group["params"]
        if not isinstance(ps, (torch.Tensor, list)):
            param_group["params"] = ps = list(ps)
        for p in ([ps] if isinstance(ps, torch.Tensor) else ps):
            _check_tensor(p, "a parameter")
        super().add_param_group(param_group)

    def _rows(self) -> List:
        """advance the step counts of the parameters that have a gradient and return their table rows"""
        rows = []
        for group in self.param_groups:
            for flag in _UNSUPPORTED:
                if group.get(flag):
                    raise NotImplementedError(f"HIPAdam: {flag}=True is not implemented")
            lr, (b1, b2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
            for p in group["params"]:
                if p.grad is None:
                    continue
                _check_tensor(p, "a parameter")
                g = p.grad
                if g.is_sparse:
                    raise RuntimeError("HIPAdam does not support sparse gradients")
                if g.dtype != torch.float32 or g.device != p.device:
                    raise TypeError(f"HIPAdam: the gradient must be fp32 on {p.device}, got {g.dtype} on {g.device}")
                g = g.contiguous()
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                for t, name in ((m, "exp_avg"), (v, "exp_avg_sq")):
                    _check_tensor(t, name)
                    if t.shape != p.shape or t.device != p.device:
                        raise ValueError(f"HIPAdam: {name} is {tuple(t.shape)} on {t.device}, its parameter {tuple(p.shape)} on {p.device}")
                if isinstance(state["step"], torch.Tensor):
                    state["step"] += 1
                else:                                                # a state loaded from a checkpoint that kept a plain number
                    state["step"] = state["step"] + 1
                step = float(state["step"])
                # the host scalars of this step, in double (torch forms the same Python floats)
                step_size = lr / (1.0 - float(b1) ** step)
                bc2_sqrt = math.sqrt(1.0 - float(b2) ** step)
                if p.numel() > 0:
                    rows.append(((p.device.index, float(b1), float(b2), eps), p, g, m, v, step_size, bc2_sqrt, wd))
        return rows

    @torch.no_grad()
    def step(self, closure=None):
        """one Adam step of every parameter that has a gradient (one launch per ``CAPACITY`` tensors); inside ``step_all`` the rows join the
        launch of the whole list"""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        rows = self._rows()
        if _pending is not None:
            _pending.extend(rows)
        else:
            _launch(rows)
        return loss


def _launch(rows: List) -> None:
    global launches, _table
    if not rows:
        return
    lib = C.lib()
    if _table is None:
        if lib.ssdnerf_adam_max_tensors() != CAPACITY:
            raise RuntimeError(f"libssdnerf_hip.so takes {lib.ssdnerf_adam_max_tensors()} tensors per Adam launch, optim.CAPACITY says {CAPACITY}: rebuild")
        _table = (C.AdamTensor * CAPACITY)()
    by_key = {}
    for row in rows:                                                 # one launch per (device, betas, eps); dicts keep insertion order
        by_key.setdefault(row[0], []).append(row)
    for (dev, b1, b2, eps), group in by_key.items():
        with torch.cuda.device(dev):
            for start in range(0, len(group), CAPACITY):
                part = group[start:start + CAPACITY]
                for e, (_, p, g, m, v, step_size, bc2_sqrt, wd) in zip(_table, part):
                    e.param, e.grad, e.exp_avg, e.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
                    e.numel, e.step_size, e.bc2_sqrt, e.weight_decay = p.numel(), step_size, bc2_sqrt, wd
                C.check(lib.ssdnerf_adam_step_multi(_table, len(part), b1, b2, eps, C.stream()), "adam_step_multi")
                launches += 1
                # the kernel wrote through raw pointers: tell autograd, and everything keyed on ``_version`` (the decoder's packed weights)
                torch.autograd.graph.increment_version([t for row in part for t in (row[1], row[3], row[4])])


def step_all(optimizers: Iterable[torch.optim.Optimizer]) -> None:
    """``opt.step()`` for every optimizer, in order.  When all of them are ``HIPAdam`` their parameters share table launches: one launch for
    up to ``CAPACITY`` tensors with the same device, betas and eps (learning rates, step counts and weight decays are per tensor)."""
    global _pending
    opts = list(optimizers)
    if not opts or not all(isinstance(o, HIPAdam) for o in opts) or _pending is not None:
        for o in opts:
            o.step()
        return
    _pending = []
    try:
        for o in opts:
            o.step()                                                 # through torch's step hooks and the schedulers' call counters
        rows = _pending
    finally:
        _pending = None
    _launch(rows)
