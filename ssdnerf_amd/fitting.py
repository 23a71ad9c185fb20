"""Fitting scene codes to posed observations: the machinery behind rendering guidance (``val_guide``), optimisation-based inversion
(``inverse_code``) and the fine-tuning half of ``cond_mode='guide_optim'`` (``val_optim``).  Behaviour: lib/models/autodecoders/
base_nerf.py:231-316, 403-492 and diffusion_nerf.py:241-404; SURVEY.md section 8 rows a15, (f)1.

The reference spreads this over nested closures and long method bodies; here it is four small objects that the model classes compose:

  Conditioning      the observations of a batch of scenes: images, their rays (generated on the device by one HIP pass) and the per-scene
                    cone angle ``dt_gamma`` -- or, store-backed, a ``datasets.StoredViews`` handle in place of the three arrays;
  RayBatcher        which pixels each step looks at: disjoint chunks of one random permutation per scene, cycled (or everything, when the
                    views are small), gathered on the device -- from the arrays, or by one launch straight from the uint8 image store;
  CodeFitter        N rendering-loss iterations on pre-activation code leaves: activation -> (periodic) density refresh -> train-branch
                    render + loss -> backward on top of an optional seed gradient (the diffusion prior's) -> optimizer / scheduler step;
  GuidanceObjective the ``grad_guide_fn`` of rendering-guided DDIM as an object that owns its density grid and step counter.

Everything that draws random numbers accepts injected draws (march jitter, grid jitter), so parity runs reproduce across devices.
The model passes ITSELF in: ``loss`` / ``update_extra_state`` are looked up on it at call time (they are the reference's public hooks).
"""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Sequence, Union

import torch

from . import nerf
from .datasets import StoredViews
from .optim import step_all


class Conditioning:
    """``Conditioning(images, rays_o, rays_d, dt_gamma)``: three (S, V, h, w, 3) arrays and the (S,) cone angle of the march,
    dt_gamma_scale / mean focal length.  Store-backed: ``images`` is a ``datasets.StoredViews`` and ``rays_o = rays_d = None``; ``stored`` is
    then that handle, ``RayBatcher`` samples from it, and ``images`` / ``rays_o`` / ``rays_d`` are its ``dense()`` arrays, built when first read."""

    def __init__(self, images, rays_o: Optional[torch.Tensor], rays_d: Optional[torch.Tensor], dt_gamma):
        self.stored: Optional[StoredViews] = images if isinstance(images, StoredViews) else None
        if self.stored is not None and (rays_o is not None or rays_d is not None):
            raise ValueError("Conditioning: a StoredViews handle makes its own rays; pass rays_o = rays_d = None with it")
        self._arrays = (images, rays_o, rays_d)
        self.dt_gamma = dt_gamma

    @classmethod
    def from_batch(cls, data: Dict, dt_gamma_scale: float) -> "Conditioning":
        imgs, intr, poses = data["cond_imgs"], data["cond_intrinsics"], data["cond_poses"]
        if isinstance(imgs, StoredViews):                                # nothing per pixel happens here
            return cls(imgs, None, None, dt_gamma_scale / imgs.intrinsics[..., :2].mean(dim=(-2, -1)))
        h, w = imgs.shape[2:4]
        o, d = nerf.get_cam_rays(poses, intr, h, w)
        return cls(imgs, o, d, dt_gamma_scale / intr[..., :2].mean(dim=(-2, -1)))

    def _array(self, i: int) -> torch.Tensor:
        return self._arrays[i] if self.stored is None else self.stored.dense()[i]

    @property
    def images(self) -> torch.Tensor:
        return self._array(0)

    @property
    def rays_o(self) -> torch.Tensor:
        return self._array(1)

    @property
    def rays_d(self) -> torch.Tensor:
        return self._array(2)

    def ray_args(self):
        """(cond_imgs, cond_rays_o, cond_rays_d) as ``BaseNeRF.inverse_code`` / ``loss_decoder`` / ``ray_sample`` take them: the arrays, or
        (handle, None, None) -- handing these on never builds the dense arrays"""
        return self._arrays

    @property
    def device(self) -> torch.device:
        return self._arrays[0].device

    @property
    def num_scenes(self) -> int:
        return self._arrays[0].size(0)

    @property
    def pixels_per_scene(self) -> int:
        return self._arrays[0].shape[1:4].numel()


INDEX_SOURCES = ("host", "device")


def check_index_source(value) -> str:
    """``cfg['ray_index_source']``: 'host' (torch.randperm, the default) or 'device' (the keyed permutation of csrc/keyed_perm.h)"""
    if value not in INDEX_SOURCES:
        raise ValueError(f"ray_index_source must be one of {INDEX_SOURCES}, got {value!r}")
    return value


class RayBatcher:
    """``batch(k)`` -> (rays_o, rays_d, target), each (S, R, 3).  With more pixels than ``rays_per_step`` the pixels of every scene are
    permuted once and step k takes chunk k mod n_chunks (``fixed=True``: base_nerf.py:263-274, used by inversion and guidance), or a fresh
    random subset is drawn per call (``fixed=False``: base_nerf.py:231-261 without indices, used by ``loss_decoder``).  On a store-backed
    ``Conditioning`` the indices are drawn by the same calls in the same order and the gather is ``StoredViews.sample``: one launch per batch.

    ``index_source='device'`` (opt-in) draws no index on the host: pixel numbers are positions of the keyed permutation
    pi(seed, scene, draw, P) of csrc/keyed_perm.h.  ``fixed=True``: chunk k is positions [kR, min((k+1)R, P)) of draw 0, cycled after ceil(P/R)
    chunks as the host chunks are; ``fixed=False``: take number n is positions [0, R) of draw n.  A store-backed conditioning evaluates pi inside
    the sampling launch (``StoredViews.sample_permuted``), a dense one indexes with the output of ``ssdnerf_perm_indices``: the same pixels.
    ``seed=None`` takes one 64-bit draw from torch's CPU generator here, so ``torch.manual_seed`` reproduces a run.  Not torch.randperm's stream."""

    def __init__(self, cond: Conditioning, rays_per_step: int, fixed: bool = True, index_source: str = "host", seed: Optional[int] = None):
        self.index_source = check_index_source(index_source)
        self.S, self.P, self.R = cond.num_scenes, cond.pixels_per_scene, rays_per_step
        self.stored, self.device = cond.stored, cond.device
        if index_source == "device" and self.device.type != "cuda":
            raise ValueError(f"RayBatcher: index_source='device' draws on the GPU, the conditioning is on {self.device} (there is no CPU path)")
        self.flat = None
        if self.stored is None:
            self.flat = (cond.rays_o.reshape(self.S, self.P, 3), cond.rays_d.reshape(self.S, self.P, 3), cond.images.reshape(self.S, self.P, 3))
        self.chunks: Optional[Sequence[torch.Tensor]] = None
        self.fixed, self.n_chunks, self.takes = fixed, -(-self.P // self.R), 0
        if index_source == "device":
            self.seed = (int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64)) if seed is None else int(seed)) & (2 ** 64 - 1)
            return
        if fixed and self.P > self.R:
            perms = torch.stack([torch.randperm(self.P, device=self.device) for _ in range(self.S)], dim=0)
            if self.stored is None:
                self.chunks = perms.split(self.R, dim=1)
            else:       # the same chunks, each (S, R) contiguous as the kernel reads them: one reordering copy here, none per batch
                whole = self.P // self.R
                self.chunks = tuple(perms[:, :whole * self.R].reshape(self.S, whole, self.R).transpose(0, 1).contiguous())
                if whole * self.R < self.P:
                    self.chunks += (perms[:, whole * self.R:].contiguous(),)

    def _span(self, k: int):
        """(draw, start, count) of batch k in device mode: a chunk of draw 0, or the head of the next unused draw"""
        if self.fixed:
            start = (k % self.n_chunks) * self.R
            return 0, start, min(self.R, self.P - start)
        self.takes += 1
        return self.takes - 1, 0, self.R

    def device_indices(self, draw: int, start: int, count: int) -> torch.Tensor:
        """(S, count) int64: pi(seed, s, draw, P)(start + r), one launch of ``ssdnerf_perm_indices``"""
        from . import _cabi as C
        with torch.cuda.device(self.device):
            inds = torch.empty((self.S, count), dtype=torch.int64, device=self.device)
            C.check(C.lib().ssdnerf_perm_indices(C.ptr(inds), self.S, self.P, start, count, self.seed, draw, C.stream()), "perm_indices")
        return inds

    def _permuted(self, draw: int, start: int, count: int):
        if self.stored is not None:                  # pi is evaluated inside the sampling launch: no index tensor
            return self.stored.sample_permuted(self.seed, draw, start, count)
        return self.take(self.device_indices(draw, start, count))

    def indices(self, k: int) -> Optional[torch.Tensor]:
        if self.index_source == "device":
            return self.device_indices(*self._span(k)) if self.fixed and self.P > self.R else None
        return None if self.chunks is None else self.chunks[k % len(self.chunks)]

    def take(self, inds: Optional[torch.Tensor]):
        if self.P <= self.R:
            return self.flat if self.stored is None else self.stored.sample(None)
        if inds is None and self.index_source == "device":
            return self._permuted(*self._span(0))
        if inds is None:
            inds = torch.stack([torch.randperm(self.P, device=self.device)[:self.R] for _ in range(self.S)], dim=0)
        if self.stored is not None:
            return self.stored.sample(inds)
        rows = torch.arange(self.S, device=inds.device)[:, None]
        return tuple(t[rows, inds] for t in self.flat)

    def batch(self, k: int):
        if self.index_source == "device" and self.fixed and self.P > self.R:
            return self._permuted(*self._span(k))
        return self.take(self.indices(k))


def _as_iter(x) -> Optional[Iterator]:
    return None if x is None else iter(x)


class CodeFitter:
    """Rendering-loss iterations on code leaves (``code_``: one (S, ...) leaf, or a list of per-scene leaves with one optimizer each).

    One iteration k:  code = activation(code_)  ->  every ``update_extra_interval`` iterations the density grid is refreshed from the detached
    code  ->  ray batch k  ->  ``model.loss`` through the decoder's TRAIN branch  ->  gradients: zeroed, or -- ``seed_grad`` -- overwritten
    with a gradient computed elsewhere (the diffusion prior's), so that the rendering gradient ACCUMULATES on top of it  ->  backward  ->
    optimizer step(s)  ->  scheduler step(s)."""

    def __init__(self, model, decoder, cond: Conditioning, cfg: Dict, code_, density_grid, density_bitfield, optimizers, schedulers=None,
                 march_noises=None, density_jitters=None):
        self.model, self.decoder, self.cond, self.cfg = model, decoder, cond, cfg
        self.code_, self.grid, self.bits = code_, density_grid, density_bitfield
        self.optimizers = list(optimizers) if isinstance(optimizers, (list, tuple)) else [optimizers]
        self.schedulers = [] if schedulers is None else (list(schedulers) if isinstance(schedulers, (list, tuple)) else [schedulers])
        self.batcher = RayBatcher(cond, cfg.get("n_inverse_rays", 4096), fixed=True, index_source=cfg.get("ray_index_source", "host"))
        self.march_noises, self.density_jitters = _as_iter(march_noises), _as_iter(density_jitters)
        self.k = 0
        self.last = None            # (code, loss, loss_dict, rendered rgb, target rgb) of the latest iteration

    def _leaves(self) -> List[torch.Tensor]:
        return self.code_ if isinstance(self.code_, list) else [self.code_]

    def activated(self, **kw) -> torch.Tensor:
        return self.model.code_activation(torch.stack(self.code_, dim=0) if isinstance(self.code_, list) else self.code_, **kw)

    def step(self, seed_grad: Optional[Union[torch.Tensor, Sequence[torch.Tensor]]] = None):
        m, cfg = self.model, self.cfg
        code = self.activated()
        if self.k % m.update_extra_interval == 0:
            m.update_extra_state(self.decoder, code.detach(), self.grid, self.bits, 0, density_thresh=cfg.get("density_thresh", 0.01),
                                 jitter=None if self.density_jitters is None else next(self.density_jitters))
        rays_o, rays_d, target = self.batcher.batch(self.k)
        if self.march_noises is not None:
            self.decoder.injected_noises = next(self.march_noises)
        try:
            rgb, loss, parts = m.loss(self.decoder, code, self.bits, target, rays_o, rays_d, self.cond.dt_gamma,
                                      scale_num_ray=self.cond.pixels_per_scene, cfg=cfg)
        finally:
            self.decoder.injected_noises = None
        if seed_grad is None:
            for opt in self.optimizers:
                opt.zero_grad()
        else:
            seeds = seed_grad if isinstance(self.code_, list) else [seed_grad]
            for leaf, g in zip(self._leaves(), seeds):
                leaf.grad.copy_(g)
        loss.backward()
        step_all(self.optimizers)
        for sch in self.schedulers:
            sch.step()
        self.k += 1
        self.last = (code.detach(), loss, parts, rgb, target)
        return self.last

    def run(self, n_steps: int, seed_grad=None):
        assert n_steps > 0
        was_training = self.decoder.training
        self.decoder.train(True)                     # the renderer's TRAIN branch: packed march with jitter, differentiable composite
        try:
            for _ in range(n_steps):
                self.step(seed_grad)
        finally:
            self.decoder.train(was_training)
        return self.last


class GuidanceObjective:
    """``loss = GuidanceObjective(...)(x0_pred)``: the rendering loss that steers every DDIM step of ``val_guide``
    (diffusion_nerf.py:282-294).  Per call: x0 -> scene codes, ONE density-grid refresh from them (decay 0.9 against the previous step's
    grid, which this object owns), ray batch k, train-branch render, pixel (+ regularisation) loss, summed over the scenes of the batch."""

    def __init__(self, model, decoder, cond: Conditioning, cfg: Dict, march_noises=None, density_jitters=None):
        self.model, self.decoder, self.cond, self.cfg = model, decoder, cond, cfg
        dev, S, H3 = cond.device, cond.num_scenes, model.grid_size ** 3
        self.grid = torch.zeros((S, H3), device=dev)                                   # fp32 here, as in the reference (diffusion_nerf.py:278)
        self.bits = torch.zeros((S, H3 // 8), dtype=torch.uint8, device=dev)
        self.batcher = RayBatcher(cond, cfg.get("n_inverse_rays", 4096), fixed=True, index_source=cfg.get("ray_index_source", "host"))
        self.march_noises, self.density_jitters = march_noises, density_jitters
        self.calls = 0

    def __call__(self, x0_pred: torch.Tensor) -> torch.Tensor:
        m, k = self.model, self.calls
        code = m.code_diff_pr_inv(x0_pred)
        m.update_extra_state(self.decoder, code.detach().float(), self.grid, self.bits, 0, density_thresh=self.cfg.get("density_thresh", 0.01),
                             jitter=None if self.density_jitters is None else self.density_jitters[k])
        rays_o, rays_d, target = self.batcher.batch(k)
        if self.march_noises is not None:
            self.decoder.injected_noises = self.march_noises[k]
        try:
            _, loss, _ = m.loss(self.decoder, code, self.bits, target, rays_o, rays_d, self.cond.dt_gamma, scale_num_ray=target.size(1), cfg=self.cfg)
        finally:
            self.decoder.injected_noises = None
        self.calls += 1
        return loss * self.cond.num_scenes
