"""``VolumeRenderer`` and ``TriPlaneDecoder``: the reference's renderer types
(lib/models/decoders/base_volume_renderer.py, lib/models/decoders/triplane_decoder.py) with the same constructor
keywords, state-dict keys (``base_net.0.weight`` ...), ``forward`` signature and result dict - and the MI355X
fast path behind them:

* eval branch (``self.training == False``)  -> ONE fused HIP launch per scene
  (``ssdnerf_render_rays_fused``: AABB + march + gather + MLP + composite on chip, on-device compaction)
  instead of the reference's <=256-iteration host loop with a device->host sync per iteration.
* ``point_decode`` / ``point_density_decode`` on packed sample lists -> one fused HIP decode per scene; when only the
  scene code needs a gradient (guidance, fine-tuning) the backward is fused too (``_PointDecodeFn``: re-gather +
  recomputed MLP + atomic scatter); an eager PyTorch-ROCm path remains for decoder-parameter gradients (autograd;
  also the "reference-shaped eager" baseline B1), unless ``param_grad='fused'`` opts in: the same ``_PointDecodeFn``, whose
  backward then also runs the parameter gradients of csrc/decode_bwd_params.hip.
* train branch -> per-scene ``march_rays_train`` (deterministic prefix-sum packing) + decode +
  ``batch_composite_rays_train`` (HIP forward/backward kernels).

``render_mode='stepwise'`` runs the reference-shaped loop over the unfused operators instead (used by the
parity tests and as the exact fallback when the fused kernel reports a ray at the global step cap).
"""
from __future__ import annotations

import itertools
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _cabi as C
from .activation import TruncExp
from .raymarching import (batch_composite_rays_train, batch_near_far_from_aabb, composite_rays, composite_rays_train, march_rays,
                          march_rays_train)
from .registry import MODULES, build_module
from .shencoder import SHEncoder

MLP_OFF_WD = 64 * 24                      # the packed parameter block: SSDNERF_MLP_OFF_* / SSDNERF_MLP_PARAM_FLOATS of include/ssdnerf_hip.h (layout: csrc/decode_core.h)
MLP_OFF_BD = MLP_OFF_WD + 64 * 16
MLP_OFF_TAIL = MLP_OFF_BD + 64
MLP_PARAM_FLOATS = MLP_OFF_TAIL + 4
#: the eight tensors of the block in pack order: W1, b1, ws, bs, Wd, bd, Wc, bc
MLP_PARAM_KEYS = tuple(f"{net}.0.{kind}" for net in ("base_net", "density_net", "dir_net", "color_net") for kind in ("weight", "bias"))


def _per_scene_floats(dt_gamma, num_scenes):
    if isinstance(dt_gamma, (float, int)):
        return [float(dt_gamma)] * num_scenes
    if isinstance(dt_gamma, torch.Tensor):
        return [float(v) for v in dt_gamma.detach().reshape(-1).tolist()]
    return dt_gamma


def _xavier_uniform_(m: nn.Linear):
    nn.init.xavier_uniform_(m.weight, gain=1.0)
    if m.bias is not None:
        nn.init.constant_(m.bias, 0.0)


def pack_triplanes(code: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(S,3,C,H,W) NCHW code -> (S,3,H,W,8) channel-last zero-padded planes (fp32 or fp16) via the HIP repack kernel."""
    assert code.dim() == 5 and code.size(1) == 3 and code.size(2) <= 8
    code = code.contiguous()
    if code.dtype not in (torch.float32, torch.float16):
        code = code.float()
    s, _, c, h, w = code.shape
    planes = torch.empty(s, 3, h, w, 8, dtype=dtype, device=code.device)
    C.check(C.lib().ssdnerf_triplane_pack(C.ptr(code), C.dtype_code(code), C.u32(s), C.u32(c), C.u32(h), C.u32(w), C.ptr(planes),
                                          C.dtype_code(planes), C.stream()), "triplane_pack")
    return planes


def pack_mlp_params(sd: Dict[str, torch.Tensor], device) -> torch.Tensor:
    """Reference state-dict tensors -> the packed parameter block of the fused kernels (layout: csrc/decode_core.h)."""
    out = torch.zeros(MLP_PARAM_FLOATS, dtype=torch.float32, device=sd["base_net.0.weight"].device)      # (the records' unused column stays 0)
    for dst, key in zip(unpack_mlp_grads(out), MLP_PARAM_KEYS):
        dst.copy_(sd[key])
    return out.to(device).contiguous()


def unpack_mlp_grads(gp: torch.Tensor):
    """The inverse of ``pack_mlp_params``: a packed block (the parameter gradient of csrc/decode_bwd_params.hip) -> views of it with the shapes of the eight tensors,
    in the order of ``MLP_PARAM_KEYS``.  Wc sits transposed in the records."""
    rec = gp[:MLP_OFF_WD].view(64, 24)
    return (rec[:, :18], rec[:, 18], rec[:, 19].unsqueeze(0), gp[MLP_OFF_TAIL:MLP_OFF_TAIL + 1],          # W1 (64,18), b1 (64), ws (1,64), bs (1)
            gp[MLP_OFF_WD:MLP_OFF_BD].view(64, 16), gp[MLP_OFF_BD:MLP_OFF_TAIL], rec[:, 20:23].t(), gp[MLP_OFF_TAIL + 1:])     # Wd (64,16), bd (64), Wc (3,64), bc (3)


class _PointDecodeFn(torch.autograd.Function):
    """Fused point decode, differentiable w.r.t. the scene code and the decoder's eight parameter tensors (pack order; inputs so that autograd routes their gradients:
    the kernels read the packed block the forward read, ``ctx.packed``).  forward = ``ssdnerf_point_decode`` per scene.  backward, for the whole batch and only where an
    input needs it: ONE ``ssdnerf_point_decode_backward_params`` (the sum over the samples in per-lane registers, no atomics, fixed order: bit-reproducible) and ONE
    ``ssdnerf_point_decode_backward`` (binned reduction of the corner contributions in LDS, gradient in the code's NCHW layout; a frozen decoder launches this one only),
    both on re-gathered features and recomputed hidden units, instead of autograd through grid_sample + 4 nn.Linear (~20 eager kernels each way and
    ``grid_sampler_2d_backward``, alone 30 % of a guided DDIM step).  Sample positions and view directions are data: no gradient flows to them."""

    @staticmethod
    def forward(ctx, code, w1, b1, ws, bs, wd, bd, wc, bc, decoder, xyzs, dirs):
        planes = pack_triplanes(code.detach(), decoder.plane_dtype)
        xyzs = [x.detach().reshape(-1, 3).float().contiguous() for x in xyzs]
        dirs = [d.detach().reshape(-1, 3).float().contiguous() for d in dirs]
        sigmas, rgbs, num_points = decoder._point_decode_hip(xyzs, dirs, code, False, planes=planes)
        ctx.decoder, ctx.planes, ctx.xyzs, ctx.dirs, ctx.num_points = decoder, planes, xyzs, dirs, num_points
        ctx.packed = decoder.packed_params()                                   # the block the forward read (a change of the weights before backward re-packs into a new tensor)
        ctx.code_meta, ctx.param_dtypes = (code.shape, code.dtype), tuple(p.dtype for p in (w1, b1, ws, bs, wd, bd, wc, bc))
        return sigmas, rgbs

    @staticmethod
    def backward(ctx, g_sigmas, g_rgbs):
        decoder, planes = ctx.decoder, ctx.planes
        (s_, _, c, hp, wp), code_dtype = ctx.code_meta
        assert c == 6, "the fused decode gradient is written for 6-channel planes (18 features)"
        total, dev = sum(ctx.num_points), planes.device
        g_sigmas = torch.zeros(total, dtype=torch.float32, device=dev) if g_sigmas is None else g_sigmas.float().contiguous()
        g_rgbs = torch.zeros(total, 3, dtype=torch.float32, device=dev) if g_rgbs is None else g_rgbs.float().contiguous()
        xyzs = ctx.xyzs[0] if s_ == 1 else torch.cat(ctx.xyzs, dim=0)
        dirs = ctx.dirs[0] if s_ == 1 else torch.cat(ctx.dirs, dim=0)
        offsets = torch.tensor([0, *itertools.accumulate(ctx.num_points)], dtype=torch.int32, device=dev)          # (a blocking copy: the host list dies with this frame)
        lib = C.lib()
        batch = (C.u32(s_), C.u32(hp), C.u32(wp), C.ptr(ctx.packed), C.ptr(xyzs), C.ptr(dirs), C.ptr(offsets), C.u32(total), C.f32(decoder.sigmoid_saturation),
                 C.ptr(g_sigmas), C.ptr(g_rgbs))                                # what the two entry points share, between planes_dtype and the result
        grads = [None] * 9
        if any(ctx.needs_input_grad[1:9]):
            gp = torch.empty(MLP_PARAM_FLOATS, dtype=torch.float32, device=dev)
            ws_bytes = int(lib.ssdnerf_point_decode_backward_params_workspace(C.u32(s_), C.u32(total), C.u32(0)))
            ws = decoder._workspace(max(ws_bytes, 1), dev, "decode_bwd_params")            # the decoder's cached scratch (grown on demand), not a fresh tensor per backward
            C.check(lib.ssdnerf_point_decode_backward_params(C.ptr(planes), C.dtype_code(planes), *batch, C.ptr(gp), C.u32(0), C.ptr(ws), C.ctypes.c_size_t(ws_bytes),
                                                             C.stream()), "point_decode_backward_params")
            for i, (g, dt) in enumerate(zip(unpack_mlp_grads(gp), ctx.param_dtypes)):
                if ctx.needs_input_grad[1 + i]:
                    grads[1 + i] = g.to(dt).contiguous()
        if ctx.needs_input_grad[0]:
            grad_code = torch.empty(s_, 3, 6, hp, wp, dtype=torch.float32, device=dev)
            ws_bytes = int(lib.ssdnerf_point_decode_backward_workspace(C.u32(s_), C.u32(total), C.u32(hp), C.u32(wp)))
            ws = decoder._workspace(max(ws_bytes, 1), dev, "decode_bwd")
            C.check(lib.ssdnerf_point_decode_backward(C.ptr(planes), C.dtype_code(planes) | (0x100 if getattr(decoder, "decode_bwd_feat_mfma", False) else 0), *batch,
                                                      C.ptr(grad_code), C.ptr(ws), C.ctypes.c_size_t(ws_bytes), C.stream()), "point_decode_backward")
            grads[0] = grad_code.to(code_dtype)
        return (*grads, None, None, None)


class VolumeRenderer(nn.Module):
    def __init__(self, bound=1, min_near=0.2, bg_radius=-1, max_steps=256, decoder_reg_loss=None, render_mode="fused",
                 plane_dtype="float32"):
        super().__init__()
        self.bound = bound
        self.min_near = min_near
        self.bg_radius = bg_radius  # accepted and never consumed, like the reference (base_volume_renderer.py:23)
        self.max_steps = max_steps
        self.decoder_reg_loss = build_module(decoder_reg_loss) if decoder_reg_loss is not None else None
        self.render_mode = render_mode
        self.fused_pipeline = "queue_mfma"  # "queue_mfma": first-hit + MFMA shading kernel; "queue": VALU shading kernel; "single": one persistent kernel (any grid size)
        self.injected_noises = None        # optional (S,R) march jitter for the train branch (parity runs inject it; None -> torch.rand)
        self.stage_events = None           # bench.py sets this to a list to get HIP events between the stages
        self._ws_cache = {}
        self.plane_dtype = getattr(torch, plane_dtype) if isinstance(plane_dtype, str) else plane_dtype
        self.register_buffer("aabb", torch.tensor([-bound, -bound, -bound, bound, bound, bound], dtype=torch.float32))
        self.last_render_stats: Dict[str, object] = {}

    def _workspace(self, nbytes: int, device, tag: str = "render") -> torch.Tensor:
        key = (device.index, torch.cuda.current_stream().cuda_stream, tag)
        buf = self._ws_cache.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self._ws_cache[key] = buf
        return buf

    def point_decode(self, xyzs, dirs, code):
        raise NotImplementedError

    def point_density_decode(self, xyzs, code):
        raise NotImplementedError

    def loss(self):
        assert self.decoder_reg_loss is None
        return None

    # -------------------------------------------------------------------------------------- forward
    def forward(self, rays_o, rays_d, code, density_bitfield, grid_size, dt_gamma=0, perturb=False, T_thresh=1e-4,
                return_loss=False, bg_color=None):
        """Same arguments/result dict as the reference (base_volume_renderer.py:41-133).  ``bg_color`` (extra, eval
        branch only): when given, the returned ``image`` is ALREADY blended with the background and the dict carries
        ``blended=True`` - this is what lets the fused kernel keep the blend on chip."""
        num_scenes = len(rays_o)
        assert num_scenes > 0
        if isinstance(grid_size, int):
            grid_size = [grid_size] * num_scenes
        dt_gamma_in = dt_gamma
        if not self.training:
            dt_gamma = _per_scene_floats(dt_gamma, num_scenes)

        if self.training:
            dense = (isinstance(rays_o, torch.Tensor) and rays_o.dim() == 3 and rays_o.is_cuda and isinstance(density_bitfield, torch.Tensor)
                     and all(g == grid_size[0] for g in grid_size))
            if dense and self.batched_train_march:
                xyzs, dirs, deltas, rays, num_points = self._march_train_batch(rays_o, rays_d, density_bitfield, grid_size[0], dt_gamma_in, perturb)
                sigmas, rgbs, _ = self.point_decode(list(xyzs.split(num_points)), list(dirs.split(num_points)), code)
                weights_sum, depth, image = composite_rays_train(sigmas, rgbs, deltas, rays, T_thresh)
                n = rays_o.size(1)
                results = dict(weights_sum=weights_sum.reshape(num_scenes, n), depth=depth.reshape(num_scenes, n), image=image.reshape(num_scenes, n, 3))
            else:
                dt_gamma = _per_scene_floats(dt_gamma_in, num_scenes)
                nears, fars = batch_near_far_from_aabb(rays_o, rays_d, self.aabb, self.min_near)
                xyzs, dirs, deltas, rays = [], [], [], []
                for s in range(num_scenes):
                    x, d, dl, r = march_rays_train(rays_o[s], rays_d[s], self.bound, density_bitfield[s], 1, grid_size[s], nears[s],
                                                   fars[s], perturb=perturb, align=128, force_all_rays=True, dt_gamma=dt_gamma[s],
                                                   max_steps=self.max_steps,
                                                   noises=None if self.injected_noises is None else self.injected_noises[s])
                    xyzs.append(x); dirs.append(d); deltas.append(dl); rays.append(r)
                sigmas, rgbs, num_points = self.point_decode(xyzs, dirs, code)
                weights_sum, depth, image = batch_composite_rays_train(sigmas, rgbs, deltas, rays, num_points, T_thresh)
                results = dict(weights_sum=weights_sum, depth=depth, image=image)
        elif self.render_mode == "fused" and self.fused_supported(code):
            results = self._forward_eval_fused(rays_o, rays_d, code, density_bitfield, grid_size, dt_gamma, T_thresh, bg_color)
        else:
            results = self._forward_eval_stepwise(rays_o, rays_d, code, density_bitfield, grid_size, dt_gamma, perturb, T_thresh)
        if return_loss:
            results.update(decoder_reg_loss=self.loss())
        return results

    def fused_supported(self, code) -> bool:
        return False

    #: False sends the train branch through one ``march_rays_train`` per scene (the reference's call pattern; parity / A-B runs)
    batched_train_march = os.environ.get("SSDNERF_TRAIN_MARCH_BATCH", "1") != "0"

    def _march_train_batch(self, rays_o, rays_d, bitfields, grid_size, dt_gamma, perturb):
        """All scenes' train-branch march in two library calls around ONE host read (the per-scene sample totals, needed to size the packed
        arrays); the reference -- and the per-scene path above -- reads one total per scene (raymarching.py:268-274) and allocates
        N * max_steps rows per scene.  rays_o / rays_d (S,N,3), bitfields (S, H^3/8); dt_gamma: float, list of floats, or a DEVICE tensor (S,)."""
        S, N, _ = rays_o.shape
        dev = rays_o.device
        ro, rd = rays_o.detach().float().contiguous(), rays_d.detach().float().contiguous()
        nears, fars = batch_near_far_from_aabb(ro, rd, self.aabb, self.min_near)
        if self.injected_noises is not None:
            nz = self.injected_noises
            noises = (torch.stack(list(nz)) if not isinstance(nz, torch.Tensor) else nz).to(dev).float().reshape(S, N).contiguous()
        elif perturb:
            noises = torch.rand(S, N, dtype=torch.float32, device=dev)
        else:
            noises = torch.zeros(S, N, dtype=torch.float32, device=dev)
        if isinstance(dt_gamma, torch.Tensor):
            dtg_scalar, dtgs = 0.0, dt_gamma.detach().to(dev).float().reshape(-1).contiguous()
            assert dtgs.numel() == S
        elif isinstance(dt_gamma, (list, tuple)):
            dtg_scalar, dtgs = 0.0, torch.tensor([float(v) for v in dt_gamma], dtype=torch.float32, device=dev)
        else:
            dtg_scalar, dtgs = float(dt_gamma), None
        bits = bitfields.contiguous()
        need = int(C.lib().ssdnerf_march_rays_train_batch_workspace(C.u32(S), C.u32(N)))
        ws = self._workspace(need, dev)
        offsets = torch.empty(S + 1, dtype=torch.int32, device=dev)
        common = (C.ptr(ro), C.ptr(rd), C.ptr(bits), C.f32(self.bound), C.f32(dtg_scalar), C.ptr(dtgs), C.u32(self.max_steps), C.u32(S), C.u32(N),
                  C.u32(1), C.u32(grid_size))
        C.check(C.lib().ssdnerf_march_rays_train_batch_count(*common, C.ptr(nears), C.ptr(fars), C.ptr(noises), C.ptr(offsets), C.ptr(ws),
                                                             C.ctypes.c_size_t(ws.numel()), C.stream()), "march_rays_train_batch_count")
        offs = offsets.tolist()                                  # the one device->host read of the train branch
        total = offs[-1]
        xyzs = torch.empty(total, 3, dtype=torch.float32, device=dev)
        dirs = torch.empty(total, 3, dtype=torch.float32, device=dev)
        deltas = torch.empty(total, 2, dtype=torch.float32, device=dev)
        rays = torch.empty(S * N, 3, dtype=torch.int32, device=dev)
        C.check(C.lib().ssdnerf_march_rays_train_batch_write(*common, C.u32(total), C.ptr(nears), C.ptr(fars), C.ptr(noises), C.ptr(xyzs), C.ptr(dirs),
                                                             C.ptr(deltas), C.ptr(rays), C.ptr(ws), C.ctypes.c_size_t(ws.numel()), C.stream()),
                "march_rays_train_batch_write")
        return xyzs, dirs, deltas, rays, [offs[s + 1] - offs[s] for s in range(S)]

    def _forward_eval_stepwise(self, rays_o, rays_d, code, density_bitfield, grid_size, dt_gamma, perturb, T_thresh):
        """The reference's alive-ray loop, verbatim in structure, over the unfused HIP operators."""
        nears, fars = batch_near_far_from_aabb(rays_o, rays_d, self.aabb, self.min_near)
        device = rays_o[0].device
        weights_sum, depth, image = [], [], []
        history = []
        for s in range(len(rays_o)):
            o_s, d_s = rays_o[s], rays_d[s]
            n = o_s.size(0)
            ws = torch.zeros(n, dtype=torch.float32, device=device)
            dp = torch.zeros(n, dtype=torch.float32, device=device)
            im = torch.zeros(n, 3, dtype=torch.float32, device=device)
            rays_alive = torch.arange(n, dtype=torch.int32, device=device)
            rays_t = nears[s].clone()
            step = 0
            hist = []
            while step < self.max_steps:
                n_alive = rays_alive.size(0)
                if n_alive == 0:
                    break
                n_step = min(max(n // n_alive, 1), 8)
                xyzs, dirs, deltas = march_rays(n_alive, n_step, rays_alive, rays_t, o_s, d_s, self.bound, density_bitfield[s], 1,
                                                grid_size[s], nears[s], fars[s], align=128, perturb=perturb, dt_gamma=dt_gamma[s],
                                                max_steps=self.max_steps)
                sigmas, rgbs, _ = self.point_decode([xyzs], [dirs], code[s][None])
                composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, ws, dp, im, T_thresh)
                hist.append((n_alive, n_step))
                rays_alive = rays_alive[rays_alive >= 0]
                step += n_step
            weights_sum.append(ws); depth.append(dp); image.append(im)
            history.append(hist)
        self.last_render_stats = dict(mode="stepwise", iterations=history)
        return dict(weights_sum=weights_sum, depth=depth, image=image)

    def _forward_eval_fused(self, rays_o, rays_d, code, density_bitfield, grid_size, dt_gamma, T_thresh, bg_color):
        raise NotImplementedError


@MODULES.register_module()
class TriPlaneDecoder(VolumeRenderer):
    activation_dict = {"relu": nn.ReLU, "silu": nn.SiLU, "softplus": nn.Softplus, "trunc_exp": TruncExp}

    def __init__(self, *args, interp_mode="bilinear", base_layers=[3 * 32, 128], density_layers=[128, 1],
                 color_layers=[128, 128, 3], use_dir_enc=True, dir_layers=None, scene_base_size=None, scene_rand_dims=(0, 1),
                 activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001, code_dropout=0.0, flip_z=False,
                 param_grad=None, **kwargs):
        super().__init__(*args, **kwargs)
        if param_grad is not None:                                       # None: the class default (SSDNERF_DECODE_PARAM_GRAD)
            if param_grad not in ("eager", "fused"):
                raise ValueError(f"param_grad must be 'eager' or 'fused', got {param_grad!r}")
            self.param_grad = param_grad
        base_layers, density_layers, color_layers = list(base_layers), list(density_layers), list(color_layers)
        self.interp_mode = interp_mode
        self.in_chn = base_layers[0]
        self.use_dir_enc = use_dir_enc
        if scene_base_size is None:
            self.scene_base = None
        else:
            rand_size = [1 for _ in scene_base_size]
            for dim in scene_rand_dims:
                rand_size[dim] = scene_base_size[dim]
            self.scene_base = nn.Parameter(torch.randn(rand_size).expand(scene_base_size).clone())
        self.dir_encoder = SHEncoder() if use_dir_enc else None
        self.sigmoid_saturation = sigmoid_saturation
        act = self.activation_dict[activation.lower()]
        self._activation_name, self._sigma_activation_name = activation.lower(), sigma_activation.lower()

        def mlp(layers, final=None):
            mods = []
            for i in range(len(layers) - 1):
                mods.append(nn.Linear(layers[i], layers[i + 1]))
                if i != len(layers) - 2:
                    mods.append(act())
            if final is not None:
                mods.append(final)
            return nn.Sequential(*mods)

        self.base_net = mlp(base_layers)
        self.base_activation = act()
        self.density_net = mlp(density_layers, self.activation_dict[sigma_activation.lower()]())
        self.dir_net = None
        if use_dir_enc:
            if dir_layers is not None:
                self.dir_net = mlp(list(dir_layers))
            else:
                color_layers[0] = color_layers[0] + 16
        self.color_net = mlp(color_layers, nn.Sigmoid())
        self.code_dropout = nn.Dropout2d(code_dropout) if code_dropout > 0 else None
        self.flip_z = flip_z
        self._layer_cfg = (tuple(base_layers), tuple(density_layers), tuple(color_layers), tuple(dir_layers) if dir_layers else None)
        self._packed: Optional[torch.Tensor] = None
        self._packed_key = None
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Linear):
                _xavier_uniform_(m)
        if self.dir_net is not None:
            nn.init.constant_(self.dir_net[-1].weight, 0.0)
            nn.init.constant_(self.dir_net[-1].bias, 0.0)

    # ------------------------------------------------------------------------------ fused-path plumbing
    def fused_supported(self, code=None) -> bool:
        ok = (self._layer_cfg == ((18, 64), (64, 1), (64, 3), (16, 64)) and self.use_dir_enc and self.interp_mode == "bilinear"
              and self._activation_name == "silu" and self._sigma_activation_name == "trunc_exp" and self.scene_base is None
              and not self.flip_z and (self.code_dropout is None or not self.training))
        if code is not None:
            ok = ok and code.dim() == 5 and code.size(1) == 3 and code.size(2) == 6 and code.is_cuda
        return ok

    def _mlp_parameters(self) -> List[torch.Tensor]:
        """the eight parameter tensors in pack order (``MLP_PARAM_KEYS``)"""
        cached = self.__dict__.get("_packed_ps")                         # (the four Linear modules, looked up once: Sequential.__getitem__ is slow)
        if cached is None:
            cached = self.__dict__["_packed_ps"] = (self.base_net[0], self.density_net[0], self.dir_net[0], self.color_net[0])
        return [p for m in cached for p in (m._parameters["weight"], m._parameters["bias"])]

    def packed_params(self) -> torch.Tensor:
        ps = self._mlp_parameters()
        key = tuple((p.data_ptr(), p._version, p.device.index, p.dtype) for p in ps)     # (writes through p.data bypass this: call invalidate_packed())
        if self._packed is None or key != self._packed_key:
            self._packed = pack_mlp_params({k: p.detach() for k, p in zip(MLP_PARAM_KEYS, ps)}, ps[0].device)
            self._packed_key = key
        return self._packed

    #: split products of the direction term formed by the MFMA shading kernel: 6 (default since r04: all of them, the fp32 class of the other
    #: layers, whatever the decoder's weights) or 3 (opt-in: 16 significand bits per factor of that additive term; <= 1.6e-6 on the image with
    #: Xavier-scale weights, growing with |Wd.SH(d)| |Wc|; the kernel is 5 % faster); SSDNERF_SHADE_DIR_PRODUCTS=3 sets the default of new decoders
    shade_dir_products = 3 if os.environ.get("SSDNERF_SHADE_DIR_PRODUCTS", "6") == "3" else 6

    def _shade_flags(self) -> int:
        return 0x100 if self.shade_dir_products != 3 else 0          # SSDNERF_SHADE_FULL_DIR_PRODUCTS (include/ssdnerf_hip.h)

    def invalidate_packed(self):
        """Forget the packed parameter block (re-packed on the next fused call).  Automatic after ``load_state_dict`` / ``.to()``; needed by hand
        only after writing weights through ``p.data``, which no version counter sees."""
        self._packed, self._packed_key = None, None
        self.__dict__.pop("_packed_ps", None)

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_packed()
        return out

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.invalidate_packed()
        return out

    # ------------------------------------------------------------------------------ decode
    def xyz_transform(self, xyz):
        if self.flip_z:
            xyz = torch.cat([xyz[..., :2], -xyz[..., 2:]], dim=-1)
        xy, xz, yz = xyz[..., :2], xyz[..., ::2], xyz[..., 1:]
        if xyz.dim() == 2:
            return torch.stack([xy, xz, yz], dim=0).unsqueeze(1)
        if xyz.dim() == 3:
            s, p, _ = xyz.size()
            return torch.stack([xy, xz, yz], dim=1).reshape(s * 3, 1, p, 2)
        raise ValueError

    def point_decode(self, xyzs, dirs, code, density_only=False):
        """xyzs/dirs: per-scene lists of (P_s,3) (or a (S,P,3) tensor); code (S,3,C,h,w).  Returns sigmas (sum P), rgbs (sum P,3),
        num_points (reference: triplane_decoder.py:119-179).  Uses the fused HIP decode when no gradient is required."""
        params_need_grad = any(p.requires_grad for p in self.parameters())
        need_grad = torch.is_grad_enabled() and (code.requires_grad or params_need_grad)
        if self.eager_decode:                                   # the reference-shaped baseline (bench.py gpu_baseline): grid_sample + nn.Linear
            return self.point_decode_eager(xyzs, dirs, code, density_only)
        if not need_grad and self.fused_supported(code):
            return self._point_decode_hip(xyzs, dirs, code, density_only)
        if ((self.param_grad == "fused" if params_need_grad else self.fused_code_grad) and not density_only and dirs is not None and code.is_cuda
                and self.fused_supported(code)):
            # fused forward AND backward: the code's gradient with the decoder frozen (guidance, val_optim / inverse_code), or -- a trainable decoder, opted in: the
            # closing joint iteration of a training step -- the parameters' and, when it needs one, the code's.  Dropout in training, scene_base, other layer shapes
            # and CPU tensors are not ``fused_supported``: eager, below
            if isinstance(xyzs, torch.Tensor):
                xyzs, dirs = list(xyzs), list(dirs)
            sigmas, rgbs = _PointDecodeFn.apply(code, *self._mlp_parameters(), self, xyzs, dirs)
            return sigmas, rgbs, [int(x.size(-2)) for x in xyzs]
        return self.point_decode_eager(xyzs, dirs, code, density_only)

    #: True forces ``point_decode`` through the eager PyTorch statement (measurement of the reference-shaped path only)
    eager_decode = False

    #: SSDNERF_DECODE_GRAD=0 sends the code-gradient decode through PyTorch autograd (grid_sample + nn.Linear) instead of the fused kernels
    fused_code_grad = os.environ.get("SSDNERF_DECODE_GRAD", "1") != "0"
    #: r06, opt-in (SSDNERF_DECODE_BWD_FEAT_MFMA=1): the decode backward's per-sample feature gradients on the matrix cores (csrc/decode_bwd.hip: k_decode_bwd_feat_mfma; bf16-pair
    #: products instead of fp32 FMAs).  Measured: 1.55 -> 1.27 ms on 7 M march-ordered samples, 1.60 -> 1.56 ms on uniformly scattered ones (the gather and the compaction are
    #: 0.4 - 0.6 ms of either), guided step -0.1 ms: not worth a lower arithmetic class by default.
    decode_bwd_feat_mfma = os.environ.get("SSDNERF_DECODE_BWD_FEAT_MFMA", "0") == "1"
    #: 'eager' (default): a decode whose decoder parameters need a gradient runs grid_sample + nn.Linear under autograd.  'fused' (opt-in: the constructor's
    #: ``param_grad=``, a config's decoder dict, or SSDNERF_DECODE_PARAM_GRAD=1 for the default of new decoders): the fused decode forward and the parameter
    #: gradients of csrc/decode_bwd_params.hip (``_PointDecodeFn``; fp32 fmas, no atomics, bit-reproducible)
    param_grad = "fused" if os.environ.get("SSDNERF_DECODE_PARAM_GRAD", "0") == "1" else "eager"

    def _point_decode_hip(self, xyzs, dirs, code, density_only, planes=None):
        if planes is None:
            planes = pack_triplanes(code.detach(), self.plane_dtype)
        params = self.packed_params()
        if isinstance(xyzs, torch.Tensor):
            xyzs = list(xyzs)
            dirs = list(dirs) if dirs is not None else None
        num_points = [int(x.size(-2)) for x in xyzs]
        total = sum(num_points)
        dev = code.device
        sigmas = torch.empty(total, dtype=torch.float32, device=dev)
        rgbs = None if density_only else torch.empty(total, 3, dtype=torch.float32, device=dev)
        off = 0
        _, _, hp, wp, _ = planes.shape
        for s, x in enumerate(xyzs):
            n = num_points[s]
            if n == 0:
                continue
            x = x.reshape(-1, 3).float().contiguous()
            d = None if density_only else dirs[s].reshape(-1, 3).float().contiguous()
            C.check(C.lib().ssdnerf_point_decode(C.ptr(planes[s]), C.dtype_code(planes), C.u32(hp), C.u32(wp), C.ptr(params), C.ptr(x),
                                                 C.ptr(d), C.u32(n), C.f32(self.sigmoid_saturation), C.ptr(sigmas[off:off + n]),
                                                 C.ptr(None if rgbs is None else rgbs[off:off + n]), C.stream()), "point_decode")
            off += n
        return sigmas, rgbs, num_points

    def point_decode_eager(self, xyzs, dirs, code, density_only=False):
        """PyTorch-ROCm eager statement of the reference decode (autograd-capable; baseline B1 of BASELINE.md)."""
        num_scenes, _, n_channels, h, w = code.size()
        if self.code_dropout is not None:
            code = self.code_dropout(code.reshape(num_scenes * 3, n_channels, h, w)).reshape(num_scenes, 3, n_channels, h, w)
        if self.scene_base is not None:
            code = code + self.scene_base
        if isinstance(xyzs, torch.Tensor):
            assert xyzs.dim() == 3
            num_points = xyzs.size(-2)
            point_code = F.grid_sample(code.reshape(num_scenes * 3, -1, h, w), self.xyz_transform(xyzs), mode=self.interp_mode,
                                       padding_mode="border", align_corners=False).reshape(num_scenes, 3, -1, num_points)
            point_code = point_code.permute(0, 3, 2, 1).reshape(num_scenes * num_points, -1)
            num_points = [num_points] * num_scenes
        else:
            num_points, pcs = [], []
            for code_s, xyz_s in zip(code, xyzs):
                n = xyz_s.size(-2)
                pc = F.grid_sample(code_s, self.xyz_transform(xyz_s), mode=self.interp_mode, padding_mode="border",
                                   align_corners=False).squeeze(-2)
                pcs.append(pc.permute(2, 1, 0).reshape(n, 3 * n_channels))
                num_points.append(n)
            point_code = torch.cat(pcs, dim=0) if len(pcs) > 1 else pcs[0]
        base_x = self.base_net(point_code)
        base_x_act = self.base_activation(base_x)
        sigmas = self.density_net(base_x_act).squeeze(-1)
        if density_only:
            return sigmas, None, num_points
        if self.use_dir_enc:
            dirs = torch.cat(list(dirs), dim=0) if num_scenes > 1 else dirs[0]
            sh_enc = self.dir_encoder(dirs)
            if self.dir_net is not None:
                color_in = self.base_activation(base_x + self.dir_net(sh_enc))
            else:
                color_in = torch.cat([base_x_act, sh_enc], dim=-1)
        else:
            color_in = base_x_act
        rgbs = self.color_net(color_in)
        if self.sigmoid_saturation > 0:
            rgbs = rgbs * (1 + self.sigmoid_saturation * 2) - self.sigmoid_saturation
        return sigmas, rgbs, num_points

    def point_density_decode(self, xyzs, code, **kwargs):
        sigmas, _, num_points = self.point_decode(xyzs, None, code, density_only=True, **kwargs)
        return sigmas, num_points

    def visualize(self, code, scene_name, viz_dir, code_range=[-1, 1], level=6):
        """``scene_<name>.png`` per scene under ``viz_dir``: the three planes of ``code`` (S, 3, C, h, w) as one viridis image of 3 h rows and C w
        columns, rows reversed within each plane unless ``flip_z`` (triplane_decoder.py:186-194; ``viz.write_code_planes``).  ``level`` (extra):
        the files' deflate level."""
        from .viz import write_code_planes
        return write_code_planes(viz_dir, code, scene_name, code_range=code_range, flip_z=self.flip_z, level=level)

    # ------------------------------------------------------------------------------ fused eval render
    def _forward_eval_fused(self, rays_o, rays_d, code, density_bitfield, grid_size, dt_gamma, T_thresh, bg_color):
        planes = pack_triplanes(code.detach(), self.plane_dtype)
        out = self.render_packed(planes, rays_o, rays_d, density_bitfield, grid_size, dt_gamma, T_thresh, bg_color, check_overflow=False)
        if int(self.last_render_stats["overflow"].item()) != 0:   # one sync per batch (the reference: one per loop iteration)
            # a ray reached the reference loop's global step cap, where the reference's answer depends on its n_step
            # schedule: redo the batch through the reference-shaped stepwise path (exact by construction).
            out = self._forward_eval_stepwise(rays_o, rays_d, code, density_bitfield, grid_size, dt_gamma, False, T_thresh)
            if bg_color is not None:
                out["image"] = [im + float(bg_color) * (1 - ws.unsqueeze(-1)) for im, ws in zip(out["image"], out["weights_sum"])]
                out["blended"] = True
        return out

    def render_packed(self, planes, rays_o, rays_d, density_bitfield, grid_size, dt_gamma, T_thresh=1e-4, bg_color=None,
                      want_counts=False, check_overflow=True, cams=None, want_u8=False, prefetch=None):
        """Fused render of S scenes from already-packed planes (S,3,h,w,8).  ``want_u8`` (camera-fed renders with a background colour): the result
        also carries ``image_u8`` (S,N,3) uint8 -- the image quantised as ``eval_and_viz`` does, written by the render kernels themselves.

        rays_o/rays_d: a dense (S,N,3) tensor -> ONE launch for the whole batch (outputs are (S,N,3)/(S,N) tensors, indexable
        per scene like the reference's lists); or per-scene lists of (N_s,3) -> one launch per scene.
        cams=(c2w (S,V,4,4), intrinsics (S,V,4), h, w) instead of ray arrays (rays_o = rays_d = None): the kernels generate ray n =
        pixel n % (h*w) of view n // (h*w) themselves (the arithmetic of ``nerf.get_cam_rays``), N = V*h*w.
        dt_gamma: per-scene list of floats, or a DEVICE tensor (S,) (no host sync).
        prefetch (camera-fed renders, r06): ``dict(cams=..., density_bitfield=...)`` of the NEXT call on this decoder (same grid size, cone angles, background and
        ``want_u8``).  Stage A of that render -- cull + survivor march, which needs neither the planes nor anything this render produces -- is launched NOW on a second
        stream, with its own workspace and output tensors, and runs beside this render's shading kernel; the next call recognises its inputs (same tensors, unchanged)
        and only launches its shading kernel.  The next render's inputs must be complete on the current stream when this call is made; a next call with other inputs
        just renders normally.  Streaming loops over cached scenes: 5.4 -> 5.0 ms per render of the bench workload (profiles/r06/i_pipeline_probe.txt)."""
        if cams is not None:
            assert rays_o is None and rays_d is None, "render_packed: give ray arrays or cameras, not both"
            return self._render_packed_cams(planes, cams, density_bitfield, grid_size, dt_gamma, T_thresh, bg_color, want_counts, check_overflow, want_u8, prefetch)
        params = self.packed_params()
        num_scenes = len(rays_o)
        dev = planes.device
        _, _, hp, wp, _ = planes.shape
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        blend = 0.0 if bg_color is None else float(bg_color)
        gs = grid_size if isinstance(grid_size, int) else grid_size[0]
        if not isinstance(grid_size, int):
            assert all(g == gs for g in grid_size), "one grid size per batch"
        dense = isinstance(rays_o, torch.Tensor) and rays_o.dim() == 3
        boundary = None
        if isinstance(dt_gamma, torch.Tensor):
            dtg_dev, dtg_host = dt_gamma.float().contiguous(), None
        else:
            dtg_host = [float(g) for g in dt_gamma]
            dtg_dev = None
            if dense and not all(g == dtg_host[0] for g in dtg_host):
                dtg_dev = torch.tensor(dtg_host, dtype=torch.float32, device=dev)
        bits = density_bitfield if isinstance(density_bitfield, torch.Tensor) else torch.stack(list(density_bitfield), dim=0)
        bits = bits.contiguous()
        if dense:
            o = rays_o.float().contiguous()
            d = rays_d.float().contiguous()
            n = o.size(1)
            im = torch.empty(num_scenes, n, 3, dtype=torch.float32, device=dev)
            dp = torch.empty(num_scenes, n, dtype=torch.float32, device=dev)
            ws = torch.empty(num_scenes, n, dtype=torch.float32, device=dev)
            cn = torch.empty(num_scenes, n, dtype=torch.int32, device=dev) if want_counts else None
        if dense and self.fused_pipeline in ("queue", "queue_mfma") and gs >= 8 and (gs & (gs - 1)) == 0:
            g0 = 0.0 if dtg_host is None else dtg_host[0]
            need = C.lib().ssdnerf_render_queue_workspace(num_scenes, n, gs)
            wsp = self._workspace(need, dev)
            ev = self.stage_events
            if ev is not None:
                ev.append(torch.cuda.Event(enable_timing=True)); ev[-1].record()
            C.check(C.lib().ssdnerf_render_first_hit(
                C.ptr(bits), C.u32(gs), C.ptr(o), C.ptr(d), C.u32(num_scenes), C.u32(n), C.f32(self.bound), C.f32(self.min_near), C.f32(g0),
                C.ptr(dtg_dev), C.u32(self.max_steps), C.f32(blend), C.ptr(im), C.ptr(dp), C.ptr(ws), C.ptr(cn), C.ptr(wsp),
                C.ctypes.c_size_t(wsp.numel()), C.stream()), "render_first_hit")
            if ev is not None:
                ev.append(torch.cuda.Event(enable_timing=True)); ev[-1].record()
            shade = C.lib().ssdnerf_render_shade_queue_mfma if self.fused_pipeline == "queue_mfma" else C.lib().ssdnerf_render_shade_queue
            C.check(shade(
                C.ptr(planes), C.dtype_code(planes) | (self._shade_flags() if self.fused_pipeline == "queue_mfma" else 0), C.u32(hp), C.u32(wp), C.ptr(params), C.u32(gs), C.ptr(o), C.ptr(d), C.u32(num_scenes),
                C.u32(n), C.f32(self.bound), C.f32(self.min_near), C.f32(g0), C.ptr(dtg_dev), C.u32(self.max_steps), C.f32(T_thresh),
                C.f32(blend), C.f32(self.sigmoid_saturation), C.ptr(im), C.ptr(dp), C.ptr(ws), C.ptr(cn), C.ptr(overflow), C.ptr(wsp),
                C.ctypes.c_size_t(wsp.numel()), C.stream()), "render_shade_queue")
            if ev is not None:
                ev.append(torch.cuda.Event(enable_timing=True)); ev[-1].record()
            weights_sum, depth, image, counts = ws, dp, im, cn
            boundary = self._boundary_tests(wsp, num_scenes) if want_counts and self.fused_pipeline == "queue_mfma" else None
        elif dense:
            C.check(C.lib().ssdnerf_render_rays_fused_batch(
                C.ptr(planes), C.dtype_code(planes), C.u32(hp), C.u32(wp), C.ptr(params), C.ptr(bits), C.u32(gs), C.ptr(o), C.ptr(d),
                C.u32(num_scenes), C.u32(n), C.f32(self.bound), C.f32(self.min_near), C.f32(0.0 if dtg_host is None else dtg_host[0]),
                C.ptr(dtg_dev), C.u32(self.max_steps), C.f32(T_thresh), C.f32(blend), C.f32(self.sigmoid_saturation), C.ptr(im), C.ptr(dp),
                C.ptr(ws), C.ptr(cn), C.ptr(overflow), C.stream()), "render_rays_fused_batch")
            weights_sum, depth, image, counts = ws, dp, im, cn
        else:
            weights_sum, depth, image, counts = [], [], [], []
            for s in range(num_scenes):
                o = rays_o[s].reshape(-1, 3).float().contiguous()
                d = rays_d[s].reshape(-1, 3).float().contiguous()
                n = o.size(0)
                im = torch.empty(n, 3, dtype=torch.float32, device=dev)
                dp = torch.empty(n, dtype=torch.float32, device=dev)
                ws = torch.empty(n, dtype=torch.float32, device=dev)
                cn = torch.empty(n, dtype=torch.int32, device=dev) if want_counts else None
                g_s = float(dtg_dev[s]) if dtg_host is None else dtg_host[s]
                C.check(C.lib().ssdnerf_render_rays_fused(
                    C.ptr(planes[s]), C.dtype_code(planes), C.u32(hp), C.u32(wp), C.ptr(params), C.ptr(bits[s]), C.u32(gs), C.ptr(o),
                    C.ptr(d), C.u32(n), C.f32(self.bound), C.f32(self.min_near), C.f32(g_s), C.u32(self.max_steps), C.f32(T_thresh),
                    C.f32(blend), C.f32(self.sigmoid_saturation), C.ptr(im), C.ptr(dp), C.ptr(ws), C.ptr(cn), C.ptr(overflow), C.stream()),
                    "render_rays_fused")
                weights_sum.append(ws); depth.append(dp); image.append(im); counts.append(cn)
        self.last_render_stats = dict(mode="fused", overflow=overflow, sample_counts=counts if want_counts else None,
                                      boundary_tests=boundary if dense and want_counts else None)
        if check_overflow and int(overflow.item()) != 0:
            raise RuntimeError("render_rays_fused: a ray hit the max_steps cap; use render_mode='stepwise' for this batch")
        return dict(weights_sum=weights_sum, depth=depth, image=image, blended=bg_color is not None)

    @staticmethod
    def _boundary_tests(wsp, num_scenes):
        """per-scene count of termination tests that landed within 2e-6 of T_thresh (diagnostic counters at the head of the workspace)"""
        return wsp[:4 * num_scenes * 128].view(torch.int32).view(4, num_scenes, 32)[3, :, 0].clone()        # csrc/common.h: ssd_counter(SSD_CNT_BOUNDARY, ...)

    def _render_packed_cams(self, planes, cams, density_bitfield, grid_size, dt_gamma, T_thresh, bg_color, want_counts, check_overflow, want_u8=False, prefetch=None):
        c2w, intr, h, w = cams
        dev = planes.device
        num_scenes, nv = int(c2w.shape[0]), int(c2w.shape[1])
        gs = grid_size if isinstance(grid_size, int) else grid_size[0]
        if self.fused_pipeline != "queue_mfma" or gs < 8 or (gs & (gs - 1)) != 0:
            from .nerf import get_cam_rays                                   # forms without in-kernel ray generation: materialise the arrays
            o, d = get_cam_rays(c2w, intr, h, w)
            out = self.render_packed(planes, o.reshape(num_scenes, -1, 3), d.reshape(num_scenes, -1, 3), density_bitfield, grid_size, dt_gamma,
                                     T_thresh, bg_color, want_counts, check_overflow)
            if want_u8:
                from .nerf import quantize_u8
                out["image_u8"] = quantize_u8(out["image"])
            return out
        params = self.packed_params()
        _, _, hp, wp, _ = planes.shape
        blend = 0.0 if bg_color is None else float(bg_color)
        if isinstance(dt_gamma, torch.Tensor):
            dtg_dev, g0 = dt_gamma.float().contiguous(), 0.0
        else:
            host = [float(g) for g in dt_gamma]
            g0 = host[0]
            dtg_dev = None if all(g == g0 for g in host) else torch.tensor(host, dtype=torch.float32, device=dev)
        main = torch.cuda.current_stream()
        ev = self.stage_events
        if ev is not None:
            ev.append(torch.cuda.Event(enable_timing=True)); ev[-1].record()
        # ---- stage A: cull + survivor march -> hit queues in the workspace, background pixels in the outputs; or the one a previous call launched ahead
        st, parity = None, 0                                                 # two workspaces: a render's own, and the one stage A of the NEXT render is launched into
        pre = self.__dict__.pop("_prefetched", None)
        if pre is not None:
            main.wait_event(pre["event"])                                    # (also when it is not used: nothing of it is in flight behind this point)
            if not want_counts and pre["key"] == self._stage_a_key(density_bitfield, c2w, intr, h, w, gs, g0, dtg_dev, blend, want_u8):
                st, parity = pre["stage"], pre["parity"]
        if st is None:
            st = self._stage_a(density_bitfield, c2w, intr, h, w, gs, g0, dtg_dev, blend, want_counts, want_u8, parity, small_blocks=False)
        if prefetch is not None and not want_counts:
            n_c2w, n_intr, n_h, n_w = prefetch["cams"]
            n_bits = prefetch["density_bitfield"]
            n_key = self._stage_a_key(n_bits, n_c2w, n_intr, n_h, n_w, gs, g0, dtg_dev, blend, want_u8)
            side = self.__dict__.get("_side_stream")
            if side is None:
                side = self._side_stream = torch.cuda.Stream(device=dev)
            ready = torch.cuda.Event()
            ready.record(main)                                               # the next render's inputs are complete here; this render's shading kernel is queued BEHIND this point
            # the next render's tensors come from the current stream's pool (allocated here, first written on the side stream, then only by work the main stream orders
            # behind the side stream's event): a later reuse of their memory is ordered behind every use
            n_st = self._stage_a(n_bits, n_c2w, n_intr, n_h, n_w, gs, g0, dtg_dev, blend, False, want_u8, parity ^ 1, small_blocks=True, stream=side, after=ready)
            done = torch.cuda.Event()
            done.record(side)
            self._prefetched = dict(key=n_key, stage=n_st, event=done, parity=parity ^ 1)
        if ev is not None:
            ev.append(torch.cuda.Event(enable_timing=True)); ev[-1].record()
        # ---- stage B: the shading kernel over the queues
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        im, dp, ws, cn, im8, wsp, pose, k = st["im"], st["dp"], st["ws"], st["cn"], st["im8"], st["wsp"], st["pose"], st["k"]
        C.check(C.lib().ssdnerf_render_shade_queue_mfma_cams(
            C.ptr(planes), C.dtype_code(planes) | self._shade_flags(), C.u32(hp), C.u32(wp), C.ptr(params), C.u32(gs), C.ptr(pose), C.ptr(k), C.u32(num_scenes), C.u32(nv),
            C.u32(h), C.u32(w), C.f32(self.bound), C.f32(self.min_near), C.f32(g0), C.ptr(dtg_dev), C.u32(self.max_steps), C.f32(T_thresh), C.f32(blend),
            C.f32(self.sigmoid_saturation), C.ptr(im), C.ptr(dp), C.ptr(ws), C.ptr(cn), C.ptr(overflow), C.ptr(im8), C.ptr(wsp),
            C.ctypes.c_size_t(wsp.numel()), C.stream()), "render_shade_queue_mfma_cams")
        if ev is not None:
            ev.append(torch.cuda.Event(enable_timing=True)); ev[-1].record()
        self.last_render_stats = dict(mode="fused", overflow=overflow, sample_counts=cn if want_counts else None,
                                      boundary_tests=self._boundary_tests(wsp, num_scenes) if want_counts else None)
        if check_overflow and int(overflow.item()) != 0:
            raise RuntimeError("render_rays_fused: a ray hit the max_steps cap; use render_mode='stepwise' for this batch")
        out = dict(weights_sum=ws, depth=dp, image=im, blended=bg_color is not None)
        if im8 is not None:
            out["image_u8"] = im8
        return out

    @staticmethod
    def _stage_a_key(bits, c2w, intr, h, w, gs, g0, dtg_dev, blend, want_u8):
        """what decides stage A's results: the tensors (identity and in-place version) and the scalars"""
        def ident(t):
            return None if t is None else (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype) if isinstance(t, torch.Tensor) else tuple(id(x) for x in t)
        return (ident(bits), ident(c2w), ident(intr), int(h), int(w), int(gs), float(g0), ident(dtg_dev), float(blend), bool(want_u8))

    def _stage_a(self, density_bitfield, c2w, intr, h, w, gs, g0, dtg_dev, blend, want_counts, want_u8, parity, small_blocks, stream=None, after=None):
        """allocate a render's outputs and launch ``ssdnerf_render_first_hit_cams`` into workspace ``parity`` -- on the current stream, or on ``stream`` behind the event
        ``after`` (everything is allocated and prepared on the CURRENT stream first)"""
        num_scenes, nv = int(c2w.shape[0]), int(c2w.shape[1])
        dev = c2w.device
        pose = c2w.detach().to(torch.float32).reshape(num_scenes, nv, 16).contiguous()
        k = intr.detach().to(torch.float32).expand(num_scenes, nv, 4).contiguous()
        bits = density_bitfield if isinstance(density_bitfield, torch.Tensor) else torch.stack(list(density_bitfield), dim=0)
        bits = bits.contiguous()
        n = nv * h * w
        im = torch.empty(num_scenes, n, 3, dtype=torch.float32, device=dev)
        dp = torch.empty(num_scenes, n, dtype=torch.float32, device=dev)
        ws = torch.empty(num_scenes, n, dtype=torch.float32, device=dev)
        cn = torch.empty(num_scenes, n, dtype=torch.int32, device=dev) if want_counts else None
        im8 = torch.empty(num_scenes, n, 3, dtype=torch.uint8, device=dev) if want_u8 else None      # the quantised image, written by the same kernels
        wsp = self._workspace(C.lib().ssdnerf_render_queue_workspace(num_scenes, n, gs), dev, tag=f"render{parity}")
        flags = 0x10000 if small_blocks else 0                               # SSDNERF_FIRST_HIT_SMALL_BLOCKS (include/ssdnerf_hip.h)

        def launch():
            C.check(C.lib().ssdnerf_render_first_hit_cams(
                C.ptr(bits), C.u32(gs | flags), C.ptr(pose), C.ptr(k), C.u32(num_scenes), C.u32(nv), C.u32(h), C.u32(w), C.f32(self.bound), C.f32(self.min_near),
                C.f32(g0), C.ptr(dtg_dev), C.u32(self.max_steps), C.f32(blend), C.ptr(im), C.ptr(dp), C.ptr(ws), C.ptr(cn), C.ptr(im8), C.ptr(wsp),
                C.ctypes.c_size_t(wsp.numel()), C.stream()), "render_first_hit_cams")
        if stream is None:
            launch()
        else:
            with torch.cuda.stream(stream):
                if after is not None:
                    stream.wait_event(after)
                launch()
        return dict(im=im, dp=dp, ws=ws, cn=cn, im8=im8, wsp=wsp, pose=pose, k=k, bits=bits)

    def drop_prefetch(self):
        """forget a stage A launched ahead by ``render_packed(..., prefetch=...)`` that no render will use (end of a streaming loop); the current stream waits for it"""
        pre = self.__dict__.pop("_prefetched", None)
        if pre is not None:
            torch.cuda.current_stream().wait_event(pre["event"])
