"""LPIPS v0.1 with the VGG16 trunk (``lpips.LPIPS(net='vgg')``), the reference's third test-view score (``eval_and_viz``, base_nerf.py:560-570), on
this library's HIP kernels: the thirteen 3 x 3 convolutions are ``conv2d_nhwc_f32x2`` / ``_presplit`` (csrc/conv_igemm.hip, fp32-class products),
everything between them is one pass of csrc/lpips.hip per activation.

No weights ship with this project.  ``LPIPSVGG.load(path)`` / ``from_state_dict`` take a state dict of the ``lpips`` package or a torchvision
``vgg16`` dict merged with the five ``lin`` tensors; ``synthetic.make_lpips_params`` makes seeded random ones for tests and benchmarks."""
from __future__ import annotations

import ctypes
import re
from typing import Dict, List, Optional, Tuple

import torch

from . import _cabi as C

# torchvision's vgg16().features: index of every convolution, (Cin, Cout); a 2 x 2 max-pool follows convolutions 2, 4, 7 and 10
FEATURE_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512), (512, 512), (512, 512),
            (512, 512))
TAPS = (1, 3, 6, 9, 12)                      # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 as positions in FEATURE_IDX; every tap but the last is pooled
TAP_CHANNELS = (64, 128, 256, 512, 512)
CIN_PAD = 8                                  # the convolution kernels take channel counts that are multiples of 8: RGB + five zero channels
MIN_SIZE = 16                                # four floor-mode pools must leave at least one pixel
_LIMIT = 1 << 31                             # the convolutions address a tensor with 31 bits

_LIN_KEY = re.compile(r"(?:^|\.)lin(?:s\.)?(\d)(?:\.|$)")
# <idx>.weight|bias directly under ``features`` or a ``slice<k>`` of the lpips package, or bare (a dict of ``vgg16().features`` itself); not under
# ``classifier`` or any other module, whose indices overlap the trunk's
_TRUNK_KEY = re.compile(r"(?:^|(?:^|\.)(?:features|slice\d+)\.)(\d+)\.(weight|bias)$")


# ---- the three kernels of csrc/lpips.hip on torch tensors: activations are (B, C, H, W) channels_last, as everywhere in unet_fast ---------------------------
def _nhwc(x: torch.Tensor, what: str):
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError(f"{what}: fp32 (B, C, H, W) channels_last GPU tensor")
    return x.shape


def lpips_input(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """two (n, h, w, 3) fp32 contiguous image sets in [0, 1] -> the trunk's input (2n, 8, h, w) channels_last: scaled as the lpips package's scaling
    layer does, predictions first, channels 3 .. 7 zero"""
    if pred.shape != target.shape or pred.dim() != 4 or pred.shape[-1] != 3 or pred.dtype != torch.float32 or target.dtype != torch.float32 \
            or not (pred.is_cuda and target.is_cuda and pred.is_contiguous() and target.is_contiguous()):
        raise RuntimeError("lpips_input: two contiguous fp32 (n, h, w, 3) GPU tensors of one shape")
    n, h, w = pred.shape[:3]
    out = torch.empty((2 * n, CIN_PAD, h, w), dtype=torch.float32, device=pred.device, memory_format=torch.channels_last)
    C.check(C.lib().ssdnerf_lpips_input(C.ptr(pred), C.ptr(target), C.u32(n), C.u32(h), C.u32(w), C.ptr(out), C.stream()), "lpips_input")
    return out


def relu_pool_nhwc(x: torch.Tensor, pool: bool = False, split_out: bool = False) -> torch.Tensor:
    """ReLU of a convolution's output, with ``pool`` followed by the 2 x 2 / stride 2 max-pool (floor mode); ``split_out``: the result is the carrier
    tensor of its PRE-SPLIT form (``unet_fast.split_f32_nhwc`` of the plain result) for ``conv2d_nhwc_f32x2_presplit``"""
    B, Cc, H, W = _nhwc(x, "relu_pool_nhwc")
    y = torch.empty((B, Cc, H // 2, W // 2) if pool else (B, Cc, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    C.check(C.lib().ssdnerf_relu_pool_nhwc(C.ptr(x), C.u32(B), C.u32(H), C.u32(W), C.u32(Cc), int(pool), int(split_out), C.ptr(y), C.stream()), "relu_pool_nhwc")
    return y


def lpips_layer(x: torch.Tensor, lin_w: torch.Tensor, acc: torch.Tensor, pool_out: bool = True, split_out: bool = False) -> Optional[torch.Tensor]:
    """One tap: ``x`` (2n, C, H, W) is a tapped convolution's raw output for n predictions and their n targets, ``lin_w`` (C,) the tap's weight;
    ``acc`` (n,) fp32 += the pairs' distances at this tap.  Returns the pooled ReLU output for the next stage (``relu_pool_nhwc(x, True, split_out)``'s
    bytes) unless ``pool_out`` is unset."""
    B, Cc, H, W = _nhwc(x, "lpips_layer")
    n = B // 2
    if B % 2 or acc.shape != (n,) or acc.dtype != torch.float32 or not acc.is_contiguous() or lin_w.shape != (Cc,) or lin_w.dtype != torch.float32 \
            or not lin_w.is_contiguous() or acc.device != x.device or lin_w.device != x.device:
        raise RuntimeError("lpips_layer: x (2n, C, H, W), lin_w (C,) and acc (n,) fp32 contiguous on one GPU")
    y = torch.empty((B, Cc, H // 2, W // 2), dtype=torch.float32, device=x.device, memory_format=torch.channels_last) if pool_out else None
    ws = torch.empty(int(C.lib().ssdnerf_lpips_layer_workspace(C.u32(n))) // 8, dtype=torch.float64, device=x.device)
    C.check(C.lib().ssdnerf_lpips_layer(C.ptr(x), C.u32(n), C.u32(H), C.u32(W), C.u32(Cc), C.ptr(lin_w), C.ptr(acc), C.ptr(y), int(split_out), C.ptr(ws),
                                        C.stream()), "lpips_layer")
    return y


def _match_state_dict(sd: Dict[str, torch.Tensor]) -> Tuple[List[torch.Tensor], List[torch.Tensor], List[torch.Tensor]]:
    """trunk weights, trunk biases and lin weights of ``sd``, matched by the index in ``features`` (any prefix: ``features.<idx>``,
    ``net.slice<k>.<idx>``) and by ``lin<k>`` / ``lins.<k>``; other modules' tensors (``classifier.<idx>``, the scaling layer) are passed over; the same
    tensor under two names (the lpips package registers its lin layers twice) is accepted when the copies are equal"""
    found: Dict[Tuple[str, int], Tuple[str, torch.Tensor]] = {}

    def put(slot, key, value):
        if slot in found and not (found[slot][1].shape == value.shape and torch.equal(found[slot][1], value)):
            raise ValueError(f"LPIPSVGG: {key!r} and {found[slot][0]!r} name the same tensor with different contents")
        found.setdefault(slot, (key, value))

    for key, value in sd.items():
        if not torch.is_tensor(value):
            continue
        m = _LIN_KEY.search(key)
        if m is not None:
            if key.endswith("weight") and int(m.group(1)) < len(TAPS):
                put(("lin", int(m.group(1))), key, value)
            continue
        m = _TRUNK_KEY.search(key)
        if m is not None and int(m.group(1)) in FEATURE_IDX:
            put((m.group(2), FEATURE_IDX.index(int(m.group(1)))), key, value)
    weights, biases, lins = [], [], []
    for i, (idx, (cin, cout)) in enumerate(zip(FEATURE_IDX, CHANNELS)):
        for kind, shape, out in (("weight", (cout, cin, 3, 3), weights), ("bias", (cout,), biases)):
            if (kind, i) not in found:
                raise KeyError(f"LPIPSVGG: no tensor for features.{idx}.{kind} (the trunk's convolution {i + 1}) in the state dict")
            key, value = found[(kind, i)]
            if tuple(value.shape) != shape:
                raise ValueError(f"LPIPSVGG: {key!r} has shape {tuple(value.shape)}, expected {shape}")
            out.append(value.detach().to(torch.float32))
    for k, c in enumerate(TAP_CHANNELS):
        if ("lin", k) not in found:
            raise KeyError(f"LPIPSVGG: no tensor for lin{k} (lin{k}.model.1.weight or lins.{k}.model.1.weight) in the state dict")
        key, value = found[("lin", k)]
        if tuple(value.shape) not in ((1, c, 1, 1), (c,)):
            raise ValueError(f"LPIPSVGG: {key!r} has shape {tuple(value.shape)}, expected (1, {c}, 1, 1) or ({c},)")
        lins.append(value.detach().to(torch.float32).reshape(c))
    return weights, biases, lins


class LPIPSVGG:
    """``net(pred, target, chunk=32)`` -> LPIPS per pair.  Not an ``nn.Module``: a model holds it outside its ``state_dict()`` (the reference keeps its
    net in a plain list for the same reason).  Weights are prepared once per device: split into the bf16 pair of the convolution kernels, channels
    last, the first layer's three input channels zero-padded to eight.

    Calls on one device must be ordered on one stream: the intermediate buffers are kept per device from call to call (and grown when a call needs
    more), and the convolutions use ``unet_fast.shared_splitk_ws``.  At chunk 32 and 128 x 128 the two buffers hold 268 MB each;
    ``release_buffers()`` gives them back."""

    def __init__(self, weights: List[torch.Tensor], biases: List[torch.Tensor], lins: List[torch.Tensor]):
        w0 = weights[0].detach().to("cpu", torch.float32)
        w0 = torch.cat([w0, w0.new_zeros(w0.shape[0], CIN_PAD - w0.shape[1], 3, 3)], dim=1)
        self._weights = [w0] + [w.detach().to("cpu", torch.float32) for w in weights[1:]]
        self._biases = [b.detach().to("cpu", torch.float32) for b in biases]
        self._lins = [l.detach().to("cpu", torch.float32).reshape(-1) for l in lins]
        self._dev: Dict[torch.device, tuple] = {}
        self._bufs: Dict[torch.device, tuple] = {}

    @classmethod
    def from_state_dict(cls, sd: Dict[str, torch.Tensor]) -> "LPIPSVGG":
        return cls(*_match_state_dict(sd))

    @classmethod
    def load(cls, path: str) -> "LPIPSVGG":
        sd = torch.load(path, map_location="cpu")
        return cls.from_state_dict(sd.get("state_dict", sd) if isinstance(sd, dict) else sd)

    # ---- per-device state ------------------------------------------------------------------------------------------------------------------------
    def _params(self, device: torch.device):
        """[(w_hi, w_lo, bias)] * 13 and [lin] * 5 on ``device``, made on first use: each weight pair is one buffer, lo directly behind hi"""
        if device not in self._dev:
            from .unet_fast import split_bf16x2_adjacent
            convs = [split_bf16x2_adjacent(w.to(device)) + (b.to(device),) for w, b in zip(self._weights, self._biases)]
            self._dev[device] = (convs, [l.to(device) for l in self._lins])
        return self._dev[device]

    def _buffers(self, device: torch.device, floats: int, pairs: int):
        """two flat fp32 buffers of at least ``floats`` elements (convolution outputs; activations) and the fp64 partial sums of ``pairs`` pairs: kept
        from chunk to chunk and from call to call, replaced by larger ones when a call needs more"""
        doubles = int(C.lib().ssdnerf_lpips_layer_workspace(C.u32(pairs))) // 8
        cur = self._bufs.get(device)
        if cur is None or cur[0].numel() < floats or cur[2].numel() < doubles:
            if cur is not None:
                floats, doubles = max(floats, cur[0].numel()), max(doubles, cur[2].numel())
            self._bufs[device] = cur = None                                      # (the old ones go before the new are allocated)
            self._bufs[device] = cur = (torch.empty(floats, dtype=torch.float32, device=device), torch.empty(floats, dtype=torch.float32, device=device),
                                        torch.empty(doubles, dtype=torch.float64, device=device))
        return cur

    def release_buffers(self) -> None:
        """drop the kept intermediate buffers of every device (the next call allocates them again); the prepared weights stay"""
        self._bufs.clear()

    # ---- the trunk on one chunk ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def max_chunk(h: int, w: int) -> int:
        """pairs per chunk for which the largest tensor, the 64-channel activations of both image sets at full size, stays below 2^31 bytes"""
        return (_LIMIT - 1) // (2 * h * w * 64 * 4)

    def _run_chunk(self, pred: torch.Tensor, target: torch.Tensor, acc: torch.Tensor) -> None:
        """``acc`` (n,) fp32, zero on entry, += the five taps of the n pairs ``pred[i]``, ``target[i]`` ((n, h, w, 3) fp32 contiguous)"""
        from .unet_fast import shared_splitk_ws
        lib, st = C.lib(), C.stream()
        n, h, w = pred.shape[:3]
        B = 2 * n
        convs, lins = self._params(pred.device)
        raw, act, ws = self._buffers(pred.device, B * h * w * 64, n)
        sk = shared_splitk_ws(pred.device)
        sk_bytes = ctypes.c_size_t(sk.numel() * 4)
        # the spatial size each convolution runs at, and whether it takes its input PRE-SPLIT (then whatever writes that input writes it so)
        sizes, H, W = [], h, w
        for i in range(len(FEATURE_IDX)):
            sizes.append((H, W))
            if i in TAPS[:-1]:
                H, W = H // 2, W // 2
        ps = [cin % 32 == 0 and int(lib.ssdnerf_conv2d_nhwc_f32x2_presplit_supported(C.u32(B), C.u32(H), C.u32(W), C.u32(cin), C.u32(cout), C.u32(3), 0)) != 0
              for (cin, cout), (H, W) in zip(CHANNELS, sizes)]
        C.check(lib.ssdnerf_lpips_input(C.ptr(pred), C.ptr(target), C.u32(n), C.u32(h), C.u32(w), C.ptr(act), st), "lpips_input")
        tap = 0
        for i, ((cin, cout), (H, W), (w_hi, w_lo, bias)) in enumerate(zip(CHANNELS, sizes, convs)):
            cin = max(cin, CIN_PAD)
            if ps[i]:
                C.check(lib.ssdnerf_conv2d_nhwc_f32x2_presplit(C.ptr(act), C.ptr(w_hi), C.ptr(w_lo), C.ptr(bias), C.ptr(None), C.ptr(raw), C.u32(B), C.u32(H), C.u32(W),
                                                               C.u32(cin), C.u32(cout), C.u32(3), C.ptr(None), C.u32(0), 0, 0, C.ptr(sk), sk_bytes, st),
                        "conv2d_nhwc_f32x2_presplit")
            else:
                C.check(lib.ssdnerf_conv2d_nhwc_f32x2(C.ptr(act), C.ptr(None), C.u32(cin), C.ptr(w_hi), C.ptr(w_lo), C.ptr(bias), C.ptr(None), C.ptr(raw), C.u32(B),
                                                      C.u32(H), C.u32(W), C.u32(cin), C.u32(cout), C.u32(3), C.u32(1), C.u32(0), C.ptr(None), C.u32(0), 0, 0, 0,
                                                      C.ptr(sk), sk_bytes, st), "conv2d_nhwc_f32x2")
            split_next = int(i + 1 < len(ps) and ps[i + 1])
            if i in TAPS:
                last = i == TAPS[-1]
                C.check(lib.ssdnerf_lpips_layer(C.ptr(raw), C.u32(n), C.u32(H), C.u32(W), C.u32(cout), C.ptr(lins[tap]), C.ptr(acc), C.ptr(None if last else act),
                                                split_next, C.ptr(ws), st), "lpips_layer")
                tap += 1
            else:
                C.check(lib.ssdnerf_relu_pool_nhwc(C.ptr(raw), C.u32(B), C.u32(H), C.u32(W), C.u32(cout), 0, split_next, C.ptr(act), st), "relu_pool_nhwc")

    def __call__(self, pred: torch.Tensor, target: torch.Tensor, chunk: int = 32) -> torch.Tensor:
        """LPIPS of every pair of two ``(..., h, w, 3)`` fp32 GPU tensors of equal shape with values in [0, 1], as an fp32 tensor of the leading
        shape.  Pairs are worked on ``chunk`` at a time (the reference's ``LPIPS_BS``; fewer when a tensor would reach 2^31 bytes).  Inputs are
        checked like ``metrics.image_metrics``; ``h, w >= 16``, odd sizes included."""
        if pred.shape != target.shape:
            raise ValueError(f"LPIPSVGG: shapes differ: {tuple(pred.shape)} vs {tuple(target.shape)}")
        if pred.dim() < 3 or pred.shape[-1] != 3:
            raise ValueError(f"LPIPSVGG: expected (..., h, w, 3) images, got {tuple(pred.shape)}")
        if pred.dtype != torch.float32 or target.dtype != torch.float32:
            raise TypeError(f"LPIPSVGG: fp32 images only, got {pred.dtype} and {target.dtype}")
        if not (pred.is_cuda and target.is_cuda) or pred.device != target.device:
            raise ValueError(f"LPIPSVGG: both images must be on one GPU, got {pred.device} and {target.device}")
        lead, (h, w) = pred.shape[:-3], pred.shape[-3:-1]
        if h < MIN_SIZE or w < MIN_SIZE:
            raise ValueError(f"LPIPSVGG: images of {h} x {w} are smaller than {MIN_SIZE} x {MIN_SIZE}")
        chunk = min(int(chunk), self.max_chunk(h, w))
        if chunk < 1:
            raise ValueError(f"LPIPSVGG: chunk must be positive and one pair of {h} x {w} images must fit the convolutions' 2^31-byte limit")
        a, b = pred.reshape(-1, h, w, 3).contiguous(), target.reshape(-1, h, w, 3).contiguous()
        out = torch.zeros(a.shape[0], dtype=torch.float32, device=pred.device)
        with torch.cuda.device(pred.device):
            for lo in range(0, a.shape[0], chunk):
                self._run_chunk(a[lo:lo + chunk], b[lo:lo + chunk], out[lo:lo + chunk])
        return out.reshape(lead)


def flops_per_image(h: int, w: int, cin0: int = 3) -> int:
    """2 * 9 * Cin * Cout * H * W summed over the thirteen convolutions of one ``h x w`` image"""
    total, H, W = 0, h, w
    for i, (cin, cout) in enumerate(CHANNELS):
        total += 2 * 9 * (cin0 if i == 0 else cin) * cout * H * W
        if i in TAPS[:-1]:
            H, W = H // 2, W // 2
    return total
