"""TEST INFRASTRUCTURE for ssdnerf_amd/ema.py and csrc/ema.hip: the reference's EMA update restated twice, independent of the package.

``update32``: the arithmetic of one tensor in numpy float32, three separately rounded operations
    ema <- fl32( src + fl32( fl32(ema - src) * fl32(m) ) )
(what eager ``src + (ema - src) * m`` computes on fp32 tensors, bit for bit; ``torch.lerp`` does not).

``hook_step``: mmgen 0.7.2's ExponentialMovingAverageHook for whole modules in plain torch -- the schedule, the ``rampup`` policy and the
per-entry eager formula over ``state_dict()`` followed by what ``load_state_dict`` does (a ``copy_`` per entry) -- on state dicts, returning
the expected EMA state dict without touching a module."""
from collections import OrderedDict

import numpy as np
import torch

CFG_MOMENTUM = dict(ema_kimg=4, ema_rampup=0.05, batch_size=16, eps=1e-8)        # the configs' momentum_cfg


def update32(ema, src, m):
    ema, src = np.asarray(ema, np.float32), np.asarray(src, np.float32)
    with np.errstate(all="ignore"):
        d = (ema - src).astype(np.float32)
        p = (d * np.float32(m)).astype(np.float32)
        return (src + p).astype(np.float32)


def rampup(iteration, ema_kimg=10, ema_rampup=0.05, batch_size=4, eps=1e-8):
    cur_nimg = (iteration + 1) * batch_size
    ema_nimg = ema_kimg * 1000
    if ema_rampup is not None:
        ema_nimg = min(ema_nimg, cur_nimg * ema_rampup)
    return 0.5 ** (batch_size / max(ema_nimg, eps))


def acts(iteration, interval, start_iter):
    if iteration < start_iter:
        return True
    return (iteration + 1 - start_iter) % interval == 0 if interval > 0 else False


def snapshot(module):
    """(state dict cloned, {key: requires_grad}) of a module"""
    sd = module.state_dict(keep_vars=True)
    return OrderedDict((k, v.detach().clone()) for k, v in sd.items()), {k: bool(v.requires_grad) for k, v in sd.items()}


def hook_step(src_state, src_trainable, ema_state, iteration, interval=1, start_iter=0, momentum=0.999, momentum_nontrainable=0.0,
              momentum_policy="fixed", momentum_cfg=None):
    """the EMA state dict after ``after_train_iter`` at ``runner.iter == iteration`` (inputs are not modified)"""
    out = OrderedDict((k, v.clone()) for k, v in ema_state.items())
    if not acts(iteration, interval, start_iter):
        return out
    if momentum_policy == "rampup":
        momentum = rampup(iteration, **(momentum_cfg or {}))
    for k, v in src_state.items():
        if iteration < start_iter:
            out[k].copy_(v)
        else:
            m = momentum if src_trainable[k] else momentum_nontrainable
            out[k].copy_(v + (ema_state[k] - v) * m)                      # the formula, then load_state_dict's copy_ (casts integer buffers back)
    return out


def bits(t):
    """a tensor's bytes as a numpy array of unsigned integers (NaN payloads and signed zeros count)"""
    a = t.detach().cpu().contiguous().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind in "fc" else a


def assert_state_bits_equal(module, want, what=""):
    got = module.state_dict()
    assert list(got.keys()) == list(want.keys()), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        a, b = bits(got[k]), bits(want[k])
        assert np.array_equal(a, b), (what, k, int((a != b).sum()))


def make_values(n, seed):
    """(ema, src) float32 arrays of n elements: normal values with planted +-0, +-inf, denormals, equal pairs and NaNs"""
    rng = np.random.default_rng(seed)
    ema = (rng.standard_normal(n) * 0.5).astype(np.float32)
    src = (ema + rng.standard_normal(n).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1e-38, -3e-39, 1.0, np.nan], np.float32)
    k = 0
    for i in range(min(n, 4 * len(special))):                            # every special value in ema against a normal src, and the reverse
        tgt = ema if (i // len(special)) % 2 == 0 else src
        tgt[(i * 7) % n] = special[i % len(special)]
        k += 1
    for i in range(0, n, 11):                                             # pairs with ema == src (difference exactly +0)
        src[i] = ema[i]
    if n > 40:
        ema[37], src[37] = np.float32(1e-45), np.float32(-1e-45)          # denormal difference
        ema[38], src[38] = np.float32(-0.0), np.float32(0.0)
        ema[39], src[39] = np.float32(np.inf), np.float32(np.inf)         # inf - inf: NaN
    return ema, src
