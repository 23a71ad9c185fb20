"""Inputs and expected bits for the scene cache's conversions (ssdnerf_amd/csrc/cache_cvt.h), shared by tests/test_scene_cache_cpu.py (the gcc
build of the header) and tests/test_scene_cache_gpu.py (the store kernel).  The expected value is always what the host cache computes on the
CPU: ``scene_cache._clamp_to(x, dtype).to(dtype)``."""
import numpy as np
import torch

SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 3.4028234663852886e38, -3.4028234663852886e38, 65504.0, 65519.9, 65520.0, 70000.0, -65504.0, -65519.9,
                     -65520.0, -70000.0, 2.0 ** -24, 2.0 ** -25, -2.0 ** -24, -2.0 ** -25, 1e-10, -1e-10, 2.0 ** -14, 2.0 ** -126, 2.0 ** -133, 2.0 ** -149,
                     np.nan], dtype=np.float32)


def _with_neighbours(mid_bits: np.ndarray) -> np.ndarray:
    """fp32 patterns: every midpoint, one ulp below and one ulp above it, with both signs"""
    pos = np.concatenate([mid_bits - 1, mid_bits, mid_bits + 1]).astype(np.uint32)
    return np.concatenate([pos, pos | np.uint32(0x80000000)])


def inputs(dtype: torch.dtype) -> np.ndarray:
    """fp32 bit patterns (uint32): all 65 536 patterns of ``dtype`` widened; the midpoint of every pair of neighbouring finite values of ``dtype``
    (a tie), one fp32 ulp below and above it; the specials"""
    every = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype).float().numpy().view(np.uint32)
    if dtype == torch.float16:
        finite = torch.arange(0x7c00, dtype=torch.int32).to(torch.int16).view(torch.float16).double().numpy()      # 0 .. 65504, ascending
        mids = ((finite[:-1] + finite[1:]) / 2).astype(np.float32)                                                     # exact in fp32
        assert np.array_equal(mids.astype(np.float64) * 2, finite[:-1] + finite[1:])
        mid_bits = mids.view(np.uint32)
    else:
        mid_bits = (np.arange(0x7f7f, dtype=np.uint32) << 16) + np.uint32(0x8000)                                      # between bf16 patterns p and p + 1
    return np.concatenate([every, _with_neighbours(mid_bits), SPECIALS.view(np.uint32)])


def expected(bits32: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    """``_clamp_to(x, dtype).to(dtype)`` on the CPU, as uint16 patterns"""
    from ssdnerf_amd.scene_cache import _clamp_to
    x = torch.from_numpy(bits32.view(np.float32).copy())
    return _clamp_to(x, dtype).to(dtype).view(torch.int16).numpy().view(np.uint16)


def is_nan16(bits16: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    return torch.from_numpy(bits16.view(np.int16).copy()).view(dtype).float().isnan().numpy()


def assert_same_bits(got16: np.ndarray, want16: np.ndarray, dtype: torch.dtype, what: str) -> None:
    """equal patterns, NaN compared by ``isnan`` on both sides"""
    nan_got, nan_want = is_nan16(got16, dtype), is_nan16(want16, dtype)
    assert np.array_equal(nan_got, nan_want), f"{what}: NaNs differ at {np.flatnonzero(nan_got != nan_want)[:8]}"
    bad = np.flatnonzero((got16 != want16) & ~nan_want)
    assert bad.size == 0, f"{what}: {bad.size} patterns differ, first at {bad[:8]}: got {got16[bad[:8]]}, want {want16[bad[:8]]}"
