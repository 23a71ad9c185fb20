"""Test-view scores without a GPU: the float64 restatement against closed forms, the host-side argument checks of ``ssdnerf_image_metrics``, and
``parallel.evaluate_3d`` on a world-2 gloo group with a stub model."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _metrics_ref import C1, ssim_ref


def test_restatement_reproduces_closed_forms():
    g = np.random.default_rng(0)
    x = g.random((20, 23, 3))
    assert ssim_ref(x, x) == pytest.approx(1.0, abs=1e-12)
    for p, q in [(0.2, 0.7), (0.9, 0.9 + 1 / 255), (0.0, 1.0)]:
        got = ssim_ref(np.full((9, 11, 3), p), np.full((9, 11, 3), q))
        assert got == pytest.approx((2 * p * q + C1) / (p * p + q * q + C1), abs=1e-12)


def test_image_metrics_rejects_bad_arguments_host_side():
    """Rejected before any HIP call (no device needed): the pointers below are never dereferenced."""
    from ssdnerf_amd import _cabi as C
    assert "ssdnerf_image_metrics" in C.EXPORTS
    lib = C.lib()
    fake = ctypes.c_void_p(256)
    u32 = ctypes.c_uint32

    def call(a, n, h, w):
        return lib.ssdnerf_image_metrics(a, fake, u32(n), u32(h), u32(w), fake, fake, None)

    for args, cause in [((fake, 2, 6, 32), "smaller than the 7 x 7"), ((fake, 2, 32, 6), "smaller than the 7 x 7"),
                        ((fake, 0, 32, 32), "n == 0"), ((None, 2, 32, 32), "null pointer")]:
        assert call(*args) == -1
        msg = lib.ssdnerf_last_error().decode()
        assert msg.startswith("image_metrics") and cause in msg, msg


class _StubModel:
    """val_step returns known scalars: batch j of rank r logs psnr 20 + 10 r + j, ssim 0.5 + 0.1 r + 0.01 j for its ``n`` scenes"""

    def __init__(self, rank):
        self.rank = rank

    def val_step(self, data, **kwargs):
        assert kwargs == dict(tag="x")
        r, j, n = self.rank, data["j"], data["n"]
        return dict(log_vars=dict(test_psnr=20.0 + 10 * r + j, test_ssim=0.5 + 0.1 * r + 0.01 * j), num_samples=n)


SIZES = {0: [3, 3, 1], 1: [3, 2]}          # ragged: three batches on rank 0, two on rank 1


def _expected():
    num = {"test_psnr": 0.0, "test_ssim": 0.0}
    for r, sizes in SIZES.items():
        for j, n in enumerate(sizes):
            num["test_psnr"] += n * (20.0 + 10 * r + j)
            num["test_ssim"] += n * (0.5 + 0.1 * r + 0.01 * j)
    total = sum(sum(s) for s in SIZES.values())
    return {k: v / total for k, v in num.items()}


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ssdnerf_amd import parallel
    batches = [dict(j=j, n=n) for j, n in enumerate(SIZES[rank])]
    q.put((rank, parallel.evaluate_3d(_StubModel(rank), batches, tag="x")))
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_3d_scene_weighted_mean_on_two_ranks():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = _expected()
    for r in range(2):
        assert set(res[r]) == set(want)
        for k, v in want.items():
            assert res[r][k] == pytest.approx(v, rel=1e-6), (r, k)


def test_evaluate_3d_without_a_process_group():
    from ssdnerf_amd import parallel
    out = parallel.evaluate_3d(_StubModel(0), [dict(j=0, n=2), dict(j=1, n=1)], tag="x")
    assert out["test_psnr"] == pytest.approx((2 * 20.0 + 21.0) / 3, rel=1e-6)
    assert out["test_ssim"] == pytest.approx((2 * 0.5 + 0.51) / 3, rel=1e-6)
