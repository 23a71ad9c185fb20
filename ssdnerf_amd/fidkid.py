"""FID and KID of rendered views (reference: ``FIDKID``, lib/core/evaluation/metrics.py:135-215, fed by ``evaluate_3d``, lib/apis/test.py:41-53): everything
behind the feature extractor.

The reference keeps every feature on the host, runs ``np.cov`` over them at the end and forms 100 x 3 Gram matrices of 1000 x 1000 in float32 numpy.  Here
the first two moments are accumulated per batch on the GPU as the views are rendered (``FeatureMoments``, csrc/feature_stats.hip, fp64 on
``v_mfma_f64_16x16x4_f64``), KID's cubic-kernel sums come from gathered rows of the device feature stores in fp64 without a Gram matrix in memory
(``kid_subset_sums``), and only the Frechet distance -- two symmetric eigen-decompositions of D x D, once per evaluation -- runs on the host.

The Inception network is not part of this project: with ``inception_args=dict(type='StyleGAN', inception_path=...)`` the TorchScript file the reference
uses is loaded from that path (never fetched); any other ``extractor`` is a callable ``(n, 3, h, w) -> (n, D)``."""
from __future__ import annotations

import os
import pickle
from typing import Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import _cabi as C
from .registry import METRICS


def _distributed() -> bool:
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


class FeatureMoments:
    """Running ``count``, ``sum`` (D) and ``outer = sum_k x_k x_k^T`` (D x D) of feature batches, in fp64.  GPU batches go through
    ``ssdnerf_feature_moments_accumulate`` (only the tiles on and above the diagonal are computed; ``outer`` mirrors them), CPU batches through plain torch."""

    def __init__(self, dim: int, device=None):
        self.dim = int(dim)
        self.count = 0
        self.sum = torch.zeros(self.dim, dtype=torch.float64, device="cpu" if device is None else device)
        self.device = self.sum.device                                 # ("cuda" has become "cuda:<current>")
        self._outer = torch.zeros(self.dim, self.dim, dtype=torch.float64, device=self.device)

    def update(self, feats: torch.Tensor) -> "FeatureMoments":
        if feats.dim() != 2 or feats.shape[1] != self.dim:
            raise ValueError(f"FeatureMoments.update: expected (n, {self.dim}) features, got {tuple(feats.shape)}")
        if feats.dtype != torch.float32:
            raise TypeError(f"FeatureMoments.update: fp32 features only, got {feats.dtype}")
        if feats.device != self.device:
            raise ValueError(f"FeatureMoments.update: features on {feats.device}, moments on {self.device}")
        n = feats.shape[0]
        if n == 0:
            return self
        if feats.is_cuda:
            x = feats.contiguous()
            with torch.cuda.device(self.device):
                C.check(C.lib().ssdnerf_feature_moments_accumulate(C.ptr(x), C.u32(n), C.u32(self.dim), C.ptr(self.sum), C.ptr(self._outer), C.stream()),
                        "feature_moments_accumulate")
        else:
            x = feats.double()
            self.sum += x.sum(0)
            self._outer += x.T @ x
        self.count += n
        return self

    @property
    def outer(self) -> torch.Tensor:
        """the full symmetric matrix: the upper triangle and its mirror image"""
        up = torch.triu(self._outer)
        return up + torch.triu(self._outer, 1).T

    @property
    def mean(self) -> torch.Tensor:
        return self.sum / self.count

    @property
    def cov(self) -> torch.Tensor:
        """``np.cov(feats, rowvar=False)``: (outer - N mu mu^T) / (N - 1)"""
        mu = self.mean
        return (self.outer - self.count * torch.outer(mu, mu)) / (self.count - 1)

    def clone(self) -> "FeatureMoments":
        other = FeatureMoments.__new__(FeatureMoments)
        other.dim, other.device, other.count = self.dim, self.device, self.count
        other.sum, other._outer = self.sum.clone(), self._outer.clone()
        return other

    def all_reduce_(self, group=None) -> "FeatureMoments":
        """count, sum and outer summed over the process group, in place (a no-op without one)"""
        if dist.is_available() and dist.is_initialized():
            cnt = torch.tensor([self.count], dtype=torch.int64, device=self.device)
            for t in (cnt, self.sum, self._outer):
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
            self.count = int(cnt.item())
        return self


def frechet_distance(mean1, cov1, mean2, cov2) -> Tuple[float, float, float]:
    """``(fid, mean_term, cov_term)`` with ``mean_term = |mu1 - mu2|^2`` and ``cov_term = tr S1 + tr S2 - 2 tr (S1 S2)^(1/2)``, in fp64 on the host.
    (S1 S2) has the eigenvalues of the symmetric positive semi-definite S1^(1/2) S2 S1^(1/2), so the trace of the root is the sum of the square roots of
    that matrix's eigenvalues, clamped at zero: two ``eigh``-class decompositions, no general matrix square root, no "add eps and retry" branch."""
    def arr(v):
        return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64)
    m1, s1, m2, s2 = arr(mean1), arr(cov1), arr(mean2), arr(cov2)
    if s1.ndim != 2 or s1.shape != s2.shape or s1.shape[0] != s1.shape[1] or m1.shape != (s1.shape[0],) or m2.shape != m1.shape:
        raise ValueError(f"frechet_distance: shapes {m1.shape}, {s1.shape}, {m2.shape}, {s2.shape}")
    w, q = np.linalg.eigh((s1 + s1.T) / 2)
    root1 = (q * np.sqrt(np.maximum(w, 0.0))) @ q.T
    inner = root1 @ ((s2 + s2.T) / 2) @ root1
    lam = np.linalg.eigvalsh((inner + inner.T) / 2)
    tr_root = float(np.sqrt(np.maximum(lam, 0.0)).sum())
    d = m1 - m2
    mean_term = float(d @ d)
    cov_term = float(np.trace(s1)) + float(np.trace(s2)) - 2.0 * tr_root
    return mean_term + cov_term, mean_term, cov_term


def kid_subset_sums(fake_store: torch.Tensor, real_store: torch.Tensor, idx_fake, idx_real) -> np.ndarray:
    """``(num_subsets, 3)`` fp64 ``[Sxx, Syy, Sxy]`` per subset: with x_i = fake_store[idx_fake[s, i]], y_j = real_store[idx_real[s, j]] (both (N, D) fp32 on
    one device, the index tables (num_subsets, m) integers on the host), Sxx = sum over positions i != j of (x_i . x_j / D + 1)^3, Syy alike, Sxy over all
    i, j.  The index range is checked here, on the host; GPU stores go through ``ssdnerf_kid_subset_sums``, CPU stores through plain torch fp64."""
    idx_f, idx_r = np.ascontiguousarray(idx_fake, dtype=np.int64), np.ascontiguousarray(idx_real, dtype=np.int64)
    if fake_store.dim() != 2 or real_store.dim() != 2 or fake_store.shape[1] != real_store.shape[1] or fake_store.shape[1] == 0:
        raise ValueError(f"kid_subset_sums: stores of shape {tuple(fake_store.shape)} and {tuple(real_store.shape)}")
    if fake_store.dtype != torch.float32 or real_store.dtype != torch.float32:
        raise TypeError(f"kid_subset_sums: fp32 stores only, got {fake_store.dtype} and {real_store.dtype}")
    if fake_store.device != real_store.device:
        raise ValueError(f"kid_subset_sums: stores on {fake_store.device} and {real_store.device}")
    if idx_f.ndim != 2 or idx_f.shape != idx_r.shape or idx_f.shape[0] < 1 or idx_f.shape[1] < 2:
        raise ValueError(f"kid_subset_sums: index tables of shape {idx_f.shape} and {idx_r.shape} (need equal (num_subsets >= 1, m >= 2))")
    for name, idx, store in (("fake", idx_f, fake_store), ("real", idx_r, real_store)):
        if int(idx.min()) < 0 or int(idx.max()) >= store.shape[0]:
            raise IndexError(f"kid_subset_sums: {name} indices span [{int(idx.min())}, {int(idx.max())}], the store has {store.shape[0]} rows")
    num_subsets, m = idx_f.shape
    D = fake_store.shape[1]
    if fake_store.is_cuda:
        dev = fake_store.device
        x, y = fake_store.contiguous(), real_store.contiguous()
        di, dr = torch.from_numpy(idx_f).to(dev), torch.from_numpy(idx_r).to(dev)
        out = torch.empty(num_subsets, 3, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            nbytes = int(C.lib().ssdnerf_kid_subset_sums_workspace(C.u32(num_subsets), C.u32(m)))
            ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
            C.check(C.lib().ssdnerf_kid_subset_sums(C.ptr(x), C.ptr(y), C.ptr(di), C.ptr(dr), C.u32(num_subsets), C.u32(m), C.u32(D), C.ptr(out), C.ptr(ws),
                                                    C.ctypes.c_size_t(nbytes), C.stream()), "kid_subset_sums")
        return out.cpu().numpy()
    out = np.empty((num_subsets, 3), dtype=np.float64)
    for s in range(num_subsets):
        x, y = fake_store[torch.from_numpy(idx_f[s])].double(), real_store[torch.from_numpy(idx_r[s])].double()
        kxx, kyy, kxy = (x @ x.T / D + 1) ** 3, (y @ y.T / D + 1) ** 3, (x @ y.T / D + 1) ** 3
        out[s] = [float(kxx.sum() - kxx.diagonal().sum()), float(kyy.sum() - kyy.diagonal().sum()), float(kxy.sum())]
    return out


def kid(fake_store: torch.Tensor, real_store: torch.Tensor, num_subsets: int = 100, max_subset_size: int = 1000, rng=None) -> float:
    """``FIDKID._calc_kid``: ``m = min(Nf, Nr, max_subset_size)``; per subset ``rng.choice(N, m, replace=False)`` for the fakes, then for the reals (the
    reference's order of draws; ``rng``: a ``numpy.random.Generator`` or ``RandomState``, default the global ``np.random`` as in the reference); the sums
    from ``kid_subset_sums``; their combination, the mean over the subsets and ``/ m`` in Python floats.  (The caller multiplies by 1000.)"""
    rng = np.random if rng is None else rng
    nf, nr = fake_store.shape[0], real_store.shape[0]
    m = min(nf, nr, int(max_subset_size))
    if m < 2:
        raise ValueError(f"kid: subsets of {m} rows (stores of {nf} and {nr}, max_subset_size {max_subset_size}): at least 2 are needed")
    idx_f, idx_r = np.empty((num_subsets, m), dtype=np.int64), np.empty((num_subsets, m), dtype=np.int64)
    for s in range(num_subsets):
        idx_f[s] = rng.choice(nf, m, replace=False)
        idx_r[s] = rng.choice(nr, m, replace=False)
    t = 0.0
    for sxx, syy, sxy in kid_subset_sums(fake_store, real_store, idx_f, idx_r).tolist():
        t += (sxx + syy) / (m - 1) - 2 * sxy / m
    return float(t / num_subsets / m)


def _gather_rows(rows: torch.Tensor) -> torch.Tensor:
    """the rows of every rank, in rank order, on every rank (ranks may hold different numbers)"""
    world = dist.get_world_size()
    n = torch.tensor([rows.shape[0]], dtype=torch.int64, device=rows.device)
    sizes = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(sizes, n)
    sizes = [int(s.item()) for s in sizes]
    pad = rows.new_zeros((max(sizes),) + tuple(rows.shape[1:]))
    pad[: rows.shape[0]] = rows
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad)
    return torch.cat([p[:k] for p, k in zip(parts, sizes)])


@METRICS.register_module()
class FIDKID:
    """The reference's ``FIDKID`` metric (mmgen's ``FID`` with KID added) behind ``feed`` / ``summary``.

    ``num_images`` per mode are counted; ``inception_pkl``: a reference file with the keys ``mean``, ``cov``, ``feats_np`` (what ``save_reference`` and the
    reference's tools/inception_stat.py write), loaded by ``prepare()``, after which fed reals are ignored; ``inception_args``:
    ``dict(type='StyleGAN', inception_path=...)`` names the TorchScript extractor, loaded on the first ``feed`` of images; ``extractor``: any callable
    ``(n, 3, h, w) fp32 in [-1, 1] -> (n, feature_dim)`` instead; ``seed``: KID's subsets are drawn from ``RandomState(seed)`` at every ``summary()``
    (default: the global ``np.random``, as the reference)."""
    name = "FIDKID"

    def __init__(self, num_images, num_subsets=100, max_subset_size=1000, inception_pkl=None, inception_args=None, bgr2rgb=True, extractor=None,
                 feature_dim=2048, seed=None):
        self.num_images = int(num_images)
        self.num_subsets, self.max_subset_size = int(num_subsets), int(max_subset_size)
        self.inception_pkl = inception_pkl
        self.inception_args = dict(inception_args) if inception_args else None
        self.bgr2rgb = bool(bgr2rgb)
        self.extractor = extractor
        self.feature_dim = int(feature_dim)
        self.seed = seed
        self._style = "callable" if extractor is not None else None
        self._stores = dict(reals=None, fakes=None)
        self._moments = dict(reals=None, fakes=None)
        self.num_real_feeded = self.num_fake_feeded = 0
        self.real_mean = self.real_cov = self.real_feats_np = None
        self._result_str, self._result_dict = None, {}

    # ------------------------------------------------------------------ the extractor
    def _load_extractor(self):
        if self.extractor is not None:
            return
        args = self.inception_args or {}
        path = args.get("inception_path")
        if str(args.get("type", "")).lower() != "stylegan" or path is None:
            raise RuntimeError(f"FIDKID: no extractor was given and inception_args {self.inception_args!r} do not name a StyleGAN TorchScript file "
                               "(inception_args=dict(type='StyleGAN', inception_path=...))")
        if not os.path.exists(path):
            raise FileNotFoundError(f"FIDKID: the Inception TorchScript file {path!r} (inception_args['inception_path']) does not exist; it is not part of "
                                    "this project and is never downloaded: place the file there or pass extractor=")
        self.extractor = torch.jit.load(path).eval()
        self._style = "stylegan"

    def _extract(self, batch: torch.Tensor) -> torch.Tensor:
        self._load_extractor()
        if self.bgr2rgb:
            batch = batch.flip(1)
        with torch.no_grad():
            if self._style == "stylegan":
                self.extractor.to(batch.device)
                feats = self.extractor((batch * 127.5 + 128).clamp(0, 255).to(torch.uint8), return_features=True)
            else:
                feats = self.extractor(batch)
        return feats

    # ------------------------------------------------------------------ feeding
    def prepare(self):
        """load the reference statistics of the real images, if a file is named; reals fed afterwards are ignored"""
        if self.inception_pkl is not None:
            if not os.path.exists(self.inception_pkl):
                raise FileNotFoundError(f"FIDKID.prepare: the reference statistics {self.inception_pkl!r} (inception_pkl) do not exist; "
                                        "FIDKID.save_reference writes them from fed real images")
            with open(self.inception_pkl, "rb") as f:
                ref = pickle.load(f)
            self.real_mean, self.real_cov = np.asarray(ref["mean"], dtype=np.float64), np.asarray(ref["cov"], dtype=np.float64)
            self.real_feats_np = np.ascontiguousarray(ref["feats_np"], dtype=np.float32)
            self.num_real_feeded = self.num_images

    def _wanted(self, mode: str) -> int:
        if mode not in ("reals", "fakes"):
            raise ValueError(f"FIDKID: mode {mode!r} (expected 'reals' or 'fakes')")
        fed = self.num_real_feeded if mode == "reals" else self.num_fake_feeded
        return max(self.num_images - fed, 0)

    def wants(self, mode: str) -> bool:
        return self._wanted(mode) > 0

    def feed(self, batch: torch.Tensor, mode: str) -> int:
        """``batch``: (n, 3, h, w) images in [-1, 1]; returns how many of them were counted (the last batch is trimmed to ``num_images``)"""
        take = min(self._wanted(mode), batch.shape[0])
        if take == 0:
            return 0
        if batch.dim() != 4 or batch.shape[1] != 3:
            raise ValueError(f"FIDKID.feed: expected (n, 3, h, w) images, got {tuple(batch.shape)}")
        return self.feed_features(self._extract(batch[:take].float()), mode)

    def feed_features(self, feats: torch.Tensor, mode: str) -> int:
        take = min(self._wanted(mode), feats.shape[0])
        if take == 0:
            return 0
        if feats.dim() != 2 or feats.shape[1] != self.feature_dim:
            raise ValueError(f"FIDKID: expected (n, {self.feature_dim}) features, got {tuple(feats.shape)}")
        feats = feats[:take].detach().float().contiguous()
        if self._stores[mode] is None:
            self._stores[mode] = torch.empty(self.num_images, self.feature_dim, dtype=torch.float32, device=feats.device)
            self._moments[mode] = FeatureMoments(self.feature_dim, feats.device)
        fed = self.num_real_feeded if mode == "reals" else self.num_fake_feeded
        self._stores[mode][fed: fed + take] = feats
        self._moments[mode].update(feats)
        if mode == "reals":
            self.num_real_feeded += take
        else:
            self.num_fake_feeded += take
        return take

    def features(self, mode: str) -> torch.Tensor:
        """the rows fed so far on this rank, (fed, feature_dim) fp32"""
        fed = self.num_real_feeded if mode == "reals" else self.num_fake_feeded
        if self._stores[mode] is None:
            return torch.empty(0, self.feature_dim)
        return self._stores[mode][:fed]

    # ------------------------------------------------------------------ results
    def _collected(self, mode: str):
        """(moments, feature rows) of a fed mode over all ranks"""
        fed = self.num_real_feeded if mode == "reals" else self.num_fake_feeded
        if self._stores[mode] is None:
            if not _distributed():
                raise RuntimeError(f"FIDKID: no {mode} were fed")
            raise RuntimeError(f"FIDKID: no {mode} were fed on rank {dist.get_rank()} (every rank must feed at least one batch)")
        moments, rows = self._moments[mode], self._stores[mode][:fed]
        if _distributed():
            moments, rows = moments.clone().all_reduce_(), _gather_rows(rows)
        return moments, rows

    def _real_side(self, device):
        if self.real_feats_np is not None:
            return self.real_mean, self.real_cov, torch.from_numpy(self.real_feats_np).to(device)
        moments, rows = self._collected("reals")
        assert moments.count == self.num_images, f"FIDKID: {moments.count} real images were fed, num_images is {self.num_images}"
        return moments.mean, moments.cov, rows

    @torch.no_grad()
    def summary(self):
        """``(fid, fid_mean, fid_cov, kid x 1000)``; every rank of a process group returns the same values"""
        moments, fakes = self._collected("fakes")
        assert moments.count == self.num_images, f"FIDKID: {moments.count} fake images were fed, num_images is {self.num_images}"
        real_mean, real_cov, reals = self._real_side(fakes.device)
        fid, mean, cov = frechet_distance(moments.mean, moments.cov, real_mean, real_cov)
        rng = None if self.seed is None else np.random.RandomState(self.seed)
        k = kid(fakes, reals, self.num_subsets, self.max_subset_size, rng) * 1000
        self._result_str = f"{fid:.4f} ({mean:.5f}/{cov:.5f}), {k:.4f}"
        self._result_dict = dict(fid=fid, fid_mean=mean, fid_cov=cov, kid=k)
        return fid, mean, cov, k

    @property
    def result_str(self):
        return self._result_str

    @property
    def result_dict(self):
        return self._result_dict

    def save_reference(self, path: str) -> None:
        """write the statistics of the fed reals as the reference's tools/inception_stat.py does (keys mean, cov, feats_np, size, name)"""
        moments, rows = self._collected("reals")
        assert moments.count == self.num_images, f"FIDKID.save_reference: {moments.count} real images were fed, num_images is {self.num_images}"
        with open(path, "wb") as f:
            pickle.dump(dict(feats_np=rows.cpu().numpy(), mean=moments.mean.cpu().numpy(), cov=moments.cov.cpu().numpy(), size=moments.count,
                             name=os.path.splitext(os.path.basename(path))[0]), f)
