"""float64 numpy restatements of what ssdnerf_amd/fidkid.py computes behind the feature extractor -- the moments (``mean``, ``np.cov``), the reference's
``FIDKID._calc_kid`` (lib/core/evaluation/metrics.py:162-187) returning the three kernel sums per subset, and the Frechet terms -- with the worst-case
first-order bounds the GPU kernels are held to (u = 2^-53; the factor 2 in every bound covers the restatement's own rounding), and the exact inputs on
which any summation order must give the same bits."""
import numpy as np

U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ inputs
def exact_features(n, D, seed=0):
    """k / 1024, k in [0, 4096): every product is a multiple of 2^-20 below 16, every partial sum of up to 2^29 of them is exact in fp64"""
    return (np.random.RandomState(seed).randint(0, 4096, size=(n, D)) / 1024.0).astype(np.float32)


def random_features(n, D, seed=0):
    """|N(0, 1)| * 0.4 as fp32: non-negative like the pooled activations of an Inception network"""
    return (np.abs(np.random.RandomState(seed).standard_normal((n, D))) * 0.4).astype(np.float32)


def exact_kid_features(n, D=16, seed=0):
    """{0, 0.5, 1, 1.5}: dot products are multiples of 1/4, (dot / 16 + 1) of 1/64 and below 3.25, cubes of 2^-18 and below 35: sums of ~10^9 terms are exact"""
    return (np.random.RandomState(seed).randint(0, 4, size=(n, D)) * 0.5).astype(np.float32)


# ------------------------------------------------------------------------------------------------ moments
def moments_ref(x):
    X = np.asarray(x, dtype=np.float64)
    return X.sum(0), X.T @ X


def abs_outer(x):
    A = np.abs(np.asarray(x, dtype=np.float64))
    return A.T @ A


def outer_bound(x, absx=None):
    """|outer - ref| <= 2 n u sum_k |x_ki x_kj| per element: n - 1 additions of exact products, in any order"""
    absx = abs_outer(x) if absx is None else absx
    return 2 * x.shape[0] * U * absx


def cov_bound(x, absx=None):
    """np.cov semantics (outer - N mu mu^T) / (N - 1): the sums' n u, and four more roundings (mean, product, difference, division) on either part"""
    N = x.shape[0]
    absx = abs_outer(x) if absx is None else absx
    mu = np.abs(np.asarray(x, dtype=np.float64)).mean(0)
    return 2 * (N + 4) * U * (absx + N * np.outer(mu, mu)) / (N - 1)


def check_le(got, ref, bound):
    """(number of elements over their bound, worst |got - ref| / bound)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    ratio = err / np.maximum(bound, np.finfo(np.float64).tiny)
    return int((err > bound).sum()), float(ratio.max())


# ------------------------------------------------------------------------------------------------ KID
def kid_sums_ref(fake, real, idx_f, idx_r):
    """per subset [Sxx, Syy, Sxy] and the sums of absolute terms the bounds scale with; the arithmetic of ``_calc_kid`` in float64, with the diagonal of the
    xx and yy kernels (POSITION i == j of the subset) zeroed before the sum instead of subtracted after it"""
    fake, real = np.asarray(fake, dtype=np.float64), np.asarray(real, dtype=np.float64)
    n = fake.shape[1]
    sums, mags = [], []
    for i_f, i_r in zip(idx_f, idx_r):
        x, y = fake[i_f], real[i_r]
        row, mag = [], []
        for a, b, drop in ((x, x, True), (y, y, True), (x, y, False)):
            k = (a @ b.T / n + 1) ** 3
            ka = (np.abs(a) @ np.abs(b).T / n + 1) ** 3
            if drop:
                np.fill_diagonal(k, 0.0)
                np.fill_diagonal(ka, 0.0)
            row.append(k.sum())
            mag.append(ka.sum())
        sums.append(row)
        mags.append(mag)
    return np.array(sums), np.array(mags)


def kid_sums_bound(mags, m, D):
    """|S - ref| <= 2 (3 D + 8 + T) u sum (|x_i| . |x_j| / D + 1)^3 with T the number of terms: a dot product of D exact products (D u), the division, the
    addition and two multiplications of the cube (each error tripled by the cube: 3 D + 8 covers them), then T - 1 additions"""
    terms = np.array([m * (m - 1), m * (m - 1), m * m], dtype=np.float64)
    return 2 * (3 * D + 8 + terms) * U * mags


def kid_from_sums(sums, m):
    """the host part of ``_calc_kid``: (Sxx + Syy) / (m - 1) - 2 Sxy / m per subset, the mean over the subsets, / m"""
    t = 0.0
    for sxx, syy, sxy in np.asarray(sums).tolist():
        t += (sxx + syy) / (m - 1) - 2 * sxy / m
    return t / len(sums) / m


def kid_bound_from_sums(bounds, mags, m):
    """what the bounds of the three sums leave of kid (x 1): the same combination of the bounds, plus 8 u of the magnitudes for the combination's own roundings"""
    b = np.asarray(bounds) + 8 * U * np.asarray(mags)
    return float(((b[:, 0] + b[:, 1]) / (m - 1) + 2 * b[:, 2] / m).mean() / m)


def draw_subsets(rng, nf, nr, num_subsets, m):
    """the draws of ``_calc_kid`` in its order: per subset the fakes, then the reals"""
    idx_f, idx_r = [], []
    for _ in range(num_subsets):
        idx_f.append(rng.choice(nf, m, replace=False))
        idx_r.append(rng.choice(nr, m, replace=False))
    return np.array(idx_f), np.array(idx_r)


def calc_kid_ref(real, fake, num_subsets, max_subset_size, rng):
    """``FIDKID._calc_kid`` in float64 with an explicit generator: (kid, a bound on what the sums' bounds leave of it)"""
    m = min(real.shape[0], fake.shape[0], max_subset_size)
    idx_f, idx_r = draw_subsets(rng, fake.shape[0], real.shape[0], num_subsets, m)
    sums, mags = kid_sums_ref(fake, real, idx_f, idx_r)
    return kid_from_sums(sums, m), kid_bound_from_sums(kid_sums_bound(mags, m, fake.shape[1]), mags, m)


# ------------------------------------------------------------------------------------------------ Frechet
def frechet_ref(mean1, cov1, mean2, cov2):
    """(fid, mean term, cov term) by another route than the code under test: the eigenvalues of the (non-symmetric) product S1 S2 itself"""
    lam = np.linalg.eigvals(np.asarray(cov1, dtype=np.float64) @ np.asarray(cov2, dtype=np.float64))
    tr_root = np.sqrt(np.maximum(lam.real, 0.0)).sum()
    d = np.asarray(mean1, dtype=np.float64) - np.asarray(mean2, dtype=np.float64)
    mean_term = float(d @ d)
    cov_term = float(np.trace(cov1) + np.trace(cov2) - 2 * tr_root)
    return mean_term + cov_term, mean_term, cov_term


def frechet_tol(cov1, cov2):
    """allowance of the eigen-solvers on a full-rank pair: 64 D u (tr S1 + tr S2)"""
    D = cov1.shape[0]
    return 64 * D * U * float(np.trace(cov1) + np.trace(cov2))


def fid_moment_tol(mean1, cov1, mean2, cov2, d1, d2):
    """What elementwise covariance errors of at most d1, d2 (``cov_bound``) leave of fid on a full-rank pair, to first order and doubled: the traces move by
    D d each; with M = S1^(1/2) S2 S1^(1/2) and eigenvalues l_k, tr M^(1/2) moves by sum dl_k / (2 sqrt l_k) <= D |dM|_2 / (2 sqrt l_min), where
    |dM|_2 <= |S1|_2 D d2 + |S2|_2 D d1 (|dS|_2 <= D d); the means (sum / N) move the mean term by less than 8 D u (|mu1|^2 + |mu2|^2)."""
    D = cov1.shape[0]
    n1, n2 = np.linalg.eigvalsh(cov1)[-1], np.linalg.eigvalsh(cov2)[-1]
    lmin = max(float(np.linalg.eigvals(cov1 @ cov2).real.min()), np.finfo(np.float64).tiny)
    root = D * (n1 * D * d2 + n2 * D * d1) / (2 * np.sqrt(lmin))
    return 2 * (D * (d1 + d2) + 2 * root + 8 * D * U * float(mean1 @ mean1 + mean2 @ mean2)) + frechet_tol(cov1, cov2)


def fid_null_tol(cov1, cov2, d1, d2, r0):
    """... and on a pair with up to r0 null directions (fewer samples than features): there the eigenvalue noise -- the solvers' 64 D u max(a) max(b) and
    what covariance errors of d1, d2 add to it, D (d1 max(b) + d2 max(a)) -- enters through the square root, once per null direction; doubled"""
    D = cov1.shape[0]
    n1, n2 = np.linalg.eigvalsh(cov1)[-1], np.linalg.eigvalsh(cov2)[-1]
    noise = 64 * D * U * n1 * n2 + D * (d1 * n2 + d2 * n1)
    return 2 * (r0 * float(np.sqrt(noise)) + D * (d1 + d2)) + frechet_tol(cov1, cov2)


# ------------------------------------------------------------------------------------------------ a seeded stand-in for the Inception network
class PoolProject:
    """8 x 8 average pool, then a fixed random projection to ``dim`` columns, in fp32: (n, 3, h, w) -> (n, dim)"""

    def __init__(self, h, w, dim=48, seed=0):
        import torch
        g = torch.Generator().manual_seed(seed)
        self.weight = torch.randn(3 * (h // 8) * (w // 8), dim, generator=g) / (3 * (h // 8) * (w // 8)) ** 0.5

    def __call__(self, x):
        import torch.nn.functional as F
        if self.weight.device != x.device:
            self.weight = self.weight.to(x.device)
        return F.avg_pool2d(x.float(), 8).flatten(1) @ self.weight
