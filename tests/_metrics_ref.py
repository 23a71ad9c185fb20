"""Independent statement of the test-view scores, shared by tests/test_metrics_cpu.py and tests/test_metrics_gpu.py: skimage's
``structural_similarity(channel_axis, data_range=1)`` (skimage >= 0.19 defaults: 7 x 7 uniform window, sample covariance, 3-pixel crop) restated in
float64 with scipy's ``uniform_filter``, and the reference's PSNR (lib/core/evaluation/metrics.py:52-55) in float64 torch."""
import math

import numpy as np
import torch
from scipy.ndimage import uniform_filter

C1, C2 = 0.01 ** 2, 0.03 ** 2


def ssim_ref(x, y) -> float:
    """SSIM of two (h, w, 3) images in [0, 1]: the mean over channels of the mean of S over the pixels whose window lies inside the image."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    cov_norm = 49.0 / 48.0
    vals = []
    for c in range(3):
        X, Y = x[..., c], y[..., c]
        ux, uy = uniform_filter(X, size=7), uniform_filter(Y, size=7)
        uxx, uyy, uxy = uniform_filter(X * X, size=7), uniform_filter(Y * Y, size=7), uniform_filter(X * Y, size=7)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        vals.append(S[3:-3, 3:-3].mean())
    return float(np.mean(vals))


def mse_psnr_ref(x, y):
    """(mse, psnr) of two (h, w, 3) images in float64."""
    d = torch.as_tensor(np.asarray(x), dtype=torch.float64) - torch.as_tensor(np.asarray(y), dtype=torch.float64)
    mse = d.square().mean()
    return float(mse), float(10 * (2 * math.log10(1.0) - torch.log10(mse + 1e-6)))
