"""Writes tests/golden/viridis_map.npz from the installed matplotlib (which is not the reference: the reference only calls ``plt.imsave``):

  table            (256, 3) uint8   viridis as ``cmap(np.arange(256), bytes=True)[:, :3]`` gives it
  x_<a>_<b>        float32 inputs for the range [vmin, vmax] = [-1, 1] and [-2, 2]
  rgb_<a>_<b>      (len(x), 3) uint8: ``ScalarMappable(Normalize(vmin, vmax), 'viridis').to_rgba(x, bytes=True)[:, :3]``

The inputs per range: every bin edge vmin + k (vmax - vmin) / 256 with its two float32 neighbours, vmin and vmax with theirs, values outside the
range, +-inf, NaN, and 4096 seeded random values over 1.5 times the range.  ``--hex`` prints the table as the 256 ``RRGGBB`` lines the package ships
(ssdnerf_amd/viridis_u8.hex).

    python tests/golden/make_golden_viridis.py [--hex]
"""
import os
import sys

import numpy as np

RANGES = ((-1.0, 1.0), (-2.0, 2.0))


def inputs(vmin: float, vmax: float) -> np.ndarray:
    edges = (vmin + np.arange(257, dtype=np.float64) * (vmax - vmin) / 256).astype(np.float32)
    edges = np.concatenate([edges, np.float32([vmin, vmax])])
    near = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf))])
    span = vmax - vmin
    outside = np.float32([vmin - span, vmin - 1e-3, vmax + 1e-3, vmax + span, -1e30, 1e30, -0.0, 0.0, np.inf, -np.inf, np.nan])
    rnd = np.random.default_rng(20).uniform(vmin - 0.25 * span, vmax + 0.25 * span, 4096).astype(np.float32)
    return np.concatenate([near, outside, rnd]).astype(np.float32)


def main() -> None:
    import matplotlib
    from matplotlib import cm, colors
    table = matplotlib.colormaps["viridis"](np.arange(256), bytes=True)[:, :3].astype(np.uint8)
    if "--hex" in sys.argv:
        print("\n".join("%02x%02x%02x" % tuple(int(v) for v in row) for row in table))
        return
    out = dict(table=table)
    for vmin, vmax in RANGES:
        x = inputs(vmin, vmax)
        mapper = cm.ScalarMappable(norm=colors.Normalize(vmin=vmin, vmax=vmax), cmap="viridis")
        with np.errstate(invalid="ignore"):
            rgba = mapper.to_rgba(x, bytes=True)
        key = f"{int(vmin)}_{int(vmax)}".replace("-", "m")
        out["x_" + key] = x
        out["rgb_" + key] = np.ascontiguousarray(rgba[:, :3]).astype(np.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "viridis_map.npz")
    np.savez_compressed(path, **out)
    print(path, {k: v.shape for k, v in out.items()}, "matplotlib", matplotlib.__version__)


if __name__ == "__main__":
    main()
