"""FID / KID behind the feature extractor (ssdnerf_amd/fidkid.py, csrc/feature_stats.hip) at the workload of ``ssdnerf_cars_uncond``: batches of 8 scenes x 251
views = 2008 features of 2048 floats, stores of 704 x 251 = 176 704 rows, 100 KID subsets of 1000.  By HIP events, after a warm-up of every shape, in windows
that ALTERNATE the two sides in this process:
  1. one moment update (``FeatureMoments.update``) next to its eager restatement on the same GPU (``X.double().T @ X.double()`` plus the column sum, added to
     fp64 accumulators),
  2. the KID sums of --subsets subsets of --subset-size (``kid_subset_sums``) next to the eager fp64 restatement on the GPU (gather, three fp64 Gram
     products, cube, sums),
each with its achieved fp64 FLOP/s on the operations the ALGORITHM needs (the symmetric half of X^T X: n D (D + 1); per subset (2 m^2 - m) 2 D), then
  3. host seconds of ``frechet_distance`` at D,
  4. on --ref-subsets subsets, the deviation of kid x 1000 from float64 numpy of (a) a float32 numpy restatement of ``_calc_kid`` -- the reference's
     arithmetic -- and (b) this library's sums.
No time is asserted anywhere.  Prints one JSON line and writes it to --out (kept as profiles/fidkid.json).
usage: python tools/bench_fidkid.py [--reps 10] [--rows 176704] [--subsets 100] [--out profiles/fidkid.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def _alternate(a, b, reps, calls):
    """ms per call of a and of b: ``reps`` rounds of one window each, a then b"""
    for fn in (a, b):
        fn()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(_window(a, calls))
        tb.append(_window(b, calls))
    return ta, tb


def _stats(ms, flop):
    mean = sum(ms) / len(ms)
    return dict(ms=round(mean, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), fp64_tflops=round(flop / mean * 1e-9, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2008)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--rows", type=int, default=704 * 251)
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--subset-size", type=int, default=1000)
    ap.add_argument("--ref-subsets", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fidkid.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fidkid: needs the GPU (no HIP device visible)")
    from ssdnerf_amd import fidkid as FK
    import _fidkid_ref as R
    n, D, m = args.batch, args.dim, args.subset_size
    g = torch.Generator(device="cuda").manual_seed(0)

    def feats(rows, shift=0.0):
        return ((torch.randn(rows, D, device="cuda", generator=g) + shift).abs() * 0.4).contiguous()

    # ---- 1. one moment update
    x = feats(n)
    fm = FK.FeatureMoments(D, "cuda")
    acc_sum, acc_outer = torch.zeros(D, dtype=torch.float64, device="cuda"), torch.zeros(D, D, dtype=torch.float64, device="cuda")

    def eager_update():
        xd = x.double()
        acc_sum.add_(xd.sum(0))
        acc_outer.add_(xd.T @ xd)

    t_hip, t_eager = _alternate(lambda: fm.update(x), eager_update, args.reps, calls=20)
    flop_moments = n * D * (D + 1)
    tiles = (D + 63) // 64
    moments = dict(n=n, D=D, algorithm_gflop=round(flop_moments / 1e9, 2), mfma_gflop_executed=round(tiles * (tiles + 1) // 2 * 64 * 64 * 2 * n / 1e9, 2),
                   hip=_stats(t_hip, flop_moments), eager_fp64=_stats(t_eager, flop_moments))
    moments["hip_no_slower_than_eager"] = bool(moments["hip"]["ms"] <= moments["eager_fp64"]["ms"])
    # the two accumulated the same batches the same number of times: compare them (any difference is summation order)
    torch.cuda.synchronize()
    scale = float(acc_outer.abs().max())
    moments["max_abs_diff_over_max"] = float((torch.triu(fm._outer) - torch.triu(acc_outer)).abs().max()) / scale

    # ---- 2. KID sums
    fake, real = feats(args.rows), feats(args.rows, shift=0.05)
    rng = np.random.RandomState(0)
    idx_f, idx_r = R.draw_subsets(rng, args.rows, args.rows, args.subsets, m)
    di, dr = torch.from_numpy(idx_f).cuda(), torch.from_numpy(idx_r).cuda()
    hip_out = {}

    def hip_kid():
        hip_out["sums"] = FK.kid_subset_sums(fake, real, idx_f, idx_r)

    def eager_kid():
        out = torch.empty(args.subsets, 3, dtype=torch.float64, device="cuda")
        for s in range(args.subsets):
            a, b = fake[di[s]].double(), real[dr[s]].double()
            kxx, kyy, kxy = (a @ a.T / D + 1) ** 3, (b @ b.T / D + 1) ** 3, (a @ b.T / D + 1) ** 3
            out[s, 0], out[s, 1], out[s, 2] = kxx.sum() - kxx.diagonal().sum(), kyy.sum() - kyy.diagonal().sum(), kxy.sum()
        hip_out["eager"] = out.cpu().numpy()

    t_hip, t_eager = _alternate(hip_kid, eager_kid, args.reps, calls=1)
    flop_kid = args.subsets * (2 * m * m - m) * 2 * D
    T = (m + 63) // 64
    kid = dict(rows=args.rows, subsets=args.subsets, m=m, D=D, algorithm_gflop=round(flop_kid / 1e9, 1),
               mfma_gflop_executed=round(args.subsets * (T * (T + 1) + T * T) * 64 * 64 * 2 * D / 1e9, 1),
               note="both sides include the upload of the index tables and the download of the sums",
               hip=_stats(t_hip, flop_kid), eager_fp64=_stats(t_eager, flop_kid))
    kid["hip_no_slower_than_eager"] = bool(kid["hip"]["ms"] <= kid["eager_fp64"]["ms"])
    kid["hip_vs_eager_max_rel_diff"] = float((np.abs(hip_out["sums"] - hip_out["eager"]) / np.abs(hip_out["eager"])).max())
    kid["kid_x1000"] = R.kid_from_sums(hip_out["sums"], m) * 1000

    # ---- 3. the Frechet distance, on the host
    other = FK.FeatureMoments(D, "cuda")
    for shift in (0.05, 0.1):
        other.update(feats(n, shift=shift))
    one = FK.FeatureMoments(D, "cuda")
    for shift in (0.0, 0.02):
        one.update(feats(n, shift=shift))
    args_f = (one.mean.cpu().numpy(), one.cov.cpu().numpy(), other.mean.cpu().numpy(), other.cov.cpu().numpy())
    t0 = time.perf_counter()
    fid = FK.frechet_distance(*args_f)
    frechet = dict(D=D, samples=2 * n, host_seconds=round(time.perf_counter() - t0, 3), fid=fid[0])

    # ---- 4. the reference's float32 arithmetic against float64, next to ours, on the first --ref-subsets subsets
    k = min(args.ref_subsets, args.subsets)
    sub_f, sub_r = np.unique(idx_f[:k]), np.unique(idx_r[:k])
    host_f, host_r = fake[torch.from_numpy(sub_f).cuda()].cpu().numpy(), real[torch.from_numpy(sub_r).cuda()].cpu().numpy()
    loc_f, loc_r = np.searchsorted(sub_f, idx_f[:k]), np.searchsorted(sub_r, idx_r[:k])
    ref64, _ = R.kid_sums_ref(host_f, host_r, loc_f, loc_r)
    t32 = 0
    for i_f, i_r in zip(loc_f, loc_r):                                          # _calc_kid on float32 arrays, as the reference runs it
        a, b = host_f[i_f], host_r[i_r]
        ka = (a @ a.T / D + 1) ** 3 + (b @ b.T / D + 1) ** 3
        kb = (a @ b.T / D + 1) ** 3
        t32 += (ka.sum() - np.diag(ka).sum()) / (m - 1) - kb.sum() * 2 / m
    kid64 = R.kid_from_sums(ref64, m) * 1000
    kid32 = float(t32 / k / m) * 1000
    ours = R.kid_from_sums(hip_out["sums"][:k], m) * 1000
    accuracy = dict(subsets=k, kid_x1000_float64=kid64, float32_restatement=kid32, float32_deviation=abs(kid32 - kid64), ours=ours, our_deviation=abs(ours - kid64))

    result = dict(tool="bench_fidkid", reps=args.reps, device=torch.cuda.get_device_name(0), moments=moments, kid=kid, frechet=frechet, kid_accuracy=accuracy)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
