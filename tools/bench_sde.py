#!/usr/bin/env python
"""tools/bench_sde.py -- stochastic sampling on device noise on one MI355X; prints one JSON line and writes it to ``--out``
(profiles/sde.json).

  device_function_ulp  (``--ulp``) the worst errors, in ulps of the exact result, of the three device-library functions the normal generator calls
             (csrc/philox.h: logf, sqrtf, sinpif / cospif), each over ALL 2^23 arguments the generator can feed it, against float64
             (tools/ubench/philox_ulp.hip, built on demand into .variants/philox_ulp/).  The constants of tests/_philox_ref.normal_bounds: a property of
             the device library, not of the kernels.  ``--ulp-only`` stops after this leg (the kernel tests need it first).
  kernel     the bare ``ssdnerf_sde_step_v`` (form 2 with e: 12 B read + 8 B written per element) and ``ssdnerf_philox_normal_fill`` (4 B written)
             launches at 8 x 18 x 128^2 against ``ssdnerf_dpmpp_step_v`` at that size and against the eager expression fed by ``_host_noise``: HIP events
             over windows alternated in one process, once on ONE set of buffers (resident in the last-level cache, as the sampler's latent is) and once
             rotating over 8 sets (from HBM); medians with their spread, bytes moved and their share of 8 TB/s
  sampling   scenes/s of unconditional sampling (tools/bench_sample.py, one fresh process per figure, bf16 UNet): DDIM 50 with eta = 1 on host and on
             device noise, dpmpp_2m_sde at 20 and 50 steps on device noise, and DDIM 50 with eta = 0 on this tree and, with ``--parent-tree DIR`` (a
             checkout of the parent commit with its library built), there; the processes of a round are interleaved and ``--rounds`` rounds show the spread
  bounds     the worst error / bound ratios of tests/test_sde_gpu.py's kernel cases and its sampler-level differences"""
import argparse, ctypes, json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ssdnerf_amd import _cabi as C

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", type=int, default=8); ap.add_argument("--views", type=int, default=251)
ap.add_argument("--windows", type=int, default=7); ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2); ap.add_argument("--parent-tree", default=None); ap.add_argument("--out", default=None)
ap.add_argument("--ulp", action="store_true"); ap.add_argument("--ulp-only", action="store_true")
ap.add_argument("--merge", default=None, help="a JSON file of an earlier run whose legs are kept where this run skips them (e.g. the --ulp-only line)")
ap.add_argument("--skip-sampling", action="store_true"); ap.add_argument("--skip-bounds", action="store_true"); ap.add_argument("--skip-kernel", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_sde.py measures on the GPU"
HBM_PEAK = 8.0e12


def spread(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3))


# ------------------------------------------------------------------------------------------------ ulp errors of the device functions
def ulp_leg():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _philox_ref as PR
    so = os.path.join(ROOT, ".variants", "philox_ulp", "libphilox_ulp.so")
    if not os.path.exists(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        from ssdnerf_amd import build as B                           # the library's own compiler and flags: the same device functions get inlined
        subprocess.run([B._hipcc()] + B.FLAGS + ["-shared", os.path.join(ROOT, "tools", "ubench", "philox_ulp.hip"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.philox_ulp_eval.argtypes = [ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 5
    chunk = 1 << 20
    bufs = [torch.empty(chunk, device="cuda") for _ in range(4)]
    worst = dict(log=0.0, sqrt=0.0, sin=0.0, cos=0.0)
    where = dict(worst)
    for first in range(0, 1 << 23, chunk):
        assert lib.philox_ulp_eval(first, chunk, *(C.ptr(b) for b in bufs), C.stream()) == 0
        torch.cuda.synchronize()
        ln, root, s, c = (b.cpu().numpy() for b in bufs)
        u = (np.arange(first, first + chunk, dtype=np.float64) + 0.5) * 2.0 ** -23
        s64, c64 = PR.sincos2pi(u)
        refs = dict(log=np.log(u), sqrt=np.sqrt(-2.0 * ln.astype(np.float64)), sin=s64, cos=c64)   # the root's argument is the fp32 value the device formed
        for name, got in (("log", ln), ("sqrt", root), ("sin", s), ("cos", c)):
            err = np.abs(got.astype(np.float64) - refs[name]) / PR.ulp32(refs[name])
            k = int(err.argmax())
            if err[k] > worst[name]:
                worst[name], where[name] = float(err[k]), first + k
    trig = max(worst["sin"], worst["cos"])
    up = lambda v: float(np.ceil(v * 100 + 1) / 100)                         # rounded up by at least 0.01 ulp: float64's own error in the references
    return dict(what="worst |device function - float64| in ulps of the exact result over the 2^23 arguments u = (m + 0.5) 2^-23 (sqrt: over the 2^23 values "
                     "-2 fl(ln u)); log / sqrt / trig are the measured figures rounded up, the constants of tests/_philox_ref.normal_bounds",
                functions=dict(log="logf", sqrt="sqrtf", trig="sinpif(2u), cospif(2u)"), measured=worst, worst_at_m=where,
                log=up(worst["log"]), sqrt=up(worst["sqrt"]), trig=up(trig))


# ------------------------------------------------------------------------------------------------ kernel
def kernel_leg():
    from ssdnerf_amd.diffusion import NoiseSchedule, SamplingPlan, _host_noise
    s = SamplingPlan(NoiseSchedule(dict(type="linear"), 1000), "dpmpp_2m_sde", 20).steps[10]
    n = a.scenes * 18 * 128 * 128
    g = torch.Generator().manual_seed(0)
    L = C.lib()
    out = dict(elements=n, bytes_moved=dict(sde_step=20 * n, fill=4 * n, dpmpp_step=20 * n), coefficients=dict(a=s.a, b=s.b, c=s.c, d=s.d, e=s.e, n=s.n),
               launches_per_window=a.launches, windows=a.windows)
    for name, n_sets in (("resident_one_buffer_set", 1), ("rotating_8_buffer_sets", 8)):
        sets = [[torch.randn(n, generator=g).cuda() for _ in range(3)] + [torch.empty(n, device="cuda") for _ in range(2)] for _ in range(n_sets)]
        shaped = sets[0][0].view(a.scenes, 18, 128, 128)

        def sde(i):
            x, v, q, x0, xn = sets[i % n_sets]
            C.check(L.ssdnerf_sde_step_v(C.ptr(x), C.ptr(v), C.ptr(q), C.ctypes.c_uint64(n), 2, C.f32(s.a), C.f32(s.b), C.f32(s.c), C.f32(s.d), C.f32(s.e),
                                         C.f32(s.n), C.f32(-2.0), C.f32(2.0), C.ctypes.c_uint64(1234), C.u32(i), C.ptr(x0), C.ptr(xn), C.stream()), "sde_step_v")

        def fill(i):
            C.check(L.ssdnerf_philox_normal_fill(C.ptr(sets[i % n_sets][4]), C.ctypes.c_uint64(n), C.ctypes.c_uint64(1234), C.u32(i), C.stream()), "philox_normal_fill")

        def dpmpp(i):
            x, v, q, x0, xn = sets[i % n_sets]
            C.check(L.ssdnerf_dpmpp_step_v(C.ptr(x), C.ptr(v), C.ptr(q), C.ctypes.c_uint64(n), C.f32(s.a), C.f32(s.b), C.f32(s.c), C.f32(s.d), C.f32(s.e),
                                           C.f32(-2.0), C.f32(2.0), C.ptr(x0), C.ptr(xn), C.stream()), "dpmpp_step_v")

        def eager(i):                                                # the generic branch's arithmetic on a host draw (pinned ring, asynchronous upload)
            x, v, q, x0, xn = sets[i % n_sets]
            z = _host_noise(shaped).view(-1)
            torch.clamp(s.a * x - s.b * v, -2.0, 2.0, out=x0)
            torch.add(s.c * x0 + s.d * x + s.e * q, z, alpha=s.n, out=xn)

        def window(fn, launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(launches):
                fn(i)
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / launches              # us per call

        fns = dict(sde_step=(sde, a.launches), fill=(fill, a.launches), dpmpp_step=(dpmpp, a.launches), eager_host_noise=(eager, max(4, a.launches // 20)))
        for fn, _ in fns.values():                                   # warm-up: code objects, the allocator's pools, the pinned ring
            for i in range(4):
                fn(i)
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(a.windows):                                   # alternated
            for k, (fn, launches) in fns.items():
                times[k].append(window(fn, launches))
        leg = {k + "_us": spread(v) for k, v in times.items()}
        for k in ("sde_step", "fill", "dpmpp_step"):
            rate = out["bytes_moved"][k] / (leg[k + "_us"]["median"] * 1e-6)
            leg[k + "_tb_per_s"], leg[k + "_share_of_8_tb_per_s"] = round(rate * 1e-12, 3), round(rate / HBM_PEAK, 3)
        leg["sde_over_dpmpp"] = round(leg["sde_step_us"]["median"] / leg["dpmpp_step_us"]["median"], 3)
        leg["eager_over_sde"] = round(leg["eager_host_noise_us"]["median"] / leg["sde_step_us"]["median"], 1)
        out[name] = leg
        del sets, shaped
    return out


# ------------------------------------------------------------------------------------------------ sampling
def sample_once(tree, method, steps, extra):
    cmd = [sys.executable, os.path.join(tree, "tools", "bench_sample.py"), "--scenes", str(a.scenes), "--views", str(a.views), "--steps", str(steps), "--dtype", "bf16",
           "--reps", "2"] + ([] if method == "ddim" else ["--sample-method", method]) + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tree, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-800:]}")
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return dict(scenes_per_s=round(line["value"], 2), sampler_ms=line["ddim_ms"], ms_per_step=line["ms_per_ddim_step"], total_s=line["total_s"])


def sampling_leg():
    dev = ["--noise-source", "device"]
    runs = [("ddim_50_eta0_this_tree", ROOT, "ddim", 50, []), ("ddim_50_eta1_host", ROOT, "ddim", 50, ["--eta", "1"]),
            ("ddim_50_eta1_device", ROOT, "ddim", 50, ["--eta", "1"] + dev), ("dpmpp_2m_sde_20_device", ROOT, "dpmpp_2m_sde", 20, dev),
            ("dpmpp_2m_sde_50_device", ROOT, "dpmpp_2m_sde", 50, dev)]
    if a.parent_tree:
        runs.insert(0, ("ddim_50_eta0_parent_commit", os.path.abspath(a.parent_tree), "ddim", 50, []))
    out = dict(scenes=a.scenes, views_per_scene=a.views, unet_dtype="bf16",
               note="tools/bench_sample.py, best of 2 repetitions per process, one process per entry, the entries of a round interleaved; random weights: timing only")
    res = {name: [] for name, *_ in runs}
    for _ in range(a.rounds):
        for name, tree, method, steps, extra in runs:
            res[name].append(sample_once(tree, method, steps, extra))
            print(f"[bench_sde] {name}: {res[name][-1]}", file=sys.stderr, flush=True)
    out.update({name: dict(scenes_per_s=[r["scenes_per_s"] for r in rs], sampler_ms=[r["sampler_ms"] for r in rs], ms_per_step=[r["ms_per_step"] for r in rs])
                for name, rs in res.items()})
    return out


def bounds_leg():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_sde_gpu as T
    return T.measure()


result = dict(what="stochastic sampling on device noise: the device functions' ulp errors, the fused step and fill kernels, unconditional sampling rates, "
                   "the kernel test's error / bound ratios", device=torch.cuda.get_device_name(0))


def save():                                                                  # after every leg: a later leg that fails loses nothing
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if a.merge:
    with open(a.merge) as f:
        result.update(json.load(f))
if a.ulp or a.ulp_only:
    result["device_function_ulp"] = ulp_leg()
    save()
if not a.ulp_only:
    if not a.skip_kernel:
        result["kernel"] = kernel_leg()
        save()
    if not a.skip_bounds:
        result.update(bounds_leg())
        save()
    if not a.skip_sampling:
        result["sampling"] = sampling_leg()
save()
print(json.dumps(result))
