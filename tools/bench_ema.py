"""The EMA update of a training iteration at the workload of ``ssdnerf_cars_uncond`` -- its two module pairs, (diffusion, diffusion_ema) with
the 122 M-parameter denoiser and (decoder, decoder_ema) -- four ways, windows alternated between them:

  * ``hook``: ``ExponentialMovingAverageHook.update`` (ssdnerf_amd/ema.py: host validity check + one launch of csrc/ema.hip + version
    counters), per update by HIP events and by the host clock over a synchronised window;
  * ``launch_alone``: the same plan straight through the C ABI (its event time is the kernel's): the bytes it moves (two reads and one
    write per element) over that time, and their share of 8 TB/s;
  * ``mmgen_shaped``: what the reference's hook does, restated: ``state_dict()`` of both modules, the eager formula per tensor,
    ``load_state_dict``;
  * ``foreach_lerp``: ``torch._foreach_lerp_`` on the parameter lists -- for information only: parameters without buffers and a DIFFERENT
    arithmetic (``differing_elements`` counts the elements of one update from a common state that are not bit-equal to the hook's).

Also: the host cost of the plan-validity check alone, tensor and element counts, and that the hook's result is the eager formula's bit for bit
on this model.  Writes one JSON line.   usage: python tools/bench_ema.py [--out profiles/ema.json] [--windows 5]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
KEYS = ("diffusion_ema", "decoder_ema")
ITERATION = 5000                                         # past the ramp-up: the momentum every later iteration uses


def _window(fn, steps):
    """(HIP-event ms per step, host wall ms per step) of ``steps`` calls between two synchronisations"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, (time.perf_counter() - t0) * 1e3 / steps


def _spread(vals):
    return dict(median=round(statistics.median(vals), 5), min=round(min(vals), 5), max=round(max(vals), 5))


def _alternate(fns, steps, windows, warmup):
    """{name: {event_ms, wall_ms, steps_per_window}}: ``windows`` windows per path, taken in turn"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    got = {name: ([], []) for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            ev, wall = _window(fn, steps[name])
            got[name][0].append(ev)
            got[name][1].append(wall)
    return {name: dict(event_ms=_spread(ev), wall_ms=_spread(wall), steps_per_window=steps[name]) for name, (ev, wall) in got.items()}


def build_model():
    """``DiffusionNeRF`` of the cars configs (bench.py's MODEL_CFG) with random weights; the sources differ from their EMA copies"""
    import bench
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd.registry import MODELS
    model = MODELS.build(copy.deepcopy(bench.MODEL_CFG))
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for mod, scale in ((model.diffusion_ema, 0.02), (model.diffusion, 0.02), (model.decoder_ema, 0.1), (model.decoder, 0.1)):
            for p in mod.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * scale)
    return model.cuda().train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="updates per window of the hook and the bare launch (the eager paths take a tenth)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema: needs the GPU (no HIP device visible)")
    from ssdnerf_amd import _cabi as C, ema
    model = build_model()
    hook = ema.ExponentialMovingAverageHook(KEYS, interp_mode="lerp", interval=1, start_iter=0, momentum_policy="rampup",
                                            momentum_cfg=dict(ema_kimg=4, ema_rampup=0.05, batch_size=16, eps=1e-8))
    momentum, nontrainable = hook.momenta(ITERATION)

    @torch.no_grad()
    def mmgen_shaped():
        for key in KEYS:
            ema_net, net = getattr(model, key), getattr(model, key[:-4])
            states_ema, states_orig = ema_net.state_dict(keep_vars=False), net.state_dict(keep_vars=True)
            for k, v in states_orig.items():
                states_ema[k] = (v + (states_ema[k] - v) * (momentum if v.requires_grad else nontrainable)).detach()
            ema_net.load_state_dict(states_ema, strict=True)

    # one update from a common state by each path: the hook against the eager formula (must be bit-equal), foreach_lerp against the hook
    start = {key: copy.deepcopy(getattr(model, key).state_dict()) for key in KEYS}
    hook.update(model, ITERATION)
    by_hook = {key: copy.deepcopy(getattr(model, key).state_dict()) for key in KEYS}
    for key in KEYS:
        getattr(model, key).load_state_dict(start[key])
    mmgen_shaped()
    unequal = sum(int((a.view(torch.int32) != b.view(torch.int32)).sum()) if a.dtype == torch.float32 else int((a != b).sum())
                  for key in KEYS for a, b in zip(by_hook[key].values(), getattr(model, key).state_dict().values()))
    ema_params = [p for key in KEYS for p in getattr(model, key).parameters()]
    src_params = [p.detach() for key in KEYS for p in getattr(model, key[:-4]).parameters()]
    for key in KEYS:
        getattr(model, key).load_state_dict(start[key])
    with torch.no_grad():
        torch._foreach_lerp_(ema_params, src_params, 1.0 - momentum)
    names = [f"{key}.{k}" for key in KEYS for k, _ in getattr(model, key).named_parameters()]
    by_name = {f"{key}.{k}": v for key in KEYS for k, v in by_hook[key].items()}
    lerp_differs = sum(int((p.detach().view(torch.int32) != by_name[n].view(torch.int32)).sum()) for n, p in zip(names, ema_params))
    del start, by_hook, by_name

    (dev, (plan, T, blocks, written)), = hook._plans.items()
    lib, stream = C.lib(), C.stream()

    def bare():
        lib.ssdnerf_ema_update_multi(plan.data_ptr(), T, blocks, momentum, nontrainable, stream)

    @torch.no_grad()
    def foreach_lerp():
        torch._foreach_lerp_(ema_params, src_params, 1.0 - momentum)

    few = max(args.steps // 10, 2)
    res = dict(tool="bench_ema", device=torch.cuda.get_device_name(0), windows=args.windows, workload="ssdnerf_cars_uncond: (diffusion, diffusion_ema) + (decoder, decoder_ema)",
               iteration=ITERATION, momentum=momentum, momentum_nontrainable=nontrainable)
    builds, count = ema.plan_builds, ema.launches
    res.update(_alternate({"hook": lambda: hook.update(model, ITERATION), "launch_alone": bare, "mmgen_shaped": mmgen_shaped, "foreach_lerp": foreach_lerp},
                          dict(hook=args.steps, launch_alone=args.steps, mmgen_shaped=few, foreach_lerp=few), args.windows, args.warmup))
    # every load_state_dict in between copies in place: the hook kept its plan over the whole run
    res["plan_builds_during_timing"], res["hook_launches_during_timing"] = ema.plan_builds - builds, ema.launches - count
    # the host side of an update alone: the validity check (every pair's pointer, dtype, shape, device, requires_grad against the plan's)
    times = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for _ in range(50):
            hook._current(model)
        times.append((time.perf_counter() - t0) * 1e3 / 50)
    res["plan_validity_check_host_ms"] = _spread(times)
    elements = sum(e.numel() for e in written)
    nbytes = 12 * elements
    res.update(tensors_in_plan=T, blocks=blocks, elements=elements, eager_path_tensors=len(hook._eager_idx), state_dict_entries=len(hook._pairs),
               parameters_in_foreach_lerp=len(ema_params), mbytes_moved=round(nbytes / 1e6, 2), min_ms_at_8tbps=round(nbytes / HBM_BYTES_PER_S * 1e3, 5),
               kernel_tbytes_per_s=round(nbytes / (res["launch_alone"]["event_ms"]["median"] * 1e-3) / 1e12, 3),
               kernel_share_of_8tbps=round(nbytes / HBM_BYTES_PER_S * 1e3 / res["launch_alone"]["event_ms"]["median"], 3),
               hook_vs_eager_formula_unequal_elements=unequal, foreach_lerp_differing_elements=lerp_differs,
               speedup_over_mmgen_shaped_wall=round(res["mmgen_shaped"]["wall_ms"]["median"] / res["hook"]["wall_ms"]["median"], 2))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
