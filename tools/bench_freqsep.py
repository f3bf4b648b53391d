"""Frequency separation: device time of each filter launch beside a device-to-device copy, and of the whole training step with fs on
against off.  Prints one JSON line:

    python tools/bench_freqsep.py [--iters 100] [--warmup 10] [--step-rounds 3] [--steps 4] [--no-step]

copy               a device-to-device copy of one 16 x 3 x 512 x 512 fp32 tensor (50.3 MB read + 50.3 MB written), HIP events, the
                   smallest of three means over --iters calls: the floor of a pass that reads a tensor once and writes it once
launches[layout][filter][name]
                   each entry point alone through the ops wrappers on preallocated tensors (no autograd, no allocation), NCHW and
                   channels-last, average and gaussian taps: low (forward = backward launch), high_fwd, high_bwd.  ms, the bytes it
                   must move (high_bwd reads the gradient AND the saved output: three tensors), gbs and ms / copy ms
step               the whole G+D step at bench.py's configuration (model built by bench.make_model) with fs off and on (average
                   filters), alternating --step-rounds times in this one process
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPE = (16, 3, 512, 512)


def _time(fn, iters, warmup, repeats=3):
    """Minimum over `repeats` of the mean ms per call over `iters` back-to-back calls (HIP events), after `warmup` calls."""
    for _ in range(warmup):
        fn()
    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / iters)
    return best


def bench_launches(iters, warmup):
    from trainner_amd import ops
    from trainner_amd.dataops import filters as EF
    g = torch.Generator().manual_seed(7)
    plane = 4.0 * SHAPE[0] * SHAPE[1] * SHAPE[2] * SHAPE[3]
    base = torch.rand(*SHAPE, generator=g).cuda() * 2.0 - 0.5
    dst = torch.empty_like(base)
    copy_ms = _time(lambda: dst.copy_(base), iters, warmup)
    res = {"copy": {"ms": round(copy_ms, 4), "gb": round(2 * plane / 1e9, 4), "gbs": round(2 * plane / copy_ms / 1e6, 1)}, "launches": {}}
    for layout, fmt in ((0, torch.contiguous_format), (1, torch.channels_last)):
        x = base.contiguous(memory_format=fmt)
        grad = (torch.rand(*SHAPE, generator=g).cuda() - 0.5).contiguous(memory_format=fmt)
        out, o = torch.empty_like(x), torch.empty_like(x)
        per = {}
        for kind in ("average", "gaussian"):
            taps = EF.FilterLow(filter_type=kind).taps
            ops.freqsep_high_fwd(x, layout, taps, o)
            calls = {"low": (lambda: ops.freqsep_low(x, layout, taps, out), 2 * plane),
                     "high_fwd": (lambda: ops.freqsep_high_fwd(x, layout, taps, out), 2 * plane),
                     "high_bwd": (lambda: ops.freqsep_high_bwd(grad, o, layout, taps, out), 3 * plane)}
            per[kind] = {}
            for tag, (fn, nbytes) in calls.items():
                ms = _time(fn, iters, warmup)
                per[kind][tag] = {"ms": round(ms, 4), "gb_min": round(nbytes / 1e9, 4), "gbs": round(nbytes / ms / 1e6, 1),
                                  "times_copy": round(ms / copy_ms, 2)}
        res["launches"]["nchw" if layout == 0 else "channels_last"] = per
    return res


def bench_step(rounds, steps, warmup):
    import bench
    from trainner_amd.dataops import filters as EF
    model = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0)
    lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, model.device)
    on = (EF.FilterLow(filter_type="average").to(model.device), EF.FilterHigh(filter_type="average").to(model.device))
    times = {"fs_off": [], "fs_on": []}
    step = [0]

    def run(n):
        for _ in range(n):
            step[0] += 1
            model.feed_data({"LR": lr, "HR": hr})
            model.optimize_parameters(step[0])
        model.get_current_log()

    run(warmup)
    for _ in range(rounds):
        for key, (f_low, f_high) in (("fs_off", (None, None)), ("fs_on", on)):
            model.f_low, model.f_high = f_low, f_high
            run(1)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(steps)
            b.record()
            torch.cuda.synchronize()
            times[key].append(a.elapsed_time(b) / steps)
    ms = {k: {"mean": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "samples": [round(x, 3) for x in v]}
          for k, v in times.items()}
    return {"batch": bench.BATCH_PER_GPU, "crop": bench.CROP, "steps_per_sample": steps, "ms_per_step": ms,
            "on_minus_off_ms": round(ms["fs_on"]["mean"] - ms["fs_off"]["mean"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    from trainner_amd import hip
    hip.require_device()
    out = {"tool": "bench_freqsep", "device": torch.cuda.get_device_name(0), "shape": list(SHAPE)}
    out.update(bench_launches(args.iters, args.warmup))
    if not args.no_step:
        out["step"] = bench_step(args.step_rounds, args.steps, min(args.warmup, 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
