"""Colour, average and multi-scale pixel losses: device time of each loss alone, of its two launches, and of the whole training step.
Prints one JSON line:

    python tools/bench_pooled_losses.py [--iters 50] [--warmup 5] [--step-rounds 3] [--steps 4] [--no-step] [--sweep-blocks]

The recipe's three terms (color-l1cosinesim and avg-l1 at scale 4, multiscale-l1) at 16 x 3 x 512 x 512 fp32, in both dense layouts
(nchw, cl), measured in this one process with HIP events: three batches of --iters back-to-back calls after a warm-up; every figure
is the smallest batch mean and `<figure>_max` beside it the largest, so the spread can be read.  A batch of 0.02 ms launches is 1 ms
long and includes the gaps between dispatches: the figures are launch-to-launch times on a busy queue, not kernel durations.
loss[layout][name]      fwd_ms: the built loss function's forward under no_grad; fwd_bwd_ms: forward + backward through autograd (the
                        module path: output allocations and the scalar ops included)
                        copy_ms: a device copy of one image of the same bytes (read 50 MB, write 50 MB)
                        floor_passes: image passes the algorithm must move (forward reads sr and hr, backward reads both and writes
                        one: 5); floor_ms = floor_passes x copy_ms / 2 (a copy is two passes); times_floor = fwd_bwd_ms / floor_ms
                        torch_fwd_ms / torch_fwd_bwd_ms: the fp32 restatement of tools/make_golden_pooled_losses.py run through plain
                        torch on the device (what the reference would launch); times_torch = torch_fwd_bwd_ms / fwd_bwd_ms
launches[layout][name]  the entry points alone on preallocated tensors: fwd_ms and bwd_ms, and launch_times_floor =
                        (fwd_ms + bwd_ms) / floor_ms
sweep_blocks            with --sweep-blocks: the NCHW forward launches against the largest grid the library may launch
                        (ops.pooled_forward_blocks; the pool forward up to 2048, the multi-scale forward up to 4096 = one block per
                        band), each output compared with the default grid's: the two must agree to 2 fp32 ulps
step                    the whole G+D step at bench.py's configuration without the three terms (the step as it was before they
                        existed) and with them at the recipe's weights, alternating --step-rounds times in this one process; every
                        sample is listed, so the difference can be read beside the run-to-run spread of either
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _time(fn, iters, warmup, repeats=3):
    """(smallest, largest) over `repeats` of the mean ms per call over `iters` back-to-back calls (HIP events), after `warmup` calls."""
    for _ in range(warmup):
        fn()
    means = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        means.append(a.elapsed_time(b) / iters)
    return min(means), max(means)


SHAPE = (16, 3, 512, 512)
SCALE = 4
TERMS = (("color-l1cosinesim", 1.0), ("avg-l1", 5.0), ("multiscale-l1", 1e-2))
CRIT = {"l1": 0, "l1cosinesim": 5}


def _pair(layout):
    g = torch.Generator().manual_seed(7)
    hr = torch.rand(*SHAPE, generator=g).cuda()
    sr = hr * 1.1 - 0.05 + 0.05 * torch.randn(*SHAPE, generator=g).cuda()
    if layout == "cl":
        sr, hr = sr.contiguous(memory_format=torch.channels_last), hr.contiguous(memory_format=torch.channels_last)
    return sr, hr


def bench_loss(name, layout, iters, warmup):
    from tools import make_golden_pooled_losses as T
    from trainner_amd import ops
    from trainner_amd.models import losses
    f = losses.get_loss_fn(name, 1, device="cuda", opt={"scale": SCALE})["function"]
    sr, hr = _pair(layout)
    sr.requires_grad_(True)
    dst = torch.empty_like(hr)
    call = lambda: f(sr, hr)          # noqa: E731
    ref = lambda: T.restate(sr, hr, name, SCALE)          # noqa: E731

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    def both(fn):
        def run():
            sr.grad = None
            fn().backward()
        return run

    passes, r = 5, {}
    for key, (lo, hi) in (("copy_ms", _time(lambda: dst.copy_(hr), iters, warmup)), ("fwd_ms", _time(fwd(call), iters, warmup)),
                          ("fwd_bwd_ms", _time(both(call), iters, warmup)), ("torch_fwd_ms", _time(fwd(ref), max(iters // 5, 3), 2)),
                          ("torch_fwd_bwd_ms", _time(both(ref), max(iters // 5, 3), 2))):
        r[key], r[key + "_max"] = lo, hi
    r["floor_passes"], r["floor_ms"] = passes, passes * r["copy_ms"] / 2
    r["times_floor"] = r["fwd_bwd_ms"] / r["floor_ms"]
    r["times_torch"] = r["torch_fwd_bwd_ms"] / r["fwd_bwd_ms"]
    # what was timed is also compared, at this size: against the fp64 restatement on the device.  A pooled difference whose sign is
    # not exact in fp32 flips a whole cell's gradient, so the gradient is held by the share of elements off by more than 1e-4 of max
    sr.grad = None
    v = call()
    v.backward()
    x64 = sr.detach().double().requires_grad_(True)
    v64 = T.restate(x64, hr.double(), name, SCALE)
    v64.backward()
    off = (sr.grad.double() - x64.grad).abs() > 1e-4 * x64.grad.abs().max()
    r["value_rel_err"], r["grad_share_off"] = abs(v.item() - v64.item()) / abs(v64.item()), off.double().mean().item()
    assert r["value_rel_err"] <= 1e-6 and r["grad_share_off"] <= 1e-4, (name, layout, r["value_rel_err"], r["grad_share_off"])
    # the two launches alone
    x, lay = sr.detach(), 1 if layout == "cl" else 0
    out, gx = torch.empty((), device="cuda"), torch.empty_like(x)
    kind, crit = T.kind_of(name), CRIT[T.crit_of(name)]
    if kind == "multiscale":
        lf = lambda: ops.multiscale_loss_fwd(x, hr, lay, crit, out)          # noqa: E731
        lb = lambda: ops.multiscale_loss_bwd(x, hr, lay, crit, None, gx)          # noqa: E731
    else:
        lf = lambda: ops.pool_loss_fwd(x, hr, lay, SCALE, kind == "color", crit, out)          # noqa: E731
        lb = lambda: ops.pool_loss_bwd(x, hr, lay, SCALE, kind == "color", crit, None, gx)          # noqa: E731
    launches = {}
    for key, (lo, hi) in (("fwd_ms", _time(lf, iters, warmup)), ("bwd_ms", _time(lb, iters, warmup))):
        launches[key], launches[key + "_max"] = lo, hi
    launches["launch_times_floor"] = (launches["fwd_ms"] + launches["bwd_ms"]) / r["floor_ms"]
    return {k: (round(v, 4) if v > 1e-3 else float("%.3g" % v)) for k, v in r.items()}, {k: round(v, 4) for k, v in launches.items()}


def sweep_blocks(iters, warmup):
    from trainner_amd import ops
    sr, hr = _pair("nchw")
    out = torch.empty((), device="cuda")
    calls = {"avg-l1": lambda: ops.pool_loss_fwd(sr, hr, 0, SCALE, False, CRIT["l1"], out),
             "color-l1cosinesim": lambda: ops.pool_loss_fwd(sr, hr, 0, SCALE, True, CRIT["l1cosinesim"], out),
             "multiscale-l1": lambda: ops.multiscale_loss_fwd(sr, hr, 0, CRIT["l1"], out)}
    default = {}
    for name, fn in calls.items():
        fn()
        default[name] = out.item()
    rows = []
    try:
        for blocks in (64, 128, 256, 512, 1024, 2048, 4096):
            ops.pooled_forward_blocks(min(blocks, 2048), blocks)
            row = {"blocks": blocks}
            for name, fn in calls.items():
                lo, hi = _time(fn, iters, warmup)
                row[name], row[name + "_max"] = round(lo, 4), round(hi, 4)
                rel = abs(out.item() - default[name]) / abs(default[name])
                assert rel <= 2 * torch.finfo(torch.float32).eps, (name, blocks, out.item(), default[name])
            rows.append(row)
    finally:
        ops.pooled_forward_blocks(0, 0)
    return rows


def bench_step(rounds, steps, warmup):
    import bench
    from trainner_amd.models import losses
    model = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0)
    lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, model.device)
    gl = model.generatorlosses
    plain = list(gl.loss_list)
    terms = plain + [losses.get_loss_fn(n, w, device=model.device, opt={"scale": SCALE}) for n, w in TERMS]
    times = {"plain": [], "pooled": []}
    step = [0]

    def run(n):
        for _ in range(n):
            step[0] += 1
            model.feed_data({"LR": lr, "HR": hr})
            model.optimize_parameters(step[0])
        model.get_current_log()

    run(warmup)
    for _ in range(rounds):
        for key, regular in (("plain", plain), ("pooled", terms)):
            gl.loss_list = regular
            run(1)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(steps)
            b.record()
            torch.cuda.synchronize()
            times[key].append(a.elapsed_time(b) / steps)
    return {"batch": bench.BATCH_PER_GPU, "crop": bench.CROP, "steps_per_sample": steps,
            "ms_per_step": {k: {"mean": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                                "samples": [round(x, 3) for x in v]} for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--sweep-blocks", action="store_true")
    args = ap.parse_args()
    from trainner_amd import hip
    hip.require_device()
    out = {"tool": "bench_pooled_losses", "device": torch.cuda.get_device_name(0), "shape": "x".join(map(str, SHAPE)), "scale": SCALE,
           "loss": {}, "launches": {}}
    for layout in ("nchw", "cl"):
        out["loss"][layout], out["launches"][layout] = {}, {}
        for name, _ in TERMS:
            out["loss"][layout][name], out["launches"][layout][name] = bench_loss(name, layout, args.iters, args.warmup)
    if args.sweep_blocks:
        out["sweep_blocks"] = sweep_blocks(args.iters, args.warmup)
    if not args.no_step:
        out["step"] = bench_step(args.step_rounds, args.steps, min(args.warmup, 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
