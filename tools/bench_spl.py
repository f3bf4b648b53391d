"""Spatial profile losses (cpl, gpl) and the overflow loss: device time of each loss alone, of its launches, and of the whole training
step.  Prints one JSON line:

    python tools/bench_spl.py [--iters 50] [--warmup 5] [--step-rounds 3] [--steps 4] [--no-step]

All at 16 x 3 x 512 x 512 fp32, in both dense layouts (nchw, cl), measured in this one process with HIP events (the smallest of three
batches of --iters back-to-back calls after a warm-up):
loss[layout][name]      fwd_ms: the built loss function's forward under no_grad; fwd_bwd_ms: forward + backward through autograd (the
                        module path: output allocations and the scalar ops included)
                        copy_ms: a device copy of one image of the same bytes (read 50 MB, write 50 MB)
                        floor_passes: image passes the algorithm must move (forward reads sr and hr, backward reads both and writes
                        one: 5; overflow reads sr, then reads sr and writes one: 3); floor_ms = floor_passes x copy_ms / 2 (a copy is
                        two passes); times_floor = fwd_bwd_ms / floor_ms
                        torch_fwd_ms / torch_fwd_bwd_ms: the fp32 restatement of tools/make_golden_spl.py run through plain torch on
                        the device (what the reference would launch); times_torch = torch_fwd_bwd_ms / fwd_bwd_ms
launches[layout][name]  the entry points alone on preallocated tensors: ms of spl_loss_fwd (statistics + finalize + sum), spl_loss_bwd,
                        overflow_loss_fwd, overflow_loss_bwd, and of the cpl | gpl mask in one launch set
step                    the whole G+D step at bench.py's configuration without and with spl_type: spl (1e-3) + of_type: overflow (1),
                        alternating --step-rounds times in this one process
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_image_losses import _time  # noqa: E402

NAMES = ("cpl", "gpl", "overflow")
SHAPE = (16, 3, 512, 512)
TERMS = (("cpl", 1e-3), ("gpl", 1e-3), ("overflow", 1.0))


def _pair(layout):
    g = torch.Generator().manual_seed(7)
    hr = torch.rand(*SHAPE, generator=g).cuda()
    sr = hr * 1.1 - 0.05 + 0.05 * torch.randn(*SHAPE, generator=g).cuda()
    if layout == "cl":
        sr, hr = sr.contiguous(memory_format=torch.channels_last), hr.contiguous(memory_format=torch.channels_last)
    return sr, hr


def bench_loss(name, layout, iters, warmup):
    from tools import make_golden_spl as T
    from trainner_amd.models import losses
    f = losses.get_loss_fn(name, 1, device="cuda", opt={})["function"]
    sr, hr = _pair(layout)
    sr.requires_grad_(True)
    dst = torch.empty_like(hr)
    call = (lambda: f(sr)) if name == "overflow" else (lambda: f(sr, hr))
    ref = lambda: T.restate(sr, hr, name)          # noqa: E731

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

    copy_ms = _time(lambda: dst.copy_(hr), iters, warmup)
    passes = 3 if name == "overflow" else 5
    r = {"fwd_ms": _time(fwd(call), iters, warmup), "fwd_bwd_ms": _time(both(call), iters, warmup), "copy_ms": copy_ms,
         "floor_passes": passes, "floor_ms": passes * copy_ms / 2,
         "torch_fwd_ms": _time(fwd(ref), max(iters // 5, 3), 2), "torch_fwd_bwd_ms": _time(both(ref), max(iters // 5, 3), 2)}
    r["times_floor"] = r["fwd_bwd_ms"] / r["floor_ms"]
    r["times_torch"] = r["torch_fwd_bwd_ms"] / r["fwd_bwd_ms"]
    return {k: round(v, 4) for k, v in r.items()}


def bench_launches(layout, iters, warmup):
    from trainner_amd import ops
    sr, hr = _pair(layout)
    lay = 1 if layout == "cl" else 0
    loss, gx, out = torch.empty(5, device="cuda"), torch.empty_like(sr), torch.empty((), device="cuda")
    res = {}
    for tag, mask in (("cpl", ops.SPL_CPL), ("gpl", ops.SPL_GPL), ("cpl|gpl", ops.SPL_CPL | ops.SPL_GPL)):
        coef = ops.spl_coef(sr, mask)
        res[tag] = {"fwd_ms": round(_time(lambda: ops.spl_loss_fwd(sr, hr, lay, mask, False, loss, coef), iters, warmup), 4),
                    "bwd_ms": round(_time(lambda: ops.spl_loss_bwd(sr, hr, lay, mask, False, coef, None, gx), iters, warmup), 4)}
    res["overflow"] = {"fwd_ms": round(_time(lambda: ops.overflow_loss_fwd(sr, 1.0 / sr.numel(), out), iters, warmup), 4),
                       "bwd_ms": round(_time(lambda: ops.overflow_loss_bwd(sr, 1.0 / sr.numel(), None, gx), iters, warmup), 4)}
    return res


def bench_step(rounds, steps, warmup):
    import bench
    from trainner_amd.models import losses
    model = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0)
    lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, model.device)
    gl = model.generatorlosses
    plain = list(gl.loss_list)
    terms = plain + [losses.get_loss_fn(n, w, device=model.device, opt={}) for n, w in TERMS]
    times = {"plain": [], "spl_overflow": []}
    step = [0]

    def run(n):
        for _ in range(n):
            step[0] += 1
            model.feed_data({"LR": lr, "HR": hr})
            model.optimize_parameters(step[0])
        model.get_current_log()

    run(warmup)
    for _ in range(rounds):
        for key, regular in (("plain", plain), ("spl_overflow", terms)):
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
    args = ap.parse_args()
    from trainner_amd import hip
    hip.require_device()
    out = {"tool": "bench_spl", "device": torch.cuda.get_device_name(0), "shape": "x".join(map(str, SHAPE)), "loss": {}, "launches": {}}
    for layout in ("nchw", "cl"):
        out["loss"][layout] = {n: bench_loss(n, layout, args.iters, args.warmup) for n in NAMES}
        out["launches"][layout] = bench_launches(layout, args.iters, args.warmup)
    if not args.no_step:
        out["step"] = bench_step(args.step_rounds, args.steps, min(args.warmup, 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
