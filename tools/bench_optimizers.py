"""The optimisers beside Adam (sgd, rmsprop, madgrad, adamp, sgdp, ranger): device time of one optimiser step over the flat buffers of
bench.py's networks (RRDBNet-23 and the 512-input Discriminator_VGG), and of the whole training step.  Prints one JSON line:

    python tools/bench_optimizers.py [--iters 30] [--warmup 3] [--step-rounds 2] [--steps 3] [--no-step]

Measured in this one process with HIP events (the smallest of three batches of --iters back-to-back calls after a warm-up):
buffers[net]            elements (with the alignment gaps), tensors, rows (of the tensors with dim() > 1), chunks; copy_ms: a device copy
                        of the buffer (one read, one write)
optim[net][name]        ms: one optimiser step through the ops entry point on preallocated buffers (for ranger: a plain step and a
                        lookahead step, `ms_lookahead`); launches; times_adam = ms / the FusedAdam launch on the same buffer;
                        floor_passes: the buffer passes the RULE must move whatever the launch plan -- adam 7 (read p g m v, write p m v),
                        sgd 5, rmsprop 5, madgrad 8, ranger 8 (one more read of g for the row means), adamp 11 and sgdp 8 (the decision
                        needs sums over every row before one element of p can be written: the moments are written in a first pass over
                        p g m v, p in a second) -- floor_ms = floor_passes x copy_ms / 2 (a copy is two passes), times_floor = ms /
                        floor_ms; moved_passes: what the launches here move
                        torch_ms: the same rule through plain torch on the device, per tensor, as the reference would run it
                        (torch.optim.SGD / RMSprop as it constructs them, the fp32 restatement of tests/optim_restate.py for the rest),
                        times_torch = torch_ms / ms
step                    the whole G+D step at bench.py's configuration with optim_G = optim_D = adam against each optimiser,
                        alternating --step-rounds times in this one process
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

from tools.bench_image_losses import _time  # noqa: E402
import optim_restate as X  # noqa: E402

NAMES = ("sgd", "rmsprop", "madgrad", "adamp", "sgdp", "ranger")
LAUNCHES = {"adam": 1, "sgd": 1, "rmsprop": 1, "madgrad": 1, "adamp": 4, "sgdp": 4, "ranger": 2}
FLOOR_PASSES = {"adam": 7, "sgd": 5, "rmsprop": 5, "madgrad": 8, "adamp": 11, "sgdp": 8, "ranger": 8}
MOVED_PASSES = {"adam": 7, "sgd": 5, "rmsprop": 5, "madgrad": 8, "adamp": 14, "sgdp": 11, "ranger": 8}
HP = {k: dict(v, lr=1e-4) for k, v in X.CONFIGS.items() if k in NAMES}


def bench_buffer(holder, iters, warmup):
    from trainner_amd import ops
    table = holder.seg_table()
    p0 = holder.flat.clone()
    g = torch.zeros_like(p0)
    gen = torch.Generator().manual_seed(11)
    for v in X.views(g, table.entries):
        v.copy_(torch.randn(v.shape, generator=gen) * 1e-3)
    dst = torch.empty_like(p0)
    copy_ms = _time(lambda: dst.copy_(p0), iters, warmup)
    info = {"elements": p0.numel(), "tensors": table.nseg, "rows": table.nrows, "chunks": table.nchunks, "copy_ms": round(copy_ms, 4)}
    res = {}

    def fresh(n, copies=()):
        return [p0.clone() if i in copies else torch.zeros_like(p0) for i in range(n)]

    p = p0.clone()
    m, v = fresh(2)
    adam_ms = _time(lambda: ops.adam_step(p, g, m, v, 1e-4, 0.9, 0.999, 1.0, 1e-8), iters, warmup)
    res["adam"] = {"ms": adam_ms}
    calls = {}
    hp = HP["sgd"]
    p1, (b1,) = p0.clone(), fresh(1)
    calls["sgd"] = lambda: ops.sgd_step(p1, g, b1, table, hp["lr"], hp["momentum"], hp["weight_decay"])
    hr = HP["rmsprop"]
    p2, (s2,) = p0.clone(), fresh(1)
    calls["rmsprop"] = lambda: ops.rmsprop_step(p2, g, s2, table, hr["lr"], hr["alpha"], hr["eps"], hr["weight_decay"])
    hm = HP["madgrad"]
    p3, (q3, s3, x3) = p0.clone(), fresh(3, copies=(2,))
    calls["madgrad"] = lambda: ops.madgrad_step(p3, g, q3, s3, x3, table, hm["lr"], hm["eps"], 7, hm["momentum"], hm["weight_decay"], hm["decay_type"])
    ha = HP["adamp"]
    p4, (m4, v4) = p0.clone(), fresh(2)
    calls["adamp"] = lambda: ops.adamp_step(p4, g, m4, v4, table, ha["lr"], *ha["betas"], ha["eps"], 8, ha["nesterov"], ha["delta"], ha["wd_ratio"],
                                            ha["weight_decay"])
    hs = HP["sgdp"]
    p5, (b5,) = p0.clone(), fresh(1)
    calls["sgdp"] = lambda: ops.sgdp_step(p5, g, b5, table, hs["lr"], hs["momentum"], hs["dampening"], hs["eps"], hs["nesterov"], hs["delta"],
                                          hs["wd_ratio"], hs["weight_decay"])
    hg = HP["ranger"]
    p6, (m6, v6, w6) = p0.clone(), fresh(3, copies=(2,))

    def ranger(t):
        return lambda: ops.ranger_step(p6, g, m6, v6, w6, table, hg["lr"], *hg["betas"], hg["eps"], hg["weight_decay"], t, 6, hg["alpha"],
                                       hg["N_sma_threshhold"], hg["use_gc"], hg["gc_conv_only"])
    calls["ranger"] = ranger(7)
    for name in NAMES:
        res[name] = {"ms": _time(calls[name], iters, warmup)}
    res["ranger"]["ms_lookahead"] = round(_time(ranger(12), iters, warmup), 4)

    # the same rules through plain torch on the device, per tensor
    t_iters = max(iters // 10, 2)
    for name in NAMES:
        ps = [q.clone() for q in X.views(p0, table.entries)]
        gs = X.views(g, table.entries)
        if name in ("sgd", "rmsprop"):
            params = [torch.nn.Parameter(q) for q in ps]
            for q, gr in zip(params, gs):
                q.grad = gr.clone()
            h = HP[name]
            o = torch.optim.SGD(params, lr=h["lr"], weight_decay=h["weight_decay"], momentum=h["momentum"]) if name == "sgd" else \
                torch.optim.RMSprop(params, lr=h["lr"], weight_decay=h["weight_decay"], eps=h["eps"])
            fn = o.step
        else:
            run = X.Run(name, ps, dict(HP[name], k=6) if name == "ranger" else HP[name], torch.float32)
            fn = lambda run=run: run.step(gs)          # noqa: E731
        res[name]["torch_ms"] = _time(fn, t_iters, 1, repeats=2)
    for name, r in res.items():
        r["launches"] = LAUNCHES[name]
        r["floor_passes"], r["moved_passes"] = FLOOR_PASSES[name], MOVED_PASSES[name]
        r["floor_ms"] = FLOOR_PASSES[name] * copy_ms / 2
        r["times_floor"] = r["ms"] / r["floor_ms"]
        r["times_adam"] = r["ms"] / adam_ms
        if "torch_ms" in r:
            r["times_torch"] = r["torch_ms"] / r["ms"]
        res[name] = {k: round(v, 4) if isinstance(v, float) else v for k, v in r.items()}
    return info, res


def bench_step(model, rounds, steps, warmup):
    import bench
    from trainner_amd.models import optimizers
    lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, model.device)
    opts = {"adam": (model.optimizer_G, model.optimizer_D)}
    for name in NAMES:
        opts[name] = (optimizers.config_optimizer({"optim_G": name}, "G", [model.netG]), optimizers.config_optimizer({"optim_D": name}, "D", [model.netD]))
    times = {k: [] for k in opts}
    step = [0]

    def run(n):
        for _ in range(n):
            step[0] += 1
            model.feed_data({"LR": lr, "HR": hr})
            model.optimize_parameters(step[0])
        model.get_current_log()

    def measure(key):
        model.optimizer_G, model.optimizer_D = opts[key]
        run(1)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run(steps)
        b.record()
        torch.cuda.synchronize()
        times[key].append(a.elapsed_time(b) / steps)

    run(warmup)
    for _ in range(rounds):
        for name in NAMES:
            measure("adam")
            measure(name)
    model.optimizer_G, model.optimizer_D = opts["adam"]
    return {"batch": bench.BATCH_PER_GPU, "crop": bench.CROP, "steps_per_sample": steps,
            "ms_per_step": {k: {"mean": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    import bench
    from trainner_amd import hip
    hip.require_device()
    model = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0)
    out = {"tool": "bench_optimizers", "device": torch.cuda.get_device_name(0), "buffers": {}, "optim": {}}
    for net in ("G", "D"):
        out["buffers"][net], out["optim"][net] = bench_buffer(getattr(model, "net" + net).flat_params(), args.iters, args.warmup)
    if not args.no_step:
        out["step"] = bench_step(model, args.step_rounds, args.steps, min(args.warmup, 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
