"""Stochastic weight averaging: device time of the averaging launch over a generator-sized flat buffer beside a device copy of the same
floats and beside torch's own per-tensor form, and the whole SR training step with `use_swa` on (regime entered) against off.
Prints one JSON line:

    python tools/bench_swa.py [--window-ms 300] [--warmup 10] [--step-rounds 3] [--steps 4] [--no-step] [--no-kernels]

launch      ops.swa_update over RRDBNet-23's flat parameter buffer (the `esrgan` generator of bench.py: `floats` elements, alignment
    gaps included), weight 1 / 8.  HIP events around back-to-back calls, the smallest of three windows; `copy_ms` is `dst.copy_(src)`
    over the same number of floats, timed in alternation, and `times_copy` the ratio: the launch moves 12 bytes per element (two reads,
    one write) against the copy's 8, so 1.5 is the figure to compare with.  `GBps`: 12 x floats / time.
    `foreach_ms`: torch._foreach_lerp_ over the per-tensor views of the same two buffers (what AveragedModel does on a GPU), timed in
    alternation with the launch (`vs_foreach_launch_ms`).  `host_enqueue_us`: one ops.swa_update call without synchronisation.
step        bench.py's shape (batch 16, crop 512, RRDBNet-23 + Discriminator_VGG(512) + VGG19 features), inputs resident in device
    memory, `optimize_parameters` + `update_learning_rate` per step as train.py drives them.  ms per step with `use_swa` off and on
    (swa_start_iter 0: every step past the first averages), alternating --step-rounds times in this one process (host clock,
    synchronised): mean, min, max, samples; `on_minus_off_ms` beside `off_spread_ms` (max - min of the off samples)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def time_beside(fn, ref, window_ms, warmup, repeats=3):
    """(ms of fn, ms of ref, [fn windows]): the smallest of `repeats` windows each, the windows alternating."""
    for _ in range(warmup):
        fn()
        ref()
    iters = max(20, int(window_ms / max(_window(lambda: (fn(), ref()), 20), 1e-4)))
    a, b = [], []
    for _ in range(repeats):
        a.append(_window(fn, iters))
        b.append(_window(ref, iters))
    return min(a), min(b), a


def bench_launch(window_ms, warmup):
    from trainner_amd import ops
    from trainner_amd.models.modules.architectures import RRDBNet_arch
    net = RRDBNet_arch.RRDBNet(3, 3, 64, 23, gaussian_noise=False).cuda()
    holder = net.flat_params()
    n = holder.flat.numel()
    p = holder.flat
    avg = p.detach().clone() + 1e-3 * torch.randn_like(p)
    src, dst = torch.randn(n, device="cuda"), torch.empty(n, device="cuda")
    views_a = [avg[o:o + k].view(q.shape) for q, o, k in holder.offsets]
    views_p = [p[o:o + k].view(q.shape).detach() for q, o, k in holder.offsets]
    launch = lambda: ops.swa_update(avg, p, 7)                      # noqa: E731
    copy = lambda: dst.copy_(src)                                   # noqa: E731
    foreach = lambda: torch._foreach_lerp_(views_a, views_p, 0.125)  # noqa: E731
    ms, cp, wins = time_beside(launch, copy, window_ms, warmup)
    ms2, fe, wins2 = time_beside(launch, foreach, window_ms, warmup)
    r = {"floats": n, "tensors": len(holder.offsets), "parameters": sum(k for _, _, k in holder.offsets),
         "ms": round(ms, 4), "windows_ms": [round(x, 4) for x in wins], "copy_ms": round(cp, 4), "times_copy": round(ms / cp, 2),
         "GBps": round(12.0 * n / ms / 1e6, 1), "copy_GBps": round(8.0 * n / cp / 1e6, 1),
         "vs_foreach_launch_ms": round(ms2, 4), "foreach_ms": round(fe, 4), "foreach_times_launch": round(fe / ms2, 2)}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(500):
        launch()
    r["host_enqueue_us"] = round((time.perf_counter() - t0) / 500 * 1e6, 2)
    torch.cuda.synchronize()
    return r


def _stats(v):
    return {"mean": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "samples": [round(x, 3) for x in v]}


def bench_steps(rounds, steps, warmup):
    import bench

    def make(flag):
        yaml = bench.YAML
        if flag:
            bench.YAML = yaml.replace("use_amp: {amp}\n", "use_amp: {amp}\nuse_swa: true\n").replace("  niter: 5e5\n", "  niter: 5e5\n  swa_start_iter: 0\n")
            assert bench.YAML.count("swa") == 2
        try:
            m = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0, 1)
        finally:
            bench.YAML = yaml
        lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, m.device)
        return m, {"LR": lr, "HR": hr}

    variants = {"off": make(False), "on": make(True)}
    assert variants["on"][0].swa and not variants["off"][0].swa
    times = {k: [] for k in variants}
    count = {k: 0 for k in variants}

    def run(key, n):
        m, data = variants[key]
        for _ in range(n):
            count[key] += 1
            m.feed_data(data)
            m.optimize_parameters(count[key])
            m.update_learning_rate(count[key], warmup_iter=-1)
        m.get_current_log()

    for key in variants:
        run(key, warmup)
    for _ in range(rounds):
        for key in variants:
            run(key, 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(key, steps)
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) * 1e3 / steps)
    on = variants["on"][0]
    assert int(on.swa_model.n_averaged) == count["on"]           # every step of the on runs averaged
    r = {"steps_per_sample": steps, "clock": "host, synchronised", "ms_per_step": {k: _stats(v) for k, v in times.items()},
         "n_averaged": int(on.swa_model.n_averaged)}
    r["on_minus_off_ms"] = round(r["ms_per_step"]["on"]["mean"] - r["ms_per_step"]["off"]["mean"], 3)
    r["off_spread_ms"] = round(r["ms_per_step"]["off"]["max"] - r["ms_per_step"]["off"]["min"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from trainner_amd import hip
    hip.require_device()
    out = {"tool": "bench_swa", "device": torch.cuda.get_device_name(0)}
    if not args.no_kernels:
        out["launch"] = bench_launch(args.window_ms, args.warmup)
    if not args.no_step:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out["step"] = bench_steps(args.step_rounds, args.steps, min(args.warmup, 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
