"""DiffAugment: device time of each launch and of whole applications beside a device-to-device copy, the same composite through plain
torch, and the whole training step with diffaug on against off.  Prints one JSON line:

    python tools/bench_diffaug.py [--iters 50] [--warmup 10] [--step-rounds 3] [--steps 4] [--no-step]

copy               a device-to-device copy of one 16 x 3 x 512 x 512 fp32 tensor (50.3 MB read + 50.3 MB written), HIP events, the
                   smallest of three means over --iters calls: the floor of a pass that reads a tensor once and writes it once
configs[layout][config]
                   the recipe policy color,transl_zoom,flip,rotate,cutout once for each of its three transl_zoom choices (flip on,
                   rotation +1), `color` alone and `translation,cutout` alone, through the ops wrappers on preallocated tensors (no
                   autograd, no allocation): every launch alone (mean, fwd, mean_bwd, bwd: ms and ms / copy ms), the forward
                   application (mean + fwd) and forward + backward (all four)
torch[config]      the restatement of tools/make_golden_diffaug.py in fp32 through plain torch on the device, forward and
                   forward + backward (autograd), NCHW
step               the whole G+D step at bench.py's configuration (model built by bench.make_model) with diffaug off (the step as it
                   is without this feature) and on (the recipe policy), alternating --step-rounds times in this one process
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_freqsep import _time  # noqa: E402

SHAPE = (16, 3, 512, 512)
RECIPE = "color,transl_zoom,flip,rotate,cutout"


def configs(dev):
    from trainner_amd.dataops import diffaug as ED
    N, _, H, W = SHAPE
    g = torch.Generator().manual_seed(11)
    color = (torch.rand(N, generator=g) - 0.5, torch.rand(N, generator=g) * 2, torch.rand(N, generator=g) + 0.5)
    transl = (torch.randint(-64, 65, (N,), generator=g), torch.randint(-64, 65, (N,), generator=g))
    cut = (torch.randint(0, H + 1, (N,), generator=g), torch.randint(0, W + 1, (N,), generator=g))
    full = dict(color=color, flip=True, rot=1, cutout=cut)
    return {"recipe_translation": ED.Params(N, H, W, kind="translation", translation=transl, **full),
            "recipe_zoom_in": ED.Params(N, H, W, kind="zoom_in", zoom=(85, 85, 341, 341), **full),          # scale 1.5, centred crop
            "recipe_zoom_out": ED.Params(N, H, W, kind="zoom_out", zoom=(70, 210, 70, 210), **full),       # scale 0.55, displaced
            "color": ED.Params(N, H, W, color=color),
            "translation_cutout": ED.Params(N, H, W, kind="translation", translation=transl, cutout=cut)}


def bench_launches(iters, warmup):
    from tools import make_golden_diffaug as T
    from trainner_amd import ops
    g = torch.Generator().manual_seed(7)
    plane = 4.0 * SHAPE[0] * SHAPE[1] * SHAPE[2] * SHAPE[3]
    base = torch.rand(*SHAPE, generator=g).cuda() * 1.2 - 0.1
    dst = torch.empty_like(base)
    copy_ms = _time(lambda: dst.copy_(base), iters, warmup)
    res = {"copy": {"ms": round(copy_ms, 4), "gb": round(2 * plane / 1e9, 4), "gbs": round(2 * plane / copy_ms / 1e6, 1)}, "configs": {},
           "torch": {}}
    cfgs = configs("cuda")

    def entry(ms):
        return {"ms": round(ms, 4), "times_copy": round(ms / copy_ms, 2)}

    for layout, fmt in ((0, torch.contiguous_format), (1, torch.channels_last)):
        x = base.contiguous(memory_format=fmt)
        grad = (torch.rand(*SHAPE, generator=g).cuda() - 0.5).contiguous(memory_format=fmt)
        out = torch.empty_like(x)
        per = {}
        for tag, prm in cfgs.items():
            geo, blk = prm.geo(), prm.block("cuda")
            color = prm.color is not None
            ws = ops.diffaug_mean(x, layout, blk, geo)          # the workspace the fused launches read (its values do not matter here)
            fwd = lambda: ((ops.diffaug_mean(x, layout, blk, geo) if color else None), ops.diffaug_fwd(x, layout, blk, geo, ws, out))
            bwd = lambda: ((ops.diffaug_mean(grad, layout, blk, geo, backward=True) if color else None),
                           ops.diffaug_bwd(grad, layout, blk, geo, ws, out))
            r = {"fwd": entry(_time(lambda: ops.diffaug_fwd(x, layout, blk, geo, ws, out), iters, warmup)),
                 "bwd": entry(_time(lambda: ops.diffaug_bwd(grad, layout, blk, geo, ws, out), iters, warmup))}
            if color:
                r["mean"] = entry(_time(lambda: ops.diffaug_mean(x, layout, blk, geo), iters, warmup))
                r["mean_bwd"] = entry(_time(lambda: ops.diffaug_mean(grad, layout, blk, geo, backward=True), iters, warmup))
            r["forward_application"] = entry(_time(fwd, iters, warmup))
            r["forward_and_backward"] = entry(_time(lambda: (fwd(), bwd()), iters, warmup))
            per[tag] = r
        res["configs"]["nchw" if layout == 0 else "channels_last"] = per
    for tag, prm in cfgs.items():
        xg = base.clone().requires_grad_(True)
        m = torch.rand(*SHAPE, generator=g).cuda() - 0.5

        def both():
            xg.grad = None
            T.restate(xg, prm).backward(m)

        with torch.no_grad():
            f = _time(lambda: T.restate(base, prm), max(3, iters // 10), 2)
        res["torch"][tag] = {"forward": entry(f), "forward_and_backward": entry(_time(both, max(3, iters // 10), 2))}
    return res


def bench_step(rounds, steps, warmup):
    import bench
    model = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0)
    lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, model.device)
    times = {"diffaug_off": [], "diffaug_on": []}
    step = [0]

    def run(n):
        for _ in range(n):
            step[0] += 1
            model.feed_data({"LR": lr, "HR": hr})
            model.optimize_parameters(step[0])
        model.get_current_log()

    run(warmup)
    for _ in range(rounds):
        for key, on in (("diffaug_off", False), ("diffaug_on", True)):
            model.adversarial.diffaug, model.adversarial.dapolicy = on, RECIPE if on else ""
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
            "on_minus_off_ms": round(ms["diffaug_on"]["mean"] - ms["diffaug_off"]["mean"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    from trainner_amd import hip
    hip.require_device()
    out = {"tool": "bench_diffaug", "device": torch.cuda.get_device_name(0), "shape": list(SHAPE)}
    out.update(bench_launches(args.iters, args.warmup))
    if not args.no_step:
        out["step"] = bench_step(args.step_rounds, args.steps, min(args.warmup, 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
