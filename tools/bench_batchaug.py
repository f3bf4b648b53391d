"""Batch augmentations: device time of every op beside a device-to-device copy of the output's bytes and beside the same op through
plain torch, the host time of `draw`, and the whole training step with `mixup` on against off.  Prints one JSON line:

    python tools/bench_batchaug.py [--window-ms 500] [--warmup 20] [--step-rounds 3] [--steps 4] [--no-step]

Before anything is timed, every op's output at the timed size is compared with the fp32 restatement of
tools/make_golden_batchaug.py on the CPU with torch.equal.

pairs[pair][layout][op]
    pair "x4": target 16 x 3 x 512 x 512 with input 16 x 3 x 128 x 128; pair "x1": 16 x 3 x 256 x 256 twice.  Per op the time of ONE
    launch on the target-sized image (`target`), on the input-sized image (`input`) and of the whole call (`call`: every launch the op
    issues, through ops.* on preallocated outputs).  HIP events around back-to-back calls, the smallest of three windows (the calls per window sized so that an op's window and its
    copy's window take --window-ms together: thousands of calls);
    the copy of the same bytes (`dst.copy_(src)`) is timed in alternation with the op, window by window, and `times_copy` is their
    ratio.  `gbs`: the bytes the op must move over the time: per output element one 4-byte write and one 4-byte read per source
    the element's region needs (SELF, PARTNER, LERP_COLOUR: one; LERP_PARTNER: two), counted from the box; the mask adds one byte per
    s x s block.  Input-sized launches of the x4 pair move 6 MB in a few microseconds: there the window measures the host's
    enqueue rate (`host_enqueue_us` is one ops call without any synchronisation), not the kernel.
    `mask_fwd_bwd`: apply_mask on a generated image that requires grad and on the target, forward + backward (three launches).
    `torch`: the restatement through plain torch on the device for the same call.
draw_host_ms[op]
    host time of one `draw` at the x4 pair (time.perf_counter, mean of 20): `cutout` makes 16 x 128 x 128 = 262 144 host draws.
step
    the whole G+D step at bench.py's configuration with mixup off, with the recipe's mixopts, and with cutout alone (the op with
    the long host draw), alternating --step-rounds times in this one process.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PAIRS = {"x4": ((16, 3, 512, 512), (16, 3, 128, 128)), "x1": ((16, 3, 256, 256), (16, 3, 256, 256))}
RECIPE = dict(mixopts=["blend", "rgb", "mixup", "cutmix", "cutmixup"], mixprob=[1.0] * 5, mixalpha=[0.6, 1.0, 1.2, 0.7, 0.7],
              aux_mixprob=1.0, aux_mixalpha=1.2)
READS = {0: 1, 1: 1, 2: 2, 3: 1}          # sources read per output element, by region code


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def time_beside(fn, ref, window_ms, warmup, repeats=3):
    """(ms of fn, ms of ref): the smallest of `repeats` windows each, the windows alternating.  The calls per window are sized so that
    one window of each takes about `window_ms` together."""
    for _ in range(warmup):
        fn()
        ref()
    iters = max(20, int(window_ms / max(_window(lambda: (fn(), ref()), 20), 1e-4)))
    best = [float("inf"), float("inf")]
    for _ in range(repeats):
        best[0] = min(best[0], _window(fn, iters))
        best[1] = min(best[1], _window(ref, iters))
    return best


def records(pair):
    """One hand-set record per op at the pair's size: the recipe's alphas, boxes at offsets that are no multiple of 4."""
    from trainner_amd.dataops import batchaug as EB
    (N, _, H, W), (_, _, h, w) = PAIRS[pair]
    s = H // h
    rng = np.random.RandomState(5)
    r = list(rng.permutation(N))
    ch, cw = int(h * 0.7), int(w * 0.7)
    box = (h // 8 + 1, w // 8 + 3, ch, cw | 1 if cw | 1 <= w - w // 8 - 3 else cw)
    kw = dict(N=N, h=h, w=w, scale=s)
    recs = {"blend": EB.Params("blend", True, v=0.8, colour=torch.rand(N, 3, generator=torch.Generator().manual_seed(3)), **kw),
            "rgb": EB.Params("rgb", True, perm=(2, 0, 1), **kw),
            "mixup": EB.Params("mixup", True, v=0.37, r=r, **kw),
            "cutmix": EB.Params("cutmix", True, box=box, r=r, **kw),
            "cutmixup": EB.Params("cutmixup", True, box=box, r=r, v=0.37, aux_hit=True, coin=True, **kw),
            "cutout": EB.Params("cutout", True, mask=(rng.random_sample((N, h, w)) >= 0.3).astype(np.uint8), **kw)}
    if s == 1:
        recs["cutblur"] = EB.Params("cutblur", True, box=box, coin=True, **kw)
    return recs


def op_bytes(prm, shape, which):
    """The bytes one launch must move on the image `which` (0 target, 1 input), or None when the op leaves that image alone."""
    from trainner_amd.dataops import batchaug as EB
    N, C, H, W = shape
    numel = N * C * H * W
    s = prm.scale if which == 0 else 1
    if prm.aug == "cutout":
        return None if which == 0 else 8 * numel + N * H * W
    if prm.aug == "cutblur":
        return None if which == 0 else 8 * numel
    if prm.aug in ("blend", "rgb"):
        return 8 * numel
    if prm.aug == "mixup":
        return 12 * numel
    inside = N * C * prm.box[2] * prm.box[3] * s * s
    code_in = EB.PARTNER if prm.aug == "cutmix" else (EB.LERP_PARTNER if prm.aug == "cutmixup" and prm.coin else EB.SELF)
    code_out = EB.SELF if (prm.aug == "cutmix" or prm.coin) else EB.LERP_PARTNER
    return 4 * numel + 4 * (inside * READS[code_in] + (numel - inside) * READS[code_out])


def bench_ops(window_ms, warmup):
    from tools import make_golden_batchaug as T
    from trainner_amd import ops
    from trainner_amd.dataops import batchaug as EB
    g = torch.Generator().manual_seed(7)
    res = {"pairs": {}, "draw_host_ms": {}}
    for pair, (s1, s2) in PAIRS.items():
        host1, host2 = torch.rand(*s1, generator=g) * 1.2 - 0.1, torch.rand(*s2, generator=g) * 1.2 - 0.1
        hostg = torch.rand(*s1, generator=g) - 0.5
        recs = records(pair)
        res["pairs"][pair] = {}
        for lname, fmt in (("nchw", torch.contiguous_format), ("channels_last", torch.channels_last)):
            d1, d2 = host1.cuda().contiguous(memory_format=fmt), host2.cuda().contiguous(memory_format=fmt)
            dg = hostg.cuda().contiguous(memory_format=fmt)
            c1, c2 = torch.empty_like(d1), torch.empty_like(d2)
            layout = 0 if lname == "nchw" else 1
            per = {}
            for op, prm in recs.items():
                # correctness first, at the timed size
                o1, o2, mask = EB.apply(prm, d1, d2)
                w1, w2 = T.restate(prm, host1, host2)
                assert torch.equal(o1.cpu(), w1) and torch.equal(o2.cpu(), w2), (pair, lname, op)
                # the launches of the call, captured once through the module and replayed on preallocated outputs
                launches = []
                real_mix, real_mask = ops.batchaug_mix, ops.batchaug_mask
                ops.batchaug_mix = lambda *a, **k: launches.append((real_mix, a, k))
                ops.batchaug_mask = lambda *a, **k: launches.append((real_mask, a, k))
                try:
                    EB.apply(prm, d1, d2)
                finally:
                    ops.batchaug_mix, ops.batchaug_mask = real_mix, real_mask
                r = {}
                for fn, a, k in launches:
                    x = a[0]
                    which = 0 if x.data_ptr() == d1.data_ptr() else 1
                    src, dst = (d1, c1) if which == 0 else (d2, c2)
                    ms, cp = time_beside(lambda: fn(*a, **k), lambda: dst.copy_(src), window_ms, warmup)
                    nbytes = op_bytes(prm, tuple(x.shape), which)
                    r["target" if which == 0 else "input"] = {"ms": round(ms, 4), "copy_ms": round(cp, 4), "times_copy": round(ms / cp, 2),
                                                              "mb": round(nbytes / 1e6, 2), "gbs": round(nbytes / ms / 1e6, 1)}
                call = lambda: [fn(*a, **k) for fn, a, k in launches]          # noqa: E731
                tor = lambda: T.restate(prm, d1, d2)                            # noqa: E731
                ms, tms = time_beside(call, tor, window_ms, 3)
                r["call"] = {"ms": round(ms, 4), "launches": len(launches)}
                r["torch"] = {"ms": round(tms, 4), "times_engine": round(tms / ms, 2)}
                per[op] = r
            # apply_mask forward + backward at the target's size
            prm = recs["cutout"]
            ba = EB.BatchAugment(dict(mixopts=["cutout"], mixprob=[1.0], mixalpha=[0.3]))
            ba.aug, ba.mask = "cutout", prm.on_device("mask", "cuda")
            mfl = T.up_mask(prm.mask, prm.scale).float().cuda()
            gen = d1.clone().requires_grad_(True)
            f1, f2 = ba.apply_mask(gen, d1)
            f1.backward(dg)
            assert torch.equal(f1.detach().cpu(), T.restate_mask(host1, prm.mask, prm.scale))
            assert torch.equal(gen.grad.cpu(), T.restate_mask(hostg, prm.mask, prm.scale))

            def engine():
                gen.grad = None
                a, _ = ba.apply_mask(gen, d1)
                a.backward(dg)

            def plain():
                gen.grad = None
                a, _ = gen * mfl, d1 * mfl
                a.backward(dg)

            ms, tms = time_beside(engine, plain, window_ms, 3)
            one, cp = time_beside(lambda: ops.batchaug_mask(d1, layout, ba.mask, prm.scale, c1), lambda: c1.copy_(d1), window_ms, warmup)
            nbytes = 8 * d1.numel() + prm.mask.size
            per["mask_fwd_bwd"] = {"ms": round(ms, 4), "launches": 3, "torch_ms": round(tms, 4), "torch_times_engine": round(tms / ms, 2),
                                   "one_launch": {"ms": round(one, 4), "copy_ms": round(cp, 4), "times_copy": round(one / cp, 2),
                                                  "gbs": round(nbytes / one / 1e6, 1)}}
            res["pairs"][pair][lname] = per
    # one ops call without synchronisation: what the host needs to enqueue a launch
    small, out = torch.rand(2, 3, 8, 8).cuda(), torch.empty(2, 3, 8, 8).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(2000):
        ops.batchaug_mix(small, 0, [0, 0, 0, 0, 0, 0, 0, 1, 2, 3], 1.0, 0.0, out)
    res["host_enqueue_us"] = round((time.perf_counter() - t0) / 2000 * 1e6, 2)
    torch.cuda.synchronize()
    # host time of the draws at the x4 pair
    s1, s2 = PAIRS["x4"]
    for op, alpha in (("blend", 0.6), ("rgb", 1.0), ("mixup", 1.2), ("cutmix", 0.7), ("cutmixup", 0.7), ("cutout", 0.001)):
        t0 = time.perf_counter()
        for _ in range(20):
            prm = EB.draw([op], [1.0], [alpha], 1.0, 1.2, None, s1, s2, "cuda")
        res["draw_host_ms"][op] = round((time.perf_counter() - t0) / 20 * 1e3, 4)
    t0 = time.perf_counter()
    for _ in range(20):
        prm._dev.clear()
        prm.on_device("mask", "cuda")
    res["draw_host_ms"]["cutout_mask_upload"] = round((time.perf_counter() - t0) / 20 * 1e3, 4)
    return res


def bench_step(rounds, steps, warmup):
    import bench
    from trainner_amd.dataops import batchaug as EB
    model = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0)
    lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, model.device)
    variants = {"mixup_off": None, "recipe": EB.BatchAugment(RECIPE),
                "cutout": EB.BatchAugment(dict(mixopts=["cutout"], mixprob=[1.0], mixalpha=[0.001]))}
    times = {k: [] for k in variants}
    step = [0]

    def run(n):
        for _ in range(n):
            step[0] += 1
            model.feed_data({"LR": lr, "HR": hr})
            model.optimize_parameters(step[0])
        model.get_current_log()

    run(warmup)
    for _ in range(rounds):
        for key, ba in variants.items():
            model.mixup, model.batchaugment = ba is not None, ba
            run(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(steps)
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) * 1e3 / steps)
    ms = {k: {"mean": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "samples": [round(x, 3) for x in v]}
          for k, v in times.items()}
    return {"batch": bench.BATCH_PER_GPU, "crop": bench.CROP, "steps_per_sample": steps, "clock": "host, synchronised", "ms_per_step": ms,
            "recipe_minus_off_ms": round(ms["recipe"]["mean"] - ms["mixup_off"]["mean"], 3),
            "cutout_minus_off_ms": round(ms["cutout"]["mean"] - ms["mixup_off"]["mean"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=500.0)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    from trainner_amd import hip
    hip.require_device()
    np.random.seed(1)
    out = {"tool": "bench_batchaug", "device": torch.cuda.get_device_name(0), "pairs_shapes": {k: [list(a), list(b)] for k, (a, b) in PAIRS.items()}}
    out.update(bench_ops(args.window_ms, args.warmup))
    if not args.no_step:
        out["step"] = bench_step(args.step_rounds, args.steps, min(args.warmup, 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
