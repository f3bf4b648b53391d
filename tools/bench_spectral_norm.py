"""Spectral normalisation: device time of one training forward's normalisation and of one backward's correction over all wrapped layers
of a discriminator, beside the same work through plain torch ops on the device and beside a device copy of the weights' bytes, and the
whole training step with the flag on against off.  Prints one JSON line:

    python tools/bench_spectral_norm.py [--window-ms 300] [--warmup 10] [--step-rounds 3] [--steps 4] [--no-step] [--no-kernels]
                                        [--plain-only] [--root DIR]

nets[net]            net "patchgan": NLayerDiscriminator(3, 64, 3); net "unet": UNetDiscriminator(3, 64) -- both with the flag
    `forward`: ops.sn_forward over the net's job table in training form (4 launches: power iteration, sigma, W / sigma of every layer);
    `forward_eval`: the eval form (2 launches); `backward`: ops.sn_backward (2 launches); `generation`: what one training forward adds in
    all -- sn_forward + the net's derived-tensor refresh + the re-pack launch; `snapshot`: the copy of the derived buffer a differentiated
    forward keeps.  HIP events around back-to-back calls, the smallest of three windows; `copy_ms` is `dst.copy_(src)` over as many floats
    as the wrapped weights hold, timed in alternation, and `times_copy` the ratio.  `torch_ms`: the same arithmetic as per-layer torch ops
    on the device (mv / norm / div / outer: about 10 launches per layer).  `host_enqueue_us`: one sn_forward call without synchronisation.
step[workload]       "pix2pix": 16 x 3 x 256 x 256, ResnetGenerator-9 + PatchGAN (tools/bench_i2i.py); "sr_unet": bench.py's shape (batch 16,
    crop 512) with the U-Net discriminator and inputs resident in device memory.  ms per step with `spectral_norm` off and on, alternating
    --step-rounds times in this one process (host clock, synchronised): mean, min, max, samples.
--plain-only / --root DIR: time only the flag-off steps, importing bench.py / tools/bench_i2i.py / trainner_amd from DIR -- another
    checkout of this project (the parent commit's) measured by the same loop."""
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


def torch_forward(layers, eps=1e-12):
    for w, u, v, wn in layers:
        W = w.view(w.shape[0], -1)
        t = W.t().mv(u)
        v.copy_(t / t.norm().clamp_min(eps))
        s = W.mv(v)
        u.copy_(s / s.norm().clamp_min(eps))
        torch.div(w, torch.dot(u, W.mv(v)), out=wn)


def torch_backward(layers, recs):
    for (w, u, v, wn), (g, dw, sig) in zip(layers, recs):
        dot = (g * wn).sum()
        dw.add_((g - dot * torch.outer(u, v).view_as(g)) / sig)


def bench_kernels(window_ms, warmup):
    from trainner_amd import ops
    from trainner_amd.models.modules.architectures import discriminators as D
    out = {}
    for name, net in (("patchgan", D.NLayerDiscriminator(3, 64, 3, use_spectral_norm=True)), ("unet", D.UNetDiscriminator(3, 64, spectral_norm=True))):
        net = net.cuda().train()
        with torch.no_grad():
            net(torch.zeros(1, 3, 64, 64, device="cuda"))
        sn = net._sn
        tab = sn.table
        n = sum(L["w"].numel() for L in tab.layers)
        src, dst = torch.randn(n, device="cuda"), torch.empty(n, device="cuda")
        copy = lambda: dst.copy_(src)                                   # noqa: E731
        layers = [(L["w"].detach().clone(), L["u"].clone(), L["v"].clone(), torch.empty_like(L["wn"])) for L in tab.layers]
        recs = [(torch.randn_like(L["g"]), torch.zeros_like(L["dw"]), torch.ones((), device="cuda")) for L in tab.layers]
        r = {"layers": len(tab.layers), "weight_floats": n, "largest": list(max((tab.dims(i) for i in range(len(tab.layers))), key=lambda d: d[0] * d[1]))}

        def generation():
            sn.derive(True)
            net._refresh_derived()
            net._packer.run()

        for key, fn, tor, launches in (("forward", lambda: ops.sn_forward(tab, True), lambda: torch_forward(layers), 4),
                                       ("forward_eval", lambda: ops.sn_forward(tab, False), None, 2),
                                       ("backward", lambda: ops.sn_backward(tab), lambda: torch_backward(layers, recs), 2),
                                       ("generation", generation, None, None),
                                       ("snapshot", lambda: sn.derived.clone(), None, None)):
            ms, cp, wins = time_beside(fn, copy, window_ms, warmup)
            e = {"ms": round(ms, 4), "windows_ms": [round(x, 4) for x in wins], "copy_ms": round(cp, 4), "times_copy": round(ms / cp, 2)}
            if launches:
                e.update(launches=launches, us_per_launch=round(1e3 * ms / launches, 2))
            if tor is not None:
                tms, _, twins = time_beside(tor, copy, window_ms, 3)
                e.update(torch_ms=round(tms, 4), torch_times_engine=round(tms / ms, 2))
            r[key] = e
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(500):
            ops.sn_forward(tab, True)
        r["host_enqueue_us"] = round((time.perf_counter() - t0) / 500 * 1e6, 2)
        torch.cuda.synchronize()
        out[name] = r
        del net, src, dst, layers, recs
        torch.cuda.empty_cache()
    return out


def _stats(v):
    return {"mean": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "samples": [round(x, 3) for x in v]}


def bench_steps(rounds, steps, warmup, plain_only):
    import bench
    from tools import bench_i2i

    def p2p(flag):
        yaml = bench_i2i.YAML
        if flag:
            bench_i2i.YAML = yaml.replace("  nf: 64\ntrain:", "  nf: 64\n  spectral_norm: true\ntrain:")
            assert bench_i2i.YAML != yaml
        try:
            return bench_i2i.build("pix2pix", "resnet", 16, 256, False, torch.device("cuda", 0))
        finally:
            bench_i2i.YAML = yaml

    def sr(flag):
        m = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0, 1, "\n  type: unet\n  spectral_norm: true" if flag else "unet", False)
        lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, m.device)
        return m, {"LR": lr, "HR": hr}

    out = {}
    for wl, make in (("pix2pix", p2p), ("sr_unet", sr)):
        variants = {"off": make(False)}
        if not plain_only:
            variants["on"] = make(True)
            assert variants["on"][0].netD._has_sn and not variants["off"][0].netD._has_sn
        times = {k: [] for k in variants}
        count = {k: 0 for k in variants}

        def run(key, n):
            m, data = variants[key]
            for _ in range(n):
                count[key] += 1
                m.feed_data(data)
                m.optimize_parameters(count[key])
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
        r = {"steps_per_sample": steps, "clock": "host, synchronised", "ms_per_step": {k: _stats(v) for k, v in times.items()}}
        if "on" in times:
            r["on_minus_off_ms"] = round(r["ms_per_step"]["on"]["mean"] - r["ms_per_step"]["off"]["mean"], 3)
        out[wl] = r
        del variants
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    from trainner_amd import hip
    hip.require_device()
    out = {"tool": "bench_spectral_norm", "device": torch.cuda.get_device_name(0), "tree": "this" if root == ROOT else "other"}
    if not (args.no_kernels or args.plain_only):
        out["nets"] = bench_kernels(args.window_ms, args.warmup)
    if not args.no_step:
        out["step"] = bench_steps(args.step_rounds, args.steps, min(args.warmup, 3), args.plain_only)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
