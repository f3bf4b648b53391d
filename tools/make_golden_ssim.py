"""tests/golden/ssim_loss.pt from the REFERENCE's own SSIM / MS_SSIM modules (codes/models/modules/ssim.py) and, for the step-level
records, its own SRModel -- run on the CPU where the reference tree exists (never on a GPU machine):

    python tools/make_golden_ssim.py

Loss cases.  Every case is an (sr, hr) pair that `make_inputs` rebuilds from a seed alone (oracle.detrand's counter-based uniforms,
fp64 arithmetic, rounded to fp32 last), because the pairs themselves (474 k pixels, twice, plus an fp64 gradient each) are several
times the size a committed file may have.  The fixture therefore holds, per case and per loss type: probes of the two inputs (so a
consumer can tell that it rebuilt the same pair), the reference's fp64 value, probes (strided samples, sum, L2 norm) of the reference's
fp64 d value / d sr, and the reference's OWN fp32 deviation from its fp64 run (`e32_val`, `e32_grad` = max |g32 - g64|): the
yardstick of the GPU test's tolerance.  `restate` below is an fp64 restatement of the two losses in plain torch; this tool asserts
restate == reference to 1e-12 (value and every gradient element) for every case before it writes the file, so the tests can
compare the engine with `restate`'s full gradient on machines where the reference does not exist.

"Regular" cases must stay away from both branches of the definition: the tool asserts that no position's variance is clamped in
the reference's fp32 and fp64 runs and that every per-level per-image `cs` / `ssim` exceeds 0.5.  Two "branch" cases are built so
that the branches do act (a constant patch in sr: the variance clamp region; one image negated and offset: a negative `cs`, so the
relu).  For those only the value is recorded.

Step records: the reference's SRModel (the harness's small ESRGAN config plus `ssim_type` / `ssim_weight: 1`), two steps per type,
in the format of oracle/make_golden.py's fixtures.
"""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import detrand  # noqa: E402
from oracle import ref_harness as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ssim_loss.pt")
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
TYPES = ("ssim", "ms-ssim")

# name -> (N, C, H, W, channels_last, seed)
REGULAR = {
    "sq192": (2, 3, 192, 192, False, 11),         # all five levels at 11 taps
    "sq136": (2, 3, 136, 136, False, 12),         # last level 7 taps
    "sq72": (2, 3, 72, 72, False, 13),            # 7 taps, then 3 taps
    "odd99x117": (2, 3, 99, 117, False, 14),      # odd sizes: pooling padding on both axes, 5 taps at the last level
    "gray72": (2, 1, 72, 72, False, 15),          # C = 1
    "cl136": (2, 3, 136, 136, True, 16),          # channels-last
}
BRANCH = {
    "clamp_patch": (2, 3, 72, 72, False, 21),     # sr with a constant 24 x 24 patch
    "relu_negated": (2, 3, 72, 72, False, 22),    # image 1 of sr negated and offset: a cs goes negative
}
STEP_YAML = dict(nb=1, batch=2, crop=64, d_nf=16)
STEP_SEED, STEP_K = 171, 2


# ------------------------------------------------------------------------------------------------ inputs
def _normal(numel, seed):
    """N(0, 1) by Box-Muller from two counter-based uniform streams, fp64."""
    u1 = 1.0 - detrand.uniform01(numel, seed).double()          # (0, 1]
    u2 = detrand.uniform01(numel, seed + 500000).double()
    return torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(2.0 * math.pi * u2)


def make_inputs(name):
    """-> (sr, hr) fp32.  hr = bicubic x4 upsampling of uniform noise plus 0.05 N(0, 1), clamped to [0, 1];
    sr = hr + 0.08 N(0, 1), clamped to [-0.1, 1.1]; the branch cases then edit sr."""
    N, C, H, W, cl, seed = (REGULAR.get(name) or BRANCH[name])
    lh, lw = -(-H // 4), -(-W // 4)
    low = detrand.uniform01(N * C * lh * lw, 7000 + seed).double().reshape(N, C, lh, lw)
    up = F.interpolate(low, scale_factor=4, mode="bicubic", align_corners=False)[..., :H, :W]
    n = N * C * H * W
    hr = (up + 0.05 * _normal(n, 8000 + seed).reshape(N, C, H, W)).clamp(0.0, 1.0)
    sr = (hr + 0.08 * _normal(n, 9000 + seed).reshape(N, C, H, W)).clamp(-0.1, 1.1)
    if name == "clamp_patch":
        sr[:, :, 20:44, 24:48] = 0.3
    if name == "relu_negated":
        sr[1] = 0.9 - hr[1]
    sr, hr = sr.float().contiguous(), hr.float().contiguous()
    if cl:
        sr, hr = sr.contiguous(memory_format=torch.channels_last), hr.contiguous(memory_format=torch.channels_last)
    return sr, hr


def probe(t, n=64):
    f = t.detach().contiguous().flatten().to(torch.float64)      # NCHW order whatever the strides
    stride = max(1, f.numel() // n)
    return {"samples": f[::stride][:n].clone(), "stride": stride, "l2": f.norm().item(), "sum": f.sum().item(), "numel": f.numel()}


def probe_error(t, pr):
    """max |sample difference| and |sum difference| of tensor t against a stored probe."""
    f = t.detach().contiguous().flatten().to(torch.float64)
    assert f.numel() == pr["numel"]
    return (f[::pr["stride"]][:len(pr["samples"])] - pr["samples"]).abs().max().item(), abs(f.sum().item() - pr["sum"])


# ------------------------------------------------------------------------------------------------ restatement
def window(size, sigma):
    """fp32 taps, as the losses define them: exp(-(x - size // 2)^2 / (2 sigma^2)) rounded to fp32, normalised in fp32."""
    g = torch.tensor([math.exp(-(x - size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(size)], dtype=torch.float32)
    return g / g.sum()


def _separable(t, taps):
    k = taps.numel()
    ow, oh = t.shape[-1] - k + 1, t.shape[-2] - k + 1
    r = sum(taps[i] * t[..., :, i:i + ow] for i in range(k))
    return sum(taps[i] * r[..., i:i + oh, :] for i in range(k))


def maps(x, y, taps, C1, C2):
    """-> (ssim_map, cs_map, clamped positions).  Variances below 0 are set to 0 (no gradient through a clamped one)."""
    taps = taps.to(x.dtype)
    mu1, mu2 = _separable(x, taps), _separable(y, taps)
    s1 = _separable(x * x, taps) - mu1 * mu1
    s2 = _separable(y * y, taps) - mu2 * mu2
    s12 = _separable(x * y, taps) - mu1 * mu2
    clamped = int((s1 < 0).sum() + (s2 < 0).sum())
    s1 = torch.where(s1 < 0, torch.zeros_like(s1), s1)
    s2 = torch.where(s2 < 0, torch.zeros_like(s2), s2)
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    return (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs, cs, clamped


def level_table(h, w, size=11, sigma=1.5, levels=5):
    """(h, w, taps, sigma) per MS-SSIM level of an h x w image (after the shave): a window that no longer fits shrinks to the
    largest odd size that does, sigma scales with it, and both carry over to the following levels."""
    out = []
    for i in range(levels):
        if size > h or size > w:
            new = min(size, h, w)
            new -= 1 - new % 2
            sigma, size = new * sigma / size, new
        out.append((h, w, size, sigma))
        h, w = (h + 2 * (h % 2) - 2) // 2 + 1, (w + 2 * (w % 2) - 2) // 2 + 1
    return out


def restate(sr, hr, kind, shave=4, detail=None):
    """The loss FUNCTION f(sr, hr) of `ssim_type: kind` (the training term is weight * (1 - f)), in the dtype of the inputs.
    detail: a dict that receives 'clamped' (count) and 'levels' ([(ssim per image, cs per image)])."""
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    x = sr[..., shave:sr.shape[-2] - shave, shave:sr.shape[-1] - shave]
    y = hr[..., shave:hr.shape[-2] - shave, shave:hr.shape[-1] - shave]
    clamped, per_level = 0, []
    if kind == "ssim":
        m, cs, clamped = maps(x, y, window(11, 1.5), C1, C2)
        per_level.append((m.mean((1, 2, 3)).detach(), cs.mean((1, 2, 3)).detach()))
        value = m.mean()
    else:
        w = torch.tensor(MS_WEIGHTS, dtype=torch.float32).to(x.dtype)
        table = level_table(x.shape[-2], x.shape[-1])
        value = 1.0
        for i, (h, wd, k, sigma) in enumerate(table):
            m, cs, c = maps(x, y, window(k, sigma), C1, C2)
            clamped += c
            mi, ci = torch.relu(m.mean((1, 2, 3))), torch.relu(cs.mean((1, 2, 3)))
            per_level.append((m.mean((1, 2, 3)).detach(), cs.mean((1, 2, 3)).detach()))
            if i < len(table) - 1:
                value = value * ci ** w[i]
                pad = (x.shape[-2] % 2, x.shape[-1] % 2)
                x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
            else:
                # the last level's ssim ** w[-1] multiplies each of the levels - 1 rows before the product over the rows
                value = value * mi ** (w[i] * (len(table) - 1))
        value = value.mean()
    if detail is not None:
        detail["clamped"], detail["levels"] = clamped, per_level
    return value


def restate_with_grad(sr, hr, kind, dtype=torch.float64):
    x = sr.detach().to(dtype).contiguous().requires_grad_(True)
    detail = {}
    v = restate(x, hr.detach().to(dtype).contiguous(), kind, detail=detail)
    v.backward()
    return v.detach(), x.grad.detach(), detail


# ------------------------------------------------------------------------------------------------ the reference
def ssim_yaml(path, ssim_type, weight=1):
    """Add the two loss lines to the train block of a yaml written by oracle.ref_harness.esrgan_yaml."""
    with open(path) as fh:
        txt = fh.read()
    assert txt.count("\nlogger:") == 1
    txt = txt.replace("\nlogger:", "\n  ssim_type: %s\n  ssim_weight: %g\nlogger:" % (ssim_type, weight))
    with open(path, "w") as fh:
        fh.write(txt)
    return path


def _reference_modules():
    with R.reference_env():
        for m in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data", "cv2", "torchvision")]:
            del sys.modules[m]
        from models.modules import ssim as S
    return S


def reference_run(S, sr, hr, kind, dtype, channels):
    """The reference module's value and d value / d sr in `dtype`, the count of variance positions its clamp touched and its
    per-level per-image (ssim, cs)."""
    kw = dict(window_size=11, window_sigma=1.5, size_average=True, data_range=1., channels=channels)
    mod = (S.SSIM(**kw) if kind == "ssim" else S.MS_SSIM(normalize="relu", **kw)).to(dtype)
    seen = {"filtered": [], "levels": []}
    real_filter, real_ssim = S.apply_gaussian_filter, S.ssim

    def spy_filter(*a, **k):
        out = real_filter(*a, **k)
        seen["filtered"].append(out.detach())
        return out

    def spy_ssim(*a, **k):
        out = real_ssim(*a, **k)
        seen["levels"].append(tuple(t.detach() for t in out))
        return out

    x = sr.detach().to(dtype).contiguous().requires_grad_(True)
    S.apply_gaussian_filter, S.ssim = spy_filter, spy_ssim
    try:
        v = mod(x, hr.detach().to(dtype).contiguous())
    finally:
        S.apply_gaussian_filter, S.ssim = real_filter, real_ssim
    v.backward()
    clamped = 0
    f = seen["filtered"]
    for i in range(0, len(f), 5):            # mu1, mu2, G[xx], G[yy], G[xy] per call
        clamped += int(((f[i + 2] - f[i].pow(2)) < 0).sum() + ((f[i + 3] - f[i + 1].pow(2)) < 0).sum())
    return v.detach(), x.grad.detach(), clamped, seen["levels"]


def loss_cases(S):
    cases = {}
    for name in list(REGULAR) + list(BRANCH):
        regular = name in REGULAR
        N, C, H, W, cl, seed = (REGULAR.get(name) or BRANCH[name])
        sr, hr = make_inputs(name)
        rec = {"shape": (N, C, H, W), "channels_last": cl, "regular": regular, "sr": probe(sr), "hr": probe(hr), "types": {}}
        for kind in TYPES:
            v64, g64, c64, lev64 = reference_run(S, sr, hr, kind, torch.float64, C)
            v32, g32, c32, lev32 = reference_run(S, sr, hr, kind, torch.float32, C)
            rv, rg, detail = restate_with_grad(sr, hr, kind)
            assert abs(rv.item() - v64.item()) <= 1e-12, (name, kind, rv.item(), v64.item())
            t = {"value": v64.item(), "e32_val": abs(v32.double().item() - v64.item()), "clamped64": c64, "clamped32": c32}
            if kind == "ms-ssim":
                per = [(cs if i < len(lev64) - 1 else sv) for i, (sv, cs) in enumerate(lev64)]
                per32 = [(cs if i < len(lev32) - 1 else sv) for i, (sv, cs) in enumerate(lev32)]
            else:
                # (size_average: the module reduces over the batch itself; the restatement's per-image means stand in)
                per = per32 = [detail["levels"][0][0]]
            t["min_level_value"] = min(min(p.min().item() for p in per), min(p.min().item() for p in per32))
            if regular:
                assert (rg - g64).abs().max().item() <= 1e-12, (name, kind, (rg - g64).abs().max().item())
                assert detail["clamped"] == 0 and c64 == 0 and c32 == 0, (name, kind, detail["clamped"], c64, c32)
                assert t["min_level_value"] > 0.5, (name, kind, t["min_level_value"])
                t["grad"] = probe(g64)
                t["grad_absmax"] = g64.abs().max().item()
                t["e32_grad"] = (g32.double() - g64).abs().max().item()
            else:
                t["relu_images"] = [n for n in range(N) if any(p[n].item() <= 0 for p in per)] if kind == "ms-ssim" else []
            rec["types"][kind] = t
            print("%-13s %-8s value %.12f e32_val %.2e" % (name, kind, t["value"], t["e32_val"]),
                  ("e32_grad %.2e of max|g| %.2e" % (t["e32_grad"], t["grad_absmax"])) if regular else
                  ("clamped64 %d clamped32 %d relu images %s" % (c64, c32, t["relu_images"])), "min level value %.3f" % t["min_level_value"])
        if name == "clamp_patch":
            assert rec["types"]["ssim"]["clamped32"] > 0 or rec["types"]["ssim"]["clamped64"] > 0, "the clamp case does not clamp"
        if name == "relu_negated":
            assert rec["types"]["ms-ssim"]["relu_images"] == [1], rec["types"]["ms-ssim"]["relu_images"]
        cases[name] = rec
    return cases


def step_record(kind):
    from oracle.make_golden import D_SEED, F_SEED, G_SEED, probe_state
    from oracle.make_golden import probe as state_probe
    yml = ssim_yaml(R.esrgan_yaml(name="golden_ssim_" + kind.replace("-", ""), **STEP_YAML), kind)
    opt, model = R.build_reference_model(yml, seed=0)
    assert [l["name"] for l in model.generatorlosses.precise_loss_list] == [kind]
    detrand.fill_state_dict_(model.netG.state_dict(), G_SEED)
    detrand.fill_state_dict_(model.netD.state_dict(), D_SEED)
    netF = R.reference_netF(model)
    detrand.fill_state_dict_({k: v for k, v in netF.state_dict().items() if k.startswith("feature_net")}, F_SEED, gain=1.0, bias_amp=0.05)
    grads = {}

    def grab(tag, net):
        def hook(optim, args, kwargs):
            if tag not in grads:
                grads[tag] = {k: state_probe(p.grad) for k, p in net.named_parameters() if p.grad is not None}
        return hook

    model.optimizer_G.register_step_pre_hook(grab("G", model.netG))
    model.optimizer_D.register_step_pre_hook(grab("D", model.netD))
    logs = []
    for s in range(1, STEP_K + 1):
        LR, HR = detrand.synthetic_pair(STEP_YAML["batch"], STEP_YAML["crop"], STEP_SEED + s)
        logs.append(R.reference_step(model, LR, HR, s))
    print("step", kind, [{k: round(v, 6) for k, v in l.items()} for l in logs])
    return {"name": "ssim_step_" + kind, "spec": {"yaml": dict(STEP_YAML), "steps": STEP_K, "seed": STEP_SEED, "ssim_type": kind},
            "network_G": dict(opt["network_G"]), "network_D": dict(opt["network_D"]),
            "seeds": {"G": G_SEED, "D": D_SEED, "F": F_SEED, "data": STEP_SEED},
            "logs": logs, "fake_H": model.fake_H.detach().clone(), "grads_step1": grads,
            "g_state": probe_state(model.netG.state_dict()), "d_state": probe_state(model.netD.state_dict()),
            "g_keys": [(k, tuple(v.shape)) for k, v in model.netG.state_dict().items()],
            "d_keys": [(k, tuple(v.shape)) for k, v in model.netD.state_dict().items()], "torch": torch.__version__}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    S = _reference_modules()
    fx = {"cases": loss_cases(S), "steps": {kind: step_record(kind) for kind in TYPES}, "torch": torch.__version__}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(fx, OUT)
    print("->", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
