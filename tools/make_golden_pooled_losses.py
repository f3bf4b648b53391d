"""tests/golden/pooled_losses.pt from the REFERENCE's own loss builder (codes/models/losses.py get_loss_fn -> modules/loss.py ColorLoss,
AverageLoss, MultiscalePixelLoss over the criteria, L1CosineSim among them) and, for the step-level record, its own SRModel -- run on
the CPU where the reference tree exists (never on a GPU machine):

    python tools/make_golden_pooled_losses.py

A case is a shape, a pool k (opt['scale'] for color-* and avg-*) and the loss names run on it (CASES below).  The shapes are the
smallest at which the kernels can go wrong:

    multi-scale   16 x 16 (level 4 is one cell), 40 x 52 (H % 16 = 8, W % 16 = 4), 37 x 45 (odd at every level, W % 4 != 0),
                  80 x 144 (several 64 x 16 bands both ways), C = 1, C = 2 and C = 4
    average       k = 4 at 10 x 11 (cut rows and columns), k = 1, k = 2 (C = 4 and C = 2), k = 3 (C = 1), k = 8 at 24 x 40 and k = 4 at
                  14 x 20 (both W % 4 = 0: the 16-byte path, the second with cut rows)
    colour        k = 4 at 10 x 11 and at 64 x 48 (16-byte path), k = 1
    recipe64x48   the 64 x 48 pair with the three names of the shipped recipe (color-l1cosinesim, avg-l1, multiscale-l1), which the
                  GeneratorLoss test logs together
C = 2 and the k = 4 case with cut rows on the 16-byte path are additions to the list the feature was specified with: every channel
count is its own kernel instantiation, and the cut cells take their own store path.

hr = U[0, 1); sr = hr + U(-0.15, 0.15), so sr leaves [0, 1] slightly, as a generator's output does.  The cases marked BLACK zero one
hr pixel in all channels: a zero-norm second operand of the cosine (finite gradient).  No case has a zero pixel in sr.

Per case and name the fixture holds the reference's fp64 value, probes of its fp64 gradient, max |gradient|, and the reference's OWN
fp32 deviations from its fp64 run: e32_val, e32_grad and, per level, e32_resp, the deviation of the pooled responses
d = M(P x) - M(P y) the criterion sees.  For the criteria with a kink at d = 0 (all but l2) the sign of a pooled d is not exact in
fp32: the cells with 0 < |d64| <= 4 e32_resp[level] are `ambiguous`, their footprint in the gradient is left out of e32_grad here and
of the comparison in the tests (`kept_mask`), and the tool asserts that at most 1 % of a case's cells are ambiguous.  Levels whose
cells are single pixels are never ambiguous: the sign of an fp32 subtraction is exact.

`restate` below is an fp64 restatement of the losses in plain torch, written from their formulas; the tool asserts
restate == reference to 1e-12 (value, every gradient element relative to max |gradient|, and every response) before it writes the
file, so the tests can compare the engine with `restate`'s full gradient on machines where the reference does not exist.

Step record: the reference's SRModel (the harness's small ESRGAN config, scale 4) with the recipe's six lines, two steps.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import detrand  # noqa: E402
from oracle import ref_harness as R  # noqa: E402
from tools import make_golden_ssim as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pooled_losses.pt")
CRITERIA = ("l1", "l2", "cb", "elastic", "clipl1", "l1cosinesim")
KINK_FREE = ("l2",)
MS_WEIGHTS = (1.0, 0.5, 0.25, 0.125, 0.125)
COS_EPS, COS_LAMBDA = 1e-20, 5.0
RECIPE = ("color-l1cosinesim", "avg-l1", "multiscale-l1")


def _all(kind):
    return tuple("%s-%s" % (kind, c) for c in CRITERIA)


# case -> (shape, k, names, seed, black hr pixel (n, i, j) or None)
CASES = {
    "ms16": ((1, 3, 16, 16), 1, ("multiscale-l1", "multiscale-l1cosinesim"), 31, (0, 5, 9)),
    "ms40x52": ((2, 3, 40, 52), 1, _all("multiscale"), 32, None),
    "ms37x45": ((2, 3, 37, 45), 1, ("multiscale-l1", "multiscale-l2"), 33, None),
    "ms80x144": ((1, 3, 80, 144), 1, ("multiscale-l1", "multiscale-l1cosinesim"), 34, None),
    "ms_c1": ((2, 1, 24, 36), 1, ("multiscale-l1", "multiscale-l1cosinesim", "multiscale-cb"), 35, None),
    "ms_c2": ((1, 2, 16, 20), 1, ("multiscale-l1", "multiscale-l1cosinesim"), 36, None),
    "ms_c4": ((1, 4, 33, 20), 1, ("multiscale-l1", "multiscale-l1cosinesim", "multiscale-elastic"), 37, None),
    "avg_k4": ((2, 3, 10, 11), 4, _all("avg"), 41, None),
    "avg_k1": ((1, 3, 5, 7), 1, ("avg-l1", "avg-l1cosinesim"), 42, (0, 2, 3)),
    "avg_k2": ((2, 4, 9, 14), 2, ("avg-l1", "avg-l2", "avg-l1cosinesim"), 43, None),
    "avg_k3": ((1, 1, 9, 13), 3, ("avg-l1", "avg-cb"), 44, None),
    "avg_k8": ((1, 3, 24, 40), 8, ("avg-l1", "avg-elastic"), 45, None),
    "avg_k4_vec": ((1, 3, 14, 20), 4, ("avg-l1", "avg-l1cosinesim"), 46, None),
    "avg_c2": ((1, 2, 7, 10), 2, ("avg-l1", "avg-l1cosinesim"), 47, None),
    "col_k4": ((2, 3, 10, 11), 4, _all("color"), 51, None),
    "col_k1": ((1, 3, 5, 7), 1, ("color-l1cosinesim", "color-clipl1"), 52, None),
    "recipe64x48": ((2, 3, 64, 48), 4, ("color-l1cosinesim", "color-l1") + RECIPE[1:], 53, None),
}
STEP_YAML = dict(nb=1, batch=2, crop=64, d_nf=16)
STEP_SEED, STEP_K = 311, 2
STEP_WEIGHTS = {"color_weight": 1.0, "avg_weight": 5.0, "ms_weight": 1e-2}          # the shipped recipe's values
STEP_LINES = {"color_weight": "color_criterion: color-l1cosinesim", "avg_weight": "avg_criterion: avg-l1",
              "ms_weight": "ms_criterion: multiscale-l1"}
STEP_TERMS = {"color-l1cosinesim": "color_weight", "avg-l1": "avg_weight", "pix-multiscale-l1": "ms_weight"}

probe, probe_error = G.probe, G.probe_error


def kind_of(name):
    return name.split("-")[0]


def crit_of(name):
    return name.split("-")[1]


def built_name(name):
    """The name get_loss_fn returns the entry under."""
    return "pix-" + name if kind_of(name) == "multiscale" else name


def names_for(case):
    return CASES[case][2]


def make_inputs(case):
    """-> (sr, hr) fp32 NCHW."""
    shape, _, _, seed, black = CASES[case]
    return make_pair(shape, seed, black)


def make_pair(shape, seed, black=None):
    """The pair of a shape and a seed (also for shapes too large for the fixture, which the GPU tests hold against `restate` alone)."""
    hr = detrand.uniform(shape, 6000 + seed, 0.0, 1.0)
    sr = (hr.double() + detrand.uniform(shape, 6500 + seed, -0.15, 0.15).double()).float()
    if black is not None:
        hr = hr.clone()
        hr[black[0], :, black[1], black[2]] = 0.0
    return sr.contiguous(), hr.contiguous()


# ------------------------------------------------------------------------------------------------ restatement
def box(t, k):
    """k x k box means with stride k, floor mode: the trailing H % k rows and W % k columns belong to no cell."""
    N, C, H, W = t.shape
    hk, wk = H // k, W // k
    return t[..., :hk * k, :wk * k].reshape(N, C, hk, k, wk, k).mean((3, 5))


def rgb_to_uv(t):
    wr, wb = 0.299, 0.114
    wg = 1 - wr - wb
    r, g, b = t[:, 0], t[:, 1], t[:, 2]
    y = wr * r + wg * g + wb * b
    return torch.stack(((b - y) * 0.493 + 0.5, (r - y) * 0.877 + 0.5), 1)


def criterion(a, b, crit):
    d = a - b
    if crit == "l1":
        return d.abs().mean()
    if crit == "l2":
        return (d * d).mean()
    if crit == "cb":
        return torch.sqrt(d * d + 1e-6 ** 2).mean()
    if crit == "elastic":
        # ElasticLoss keeps its two factors in a FloatTensor: they are the fp32 roundings of 0.2 and 0.8 in every precision
        a0, a1 = (float(v) for v in torch.tensor([0.2, 1 - 0.2], dtype=torch.float32))
        return a0 * (d * d).mean() + a1 * d.abs().mean()
    if crit == "clipl1":
        return d.abs().clamp(0.0, 10.0).mean()
    if crit == "l1cosinesim":
        na, nb = a.norm(p=2, dim=1, keepdim=True), b.norm(p=2, dim=1, keepdim=True)
        cos = ((a / na.clamp_min(COS_EPS)) * (b / nb.clamp_min(COS_EPS))).sum(1)
        return d.abs().mean() + COS_LAMBDA * (1 - cos).mean()
    raise KeyError(crit)


def operands(sr, hr, name, k):
    """-> [(weight, cell size, a, b)] per level: the pairs the criterion sees."""
    kind = kind_of(name)
    if kind == "avg":
        return [(1.0, k, box(sr, k), box(hr, k))]
    if kind == "color":
        return [(1.0, k, rgb_to_uv(box(sr, k)), rgb_to_uv(box(hr, k)))]
    if kind == "multiscale":
        if min(sr.shape[2:]) < 16:
            raise ValueError("five levels need min(H, W) >= 16")
        return [(w, 1 << i, box(sr, 1 << i), box(hr, 1 << i)) for i, w in enumerate(MS_WEIGHTS)]
    raise KeyError(name)


def restate(sr, hr, name, k):
    """The loss FUNCTION of `name` as get_loss_fn builds it (the training term is weight * f), in the dtype of the inputs."""
    return sum(w * criterion(a, b, crit_of(name)) for w, _, a, b in operands(sr, hr, name, k))


def responses(sr, hr, name, k):
    """-> [d] per level: the differences whose sign the kinked criteria take."""
    return [a - b for _, _, a, b in operands(sr, hr, name, k)]


def restate_with_grad(sr, hr, name, k, dtype=torch.float64):
    x = sr.detach().to(dtype).contiguous().requires_grad_(True)
    v = restate(x, hr.detach().to(dtype).contiguous(), name, k)
    v.backward()
    return v.detach(), x.grad.detach()


def kept_mask(sr, hr, name, k, e32_resp):
    """-> (bool N x C x H x W: the gradient elements outside the footprint of every ambiguous cell, the share of ambiguous cells).
    A colour cell that is ambiguous in u or in v takes all three channels of its footprint with it."""
    keep = torch.ones(sr.shape, dtype=torch.bool)
    if crit_of(name) in KINK_FREE:
        return keep, 0.0
    ds = responses(sr.double(), hr.double(), name, k)
    cells = amb_cells = 0
    for (_, size, _, _), d, e in zip(operands(sr.double(), hr.double(), name, k), ds, e32_resp):
        cells += d[:, :1].numel() if kind_of(name) == "color" else d.numel()
        if size == 1:
            continue
        amb = (d.abs() > 0) & (d.abs() <= 4 * e)
        if kind_of(name) == "color":
            amb = amb.any(1, keepdim=True)
        amb_cells += int(amb.sum())
        foot = amb.repeat_interleave(size, 2).repeat_interleave(size, 3)
        if kind_of(name) == "color":
            foot = foot.expand(-1, sr.shape[1], -1, -1)
        keep[..., :foot.shape[2], :foot.shape[3]] &= ~foot
    return keep, amb_cells / cells


# ------------------------------------------------------------------------------------------------ the reference
def _reference_modules():
    with R.reference_env():
        for m in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data", "cv2", "torchvision")]:
            del sys.modules[m]
        import models.losses as L
        import dataops.colors as colors
    return L, colors


def reference_fn(L, name, k):
    with R.reference_env():
        built = L.get_loss_fn(name, 1, device="cpu", opt={"scale": k})
    assert built["name"] == built_name(name), (built["name"], name)
    return built["function"]


def reference_run(fn, sr, hr, dtype):
    x = sr.detach().to(dtype).contiguous().requires_grad_(True)
    v = fn(x, hr.detach().to(dtype).contiguous())
    v.backward()
    return v.detach(), x.grad.detach()


def reference_responses(fn, colors, name, sr, hr, dtype):
    x, y = sr.detach().to(dtype), hr.detach().to(dtype)
    kind = kind_of(name)
    with torch.no_grad():
        if kind == "avg":
            return [fn.ds_f(x) - fn.ds_f(y)]
        if kind == "color":
            return [colors.rgb_to_yuv(fn.ds_f(x), consts="uv") - colors.rgb_to_yuv(fn.ds_f(y), consts="uv")]
        out = []
        for i in range(len(fn.weights)):
            out.append(x - y)
            if i != len(fn.weights) - 1:
                x, y = fn.downsample(x), fn.downsample(y)
        return out


def loss_cases(L, colors):
    cases = {}
    for case, (shape, k, names, _, black) in CASES.items():
        sr, hr = make_inputs(case)
        assert (sr < 0).any() and (sr > 1).any() and sr.min() > -0.2 and sr.max() < 1.2
        assert sr.abs().sum(1).min() > 0, "a zero pixel in sr"
        if black is not None:
            assert hr[black[0], :, black[1], black[2]].abs().max() == 0
        rec = {"shape": tuple(shape), "k": k, "sr": probe(sr), "hr": probe(hr), "names": {}}
        for name in names:
            fn = reference_fn(L, name, k)
            v64, g64 = reference_run(fn, sr, hr, torch.float64)
            v32, g32 = reference_run(fn, sr, hr, torch.float32)
            d64 = reference_responses(fn, colors, name, sr, hr, torch.float64)
            d32 = reference_responses(fn, colors, name, sr, hr, torch.float32)
            rv, rg = restate_with_grad(sr, hr, name, k)
            gmax = g64.abs().max().item()
            assert torch.isfinite(g64).all() and torch.isfinite(g32).all(), (case, name)
            assert abs(rv.item() - v64.item()) <= 1e-12 * max(1.0, abs(v64.item())), (case, name, rv.item(), v64.item())
            assert (rg - g64).abs().max().item() <= 1e-12 * max(1.0, gmax), (case, name, (rg - g64).abs().max().item(), gmax)
            for a, b in zip(responses(sr.double(), hr.double(), name, k), d64):
                assert a.shape == b.shape and (a - b).abs().max().item() <= 1e-12, (case, name)
            e32_resp = [(a.double() - b).abs().max().item() for a, b in zip(d32, d64)]
            keep, share = kept_mask(sr, hr, name, k, e32_resp)
            assert share <= 0.01, (case, name, share)
            t = {"value": v64.item(), "e32_val": abs(v32.double().item() - v64.item()), "grad": probe(g64), "grad_absmax": gmax,
                 "e32_grad": (g32.double() - g64)[keep].abs().max().item(), "e32_resp": e32_resp, "ambiguous": share}
            if black is not None and crit_of(name) == "l1cosinesim":
                t["black_grad_absmax"] = g64[black[0], :, black[1], black[2]].abs().max().item()
            rec["names"][name] = t
            print("%-12s %-24s value %.9e e32_val %.2e e32_grad %.2e of max|g| %.2e e32_resp %.1e ambiguous %.4f" % (
                case, name, t["value"], t["e32_val"], t["e32_grad"], gmax, max(e32_resp), share))
        cases[case] = rec
    return cases


# ------------------------------------------------------------------------------------------------ step record
def losses_yaml(path, weights):
    """Add the recipe's loss lines of `weights` ({'color_weight': w, ...}) to the train block of a yaml written by
    oracle.ref_harness.esrgan_yaml."""
    with open(path) as fh:
        txt = fh.read()
    assert txt.count("\nlogger:") == 1
    lines = "".join("\n  %s\n  %s: %g" % (STEP_LINES[k], k, w) for k, w in weights.items())
    with open(path, "w") as fh:
        fh.write(txt.replace("\nlogger:", lines + "\nlogger:"))
    return path


def step_record():
    from oracle.make_golden import D_SEED, F_SEED, G_SEED, probe_state
    from oracle.make_golden import probe as state_probe
    yml = losses_yaml(R.esrgan_yaml(name="golden_pooled_step", **STEP_YAML), STEP_WEIGHTS)
    opt, model = R.build_reference_model(yml, seed=0)
    detrand.fill_state_dict_(model.netG.state_dict(), G_SEED)
    detrand.fill_state_dict_(model.netD.state_dict(), D_SEED)
    netF = R.reference_netF(model)
    detrand.fill_state_dict_({k: v for k, v in netF.state_dict().items() if k.startswith("feature_net")}, F_SEED, gain=1.0, bias_amp=0.05)
    assert [l["name"] for l in model.generatorlosses.loss_list] == ["pix-l1", "fea-vgg19-l1"] + list(STEP_TERMS)
    assert model.generatorlosses.precise_loss_list == []
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
        for n in STEP_TERMS:
            assert logs[-1][n] > 0, (n, logs[-1])
    print("step weights", STEP_WEIGHTS, [{k: round(v, 6) for k, v in l.items()} for l in logs])
    return {"name": "pooled_step", "spec": {"yaml": dict(STEP_YAML), "steps": STEP_K, "seed": STEP_SEED}, "weights": dict(STEP_WEIGHTS),
            "network_G": dict(opt["network_G"]), "network_D": dict(opt["network_D"]),
            "seeds": {"G": G_SEED, "D": D_SEED, "F": F_SEED, "data": STEP_SEED},
            "logs": logs, "fake_H": model.fake_H.detach().clone(), "grads_step1": grads,
            "g_state": probe_state(model.netG.state_dict()), "d_state": probe_state(model.netD.state_dict()),
            "g_keys": [(k, tuple(v.shape)) for k, v in model.netG.state_dict().items()],
            "d_keys": [(k, tuple(v.shape)) for k, v in model.netD.state_dict().items()], "torch": torch.__version__}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    L, colors = _reference_modules()
    cases = loss_cases(L, colors)
    fx = {"cases": cases, "steps": {"recipe": step_record()}, "torch": torch.__version__}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(fx, OUT)
    print("->", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
