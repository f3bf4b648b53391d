"""tests/golden/spl.pt from the REFERENCE's own loss builder (codes/models/losses.py get_loss_fn -> modules/loss.py CPLoss, GPLoss over
SPLoss, and OFLoss) and, for the step-level record, its own SRModel -- run on the CPU where the reference tree exists (never on a GPU
machine):

    python tools/make_golden_spl.py

Cases (the (sr, hr) pairs of tools/make_golden_ssim.py's `make_inputs`, rebuilt from seeds, and three edits of them):

    sq72, odd99x117, sq136   3 channels: cpl, gpl, overflow
    gray72                   1 channel: gpl, overflow (the YUV traces of cpl need 3 channels)
    znorm99x117              the odd99x117 pair mapped by v -> 2.4 v - 1.2 (hr into [-1.2, 1.2]), built with datasets.train.znorm: true,
                             so cpl and gpl denorm on load; values fall below -1, inside and above 1 (asserted)
    blackrow72               sq72 with row 31 of sr set to exactly 0 in all channels: the eps branch of F.normalize for the RGB and Y rows
                             and for the rows of dx; the reference's fp64 gradient on that row exceeds 1e9 (asserted); cpl, gpl
    overflow99x117           sr of odd99x117 mapped by v -> 1.5 v - 0.25: at least 10 % of the elements below 0, above 1 and inside
                             (asserted); overflow only

Per case and name the fixture holds the reference's fp64 value, probes of its fp64 gradient, max |gradient| and the reference's OWN
fp32 deviations from its fp64 run (e32_val, e32_grad), the yardsticks of the GPU tests.  For blackrow72 it also holds black_rel32: the
largest deviation of the reference's fp32 gradient on the black row from the eps-branch term alone (`restate(..., eps_only=True)`:
the sum over the zero-norm lines of x . y^ / eps, whose gradient is y^ / eps times the scale, pushed through the adjoints), relative to
that term's largest magnitude on the row.

`restate` below is an fp64 restatement of the three losses in plain torch, written from their formulas; the tool asserts
restate == reference to 1e-12 (value and every gradient element, relative to max |gradient|) before it writes the file, so the tests
can compare the engine with `restate`'s full gradient on machines where the reference does not exist.

Step record: the reference's SRModel (the harness's small ESRGAN config) with spl_type: spl and of_type: overflow, two steps.  The two
weights are powers of ten chosen from a first pass with weight 1 so that, in the reference's own log, |cpl| and overflow lie between
0.1 x and 10 x the pix-l1 entry (asserted; the cpl entry is negative: SPLoss is minus a sum of cosines).  gpl shares spl_weight with
cpl and cannot be held to the same window: with this untrained generator the cosines between the finite differences of its output
and of HR nearly cancel, so |gpl| stays below 0.02 |cpl| and changes sign from step to step (ten data seeds were tried: |gpl| <= 0.14
against |cpl| >= 7.1 at weight 1), while its gradient is of the size of cpl's.  For gpl the tool asserts the upper end only
(|gpl| <= 10 x pix-l1).  A consequence for the step test: its log check compares gpl entries of order 5e-5 under an absolute floor of
5e-6 plus 2e-4 relative to max(1, |v|), which constrains almost nothing; in this record gpl is held through what its gradient does to
the generator (the recorded gradients, fake_H and G's state after two steps), and its value through the loss-level cases above.  The
overflow entry is > 0 (asserted): the generator's output leaves [0, 1].
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
from tools import make_golden_ssim as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "spl.pt")
NAMES = ("cpl", "gpl", "overflow")
CASES = ("sq72", "odd99x117", "sq136", "gray72", "znorm99x117", "blackrow72", "overflow99x117")
BLACK_ROW = 31
EPS = 1e-12
STEP_YAML = dict(nb=1, batch=2, crop=64, d_nf=16)
STEP_SEED, STEP_K = 283, 2
STEP_LINES = {"spl_weight": "spl_type: spl", "of_weight": "of_type: overflow"}
STEP_TERMS = {"cpl": "spl_weight", "gpl": "spl_weight", "overflow": "of_weight"}

probe, probe_error = G.probe, G.probe_error


def names_for(case):
    if case == "gray72":
        return ("gpl", "overflow")
    if case == "blackrow72":
        return ("cpl", "gpl")
    if case == "overflow99x117":
        return ("overflow",)
    return NAMES


def znorm_of(case):
    return case == "znorm99x117"


def make_inputs(case):
    """-> (sr, hr) fp32 NCHW."""
    if case == "znorm99x117":
        sr, hr = G.make_inputs("odd99x117")
        return (sr.double() * 2.4 - 1.2).float(), (hr.double() * 2.4 - 1.2).float()
    if case == "blackrow72":
        sr, hr = G.make_inputs("sq72")
        sr = sr.clone()
        sr[:, :, BLACK_ROW, :] = 0.0
        return sr, hr
    if case == "overflow99x117":
        sr, hr = G.make_inputs("odd99x117")
        return (sr.double() * 1.5 - 0.25).float(), hr
    return G.make_inputs(case)


# ------------------------------------------------------------------------------------------------ restatement
def denorm(t):
    return ((t + 1.0) / 2.0).clamp(0, 1)


def rgb_to_yuv(t):
    wr, wb = 0.299, 0.114
    wg = 1 - wr - wb
    r, g, b = t[:, 0], t[:, 1], t[:, 2]
    y = wr * r + wg * g + wb * b
    return torch.stack((y, (b - y) * 0.493 + 0.5, (r - y) * 0.877 + 0.5), 1)


def differences(t):
    """dx = right - t (0 in the last column), dy = bottom - t (0 in the last row); no gradient flows through the zeroed entries."""
    H, W = t.shape[-2:]
    z = F.pad(t, (0, 1, 0, 1))
    colmask = torch.ones(W, dtype=t.dtype, device=t.device)
    colmask[-1] = 0
    rowmask = torch.ones(H, 1, dtype=t.dtype, device=t.device)
    rowmask[-1] = 0
    return (z[..., :H, 1:] - t) * colmask, (z[..., 1:, :W] - t) * rowmask


def cosines(x, y, dim, eps_only=False):
    """The sum over the lines along `dim` of x / max(|x|, eps) . y / max(|y|, eps); eps_only: the lines with |x| < eps alone."""
    nx, ny = x.norm(p=2, dim=dim, keepdim=True), y.norm(p=2, dim=dim, keepdim=True)
    terms = (x / nx.clamp_min(EPS)) * (y / ny.clamp_min(EPS))
    if eps_only:
        terms = terms * (nx < EPS).to(x.dtype)
    return terms.sum()


def spl_trace(x, y, eps_only=False):
    return -(cosines(x, y, 2, eps_only) + cosines(x, y, 3, eps_only)) / (x.shape[2] * x.shape[0])


def restate(sr, hr, name, znorm=False, eps_only=False):
    """The loss FUNCTION of `name` as get_loss_fn builds it (the training term is weight * f), in the dtype of the inputs."""
    if name == "overflow":
        return torch.log((sr - sr.clamp(0, 1)).abs() + 1).sum() / sr.numel()
    x, y = (denorm(sr), denorm(hr)) if znorm else (sr, hr)
    if name == "gpl":
        (xh, xv), (yh, yv) = differences(x), differences(y)
        return spl_trace(xv, yv, eps_only) + spl_trace(xh, yh, eps_only)
    if name == "cpl":
        xu, yu = rgb_to_yuv(x), rgb_to_yuv(y)
        (xh, xv), (yh, yv) = differences(xu), differences(yu)
        return spl_trace(x, y, eps_only) + spl_trace(xu, yu, eps_only) + spl_trace(xv, yv, eps_only) + spl_trace(xh, yh, eps_only)
    raise KeyError(name)


def restate_with_grad(sr, hr, name, znorm=False, dtype=torch.float64, eps_only=False):
    x = sr.detach().to(dtype).contiguous().requires_grad_(True)
    v = restate(x, hr.detach().to(dtype).contiguous(), name, znorm, eps_only)
    v.backward()
    return v.detach(), x.grad.detach()


# ------------------------------------------------------------------------------------------------ the reference
def _reference_modules():
    with R.reference_env():
        for m in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data", "cv2", "torchvision")]:
            del sys.modules[m]
        import models.losses as L
    return L


def reference_run(L, name, sr, hr, dtype, znorm):
    with R.reference_env():
        built = L.get_loss_fn(name, 1, device="cpu", opt={"datasets": {"train": {"znorm": znorm}}})
    assert built["name"] == name, (built["name"], name)
    fn = built["function"]
    x = sr.detach().to(dtype).contiguous().requires_grad_(True)
    y = hr.detach().to(dtype).contiguous()
    v = fn(x) if name == "overflow" else fn(x, y)
    v.backward()
    return v.detach(), x.grad.detach()


def loss_cases(L):
    cases = {}
    for case in CASES:
        sr, hr = make_inputs(case)
        zn = znorm_of(case)
        rec = {"shape": tuple(sr.shape), "znorm": zn, "sr": probe(sr), "hr": probe(hr), "names": {}}
        if case == "znorm99x117":
            for t in (sr, hr):
                assert (t < -1).any() and (t > 1).any() and ((t > -1) & (t < 1)).any()
        if case == "overflow99x117":
            shares = ((sr < 0).double().mean().item(), (sr > 1).double().mean().item(), ((sr >= 0) & (sr <= 1)).double().mean().item())
            assert min(shares) >= 0.10, shares
            rec["shares"] = shares
        for name in names_for(case):
            v64, g64 = reference_run(L, name, sr, hr, torch.float64, zn)
            v32, g32 = reference_run(L, name, sr, hr, torch.float32, zn)
            rv, rg = restate_with_grad(sr, hr, name, zn)
            gmax = g64.abs().max().item()
            assert abs(rv.item() - v64.item()) <= 1e-12 * max(1.0, abs(v64.item())), (case, name, rv.item(), v64.item())
            assert (rg - g64).abs().max().item() <= 1e-12 * max(1.0, gmax), (case, name, (rg - g64).abs().max().item(), gmax)
            t = {"value": v64.item(), "e32_val": abs(v32.double().item() - v64.item()), "grad": probe(g64), "grad_absmax": gmax,
                 "e32_grad": (g32.double() - g64).abs().max().item()}
            if case == "blackrow72":
                row64 = g64[:, :, BLACK_ROW, :]
                assert row64.abs().max().item() > 1e9, (name, row64.abs().max().item())
                _, ge = restate_with_grad(sr, hr, name, zn, eps_only=True)
                want = ge[:, :, BLACK_ROW, :]
                t["black_absmax"] = want.abs().max().item()
                t["black_rel32"] = (g32.double()[:, :, BLACK_ROW, :] - want).abs().max().item() / t["black_absmax"]
                t["black_rel64"] = (row64 - want).abs().max().item() / t["black_absmax"]
                assert t["black_rel64"] <= 1e-3 * t["black_rel32"], (t["black_rel64"], t["black_rel32"])
            rec["names"][name] = t
            print("%-14s %-8s value %.9e e32_val %.2e e32_grad %.2e of max|g| %.2e" % (case, name, t["value"], t["e32_val"], t["e32_grad"],
                                                                                    gmax),
                  " ".join("%s %.2e" % (k, t[k]) for k in ("black_absmax", "black_rel32", "black_rel64") if k in t))
        cases[case] = rec
    return cases


# ------------------------------------------------------------------------------------------------ step records
def losses_yaml(path, weights):
    """Add the loss lines of `weights` ({'spl_weight': w, 'of_weight': w}) to the train block of a yaml written by
    oracle.ref_harness.esrgan_yaml; `extra` lines (e.g. 'fs: true') go with them."""
    with open(path) as fh:
        txt = fh.read()
    assert txt.count("\nlogger:") == 1
    lines = "".join("\n  %s\n  %s: %g" % (STEP_LINES[k], k, w) for k, w in weights.items())
    with open(path, "w") as fh:
        fh.write(txt.replace("\nlogger:", lines + "\nlogger:"))
    return path


def _reference_model(tag, weights):
    from oracle.make_golden import D_SEED, F_SEED, G_SEED
    yml = losses_yaml(R.esrgan_yaml(name="golden_spl_" + tag, **STEP_YAML), weights)
    opt, model = R.build_reference_model(yml, seed=0)
    detrand.fill_state_dict_(model.netG.state_dict(), G_SEED)
    detrand.fill_state_dict_(model.netD.state_dict(), D_SEED)
    netF = R.reference_netF(model)
    detrand.fill_state_dict_({k: v for k, v in netF.state_dict().items() if k.startswith("feature_net")}, F_SEED, gain=1.0, bias_amp=0.05)
    return opt, model


def step_record():
    from oracle.make_golden import D_SEED, F_SEED, G_SEED, probe_state
    from oracle.make_golden import probe as state_probe
    # first pass, weight 1: the terms' sizes next to pix-l1 in the reference's own log -> powers of ten (spl_weight from cpl: see the
    # module docstring for gpl)
    _, model = _reference_model("pass1", {k: 1.0 for k in STEP_LINES})
    LR, HR = detrand.synthetic_pair(STEP_YAML["batch"], STEP_YAML["crop"], STEP_SEED + 1)
    log = R.reference_step(model, LR, HR, 1)
    ratio = {n: math.log10(log["pix-l1"] / abs(log[n])) for n in ("cpl", "overflow")}
    weights = {"spl_weight": 10.0 ** round(ratio["cpl"]), "of_weight": 10.0 ** round(ratio["overflow"])}
    opt, model = _reference_model("step", weights)
    assert [l["name"] for l in model.generatorlosses.loss_list] == ["pix-l1", "fea-vgg19-l1", "cpl", "gpl", "overflow"]
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
        assert logs[-1]["overflow"] > 0, logs[-1]
        # gpl: the upper end only (module docstring).  At |gpl| ~ 5e-5 the step test's log check says little about it; its gradient
        # is checked through grads_step1, fake_H and g_state below
        for n in STEP_TERMS:
            assert (0.0 if n == "gpl" else 0.1) <= abs(logs[-1][n]) / logs[-1]["pix-l1"] <= 10.0, (n, logs[-1][n], logs[-1]["pix-l1"])
    print("step weights", weights, [{k: round(v, 6) for k, v in l.items()} for l in logs])
    return {"name": "spl_step", "spec": {"yaml": dict(STEP_YAML), "steps": STEP_K, "seed": STEP_SEED}, "weights": weights,
            "network_G": dict(opt["network_G"]), "network_D": dict(opt["network_D"]),
            "seeds": {"G": G_SEED, "D": D_SEED, "F": F_SEED, "data": STEP_SEED},
            "logs": logs, "fake_H": model.fake_H.detach().clone(), "grads_step1": grads,
            "g_state": probe_state(model.netG.state_dict()), "d_state": probe_state(model.netD.state_dict()),
            "g_keys": [(k, tuple(v.shape)) for k, v in model.netG.state_dict().items()],
            "d_keys": [(k, tuple(v.shape)) for k, v in model.netD.state_dict().items()], "torch": torch.__version__}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    L = _reference_modules()
    cases = loss_cases(L)
    fx = {"cases": cases, "steps": {"spl_overflow": step_record()}, "torch": torch.__version__}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(fx, OUT)
    print("->", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
