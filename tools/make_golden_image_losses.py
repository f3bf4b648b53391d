"""tests/golden/image_losses.pt from the REFERENCE's own loss builder (codes/models/losses.py get_loss_fn -> modules/loss.py HFENLoss,
GradientLoss, TVLoss and the difference-only pixel criteria) and, for the step-level record, its own SRModel -- run on the CPU where
the reference tree exists (never on a GPU machine):

    python tools/make_golden_image_losses.py

Cases are the (sr, hr) pairs of tools/make_golden_ssim.py's `make_inputs` (rebuilt from seeds): 72 x 72, 99 x 117, 136 x 136 with 3
channels, and a 1-channel 72 x 72 pair for the pix / grad / tv names only (the reference's HFEN filter is fixed at 3 channels).  Per
case and loss name the fixture holds the reference's fp64 value, probes of its fp64 gradient and the reference's OWN fp32 deviations
from its fp64 run, the yardsticks of the GPU tests:

    e32_val, e32_grad     |v32 - v64|, max |g32 - g64|
    e32_resp              max |e32 - e64| of the response map e (HFEN: L * x - L * y; grad: dir(x) - dir(y) over the directions)
    near_share            share of responses with |e64| <= 4 e32_resp (HFEN, kinked criteria; asserted <= 1e-3)
    e32_map               max |rho'(e32) - rho'(e64)| over the responses with |e64| > 4 e32_resp (HFEN)
    e32_adj, e32_adj_rand max |A32 m - A64 m| of the adjoint stencil A applied to m = rho'(e64) rounded to fp32 / to a seeded random
                          map in [-1, 1) (HFEN)
    excluded_share        share of gradient pixels within the 3 x 3 reach of a response with 0 < |e64| <= 4 e32_resp (grad, l1 / cb;
                          asserted <= 1e-3)

`restate` below is an fp64 restatement of all the losses in plain torch, written from their formulas; the tool asserts
restate == reference to 1e-12 (value and every gradient element) before it writes the file, so the tests can compare the engine
with `restate`'s full gradient on machines where the reference does not exist.

Step record: the reference's SRModel (the harness's small ESRGAN config) with hfen-l1, grad-4d-l1 and tv-l1 switched on, two steps.
The weights are powers of ten chosen from a first pass with weight 1 so that, in the reference's own log, every new term lies
between 0.1 x and 10 x the pix-l1 entry (asserted).
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

OUT = os.path.join(ROOT, "tests", "golden", "image_losses.pt")
NAMES = ("pix-l2", "pix-cb", "pix-elastic", "pix-clipl1", "hfen-l1", "hfen-l2", "hfen-cb", "hfen-elastic",
         "grad-2d-l1", "grad-4d-l1", "grad-4d-cb", "tv-l1", "tv-l2", "dtv-l1", "dtv-l2")
CASES = ("sq72", "odd99x117", "sq136", "gray72")
KINKED = ("l1", "cb", "elastic")
NEAR_CAP = 1e-3
STEP_YAML = dict(nb=1, batch=2, crop=64, d_nf=16)
STEP_SEED, STEP_K = 271, 2
STEP_TERMS = {"hfen-l1": ("hfen_criterion: l1", "hfen_weight"), "grad-4d-l1": ("grad_type: grad-4d-l1", "grad_weight"),
              "tv-l1": ("tv_type: normal\n  tv_norm: 1", "tv_weight")}

make_inputs, probe, probe_error = G.make_inputs, G.probe, G.probe_error


def names_for(case):
    return tuple(n for n in NAMES if not (case == "gray72" and n.startswith("hfen")))


def builder_type(name):
    """The loss type get_loss_fn is called with for the loss it then NAMES `name` (pixel criteria gain their 'pix-' there)."""
    return name[4:] if name.startswith("pix-") else name


# ------------------------------------------------------------------------------------------------ restatement
def log_taps():
    """The 15 x 15 LoG taps, sigma 2.5, in fp32: g(u) g(v) (u^2 + v^2 - 2 sigma^2) / (2 pi sigma^4) on the grid -7 .. 7, then
    -k / sum(k)."""
    from trainner_amd.models.modules.image_losses import log_kernel_taps
    return log_kernel_taps(15, 2.5)


def rho(e, crit):
    if crit == "l1":
        return e.abs()
    if crit == "l2":
        return e * e
    if crit == "cb":
        return torch.sqrt(e * e + 1e-6 ** 2)
    if crit == "elastic":
        a = torch.tensor([0.2, 1 - 0.2], dtype=torch.float32).to(e.dtype)       # the weights are fp32 numbers
        return (e * e) * a[0] + e.abs() * a[1]
    if crit == "clipl1":
        return e.abs().clamp(0.0, 10.0)
    raise KeyError(crit)


def drho(e, crit):
    """rho'(e) as autograd gives it."""
    e = e.detach().clone().requires_grad_(True)
    rho(e, crit).sum().backward()
    return e.grad


def hfen_response(x, y, taps):
    w = taps.to(x.dtype).expand(x.shape[1], 1, 15, 15)
    return F.conv2d(x - y, w, padding=7, groups=x.shape[1])


def fd_responses(t, four):
    """dx, dy[, dp, dn] with the reference's borders: dx is 0 in the last column, dy and dp in the last row, dn is botright - t with
    zeros beyond the image, dp = right - bottom with a zero `right` in the last column."""
    z = F.pad(t, (0, 1, 0, 1))
    H, W = t.shape[-2:]
    right, bottom, botright = z[..., :H, 1:], z[..., 1:, :W], z[..., 1:, 1:]
    colmask = torch.ones(W, dtype=t.dtype)
    colmask[-1] = 0
    rowmask = torch.ones(H, 1, dtype=t.dtype)
    rowmask[-1] = 0
    out = [(right - t) * colmask, (bottom - t) * rowmask]
    if four:
        out += [(right - bottom) * rowmask, botright - t]
    return out


def restate(sr, hr, name):
    """The loss FUNCTION of `name` as get_loss_fn builds it (the training term is weight * f), in the dtype of the inputs."""
    parts = name.split("-")
    if parts[0] == "pix":
        return rho(sr - hr, parts[1]).mean()
    if parts[0] == "hfen":
        r = rho(hfen_response(sr, hr, log_taps()), parts[1])
        return r.mean() if parts[1] in ("cb", "clipl1") else r.sum()
    if parts[0] == "grad":
        four = parts[1] == "4d"
        terms = [rho(a - b, parts[2]).mean() for a, b in zip(fd_responses(sr, four), fd_responses(hr, four))]
        return sum(terms) / len(terms)
    if parts[0] in ("tv", "dtv"):
        per_image = sum(rho(g, parts[1]).mean((1, 2, 3)) for g in fd_responses(sr, parts[0] == "dtv"))
        return per_image.sum() / sr.shape[0]
    raise KeyError(name)


def restate_with_grad(sr, hr, name, dtype=torch.float64):
    x = sr.detach().to(dtype).contiguous().requires_grad_(True)
    v = restate(x, hr.detach().to(dtype).contiguous(), name)
    v.backward()
    return v.detach(), x.grad.detach()


def adjoint(m, taps):
    """A m: the adjoint of the zero-padded correlation with `taps`, in m's dtype."""
    w = taps.to(m.dtype).expand(m.shape[1], 1, 15, 15)
    return F.conv_transpose2d(m, w, padding=7, groups=m.shape[1])


def random_map(shape, seed=4242):
    n = 1
    for s in shape:
        n *= s
    return (detrand.uniform01(n, seed).double().reshape(shape) * 2 - 1).float()


def reach3x3(mask):
    """Pixels whose 3 x 3 neighbourhood holds a marked response (any channel keeps to itself)."""
    return F.max_pool2d(mask.double(), 3, stride=1, padding=1) > 0


# ------------------------------------------------------------------------------------------------ the reference
def _reference_modules():
    with R.reference_env():
        for m in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data", "cv2", "torchvision")]:
            del sys.modules[m]
        import models.losses as L
        import dataops.filters as FL
    return L, FL


def reference_run(L, name, sr, hr, dtype):
    with R.reference_env():
        built = L.get_loss_fn(builder_type(name), 1, device="cpu")
    assert built["name"] == name, (built["name"], name)
    fn = built["function"].to(dtype)
    x = sr.detach().to(dtype).contiguous().requires_grad_(True)
    y = hr.detach().to(dtype).contiguous()
    v = fn(x) if "tv" in name else fn(x, y)
    v.backward()
    return v.detach(), x.grad.detach(), fn


def reference_responses(FL, fn, name, sr, hr, dtype):
    """The response map(s) e the criterion sees, from the reference's own filter / finite differences."""
    x, y = sr.detach().to(dtype).contiguous(), hr.detach().to(dtype).contiguous()
    with torch.no_grad():
        if name.startswith("hfen"):
            return [fn.filter(x) - fn.filter(y)]
        get = FL.get_4dim_image_gradients if "4d" in name else FL.get_image_gradients
        return [a - b for a, b in zip(get(x), get(y))]


def loss_cases(L, FL):
    taps = log_taps()
    ref_taps = None
    cases = {}
    for case in CASES:
        sr, hr = make_inputs(case)
        rec = {"shape": tuple(sr.shape), "sr": probe(sr), "hr": probe(hr), "names": {}}
        for name in names_for(case):
            v64, g64, fn64 = reference_run(L, name, sr, hr, torch.float64)
            v32, g32, fn32 = reference_run(L, name, sr, hr, torch.float32)
            rv, rg = restate_with_grad(sr, hr, name)
            assert abs(rv.item() - v64.item()) <= 1e-12 * max(1.0, abs(v64.item())), (case, name, rv.item(), v64.item())
            assert (rg - g64).abs().max().item() <= 1e-12 * max(1.0, g64.abs().max().item()), (case, name, (rg - g64).abs().max().item())
            t = {"value": v64.item(), "e32_val": abs(v32.double().item() - v64.item()), "grad": probe(g64),
                 "grad_absmax": g64.abs().max().item(), "e32_grad": (g32.double() - g64).abs().max().item()}
            crit = name.split("-")[-1]
            if name.startswith("hfen"):
                ref_taps = fn32.filter.weight.data[0, 0].detach().clone()      # the fixture stores the REFERENCE's own tensor
                assert all(torch.equal(fn32.filter.weight.data[c, 0], ref_taps) for c in range(3))
                assert torch.equal(ref_taps, taps), "the engine's LoG taps are not the reference's"
                e64 = reference_responses(FL, fn64, name, sr, hr, torch.float64)[0]
                e32 = reference_responses(FL, fn32, name, sr, hr, torch.float32)[0]
                t["e32_resp"] = (e32.double() - e64).abs().max().item()
                far = e64.abs() > 4 * t["e32_resp"]
                t["near_share"] = 1.0 - far.double().mean().item()
                t["resp_std"] = e64.std().item()
                m64 = drho(e64, crit)
                t["e32_map"] = (drho(e32, crit).double() - m64)[far].abs().max().item()
                for key, m in (("e32_adj", m64.float()), ("e32_adj_rand", random_map(e64.shape))):
                    t[key] = (adjoint(m, taps).double() - adjoint(m.double(), taps)).abs().max().item()
                if crit in KINKED:
                    assert t["near_share"] <= NEAR_CAP, (case, name, t["near_share"])
            if name.startswith("grad"):
                e64s = reference_responses(FL, fn64, name, sr, hr, torch.float64)
                e32s = reference_responses(FL, fn32, name, sr, hr, torch.float32)
                t["e32_resp"] = max((a.double() - b).abs().max().item() for a, b in zip(e32s, e64s))
                t["excluded_share"] = near_zero_mask(sr, hr, name, t["e32_resp"]).double().mean().item()
                if crit in KINKED:
                    assert t["excluded_share"] <= NEAR_CAP, (case, name, t["excluded_share"])
            rec["names"][name] = t
            print("%-10s %-13s value %.9e e32_val %.2e e32_grad %.2e of max|g| %.2e" % (case, name, t["value"], t["e32_val"], t["e32_grad"],
                                                                                     t["grad_absmax"]),
                  " ".join("%s %.2e" % (k, t[k]) for k in ("e32_resp", "near_share", "e32_map", "e32_adj", "e32_adj_rand", "excluded_share")
                           if k in t))
        cases[case] = rec
    return cases, ref_taps


def near_zero_mask(sr, hr, name, e32_resp):
    """The tests' exclusion rule for the kinked gradient-loss cases, from the fp64 restatement: gradient pixels within the 3 x 3 reach
    of a response with 0 < |e64| <= 4 e32_resp.  A response that is exactly 0 in fp64 (the zeroed borders; neighbours that both
    images clamp to the same bound) is the difference of two EQUAL exact differences of fp32 numbers, so it is exactly 0 in fp32 as
    well (rounding maps equal numbers to equal numbers): its sign is exact in every precision and it excludes nothing."""
    x, y = sr.double(), hr.double()
    four = "4d" in name
    near = torch.zeros_like(x, dtype=torch.bool)
    for a, b in zip(fd_responses(x, four), fd_responses(y, four)):
        e = a - b
        near |= (e.abs() <= 4 * e32_resp) & (e != 0)
    return reach3x3(near)


# ------------------------------------------------------------------------------------------------ step records
def losses_yaml(path, weights):
    """Add the loss lines of `weights` ({name: weight}) to the train block of a yaml written by oracle.ref_harness.esrgan_yaml."""
    with open(path) as fh:
        txt = fh.read()
    assert txt.count("\nlogger:") == 1
    lines = "".join("\n  %s\n  %s: %g" % (STEP_TERMS[n][0], STEP_TERMS[n][1], w) for n, w in weights.items())
    with open(path, "w") as fh:
        fh.write(txt.replace("\nlogger:", lines + "\nlogger:"))
    return path


def _reference_model(tag, weights):
    from oracle.make_golden import D_SEED, F_SEED, G_SEED
    yml = losses_yaml(R.esrgan_yaml(name="golden_imgloss_" + tag, **STEP_YAML), weights)
    opt, model = R.build_reference_model(yml, seed=0)
    detrand.fill_state_dict_(model.netG.state_dict(), G_SEED)
    detrand.fill_state_dict_(model.netD.state_dict(), D_SEED)
    netF = R.reference_netF(model)
    detrand.fill_state_dict_({k: v for k, v in netF.state_dict().items() if k.startswith("feature_net")}, F_SEED, gain=1.0, bias_amp=0.05)
    return opt, model


def step_record():
    from oracle.make_golden import D_SEED, F_SEED, G_SEED, probe_state
    from oracle.make_golden import probe as state_probe
    # first pass, weight 1: the terms' sizes next to pix-l1 in the reference's own log -> powers of ten
    _, model = _reference_model("pass1", {n: 1.0 for n in STEP_TERMS})
    LR, HR = detrand.synthetic_pair(STEP_YAML["batch"], STEP_YAML["crop"], STEP_SEED + 1)
    log = R.reference_step(model, LR, HR, 1)
    weights = {n: 10.0 ** round(math.log10(log["pix-l1"] / log[n])) for n in STEP_TERMS}
    opt, model = _reference_model("step", weights)
    assert [l["name"] for l in model.generatorlosses.loss_list] == ["pix-l1", "hfen-l1", "tv-l1", "fea-vgg19-l1"]
    assert [l["name"] for l in model.generatorlosses.precise_loss_list] == ["grad-4d-l1"]
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
            assert 0.1 <= logs[-1][n] / logs[-1]["pix-l1"] <= 10.0, (n, logs[-1][n], logs[-1]["pix-l1"])
    print("step weights", weights, [{k: round(v, 6) for k, v in l.items()} for l in logs])
    return {"name": "image_losses_step", "spec": {"yaml": dict(STEP_YAML), "steps": STEP_K, "seed": STEP_SEED}, "weights": weights,
            "network_G": dict(opt["network_G"]), "network_D": dict(opt["network_D"]),
            "seeds": {"G": G_SEED, "D": D_SEED, "F": F_SEED, "data": STEP_SEED},
            "logs": logs, "fake_H": model.fake_H.detach().clone(), "grads_step1": grads,
            "g_state": probe_state(model.netG.state_dict()), "d_state": probe_state(model.netD.state_dict()),
            "g_keys": [(k, tuple(v.shape)) for k, v in model.netG.state_dict().items()],
            "d_keys": [(k, tuple(v.shape)) for k, v in model.netD.state_dict().items()], "torch": torch.__version__}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    L, FL = _reference_modules()
    cases, taps = loss_cases(L, FL)
    fx = {"cases": cases, "log_taps": taps.clone(), "steps": {"recipe_terms": step_record()}, "torch": torch.__version__}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(fx, OUT)
    print("->", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
