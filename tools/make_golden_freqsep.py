"""tests/golden/freqsep.pt from the REFERENCE's own frequency-separation filters (codes/dataops/filters.py FilterLow, FilterHigh) and,
for the step-level records, its own SRModel / Pix2PixModel with `fs: true` -- run on the CPU where the reference tree exists (never on
a GPU machine):

    python tools/make_golden_freqsep.py

(a) Filter cases.  Inputs are the `sr` images of tools/make_golden_ssim.py's `make_inputs` (rebuilt from seeds): sq72, odd99x117 and
sq136 with 3 channels, the 1-channel gray72 (average only: the reference's Gaussian is fixed at 3 channels) and clamp72 = sq72's
image stretched about 0.5 by CLAMP_SCALE, so that the high-pass clamp is active (asserted: >= 1 % of its elements are clamped).  Per
case and filter (low-average, low-gaussian, high-average, high-gaussian) the fixture holds, from the REAL reference modules:

    out, grad             probes of the fp64 output and of the fp64 gradient of sum(out * m), m a seeded map in [-1, 1)
    e32_out, e32_grad     max |fp32 run - fp64 run| of the reference itself: the yardsticks of the GPU tests (e32_grad over the
                          elements the tests keep, see below)
    near_share            high-pass: share of elements whose fp64 pre-clamp value lies within 4 e32_out of 0 or 1 (asserted <= 1e-3)
    grad_left_out         high-pass: share of gradient elements with such an element inside their 9 x 9 reach -- a mask that flips
                          there moves every gradient element it reaches, so the gradient comparison leaves those out
    clamped_share         high-pass: share of elements with a pre-clamp value outside [0, 1]
    sep_dev               max |separable fp64 evaluation with the engine's fp32 1-D taps - reference fp64 output|: what evaluating
                          the 9 x 9 filter as 9 + 9 taps (average: fp32(1/9) twice instead of 1/81) costs; asserted <= e32_out

`restate` is an fp64 restatement in plain torch; the tool asserts restate == reference to 1e-12 (output and every gradient element)
before it writes the file, so the tests can compare the engine with `restate`'s full tensors where the reference does not exist.

(b) Step records: the harness's small ESRGAN config, two steps of the reference's SRModel with fs: true -- `average` filters with
pix-l1, fea, the GAN term and tv-l1; `gaussian` filters with ssim and grad-4d-l1 on top of pix-l1, fea and the GAN term (weights of
the existing image-loss and SSIM step records) -- and one Pix2Pix record (fs: true, gan_opt.form standard, average filters).
"""
import os
import random
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import detrand  # noqa: E402
from oracle import ref_harness as R  # noqa: E402
from tools import make_golden_ssim as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "freqsep.pt")
IMAGE_LOSSES = os.path.join(ROOT, "tests", "golden", "image_losses.pt")
CASES = ("sq72", "odd99x117", "sq136", "gray72", "clamp72")
FILTERS = ("low-average", "low-gaussian", "high-average", "high-gaussian")
CLAMP_SCALE = 3.5          # clamp72 = 0.5 + CLAMP_SCALE * (sq72 - 0.5), about [-1.6, 2.6]: the smallest of 2, 2.5, 3, ... that clamps >= 1 % under BOTH filters (2 does for average only: the Gaussian residual is smaller)
NEAR_CAP, CLAMPED_FLOOR = 1e-3, 1e-2
MAP_SEED = 5151
STEP_YAML = dict(nb=1, batch=2, crop=64, d_nf=16)
STEP_SEED, STEP_K = 371, 2
I2I_SPEC = dict(yaml=dict(model="pix2pix", batch=2, crop=64, n_blocks=2, ngf=16, ndf=16, pixel_weight=100.0, gan_form="standard"),
                steps=2, seed=91)

probe, probe_error = G.probe, G.probe_error


def make_input(case):
    """-> x, fp32 NCHW."""
    if case == "clamp72":
        sr, _ = G.make_inputs("sq72")
        return ((sr.double() - 0.5) * CLAMP_SCALE + 0.5).float().contiguous()
    return G.make_inputs(case)[0]


def filters_for(case):
    return tuple(f for f in FILTERS if not (case == "gray72" and f.endswith("gaussian")))


def seeded_map(shape, seed=MAP_SEED):
    n = 1
    for s in shape:
        n *= s
    return (detrand.uniform01(n, seed).double().reshape(shape) * 2 - 1).float()


# ------------------------------------------------------------------------------------------------ restatement
def taps1d(kind):
    """The engine's separable taps (fp32): what FilterLow hands to the kernels."""
    from trainner_amd.dataops import filters as EF
    return torch.tensor(EF.FilterLow(filter_type=kind).taps, dtype=torch.float32)


def taps2d(kind):
    """The reference's 9 x 9 taps: the fp32 Gaussian weights, or 1 / 81."""
    from trainner_amd.dataops import filters as EF
    if kind == "gaussian":
        return EF.gaussian_taps2d().double()
    return torch.full((9, 9), 1.0 / 81.0, dtype=torch.float64)


def low(x, kind, k2=None):
    k2 = taps2d(kind) if k2 is None else k2
    w = k2.to(x.dtype).expand(x.shape[1], 1, 9, 9)
    return F.conv2d(x, w, padding=4, groups=x.shape[1])


def low_separable(x, kind):
    """L x as the kernels evaluate it: 9 horizontal, then 9 vertical taps (here in x's dtype)."""
    k = taps1d(kind).to(x.dtype)
    C = x.shape[1]
    t = F.conv2d(x, k.reshape(1, 1, 1, 9).expand(C, 1, 1, 9), padding=(0, 4), groups=C)
    return F.conv2d(t, k.reshape(1, 1, 9, 1).expand(C, 1, 9, 1), padding=(4, 0), groups=C)


def preclamp(x, kind):
    return (x - low(x, kind) + 1.0) / 2.0


def restate(x, name):
    band, kind = name.split("-")
    return low(x, kind) if band == "low" else preclamp(x, kind).clamp(0, 1)


def restate_with_grad(x, name, m, dtype=torch.float64):
    x = x.detach().to(dtype).contiguous().requires_grad_(True)
    out = restate(x, name)
    (out * m.to(dtype)).sum().backward()
    return out.detach(), x.grad.detach()


def reach9x9(mask):
    return F.max_pool2d(mask.double(), 9, stride=1, padding=4) > 0


def near_masks(x, name, e32_out):
    """-> (near, left_out): elements whose fp64 pre-clamp value lies within 4 e32_out of a clamp edge, and the gradient elements a
    flip of such an element's mask reaches (its 9 x 9 neighbourhood, itself included).  Low-pass filters have neither."""
    band, kind = name.split("-")
    if band == "low":
        z = torch.zeros(x.shape, dtype=torch.bool)
        return z, z
    p = preclamp(x.double(), kind)
    near = (p.abs() <= 4 * e32_out) | ((p - 1).abs() <= 4 * e32_out)
    return near, reach9x9(near)


# ------------------------------------------------------------------------------------------------ the reference
def _reference_filters():
    with R.reference_env():
        for m in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data", "cv2", "torchvision")]:
            del sys.modules[m]
        import dataops.filters as FL
    return FL


def reference_run(FL, name, x, m, dtype):
    band, kind = name.split("-")
    with R.reference_env():
        mod = (FL.FilterLow if band == "low" else FL.FilterHigh)(filter_type=kind).to(dtype)
    x = x.detach().to(dtype).contiguous().requires_grad_(True)
    out = mod(x)
    (out * m.to(dtype)).sum().backward()
    return out.detach(), x.grad.detach(), mod


def filter_cases(FL):
    cases, ref_k2 = {}, None
    for case in CASES:
        x = make_input(case)
        m = seeded_map(tuple(x.shape))
        rec = {"shape": tuple(x.shape), "x": probe(x), "m": probe(m), "filters": {}}
        for name in filters_for(case):
            band, kind = name.split("-")
            o64, g64, mod = reference_run(FL, name, x, m, torch.float64)
            o32, g32, mod32 = reference_run(FL, name, x, m, torch.float32)
            if kind == "gaussian":
                fl = mod32 if band == "low" else mod32.filter_low
                ref_k2 = fl.filter.weight.data[0, 0].detach().clone()
                assert all(torch.equal(fl.filter.weight.data[c, 0], ref_k2) for c in range(3))
                assert torch.equal(ref_k2.double(), taps2d("gaussian")), "the engine's Gaussian taps are not the reference's"
            ro, rg = restate_with_grad(x, name, m)
            assert (ro - o64).abs().max().item() <= 1e-12, (case, name, (ro - o64).abs().max().item())
            assert (rg - g64).abs().max().item() <= 1e-12, (case, name, (rg - g64).abs().max().item())
            e32_out = (o32.double() - o64).abs().max().item()
            near, left_out = near_masks(x, name, e32_out)
            t = {"out": probe(o64), "grad": probe(g64), "out_absmax": o64.abs().max().item(), "grad_absmax": g64.abs().max().item(),
                 "e32_out": e32_out, "e32_grad": (g32.double() - g64)[~left_out].abs().max().item()}
            sep = low_separable(x.double(), kind)
            sep = sep if band == "low" else ((x.double() - sep + 1.0) / 2.0).clamp(0, 1)
            t["sep_dev"] = (sep - o64)[~near].abs().max().item()
            assert t["sep_dev"] <= e32_out, (case, name, t["sep_dev"], e32_out)
            if band == "high":
                p = preclamp(x.double(), kind)
                t["near_share"] = near.double().mean().item()
                t["grad_left_out"] = left_out.double().mean().item()
                t["clamped_share"] = ((p < 0) | (p > 1)).double().mean().item()
                assert t["near_share"] <= NEAR_CAP, (case, name, t["near_share"])
                if case == "clamp72":
                    assert t["clamped_share"] >= CLAMPED_FLOOR, (case, name, t["clamped_share"])
            rec["filters"][name] = t
            print("%-10s %-13s e32_out %.2e e32_grad %.2e sep_dev %.2e max|o| %.3f max|g| %.3f" % (
                case, name, t["e32_out"], t["e32_grad"], t["sep_dev"], t["out_absmax"], t["grad_absmax"]),
                " ".join("%s %.2e" % (k, t[k]) for k in ("near_share", "grad_left_out", "clamped_share") if k in t))
        cases[case] = rec
    return cases, ref_k2


# ------------------------------------------------------------------------------------------------ step records
STEP_RECORDS = {
    # record -> (filter type of both filters, extra train lines with %(name)s weights, loss_list names, precise names)
    "sr_average": ("average", "  tv_type: normal\n  tv_norm: 1\n  tv_weight: %(tv-l1)g", ["pix-l1", "tv-l1", "fea-vgg19-l1"], []),
    "sr_gaussian": ("gaussian", "  grad_type: grad-4d-l1\n  grad_weight: %(grad-4d-l1)g\n  ssim_type: ssim\n  ssim_weight: %(ssim)g",
                    ["pix-l1", "fea-vgg19-l1"], ["grad-4d-l1", "ssim"]),
}


def term_weights():
    """tv-l1 and grad-4d-l1 as in the image-loss step record (tests/golden/image_losses.pt), ssim as in the SSIM step record (1)."""
    w = torch.load(IMAGE_LOSSES, weights_only=False)["steps"]["recipe_terms"]["weights"]
    return {"tv-l1": w["tv-l1"], "grad-4d-l1": w["grad-4d-l1"], "ssim": 1.0}


def fs_yaml(path, kind, extra=""):
    """Add `fs: true` with both filter types = kind, and the lines of `extra`, to the train block of a yaml written by
    oracle.ref_harness.esrgan_yaml / i2i_yaml."""
    with open(path) as fh:
        txt = fh.read()
    assert txt.count("\nlogger:") == 1
    lines = "\n  fs: true\n  lpf_type: %s\n  hpf_type: %s" % (kind, kind) + ("\n" + extra if extra else "")
    with open(path, "w") as fh:
        fh.write(txt.replace("\nlogger:", lines + "\nlogger:"))
    return path


def sr_step_record(tag):
    from oracle.make_golden import D_SEED, F_SEED, G_SEED, probe_state
    kind, extra, names, precise = STEP_RECORDS[tag]
    weights = term_weights()
    yml = fs_yaml(R.esrgan_yaml(name="golden_freqsep_" + tag, **STEP_YAML), kind, extra % weights)
    opt, model = R.build_reference_model(yml, seed=0)
    assert model.f_low is not None and model.f_high is not None
    assert [l["name"] for l in model.generatorlosses.loss_list] == names
    assert [l["name"] for l in model.generatorlosses.precise_loss_list] == precise
    detrand.fill_state_dict_(model.netG.state_dict(), G_SEED)
    detrand.fill_state_dict_(model.netD.state_dict(), D_SEED)
    netF = R.reference_netF(model)
    detrand.fill_state_dict_({k: v for k, v in netF.state_dict().items() if k.startswith("feature_net")}, F_SEED, gain=1.0, bias_amp=0.05)
    logs = []
    for s in range(1, STEP_K + 1):
        LR, HR = detrand.synthetic_pair(STEP_YAML["batch"], STEP_YAML["crop"], STEP_SEED + s)
        logs.append(R.reference_step(model, LR, HR, s))
    print("step", tag, [{k: round(v, 6) for k, v in l.items()} for l in logs])
    return {"name": "freqsep_step_" + tag, "spec": {"yaml": dict(STEP_YAML), "steps": STEP_K, "seed": STEP_SEED}, "filter_type": kind,
            "extra": extra % weights, "loss_names": names, "precise_names": precise,
            "network_G": dict(opt["network_G"]), "network_D": dict(opt["network_D"]),
            "seeds": {"G": G_SEED, "D": D_SEED, "F": F_SEED, "data": STEP_SEED},
            "logs": logs, "fake_H": model.fake_H.detach().clone(),
            "g_state": probe_state(model.netG.state_dict()), "d_state": probe_state(model.netD.state_dict()),
            "g_keys": [(k, tuple(v.shape)) for k, v in model.netG.state_dict().items()],
            "d_keys": [(k, tuple(v.shape)) for k, v in model.netD.state_dict().items()], "torch": torch.__version__}


def i2i_step_record():
    """The layout of oracle/make_golden_i2i.run_case's records, with fs: true (average filters)."""
    from oracle.make_golden import probe_state
    from oracle.make_golden_i2i import POOL_SEED, SEEDS, ab_pair
    spec = I2I_SPEC
    yml = fs_yaml(R.i2i_yaml(name="golden_freqsep_pix2pix", **spec["yaml"]), "average")
    opt, model = R.build_reference_model(yml, seed=0)
    assert model.f_low is not None and model.f_high is not None
    names = list(model.model_names)
    for n in names:
        detrand.fill_state_dict_(getattr(model, "net" + n).state_dict(), SEEDS[n])
    batch, crop = spec["yaml"]["batch"], spec["yaml"]["crop"]
    random.seed(POOL_SEED)
    logs = []
    with R.reference_env():
        for s in range(1, spec["steps"] + 1):
            A, B = ab_pair(batch, crop, spec["seed"] + s)
            model.feed_data({"A": A, "B": B, "A_path": ["a"] * batch})
            model.optimize_parameters(s)
            logs.append(dict(model.get_current_log()))
            if s == 1:
                imgs1 = {"fake_B": model.fake_B.detach().clone()}
    print("step pix2pix", [{k: round(v, 6) for k, v in l.items()} for l in logs])
    return {"name": "freqsep_step_pix2pix", "spec": spec, "filter_type": "average", "network_G": dict(opt["network_G"]),
            "network_D": dict(opt["network_D"]), "seeds": dict(SEEDS, data=spec["seed"], pool=POOL_SEED), "model_names": names,
            "logs": logs, "images": {"fake_B": model.fake_B.detach().clone()}, "images_step1": imgs1,
            "states": {n: probe_state(getattr(model, "net" + n).state_dict()) for n in names},
            "keys": {n: [(k, tuple(v.shape)) for k, v in getattr(model, "net" + n).state_dict().items()] for n in names},
            "torch": torch.__version__}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    FL = _reference_filters()
    cases, k2 = filter_cases(FL)
    from trainner_amd.dataops import filters as EF
    fx = {"cases": cases, "gaussian_taps2d": k2.clone(), "gaussian_taps1d": EF.gaussian_taps1d().clone(),
          "clamp_scale": CLAMP_SCALE,
          "steps": {"sr_average": sr_step_record("sr_average"), "sr_gaussian": sr_step_record("sr_gaussian"),
                    "pix2pix": i2i_step_record()},
          "torch": torch.__version__}
    # the 1-D taps are the reference's own get_gaussian_kernel1d(9, 1.5), bit for bit
    with R.reference_env():
        assert torch.equal(FL.get_gaussian_kernel1d(9, FL.get_kernel_sigma(9)), fx["gaussian_taps1d"])
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(fx, OUT)
    print("->", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
