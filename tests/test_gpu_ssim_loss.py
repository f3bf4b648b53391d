"""SSIM / MS-SSIM training losses on the device (-m gpu): csrc/ssim_loss.hip through the C ABI (ops.ssim_* / the SSIM and MS_SSIM
modules) against tests/golden/ssim_loss.pt (the REAL reference's fp64 runs, tools/make_golden_ssim.py) and against the tool's fp64
restatement, which the tool pinned to the reference to 1e-12 and tests/test_cpu_ssim_loss.py pins to the fixture again.

Tolerances are measured on the reference, not on the engine: against the reference's fp64 result
    value error    <= max(4 x the largest `e32_val` in the fixture, 4 fp32 ulps of the value)
    gradient error <= 4 x the case's `e32_grad` (the reference's own max |g32 - g64|)
The factor 4 allows a different, equally fp32, summation order in the 11-tap filters.  Every figure is printed before it is
asserted (`pytest -s`); DESIGN.md section 11 quotes the worst ratios.
"""
import os

import pytest
import torch

from oracle import detrand, fixtures as FX, ref_harness
from tools import make_golden_ssim as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_loss.pt")
REGULAR = list(G.REGULAR)


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


def module_for(kind, channels):
    from trainner_amd.models.modules.ssim import MS_SSIM, SSIM
    kw = dict(window_size=11, window_sigma=1.5, size_average=True, data_range=1., channels=channels)
    return SSIM(**kw) if kind == "ssim" else MS_SSIM(normalize="relu", **kw)


def value_bound(fx, value):
    worst = max(t["e32_val"] for c in fx["cases"].values() for t in c["types"].values())
    ulp = torch.finfo(torch.float32).eps * 2.0 ** torch.tensor(abs(value)).log2().floor().item()
    return max(4 * worst, 4 * ulp)


def engine_run(kind, sr, hr, layout):
    """-> (value as a Python float, d value / d sr on the CPU in fp64) of the module on the device, operands in `layout`."""
    fmt = torch.channels_last if layout == "cl" else torch.contiguous_format
    x = sr.to(DEV).contiguous(memory_format=fmt).requires_grad_(True)
    y = hr.to(DEV).contiguous(memory_format=fmt)
    v = module_for(kind, sr.shape[1])(x, y)
    assert v.dtype == torch.float32 and v.dim() == 0
    v.backward()
    assert x.grad.stride() == x.stride()
    return v.item(), x.grad.detach().cpu().contiguous().double()


def check_inputs(rec, sr, hr):
    for t, pr in ((sr, rec["sr"]), (hr, rec["hr"])):
        es, _ = G.probe_error(t, pr)
        assert es <= 1e-6, "make_inputs no longer rebuilds the fixture's pair (%g)" % es


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("kind", G.TYPES)
@pytest.mark.parametrize("name", REGULAR)
def test_golden_value_and_gradient(fx, name, kind, layout):
    rec = fx["cases"][name]
    t = rec["types"][kind]
    sr, hr = G.make_inputs(name)
    check_inputs(rec, sr, hr)
    _, gref, _ = G.restate_with_grad(sr, hr, kind)
    es, _ = G.probe_error(gref, t["grad"])
    assert es <= 1e-12, es                       # the restatement's gradient IS the reference's (as when the fixture was written)
    value, grad = engine_run(kind, sr, hr, layout)
    ev, eg = abs(value - t["value"]), (grad - gref).abs().max().item()
    bv, bg = value_bound(fx, t["value"]), 4 * t["e32_grad"]
    print("\n%s %s %s: value err %.3e (bound %.3e, ratio %.3f)  grad err %.3e (bound %.3e, ratio %.3f; e32_grad %.3e, max|g| %.3e)"
          % (name, kind, layout, ev, bv, ev / bv, eg, bg, eg / bg, t["e32_grad"], t["grad_absmax"]))
    assert ev <= bv, (ev, bv)
    assert eg <= bg, (eg, bg)
    # the shaved border carries no gradient
    border = grad.clone()
    border[..., 4:-4, 4:-4] = 0
    assert border.abs().max().item() == 0.0


@pytest.mark.parametrize("kind", G.TYPES)
def test_two_runs_are_bit_identical(kind):
    sr, hr = G.make_inputs("odd99x117")
    v1, g1 = engine_run(kind, sr, hr, "nchw")
    v2, g2 = engine_run(kind, sr, hr, "nchw")
    assert v1 == v2 and torch.equal(g1, g2)


def test_accumulate_adds_into_the_gradient():
    from trainner_amd import ops
    from trainner_amd.models.modules.ssim import gaussian_taps
    sr, hr = G.make_inputs("sq72")
    x, y = sr.to(DEV), hr.to(DEV)
    taps = tuple(float(v) for v in gaussian_taps(11, 1.5))
    N = x.shape[0]
    coef = torch.tensor([[1e-4, 2e-5]] * N, dtype=torch.float32, device=DEV)
    gscale = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    fresh = torch.full_like(x, float("nan"))
    ops.ssim_bwd(x, y, 0, 4, taps, 1e-4, 9e-4, coef, gscale, fresh)
    assert torch.isfinite(fresh).all()
    base = torch.randn_like(x)
    acc = base.clone()
    ops.ssim_bwd(x, y, 0, 4, taps, 1e-4, 9e-4, coef, gscale, acc, accumulate=True)
    assert torch.equal(acc, base + fresh)
    assert torch.equal(acc[..., :4, :], base[..., :4, :]) and torch.equal(acc[..., :, -4:], base[..., :, -4:])
    # no gscale pointer = 1: twice the gradient at gscale 0.5
    unit = torch.empty_like(x)
    ops.ssim_bwd(x, y, 0, 4, taps, 1e-4, 9e-4, coef, None, unit)
    assert torch.allclose(unit, 2 * fresh, rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", ["sq136", "odd99x117"])
def test_identical_images_give_loss_exactly_zero(fx, name):
    """sr == hr of a regular case (no clamp acts): numerators and denominators of both SSIM fractions are bit-identical, the map is
    exactly 1, the loss 1 - f exactly 0, and the gradient is 0 within the case's gradient bound."""
    _, hr = G.make_inputs(name)
    value, grad = engine_run("ssim", hr, hr, "nchw")
    print("\n%s sr == hr: 1 - ssim = %.3e, max |grad| %.3e (bound %.3e)" % (name, 1.0 - value, grad.abs().max().item(),
                                                                        4 * fx["cases"][name]["types"]["ssim"]["e32_grad"]))
    assert 1.0 - value == 0.0
    assert grad.abs().max().item() <= 4 * fx["cases"][name]["types"]["ssim"]["e32_grad"]


@pytest.mark.parametrize("kind", G.TYPES)
@pytest.mark.parametrize("name", list(G.BRANCH))
def test_branch_cases(fx, name, kind):
    """Where the variance clamp or the relu acts only the value is compared; the gradient must be finite, and exactly 0 for an image
    whose factor the relu zeroed (the reference's autograd gives NaN there; the engine deliberately does not)."""
    rec = fx["cases"][name]
    t = rec["types"][kind]
    sr, hr = G.make_inputs(name)
    check_inputs(rec, sr, hr)
    value, grad = engine_run(kind, sr, hr, "nchw")
    ev, bv = abs(value - t["value"]), value_bound(fx, t["value"])
    print("\n%s %s: value %.9f reference %.9f err %.3e (bound %.3e)" % (name, kind, value, t["value"], ev, bv))
    assert ev <= bv, (ev, bv)
    assert torch.isfinite(grad).all()
    for n in t["relu_images"]:
        assert grad[n].abs().max().item() == 0.0
    if t["relu_images"]:
        assert grad[[n for n in range(grad.shape[0]) if n not in t["relu_images"]]].abs().max().item() > 0


def _engine_model(fxs, tmp_path, ssim_type):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = ref_harness.esrgan_yaml(name="engine_ssim", out_root=str(tmp_path), gpu_ids="[0]", **fxs["spec"]["yaml"])
    if ssim_type:
        G.ssim_yaml(yml, ssim_type)
    opt = options.parse(yml, is_train=True)
    model = create_model(opt, verbose=False)
    g, d, f = FX.initial_states(fxs)
    model.netG.load_state_dict(g)
    model.netD.load_state_dict(d)
    netF = [l["function"].network for l in model.generatorlosses.loss_list if "fea" in l["name"]][0]
    sd = netF.state_dict()
    sd.update(f)
    netF.load_state_dict(sd)
    return model


@pytest.mark.parametrize("kind", G.TYPES)
def test_step_matches_reference_record(fx, kind, tmp_path):
    """optimize_parameters with `ssim_type: kind, ssim_weight: 1` against the real reference's SRModel, two steps, with the bounds
    tests/test_gpu_step.py uses for K <= 3 (DEFAULT_TOL)."""
    fxs = fx["steps"][kind]
    T = dict(log=2e-4, fake_mean=2e-5, fake_max=5e-4, st_mean=0.02, st_worst=2.05, bn=2e-3)
    model = _engine_model(fxs, tmp_path, kind)
    assert [l["name"] for l in model.generatorlosses.precise_loss_list] == [kind]
    for (s, (LR, HR)), ref_log in zip(FX.batches(fxs), fxs["logs"]):
        model.feed_data({"LR": LR, "HR": HR})
        model.optimize_parameters(s)
        log = model.get_current_log()
        print("\nstep", s, {k: (round(log[k], 7), round(v, 7)) for k, v in ref_log.items()})
        for k, v in ref_log.items():
            assert k in log, k
            t = 2e-3 if k in ("D_real", "D_fake") else T["log"]
            assert abs(log[k] - v) <= t * max(1.0, abs(v)) + 5e-6, (k, log[k], v)
    ref, got = fxs["fake_H"], model.fake_H.detach().cpu()
    scale = max(1.0, ref.abs().max().item())
    diff = (got - ref).abs()
    assert diff.mean().item() <= T["fake_mean"] * scale and diff.max().item() <= T["fake_max"] * scale, (diff.mean().item(), diff.max().item())
    lr_steps = 1e-4 * fxs["spec"]["steps"]
    worst, mean, k = FX.state_error({k: v.detach().cpu() for k, v in model.netG.state_dict().items()}, fxs["g_state"], lr_steps=lr_steps)
    assert mean < T["st_mean"] and worst < T["st_worst"], ("G state", k, worst, mean)
    ds = {k: v.detach().cpu() for k, v in model.netD.state_dict().items()}
    worst, mean, k = FX.state_error(ds, fxs["d_state"], FX.bn_shadowed_biases(fxs["d_keys"]), lr_steps=lr_steps)
    assert mean < T["st_mean"] and worst < T["st_worst"], ("D state", k, worst, mean)


def test_step_without_ssim_weight_issues_no_ssim_launch(fx, tmp_path, monkeypatch):
    from trainner_amd import ops
    names = ("ssim_fwd", "ssim_bwd", "avgpool2_pad_fwd", "avgpool2_pad_bwd", "msssim_combine")
    calls = []
    for n in names:
        real = getattr(ops, n)
        monkeypatch.setattr(ops, n, lambda *a, _real=real, _n=n, **k: (calls.append(_n), _real(*a, **k))[1])
    fxs = fx["steps"]["ssim"]
    model = _engine_model(fxs, tmp_path / "plain", None)
    assert model.generatorlosses.precise_loss_list == []
    s, (LR, HR) = next(iter(FX.batches(fxs)))
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(s)
    assert "ssim" not in model.get_current_log()
    assert calls == []
    # ... and with the option the same wrappers are what the step goes through: 1 forward, 1 combine, 1 backward
    model = _engine_model(fxs, tmp_path / "ssim", "ssim")
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(s)
    assert sorted(calls) == ["msssim_combine", "ssim_bwd", "ssim_fwd"]


def test_shipped_recipe_with_msssim_steps(tmp_path, monkeypatch):
    """options/sr/train_sr.yml with its `ssim_type: ms-ssim` / `ssim_weight: 1` lines uncommented (nothing else changed: RRDBNet-23,
    batch 8, crop 128, use_amp: true) parses, constructs and steps.  At the recipe's crop level 5 is 8 x 8 and runs 7 taps."""
    import test_gpu_step as TS
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml, _ = TS.shipped_recipe(tmp_path, monkeypatch)

    def edit(tree):
        tree["train"]["ssim_type"], tree["train"]["ssim_weight"] = "ms-ssim", 1

    assert FX.write_recipe("sr/train_sr.yml", str(tmp_path), edit) == yml
    opt = options.parse(yml, is_train=True)
    assert opt["use_amp"] is True
    torch.manual_seed(opt["train"]["manual_seed"])
    model = create_model(opt, verbose=False)
    assert [(l["name"], l["weight"]) for l in model.generatorlosses.precise_loss_list] == [("ms-ssim", 1)]
    ds = opt["datasets"]["train"]
    LR, HR = detrand.synthetic_pair(ds["batch_size"], ds["crop_size"], 501)
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert set(log) >= {"pix-l1", "fea-vgg19-l1", "l_g_gan", "ms-ssim"}
    assert 0.0 <= log["ms-ssim"] <= 1.0 and all(v == v for v in log.values()), log


@pytest.mark.parametrize("kind", G.TYPES)
def test_bench_batch_against_chunked_restatement(fx, kind):
    """16 x 3 x 512 x 512 once, against the fp64 restatement evaluated image by image on the CPU (both losses are batch means of
    per-image terms).  The pair is not a fixture case, so the gradient bound is derived, not stored: 4 x the largest
    e32_grad / max|g| the reference shows over the fixture's regular cases of this type, times this pair's max |g|."""
    N, C, H, W = 16, 3, 512, 512
    low = detrand.uniform01(N * C * (H // 4) * (W // 4), 31).double().reshape(N, C, H // 4, W // 4)
    hr = torch.nn.functional.interpolate(low, scale_factor=4, mode="bicubic", align_corners=False)
    hr = (hr + 0.05 * (detrand.uniform01(N * C * H * W, 32).double().reshape(N, C, H, W) - 0.5)).clamp(0, 1).float()
    sr = (hr.double() + 0.16 * (detrand.uniform01(N * C * H * W, 33).double().reshape(N, C, H, W) - 0.5)).clamp(-0.1, 1.1).float()
    vref, gref = 0.0, torch.empty(N, C, H, W, dtype=torch.float64)
    for n in range(N):
        v, g, detail = G.restate_with_grad(sr[n:n + 1], hr[n:n + 1], kind)
        assert detail["clamped"] == 0
        vref += v.item() / N
        gref[n] = g[0] / N
    value, grad = engine_run(kind, sr, hr, "nchw")
    rel = max(c["types"][kind]["e32_grad"] / c["types"][kind]["grad_absmax"] for c in fx["cases"].values() if c["regular"])
    ev, eg = abs(value - vref), (grad - gref).abs().max().item()
    bv, bg = value_bound(fx, vref), 4 * rel * gref.abs().max().item()
    print("\n16x3x512x512 %s: value %.9f err %.3e (bound %.3e)  grad err %.3e (bound %.3e, max|g| %.3e)"
          % (kind, value, ev, bv, eg, bg, gref.abs().max().item()))
    assert ev <= bv and eg <= bg, (ev, bv, eg, bg)
