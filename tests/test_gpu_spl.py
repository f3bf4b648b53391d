"""Spatial profile losses (cpl, gpl) and the overflow loss on the device (-m gpu): csrc/spl_loss.hip and the overflow kernels of
csrc/image_losses.hip through the C ABI (ops.spl_loss_* / overflow_loss_*, the modules of models/modules/spl.py, GeneratorLoss, SRModel)
against tests/golden/spl.pt (the REAL reference's fp64 runs, tools/make_golden_spl.py) and against the tool's fp64 restatement, which
the tool pinned to the reference to 1e-12 and tests/test_cpu_spl.py pins to the fixture again.

Tolerances are measured on the reference, never on the engine (the fixture's e32_* entries are the reference's own fp32-vs-fp64
deviations), and every figure is printed before it is asserted (`pytest -s`):
    value     |v - v64| <= max(4 x the case's e32_val, 4 fp32 ulps of the value)
    gradient  max error over EVERY element <= 4 x e32_grad: SPL is smooth away from zero-norm lines, and the overflow kinks depend on
              comparing an fp32 input with 0 and 1, which is exact
    blackrow72 additionally: the gradient on the black row equals the eps-branch term (y^ / eps times the scale, through the adjoints)
              to 4 x black_rel32, the reference's own fp32 relative deviation from that term
The factor 4 allows a different, equally fp32, summation order; a ratio above 1 is a cause to be found, not a factor to raise.
"""
import os

import pytest
import torch

from oracle import fixtures as FX, ref_harness
from tools import make_golden_spl as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spl.pt")
MASK = {"cpl": 1 | 2 | 8, "gpl": 4}


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


_REF = {}


def reference(case, name):
    """(sr, hr, fp64 value, full fp64 gradient) of the restatement, computed once per case and name and never modified."""
    if (case, name) not in _REF:
        sr, hr = T.make_inputs(case)
        v, g = T.restate_with_grad(sr, hr, name, T.znorm_of(case))
        _REF[(case, name)] = (sr, hr, v.item(), g)
    return _REF[(case, name)]


def loss_fn(name, znorm=False):
    from trainner_amd.models import losses
    return losses.get_loss_fn(name, 1, device=DEV, opt={"datasets": {"train": {"znorm": znorm}}})["function"]


def value_bound(t):
    v = abs(t["value"])
    ulp = torch.finfo(torch.float32).eps * 2.0 ** torch.tensor(max(v, 1e-30)).log2().floor().item()
    return max(4 * t["e32_val"], 4 * ulp)


def to_dev(t, layout):
    return t.to(DEV).contiguous(memory_format=torch.channels_last if layout == "cl" else torch.contiguous_format)


def engine_run(name, sr, hr, layout="nchw", znorm=False):
    """-> (value as a Python float, d value / d sr on the CPU in fp64) of the built loss function on the device."""
    x, y = to_dev(sr, layout).requires_grad_(True), to_dev(hr, layout)
    f = loss_fn(name, znorm)
    v = f(x) if name == "overflow" else f(x, y)
    assert v.dtype == torch.float32 and v.dim() == 0
    v.backward()
    assert x.grad.stride() == x.stride()
    return v.item(), x.grad.detach().cpu().contiguous().double()


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("case", T.CASES)
def test_golden_value_and_gradient(fx, case, layout):
    rec = fx["cases"][case]
    failures = []
    for name in T.names_for(case):
        t = rec["names"][name]
        sr, hr, vref, gref = reference(case, name)
        for t_, pr in ((sr, rec["sr"]), (hr, rec["hr"])):
            assert T.probe_error(t_, pr)[0] <= 1e-6, "make_inputs no longer rebuilds the fixture's pair"
        assert abs(vref - t["value"]) <= 1e-12 * max(1.0, abs(t["value"]))
        assert T.probe_error(gref, t["grad"])[0] <= 1e-12 * max(1.0, t["grad_absmax"])
        value, grad = engine_run(name, sr, hr, layout, rec["znorm"])
        ev, bv = abs(value - t["value"]), value_bound(t)
        eg, bg = (grad - gref).abs().max().item(), 4 * t["e32_grad"]
        line = "%s %s %s: value err %.3e (bound %.3e, ratio %.3f)  grad err %.3e (bound %.3e, ratio %.3f; max|g| %.3e)" % (
            case, name, layout, ev, bv, ev / bv, eg, bg, eg / bg, t["grad_absmax"])
        ok = ev <= bv and eg <= bg and bool(torch.isfinite(grad).all())
        if case == "blackrow72":
            _, ge = T.restate_with_grad(sr, hr, name, rec["znorm"], eps_only=True)
            want, got = ge[:, :, T.BLACK_ROW, :], grad[:, :, T.BLACK_ROW, :]
            rel, brel = (got - want).abs().max().item() / t["black_absmax"], 4 * t["black_rel32"]
            line += "  black row: rel err %.3e of max %.3e (bound %.3e, ratio %.3f)" % (rel, t["black_absmax"], brel, rel / brel)
            ok = ok and rel <= brel
        print("\n" + line, end="")
        if not ok:
            failures.append(line)
    assert not failures, failures


def spl_raw(x, y, mask, denorm=False, gs=None, gx=None, accumulate=False):
    """ops.spl_loss_fwd + bwd -> (5 losses on the CPU, gx)."""
    from trainner_amd import ops
    layout = 0 if x.is_contiguous() else 1
    loss = torch.full((5,), float("nan"), device=DEV)
    coef = ops.spl_coef(x, mask)
    ops.spl_loss_fwd(x, y, layout, mask, denorm, loss, coef)
    if gx is None:
        gx = torch.full_like(x, float("nan"))
    ops.spl_loss_bwd(x, y, layout, mask, denorm, coef, gs, gx, accumulate=accumulate)
    return loss.cpu(), gx


def test_unaligned_view_takes_the_scalar_path_and_matches(fx):
    """An offset pointer (4 bytes past a 16-byte boundary) with W % 4 != 0: both images and gx are dense views of larger buffers."""
    from trainner_amd import ops
    sr, hr, _, _ = reference("odd99x117", "cpl")
    assert sr.shape[3] % 4 != 0

    def shifted(t):
        buf = torch.zeros(t.numel() + 1, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    for name in ("cpl", "gpl"):
        t = fx["cases"]["odd99x117"]["names"][name]
        _, _, _, gref = reference("odd99x117", name)
        loss, gx = spl_raw(shifted(sr), shifted(hr), MASK[name], gx=shifted(torch.full_like(sr, float("nan"))))
        ev, eg = abs(loss[4].item() - t["value"]), (gx.cpu().double() - gref).abs().max().item()
        print("\nunaligned %s: value err %.3e (bound %.3e)  grad err %.3e (bound %.3e)" % (name, ev, value_bound(t), eg, 4 * t["e32_grad"]), end="")
        assert ev <= value_bound(t) and eg <= 4 * t["e32_grad"]
    t = fx["cases"]["overflow99x117"]["names"]["overflow"]
    so, _, _, gref = reference("overflow99x117", "overflow")
    x, gx, out = shifted(so), shifted(torch.full_like(so, float("nan"))), torch.empty((), device=DEV)
    ops.overflow_loss_fwd(x, 1.0 / x.numel(), out)
    ops.overflow_loss_bwd(x, 1.0 / x.numel(), None, gx)
    ev, eg = abs(out.item() - t["value"]), (gx.cpu().double() - gref).abs().max().item()
    print("\nunaligned overflow: value err %.3e (bound %.3e)  grad err %.3e (bound %.3e)" % (ev, value_bound(t), eg, 4 * t["e32_grad"]), end="")
    assert ev <= value_bound(t) and eg <= 4 * t["e32_grad"]


def test_accumulate_adds_exactly_and_gscale_scales_per_family():
    from trainner_amd import ops
    sr, hr, _, _ = reference("odd99x117", "cpl")
    x, y = sr.to(DEV), hr.to(DEV)
    allmask = MASK["cpl"] | MASK["gpl"]
    _, unit = spl_raw(x, y, allmask)
    assert torch.isfinite(unit).all()
    half = torch.full((4,), 0.5, device=DEV)
    _, fresh = spl_raw(x, y, allmask, gs=half)
    assert torch.equal(unit, 2 * fresh)                   # halving is exact in binary floating point; a NULL gscale is 1
    base = torch.randn_like(x)
    acc = base.clone()
    spl_raw(x, y, allmask, gs=half, gx=acc, accumulate=True)
    assert torch.equal(acc, base + fresh)
    # one family at a time: gscale = the unit vector of family f in the all-family call is the call with that family's mask alone
    for f, bit in enumerate((1, 2, 4, 8)):
        e = torch.zeros(4, device=DEV)
        e[f] = 1.0
        _, picked = spl_raw(x, y, allmask, gs=e)
        _, alone = spl_raw(x, y, bit)
        err = (picked - alone).abs().max().item()
        print("\nfamily %d alone vs picked by gscale: max diff %.3e of max %.3e" % (bit, err, alone.abs().max().item()), end="")
        # the picked call still adds the other families' terms times 0.0 into the sum: same magnitude, at most rounding of +0
        assert err <= 4 * torch.finfo(torch.float32).eps * alone.abs().max().item()
    # overflow
    so = T.make_inputs("overflow99x117")[0].to(DEV)
    gs1 = torch.tensor([0.5], device=DEV)
    fresh = torch.full_like(so, float("nan"))
    ops.overflow_loss_bwd(so, 1.0, gs1, fresh)
    acc = base.clone()
    ops.overflow_loss_bwd(so, 1.0, gs1, acc, accumulate=True)
    unit = torch.empty_like(so)
    ops.overflow_loss_bwd(so, 1.0, None, unit)
    assert torch.equal(acc, base + fresh) and torch.equal(unit, 2 * fresh)
    inside = (so >= 0) & (so <= 1)
    assert unit[inside].abs().max().item() == 0.0 and (unit[~inside] != 0).all()


@pytest.mark.parametrize("name", ["cpl", "gpl", "overflow"])
def test_two_runs_are_bit_identical(name):
    sr, hr = T.make_inputs("odd99x117")
    v1, g1 = engine_run(name, sr, hr)
    v2, g2 = engine_run(name, sr, hr)
    assert v1 == v2 and torch.equal(g1, g2)


@pytest.mark.parametrize("layout", ["nchw", "cl"])
def test_family_mask_of_both_terms_in_one_call(fx, layout):
    """mask = cpl | gpl in one call: the per-family values are those of the separate calls bit for bit (every line is summed in the
    same order whatever else is selected), and the gradient is the sum of the separate calls' gradients.  The summation order of the
    gradient is NOT identical (one call adds the four families' terms in registers before the one scale and store, two calls round
    each gradient on its own), so it is held within 4 fp32 ulps of the larger operand per element."""
    sr, hr, _, _ = reference("odd99x117", "cpl")
    x, y = to_dev(sr, layout), to_dev(hr, layout)
    lc, gc = spl_raw(x, y, MASK["cpl"])
    lg, gg = spl_raw(x, y, MASK["gpl"])
    lb, gb = spl_raw(x, y, MASK["cpl"] | MASK["gpl"])
    print("\nfamilies", lb.tolist(), "cpl alone", lc.tolist(), "gpl alone", lg.tolist(), end="")
    assert lc[2].item() == 0 and lg[0].item() == 0 and lg[1].item() == 0 and lg[3].item() == 0
    assert lb[0] == lc[0] and lb[1] == lc[1] and lb[3] == lc[3] and lb[2] == lg[2]
    assert lg[4] == lg[2]
    for got, want in ((lc[4], lc[0].double() + lc[1].double() + lc[3].double()), (lb[4], lb[:4].double().sum())):
        assert abs(got.item() - want.item()) <= 2 * torch.finfo(torch.float32).eps * abs(want.item())
    err = (gb.double() - (gc.double() + gg.double())).abs()
    bound = 4 * torch.finfo(torch.float32).eps * torch.maximum(gc.abs(), gg.abs()).double()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print("  summed gradient: worst element at %.3f of 4 ulps" % ratio, end="")
    assert ratio <= 1.0


def test_cpl_refuses_other_channel_counts_and_gpl_takes_them():
    x = torch.rand(2, 1, 32, 32, device=DEV)
    with pytest.raises(NotImplementedError, match="3 x H x W"):
        loss_fn("cpl")(x, x)
    v = loss_fn("gpl")(torch.rand(2, 4, 33, 35, device=DEV), torch.rand(2, 4, 33, 35, device=DEV))
    assert torch.isfinite(v)
    # identical images: every cosine of a non-zero line is 1 -> -(C (W - 1) + C W + C H + C (H - 1)) / H for gpl's two traces
    # (dx has W - 1 non-zero columns, dy has H - 1 non-zero rows)
    h = torch.rand(2, 3, 40, 52, device=DEV) + 0.1 * torch.arange(52, device=DEV) + 0.3 * torch.arange(40, device=DEV).reshape(40, 1)
    v = loss_fn("gpl")(h.clone().requires_grad_(True), h).item()
    want = -(3 * (51 + 40) + 3 * (52 + 39)) / 40
    assert abs(v - want) <= 4 * torch.finfo(torch.float32).eps * abs(want)


def _engine_model(fxs, tmp_path, weights, extra=""):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = ref_harness.esrgan_yaml(name="engine_spl", out_root=str(tmp_path), gpu_ids="[0]", **fxs["spec"]["yaml"])
    if weights:
        T.losses_yaml(yml, weights)
    if extra:
        with open(yml) as fh:
            txt = fh.read()
        with open(yml, "w") as fh:
            fh.write(txt.replace("\nlogger:", extra + "\nlogger:"))
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


def test_step_matches_reference_record(fx, tmp_path):
    """optimize_parameters with spl_type: spl and of_type: overflow (weights of the record) against the real reference's SRModel, two
    steps, with the bounds tests/test_gpu_step.py uses (DEFAULT_TOL).  The gpl entries of this record are of order 5e-5 (the cosines of an
    untrained generator nearly cancel and spl_weight is set from cpl), so the log check says little about gpl: here it is held through
    fake_H and G's state, and its value and gradient through test_golden_value_and_gradient."""
    import test_gpu_step as TS
    fxs = fx["steps"]["spl_overflow"]
    tol = TS.DEFAULT_TOL
    model = _engine_model(fxs, tmp_path, fxs["weights"])
    assert [l["name"] for l in model.generatorlosses.loss_list] == ["pix-l1", "fea-vgg19-l1", "cpl", "gpl", "overflow"]
    assert model.generatorlosses.precise_loss_list == []
    for (s, (LR, HR)), ref_log in zip(FX.batches(fxs), fxs["logs"]):
        model.feed_data({"LR": LR, "HR": HR})
        model.optimize_parameters(s)
        log = model.get_current_log()
        print("\nstep", s, {k: (round(log[k], 7), round(v, 7)) for k, v in ref_log.items()})
        assert ref_log["overflow"] > 0 and 0.1 <= abs(ref_log["cpl"]) / ref_log["pix-l1"] <= 10.0
        TS.check_logs(log, ref_log, tol=tol["log"])
    ref, got = fxs["fake_H"], model.fake_H.detach().cpu()
    scale = max(1.0, ref.abs().max().item())
    diff = (got - ref).abs()
    assert diff.mean().item() <= tol["fake_mean"] * scale and diff.max().item() <= tol["fake_max"] * scale, (diff.mean().item(), diff.max().item())
    lr_steps = 1e-4 * fxs["spec"]["steps"]
    worst, mean, k = FX.state_error({k: v.detach().cpu() for k, v in model.netG.state_dict().items()}, fxs["g_state"], lr_steps=lr_steps)
    assert mean < tol["st_mean"] and worst < tol["st_worst"], ("G state", k, worst, mean)
    ds = {k: v.detach().cpu() for k, v in model.netD.state_dict().items()}
    worst, mean, k = FX.state_error(ds, fxs["d_state"], FX.bn_shadowed_biases(fxs["d_keys"]), lr_steps=lr_steps)
    assert mean < tol["st_mean"] and worst < tol["st_worst"], ("D state", k, worst, mean)


def test_step_without_the_new_keys_issues_none_of_the_new_launches_and_fs_steps(fx, tmp_path, monkeypatch):
    from trainner_amd import ops
    names = ("spl_loss_fwd", "spl_loss_bwd", "overflow_loss_fwd", "overflow_loss_bwd")
    calls = []
    for n in names:
        real = getattr(ops, n)
        monkeypatch.setattr(ops, n, lambda *a, _real=real, _n=n, **k: (calls.append(_n), _real(*a, **k))[1])
    fxs = fx["steps"]["spl_overflow"]
    model = _engine_model(fxs, tmp_path / "plain", None)
    assert [l["name"] for l in model.generatorlosses.loss_list] == ["pix-l1", "fea-vgg19-l1"]
    s, (LR, HR) = next(iter(FX.batches(fxs)))
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(s)
    assert not set(T.STEP_TERMS) & set(model.get_current_log())
    assert calls == []
    # one step with fs: true and the three terms: they run (one forward and one backward each) and log finite values
    model = _engine_model(fxs, tmp_path / "fs", fxs["weights"], extra="\n  fs: true\n  lpf_type: average\n  hpf_type: average")
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(s)
    log = model.get_current_log()
    print("\nfs step", {k: log[k] for k in ("pix-l1", "cpl", "gpl", "overflow")}, end="")
    assert sorted(calls) == ["overflow_loss_bwd", "overflow_loss_fwd", "spl_loss_bwd", "spl_loss_bwd", "spl_loss_fwd", "spl_loss_fwd"]
    for k in ("cpl", "gpl", "overflow"):
        assert k in log and log[k] == log[k] and abs(log[k]) != float("inf")
    assert log["cpl"] < 0
