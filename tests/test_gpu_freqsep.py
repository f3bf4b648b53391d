"""Frequency separation on the device (-m gpu): csrc/freqsep.hip through the C ABI (ops.freqsep_*), the modules of dataops/filters.py and
the models' wiring, against tests/golden/freqsep.pt (the REAL reference's fp64 runs, tools/make_golden_freqsep.py) and the tool's fp64
restatement, which the tool pinned to the reference to 1e-12 and tests/test_cpu_freqsep.py pins to the fixture again.

Tolerances are measured on the reference, never on the engine (e32_out / e32_grad are the reference's own fp32-vs-fp64 deviations), and
every ratio is printed before it is asserted (`pytest -s`):
    output    max error <= max(4 x e32_out, 4 fp32 ulps of the largest output)
    gradient  max error <= 4 x e32_grad
For the high-pass the elements within 4 x e32_out of a clamp edge are left out of the output comparison (share asserted <= 1e-3), and
the gradient elements within their 9 x 9 reach out of the gradient comparison (a mask that flips moves every element it reaches).
A ratio above 1 is a cause to be found, not a factor to raise.
"""
import os

import pytest
import torch

from oracle import detrand, fixtures as FX, ref_harness
from tools import make_golden_freqsep as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "freqsep.pt")
OPS = ("freqsep_low", "freqsep_high_fwd", "freqsep_high_bwd")


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


def to_dev(t, layout):
    return t.to(DEV).contiguous(memory_format=torch.channels_last if layout == "cl" else torch.contiguous_format)


def module_for(name):
    from trainner_amd.dataops import filters as EF
    band, kind = name.split("-")
    return (EF.FilterLow if band == "low" else EF.FilterHigh)(filter_type=kind).to(DEV)


def engine_run(name, x, m, layout):
    """-> (out, d sum(out * m) / dx) on the CPU in fp64, NCHW order."""
    xd, md = to_dev(x, layout).requires_grad_(True), to_dev(m, layout)
    out = module_for(name)(xd)
    assert out.dtype == torch.float32 and out.stride() == xd.stride()
    (out * md).sum().backward()
    assert xd.grad.stride() == xd.stride()
    return out.detach().cpu().contiguous().double(), xd.grad.detach().cpu().contiguous().double()


def ulp32(v):
    return torch.finfo(torch.float32).eps * 2.0 ** torch.tensor(max(v, 1e-30)).log2().floor().item()


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("case", T.CASES)
def test_golden_forward_and_gradient(fx, case, layout):
    rec = fx["cases"][case]
    x = T.make_input(case)
    m = T.seeded_map(tuple(x.shape))
    assert T.probe_error(x, rec["x"])[0] <= 1e-6 and T.probe_error(m, rec["m"])[0] == 0.0
    failures = []
    for name in T.filters_for(case):
        t = rec["filters"][name]
        oref, gref = T.restate_with_grad(x, name, m)
        assert T.probe_error(oref, t["out"])[0] <= 1e-12 and T.probe_error(gref, t["grad"])[0] <= 1e-12
        out, grad = engine_run(name, x, m, layout)
        near, left_out = T.near_masks(x, name, t["e32_out"])
        near_share, grad_share = near.double().mean().item(), left_out.double().mean().item()
        # the gradient comparison also leaves out the 9 x 9 reach of a near-edge element (a mask that flips there moves every gradient
        # element it reaches).  This fixture has no near-edge element at all, so nothing may be left out of either comparison
        assert near_share <= 1e-3 and near_share == t.get("near_share", 0.0) == 0.0 and grad_share == 0.0
        eo, bo = (out - oref)[~near].abs().max().item(), max(4 * t["e32_out"], 4 * ulp32(t["out_absmax"]))
        eg, bg = (grad - gref)[~left_out].abs().max().item(), 4 * t["e32_grad"]
        line = "%s %s %s: out err %.3e (bound %.3e, ratio %.3f)  grad err %.3e (bound %.3e, ratio %.3f)  left out %.2e / %.2e" % (
            case, name, layout, eo, bo, eo / bo, eg, bg, eg / bg, near_share, grad_share)
        print("\n" + line, end="")
        if not (eo <= bo and eg <= bg):
            failures.append(line)
        if name.startswith("high"):
            assert out.min().item() >= 0.0 and out.max().item() <= 1.0
            if case == "clamp72":
                clamped = ((out == 0) | (out == 1)).double().mean().item()
                assert clamped >= 1e-2, clamped
    assert not failures, failures


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("kind", ["average", "gaussian"])
def test_low_pass_is_self_adjoint_deterministic_and_accumulates_exactly(kind, layout):
    """<L x, m> == <x, L m> to the rounding of two fp32 evaluations summed in fp64; two runs bit-identical; accumulate adds exactly;
    gscale scales; the high-pass backward likewise."""
    from trainner_amd import ops
    x = to_dev(T.make_input("odd99x117"), layout)
    m = to_dev(T.seeded_map(tuple(x.shape)), layout)
    lay = 1 if layout == "cl" else 0
    taps = module_for("low-" + kind).taps
    Lx, Lm, Lx2 = (torch.full_like(x, float("nan")) for _ in range(3))
    ops.freqsep_low(x, lay, taps, Lx)
    ops.freqsep_low(m, lay, taps, Lm)
    ops.freqsep_low(x, lay, taps, Lx2)
    assert torch.isfinite(Lx).all() and torch.equal(Lx, Lx2)
    a, b = (Lx.double() * m.double()).sum().item(), (x.double() * Lm.double()).sum().item()
    # each L-value carries at most 18 fp32 roundings of partial sums <= max |.| (the taps sum to 1): an error <= 18 eps32 max|x| per
    # element, weighted by |m| <= max|m|; the elements' roundings are independent, so over n elements they add like a random walk
    # (sqrt(n), not n); once for each side of the identity
    bound = 2 * 18 * torch.finfo(torch.float32).eps * x.abs().max().item() * m.abs().max().item() * x.numel() ** 0.5
    print("\n%s %s: <Lx, m> %.9e  <x, Lm> %.9e  diff %.3e (bound %.3e)" % (kind, layout, a, b, abs(a - b), bound), end="")
    assert abs(a - b) <= bound
    gscale = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    o = torch.empty_like(x)
    ops.freqsep_high_fwd(x * 3.5 - 1.25, lay, taps, o)          # a stretched image: both clamp edges are reached
    assert (o == 0).any() and (o == 1).any()
    calls = {"low": lambda gs, out, acc: ops.freqsep_low(m, lay, taps, out, gs, accumulate=acc),
             "high": lambda gs, out, acc: ops.freqsep_high_bwd(m, o, lay, taps, out, gs, accumulate=acc)}
    for tag, call in calls.items():
        fresh, again = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        call(gscale, fresh, False)
        call(gscale, again, False)
        assert torch.isfinite(fresh).all() and torch.equal(fresh, again), tag
        base = torch.randn_like(x)
        acc = base.clone()
        call(gscale, acc, True)
        assert torch.equal(acc, base + fresh), tag
        unit = torch.empty_like(x)
        call(None, unit, False)
        assert torch.equal(unit, 2 * fresh), tag          # halving is exact in binary floating point
    # the high-pass backward passes nothing where the saved output sits on a clamp edge: with g = 1 there, gx = -L g' only
    g = torch.ones_like(x)
    gx, gp, Lgp = torch.empty_like(x), torch.where((o > 0) & (o < 1), 0.5, 0.0).to(torch.float32), torch.empty_like(x)
    ops.freqsep_high_bwd(g, o, lay, taps, gx)
    ops.freqsep_low(gp.contiguous(memory_format=torch.channels_last if lay else torch.contiguous_format), lay, taps, Lgp)
    assert torch.equal(gx, gp - Lgp)


@pytest.mark.parametrize("kind", ["average", "gaussian"])
def test_unaligned_nchw_view_takes_the_scalar_path_and_agrees_bit_for_bit(kind):
    """NCHW with W a multiple of 4 but a base pointer that is not 16-byte aligned (a view one float into a larger buffer): the host
    must pick the scalar path; the same values from an aligned allocation (16-byte path) give the same bits, for all three launches."""
    from trainner_amd import ops
    x = T.make_input("sq72").to(DEV) * 3.5 - 1.25
    m = T.seeded_map(tuple(x.shape)).to(DEV)
    taps = module_for("low-" + kind).taps

    def shifted(t, off):
        buf = torch.full((t.numel() + 8,), float("nan"), device=DEV)
        v = buf[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    def run(off):
        xs, ms = shifted(x, off), shifted(m, off)
        assert xs.is_contiguous() and (xs.data_ptr() % 16 == 0) == (off % 4 == 0)
        lo, hi, gx = (shifted(torch.zeros_like(x), off) for _ in range(3))
        ops.freqsep_low(xs, 0, taps, lo)
        ops.freqsep_high_fwd(xs, 0, taps, hi)
        ops.freqsep_high_bwd(ms, hi, 0, taps, gx)
        return lo.clone(), hi.clone(), gx.clone()

    aligned = run(0)
    assert (aligned[1] == 0).any() and (aligned[1] == 1).any()
    for off in (1, 2, 3):
        for a, b in zip(aligned, run(off)):
            assert torch.isfinite(b).all() and torch.equal(a, b), off
    # only the result pointer unaligned
    lo = shifted(torch.zeros_like(x), 1)
    ops.freqsep_low(x.contiguous(), 0, taps, lo)
    assert torch.equal(lo, aligned[0])


@pytest.mark.parametrize("layout", ["nchw", "cl"])
def test_high_pass_keeps_a_nan_as_torch_clamp_does(layout):
    """torch.clamp propagates a NaN: every output whose 9 x 9 window holds the NaN pixel is NaN (a diverged generator must not reach
    the discriminator as finite values), every other output is finite; the backward passes no gradient at a NaN output."""
    from trainner_amd import ops
    x = T.make_input("sq72").clone()
    x[0, 1, 30, 40] = float("nan")
    xd = to_dev(x, layout)
    lay = 1 if layout == "cl" else 0
    taps = module_for("high-average").taps
    o = torch.empty_like(xd)
    ops.freqsep_high_fwd(xd, lay, taps, o)
    want = torch.zeros(x.shape, dtype=torch.bool)
    want[0, 1, 26:35, 36:45] = True
    assert torch.equal(torch.isnan(o).cpu(), want)
    g, gx = torch.ones_like(xd), torch.empty_like(xd)
    ops.freqsep_high_bwd(g, o, lay, taps, gx)
    assert torch.isfinite(gx).all()


def _engine_sr_model(fxs, tmp_path, fs=True, name="engine_freqsep"):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = ref_harness.esrgan_yaml(name=name, out_root=str(tmp_path), gpu_ids="[0]", **fxs["spec"]["yaml"])
    if fs:
        T.fs_yaml(yml, fxs["filter_type"], fxs["extra"])
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


@pytest.mark.parametrize("tag", ["sr_average", "sr_gaussian"])
def test_sr_step_matches_reference_record(fx, tag, tmp_path):
    """optimize_parameters with fs: true against the real reference's SRModel, two steps, with the bounds tests/test_gpu_step.py uses."""
    import test_gpu_step as TS
    fxs = fx["steps"][tag]
    tol = TS.DEFAULT_TOL
    model = _engine_sr_model(fxs, tmp_path)
    assert [l["name"] for l in model.generatorlosses.loss_list] == fxs["loss_names"]
    assert [l["name"] for l in model.generatorlosses.precise_loss_list] == fxs["precise_names"]
    assert model.f_low.gaussian == model.f_high.gaussian == (fxs["filter_type"] == "gaussian")
    for (s, (LR, HR)), ref_log in zip(FX.batches(fxs), fxs["logs"]):
        model.feed_data({"LR": LR, "HR": HR})
        model.optimize_parameters(s)
        log = model.get_current_log()
        print("\nstep", s, {k: (round(log[k], 7), round(v, 7)) for k, v in ref_log.items()})
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


def _engine_pix2pix_model(fxs, tmp_path, fs=True):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = ref_harness.i2i_yaml(name="engine_freqsep_i2i", out_root=str(tmp_path), gpu_ids="[0]", **fxs["spec"]["yaml"])
    if fs:
        T.fs_yaml(yml, fxs["filter_type"])
    opt = options.parse(yml, is_train=True)
    model = create_model(opt, verbose=False)
    for n, sd in FX.i2i_initial_states(fxs).items():
        getattr(model, "net" + n).load_state_dict(sd)
    return opt, model


def test_pix2pix_step_matches_reference_record(fx, tmp_path):
    """Pix2Pix with fs: true (conditional D: the high-pass comes before the concatenation with the unfiltered condition), with the
    bounds of tests/test_gpu_i2i.py::test_i2i_step_matches_reference_golden."""
    import test_gpu_i2i as TI
    fxs = fx["steps"]["pix2pix"]
    opt, model = _engine_pix2pix_model(fxs, tmp_path)
    assert dict(opt["network_G"]) == fxs["network_G"] and dict(opt["network_D"]) == fxs["network_D"]
    assert list(model.model_names) == fxs["model_names"] and model.f_low is not None and model.f_high is not None
    for (s, (A, B)), ref_log in zip(FX.i2i_batches(fxs), fxs["logs"]):
        model.feed_data({"A": A, "B": B, "A_path": ["a"] * A.shape[0]})
        model.optimize_parameters(s)
        log = model.get_current_log()
        print("\nstep", s, {k: (round(log[k], 7), round(v, 7)) for k, v in ref_log.items()})
        TI.check_logs(log, ref_log, 2e-4 if s < 2 else 3e-3)
        if s == 1:
            diff = (model.fake_B.detach().cpu() - fxs["images_step1"]["fake_B"]).abs()
            assert diff.mean().item() <= 2e-5 and diff.max().item() <= 5e-4, (diff.mean().item(), diff.max().item())
    diff = (model.fake_B.detach().cpu() - fxs["images"]["fake_B"]).abs()
    assert diff.mean().item() <= 1e-2 and diff.max().item() <= 1e-1, (diff.mean().item(), diff.max().item())
    lr_steps = 2e-4 * fxs["spec"]["steps"]
    for n in fxs["model_names"]:
        sd = {k: v.detach().cpu() for k, v in getattr(model, "net" + n).state_dict().items()}
        skip = FX.norm_shadowed_biases(fxs["keys"][n], fxs["network_G"]["norm_type"]) if n.startswith("G") else ()
        worst, mean, k = FX.state_error(sd, fxs["states"][n], skip, lr_steps=lr_steps)
        assert mean < 0.15 and worst < 2.05, (n, k, worst, mean)


def _count_ops(monkeypatch):
    """Records every new op as "<name>@fwd" or "<name>@bwd": the phase is taken from the autograd functions' backward methods, so a
    forward application of the low-pass is told from its adjoint although both are the freqsep_low launch."""
    from trainner_amd import ops
    from trainner_amd.dataops import filters as EF
    calls, phase = [], ["fwd"]
    for n in OPS:
        real = getattr(ops, n)
        monkeypatch.setattr(ops, n, lambda *a, _real=real, _n=n, **k: (calls.append(_n + "@" + phase[0]), _real(*a, **k))[1])
    for fn in (EF._LowFn, EF._HighFn):
        def backward(ctx, g, _real=fn.backward):
            phase[0] = "bwd"
            try:
                return _real(ctx, g)
            finally:
                phase[0] = "fwd"
        monkeypatch.setattr(fn, "backward", staticmethod(backward))
    return calls


FULL_STEP = ["freqsep_high_bwd@bwd", "freqsep_high_fwd@fwd", "freqsep_high_fwd@fwd", "freqsep_low@bwd", "freqsep_low@fwd", "freqsep_low@fwd"]


def _count_d_forwards(model, monkeypatch):
    seen = []
    real = model.netD.engine_forward
    monkeypatch.setattr(model.netD, "engine_forward", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    return seen


@pytest.mark.parametrize("tag", ["sr_average", "sr_gaussian"])
def test_launch_counts_of_a_full_step(fx, tag, tmp_path, monkeypatch):
    """Without fs none of the new ops runs.  With fs a step in which G and D both update issues 4 forward filter launches (sr_f, hr_f,
    high(fake), high(real)) and 2 backward ones (one adjoint each), and the discriminator's forward memo hits as it does without fs."""
    calls = _count_ops(monkeypatch)
    fxs = fx["steps"][tag]
    batches = list(FX.batches(fxs))
    plain = _engine_sr_model(fxs, tmp_path / "plain", fs=False)
    assert plain.f_low is None and plain.f_high is None
    d_plain = _count_d_forwards(plain, monkeypatch)
    for s, (LR, HR) in batches:
        plain.feed_data({"LR": LR, "HR": HR})
        plain.optimize_parameters(s)
    plain.get_current_log()
    assert calls == []
    model = _engine_sr_model(fxs, tmp_path / "fs")
    d_fs = _count_d_forwards(model, monkeypatch)
    for s, (LR, HR) in batches:
        del calls[:]
        model.feed_data({"LR": LR, "HR": HR})
        model.optimize_parameters(s)
        assert sorted(calls) == FULL_STEP, calls          # 4 forward applications, 2 adjoints
    model.get_current_log()
    print("\n%s: netD.engine_forward runs per %d steps: %d without fs, %d with fs" % (tag, len(batches), len(d_plain), len(d_fs)), end="")
    assert len(d_fs) == len(d_plain)


def test_pix2pix_launch_counts(fx, tmp_path, monkeypatch):
    """Pix2Pix runs the D stage first: high(fake.detach()) and high(real_B) there, then the generator stage reuses the stored values
    behind a new autograd node: again 4 forward and 2 backward launches."""
    calls = _count_ops(monkeypatch)
    fxs = fx["steps"]["pix2pix"]
    _, model = _engine_pix2pix_model(fxs, tmp_path)
    for s, (A, B) in FX.i2i_batches(fxs):
        del calls[:]
        model.feed_data({"A": A, "B": B, "A_path": ["a"] * A.shape[0]})
        model.optimize_parameters(s)
        assert sorted(calls) == FULL_STEP, calls
    model.get_current_log()


def test_cyclegan_refuses_fs(tmp_path):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = T.fs_yaml(ref_harness.i2i_yaml(name="engine_freqsep_cyc", out_root=str(tmp_path), gpu_ids="[0]", model="cyclegan", batch=1, crop=64,
                                         n_blocks=1, ngf=16, ndf=16, pixel_weight=10.0), "average")
    with pytest.raises(NotImplementedError, match="CycleGAN"):
        create_model(options.parse(yml, is_train=True), verbose=False)


def fs_recipe_edit(tree):
    """options/sr/train_sr.yml with its three commented fs lines switched on, nothing else changed."""
    tree["train"].update({"fs": True, "lpf_type": "average", "hpf_type": "average"})


def test_shipped_recipe_with_fs_steps_under_amp(tmp_path, monkeypatch):
    """The shipped recipe (RRDBNet-23, batch 8, crop 128, use_amp: true) with fs / lpf_type / hpf_type uncommented parses, constructs
    and steps once; every log entry is finite."""
    import test_gpu_step as TS
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml, _ = TS.shipped_recipe(tmp_path, monkeypatch)
    assert FX.write_recipe("sr/train_sr.yml", str(tmp_path), fs_recipe_edit) == yml
    opt = options.parse(yml, is_train=True)
    assert opt["use_amp"] is True and opt["train"]["fs"] is True
    torch.manual_seed(opt["train"]["manual_seed"])
    model = create_model(opt, verbose=False)
    assert model.f_low is not None and model.f_high is not None
    ds = opt["datasets"]["train"]
    LR, HR = detrand.synthetic_pair(ds["batch_size"], ds["crop_size"], 501)
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert set(log) >= {"pix-l1", "fea-vgg19-l1", "l_g_gan", "l_d_real", "l_d_fake"}
    assert all(v == v and abs(v) != float("inf") for v in log.values()), log
