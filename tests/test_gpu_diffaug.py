"""DiffAugment on the device (-m gpu): csrc/diffaug.hip through the C ABI (ops.diffaug_*), dataops/diffaug.py and the models' wiring,
against tests/golden/diffaug.pt (the REAL reference's runs, tools/make_golden_diffaug.py) and the tool's fp64 restatement, which the
tool pinned to the reference to 1e-12 and tests/test_cpu_diffaug.py pins to the fixture again.

Tolerances are measured on the reference, never on the engine (e32_out / e32_grad are the reference's own fp32-vs-fp64 deviations
with the same draws), and every ratio is printed before it is asserted (`pytest -s`):
    output    max error <= max(4 x e32_out, 4 fp32 ulps of the largest output)
    gradient  max error <= max(4 x e32_grad, 4 fp32 ulps of the largest gradient)
Nothing is left out of either comparison.  A ratio above 1 is a cause to be found, not a factor to raise.
"""
import os

import pytest
import torch

from oracle import detrand, fixtures as FX, ref_harness
from tools import make_golden_diffaug as T
from trainner_amd.dataops import diffaug as ED

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diffaug.pt")
OPS = ("diffaug_mean", "diffaug_fwd", "diffaug_bwd")
EPS = torch.finfo(torch.float32).eps


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


def to_dev(t, layout):
    return t.to(DEV).contiguous(memory_format=torch.channels_last if layout == "cl" else torch.contiguous_format)


def ulp32(v):
    return EPS * 2.0 ** torch.tensor(max(v, 1e-30)).log2().floor().item()


def engine_run(x, prm, policy, m, layout):
    """-> (out, d sum(out * m) / dx) as device tensors in the input's layout."""
    xd, md = to_dev(x, layout).requires_grad_(True), to_dev(m, layout)
    out = ED.DiffAugment(xd, policy, params=prm)
    assert out.dtype == torch.float32 and out.stride() == xd.stride() and out.data_ptr() != xd.data_ptr()
    out.backward(md)
    assert xd.grad.stride() == xd.stride()
    return out.detach(), xd.grad.detach()


def host64(t):
    return t.cpu().contiguous().double()


_REFERENCE = {}


def reference(fx, case, name):
    """(x, m, parameters, fp64 restatement of output and gradient), computed once per case and set and shared by the tests."""
    key = (case, name)
    if key not in _REFERENCE:
        t = fx["cases"][case]["sets"][name]
        x = T.make_input(case)
        m = T.seeded_map(tuple(x.shape))
        prm = T.params_from_tape(t["policy"], t["tape"], tuple(x.shape))
        _REFERENCE[key] = (x, m, prm) + T.restate_with_grad(x, prm, m)
    return _REFERENCE[key]


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("case", list(T.CASES))
def test_golden_forward_and_gradient(fx, case, layout):
    rec = fx["cases"][case]
    failures = []
    for name, t in rec["sets"].items():
        x, m, prm, oref, gref = reference(fx, case, name)
        assert T.probe_error(oref, t["out"])[0] <= 1e-12 and T.probe_error(gref, t["grad"])[0] <= 1e-12
        out, grad = engine_run(x, prm, t["policy"], m, layout)
        eo, bo = (host64(out) - oref).abs().max().item(), max(4 * t["e32_out"], 4 * ulp32(t["out_absmax"]))
        eg, bg = (host64(grad) - gref).abs().max().item(), max(4 * t["e32_grad"], 4 * ulp32(t["grad_absmax"]))
        line = "%s %s %s: out err %.3e (bound %.3e, ratio %.3f)  grad err %.3e (bound %.3e, ratio %.3f)" % (
            case, name, layout, eo, bo, eo / bo, eg, bg, eg / bg)
        print("\n" + line, end="")
        if not (eo <= bo and eg <= bg):          # also false for a NaN
            failures.append(line)
    assert not failures, failures


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("case", list(T.CASES))
def test_policies_without_colour_and_zoom_are_copies_bit_for_bit(fx, case, layout):
    """Translation, flip, rotation and cutout move and zero values: output and gradient equal the restatement exactly."""
    seen = 0
    for name, t in fx["cases"][case]["sets"].items():
        if "color" in t["policy"] or t["kind"] in ("zoom_in", "zoom_out"):
            continue
        x, m, prm, oref, gref = reference(fx, case, name)
        out, grad = engine_run(x, prm, t["policy"], m, layout)
        assert torch.equal(host64(out), oref) and torch.equal(host64(grad), gref), name
        seen += 1
    assert seen >= 9, seen


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("name", ["transl-max", "zoomin-hi-last", "zoomin-lo-first", "zoomout-lo-neg", "zoomout-hi-pos", "cutout-corners-a",
                                  "rotate-plus", "rotate-minus", "flip-on", "recipe-zoom_in", "recipe-zoom_out", "recipe-translation"])
def test_adjoint_identity(fx, name, layout):
    """<A x, m> = <x, A^T m> for the linear part A = mask . Geo . (the linear part of Colour): both sides from the engine, summed in fp64.
    Rounding: a zoom output is at most four products and three sums (7 roundings <= eps32 max|v| each, the weights sum to 1); the
    colour map adds at most 8 more per element (two subtractions, two products, two sums, the channel mean and the image mean) on
    values <= (1 + sat) (1 + con) max|x| <= 7.5 max|x|; the adjoint's sums have the same terms.  The elements' roundings are
    independent and add like a random walk over the n elements (sqrt(n)), weighted by max|m|; once for each side."""
    case = "tiles"
    t = fx["cases"][case]["sets"][name]
    x, m, prm, _, _ = reference(fx, case, name)
    xd, md = to_dev(x, layout), to_dev(m, layout)
    zero = torch.zeros_like(xd).requires_grad_(True)
    A0 = ED.DiffAugment(zero, t["policy"], params=prm)          # the affine map's constant (brightness)
    A0.backward(md)
    Atm = zero.grad
    Ax = ED.DiffAugment(xd, t["policy"], params=prm) - A0
    a, b = (Ax.double() * md.double()).sum().item(), (xd.double() * Atm.double()).sum().item()
    roundings = (7 if t["kind"].startswith("zoom") else 0) + (8 if prm.color is not None else 0) + 1
    amp = 7.5 if prm.color is not None else 1.0
    bound = 2 * roundings * EPS * amp * x.abs().max().item() * m.abs().max().item() * x.numel() ** 0.5
    print("\n%s %s: <Ax, m> %.9e  <x, Atm> %.9e  diff %.3e (bound %.3e)" % (name, layout, a, b, abs(a - b), bound), end="")
    assert abs(a - b) <= bound and a != 0.0


@pytest.mark.parametrize("layout", ["nchw", "cl"])
def test_two_runs_are_bit_identical(fx, layout):
    for case in ("tiles", "odd33"):
        for name in ("seeded-recipe", "recipe-zoom_in", "recipe-zoom_out", "recipe-translation", "seeded-color"):
            x, m, prm, _, _ = reference(fx, case, name)
            policy = fx["cases"][case]["sets"][name]["policy"]
            o1, g1 = engine_run(x, prm, policy, m, layout)
            o2, g2 = engine_run(x, prm, policy, m, layout)
            assert torch.isfinite(o1).all() and torch.isfinite(g1).all()
            assert torch.equal(o1, o2) and torch.equal(g1, g2), (case, name)


def test_unaligned_nchw_view_agrees_bit_for_bit(fx):
    """An NCHW view one, two or three floats off 16-byte alignment (W a multiple of 4) gives the bits of the aligned run."""
    from trainner_amd import ops

    def shifted(t, off):
        buf = torch.full((t.numel() + 8,), float("nan"), device=DEV)
        v = buf[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    for name in ("recipe-translation", "recipe-zoom_in", "recipe-zoom_out"):
        x, m, prm, _, _ = reference(fx, "sq32", name)
        geo, blk = prm.geo(), prm.block(DEV)

        def run(off):
            xs, ms = shifted(x.to(DEV), off), shifted(m.to(DEV), off)
            assert xs.is_contiguous() and (xs.data_ptr() % 16 == 0) == (off % 4 == 0)
            out, gx = shifted(torch.zeros_like(xs), off), shifted(torch.zeros_like(xs), off)
            ops.diffaug_fwd(xs, 0, blk, geo, ops.diffaug_mean(xs, 0, blk, geo), out)
            ops.diffaug_bwd(ms, 0, blk, geo, ops.diffaug_mean(ms, 0, blk, geo, backward=True), gx)
            return out.clone(), gx.clone()

        aligned = run(0)
        for off in (1, 2, 3):
            for a, b in zip(aligned, run(off)):
                assert torch.isfinite(b).all() and torch.equal(a, b), (name, off)


@pytest.mark.parametrize("layout", ["nchw", "cl"])
def test_a_nan_pixel_reaches_exactly_the_outputs_that_read_it(fx, layout):
    """Without `color` the NaN shows where the restatement (plain torch: a weight of 0 or a mask of 0 times NaN is NaN, a gathered zero
    is not) shows it and nowhere else; with `color` the whole image is NaN through the contrast mean, as in torch, and the other images
    stay finite."""
    case = "sq32"
    for name in ("transl-max", "zoomin-hi-last", "zoomin-lo-first", "zoomout-lo-neg", "cutout-corners-a", "rotate-plus", "flip-on",
                 "seeded-recipe", "seeded-color"):
        t = fx["cases"][case]["sets"][name]
        x, m, prm, _, _ = reference(fx, case, name)
        x = x.clone()
        x[1, 1, 20, 20] = float("nan")
        want = torch.isnan(T.restate(x, prm))          # in fp32: the taps the kernel's fp32 index arithmetic names
        out = ED.DiffAugment(to_dev(x, layout), t["policy"], params=prm)
        got = torch.isnan(out).cpu()
        assert torch.equal(got, want), (name, int(got.sum()), int(want.sum()))
        assert not got[0].any() and not got[2].any()
        if name == "seeded-color":
            assert got[1].all()
        elif "color" in t["policy"]:          # everything but the zero padding of the geometric map
            assert int(got[1].sum()) >= got[1].numel() // 4
        elif name != "cutout-corners-a":
            assert 1 <= int(got.sum()) <= 25, (name, int(got.sum()))


def test_half_inputs_are_promoted_and_channels_last_is_kept(fx):
    x, m, prm, oref, _ = reference(fx, "sq32", "seeded-recipe")
    policy = fx["cases"]["sq32"]["sets"]["seeded-recipe"]["policy"]
    for dt in (torch.float16, torch.bfloat16):
        xh = x.to(DEV).to(dt)
        out = ED.DiffAugment(xh, policy, params=prm)
        assert out.dtype == torch.float32
        assert torch.equal(out, ED.DiffAugment(xh.float(), policy, params=prm))
    out = ED.DiffAugment(to_dev(x, "cl"), policy, params=prm)
    assert out.is_contiguous(memory_format=torch.channels_last)
    # a fresh draw on the device: finite, new storage, and no host synchronisation is needed to build the parameter block
    out = ED.DiffAugment(x.to(DEV), policy)
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ the models
def _replay_draws(monkeypatch, calls):
    """`draw` replaced by the recorded sequence: call i gets the reference's draws of its call i (shape and policy checked)."""
    queue, real = list(calls), ED.draw

    def draw(policy, N, H, W, device):
        c = queue.pop(0)
        assert c["policy"] == policy and (c["shape"][0], c["shape"][2], c["shape"][3]) == (N, H, W), (c["shape"], policy)
        tape = T.Tape(replay=c["tape"])
        with tape.on(ED):
            prm = real(policy, N, H, W, "cpu")
        assert not tape.replay
        return prm

    monkeypatch.setattr(ED, "draw", draw)
    return queue


def _engine_sr_model(fxs, tmp_path, diffaug=True, name="engine_diffaug"):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = ref_harness.esrgan_yaml(name=name, out_root=str(tmp_path), gpu_ids="[0]", **fxs["spec"]["yaml"])
    if diffaug:
        T.diffaug_yaml(yml, fxs["policy"])
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


def test_sr_step_matches_reference_record(fx, tmp_path, monkeypatch):
    """optimize_parameters with diffaug: true and the recipe's dapolicy against the real reference's SRModel, two steps, replaying the
    reference's draws of its eight DiffAugment calls, with the bounds tests/test_gpu_step.py uses."""
    import test_gpu_step as TS
    fxs = fx["steps"]["sr"]
    tol = TS.DEFAULT_TOL
    model = _engine_sr_model(fxs, tmp_path)
    assert model.adversarial.diffaug and model.adversarial.dapolicy == T.RECIPE
    assert [l["name"] for l in model.generatorlosses.loss_list] == fxs["loss_names"]
    queue = _replay_draws(monkeypatch, fxs["calls"])
    for (s, (LR, HR)), ref_log in zip(FX.batches(fxs), fxs["logs"]):
        model.feed_data({"LR": LR, "HR": HR})
        model.optimize_parameters(s)
        log = model.get_current_log()
        print("\nstep", s, {k: (round(log[k], 7), round(v, 7)) for k, v in ref_log.items()})
        TS.check_logs(log, ref_log, tol=tol["log"])
    assert queue == []          # eight calls, no more and no fewer
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


def test_pix2pix_step_matches_reference_record(fx, tmp_path, monkeypatch):
    """Pix2Pix with diffaug: true (conditional D: the augmentation comes before the concatenation with the condition, which is not
    augmented; the standard form's generator stage has no real image: three calls per step), with the bounds of
    tests/test_gpu_i2i.py::test_i2i_step_matches_reference_golden."""
    import test_gpu_i2i as TI
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    fxs = fx["steps"]["pix2pix"]
    yml = T.diffaug_yaml(ref_harness.i2i_yaml(name="engine_diffaug_i2i", out_root=str(tmp_path), gpu_ids="[0]", **fxs["spec"]["yaml"]),
                         fxs["policy"])
    opt = options.parse(yml, is_train=True)
    model = create_model(opt, verbose=False)
    for n, sd in FX.i2i_initial_states(fxs).items():
        getattr(model, "net" + n).load_state_dict(sd)
    assert dict(opt["network_G"]) == fxs["network_G"] and dict(opt["network_D"]) == fxs["network_D"]
    assert list(model.model_names) == fxs["model_names"] and model.adversarial.diffaug
    queue = _replay_draws(monkeypatch, fxs["calls"])
    for (s, (A, B)), ref_log in zip(FX.i2i_batches(fxs), fxs["logs"]):
        model.feed_data({"A": A, "B": B, "A_path": ["a"] * A.shape[0]})
        model.optimize_parameters(s)
        log = model.get_current_log()
        print("\nstep", s, {k: (round(log[k], 7), round(v, 7)) for k, v in ref_log.items()})
        TI.check_logs(log, ref_log, 2e-4 if s < 2 else 3e-3)
        if s == 1:
            diff = (model.fake_B.detach().cpu() - fxs["images_step1"]["fake_B"]).abs()
            assert diff.mean().item() <= 2e-5 and diff.max().item() <= 5e-4, (diff.mean().item(), diff.max().item())
    assert queue == []
    diff = (model.fake_B.detach().cpu() - fxs["images"]["fake_B"]).abs()
    assert diff.mean().item() <= 1e-2 and diff.max().item() <= 1e-1, (diff.mean().item(), diff.max().item())
    lr_steps = 2e-4 * fxs["spec"]["steps"]
    for n in fxs["model_names"]:
        sd = {k: v.detach().cpu() for k, v in getattr(model, "net" + n).state_dict().items()}
        skip = FX.norm_shadowed_biases(fxs["keys"][n], fxs["network_G"]["norm_type"]) if n.startswith("G") else ()
        worst, mean, k = FX.state_error(sd, fxs["states"][n], skip, lr_steps=lr_steps)
        assert mean < 0.15 and worst < 2.05, (n, k, worst, mean)


def _count_ops(monkeypatch):
    """Records every new op as "<name>@fwd" or "<name>@bwd" (the phase from the autograd function's backward)."""
    from trainner_amd import ops
    calls, phase = [], ["fwd"]
    for n in OPS:
        real = getattr(ops, n)
        monkeypatch.setattr(ops, n, lambda *a, _real=real, _n=n, **k: (calls.append(_n + "@" + phase[0]), _real(*a, **k))[1])

    def backward(ctx, g, _real=ED._DiffAugFn.backward):
        phase[0] = "bwd"
        try:
            return _real(ctx, g)
        finally:
            phase[0] = "fwd"
    monkeypatch.setattr(ED._DiffAugFn, "backward", staticmethod(backward))
    return calls


def test_launch_counts_of_a_full_step(fx, tmp_path, monkeypatch):
    """Without diffaug none of the new ops runs.  With the recipe policy a step issues four forward applications (fake and real in each
    stage) and ONE backward (the generator stage's fake: real is under no_grad there, the discriminator stage feeds detached inputs);
    each application is one reduction and one fused launch: the two-launch budget."""
    calls = _count_ops(monkeypatch)
    fxs = fx["steps"]["sr"]
    batches = list(FX.batches(fxs))
    plain = _engine_sr_model(fxs, tmp_path / "plain", diffaug=False)
    assert not plain.adversarial.diffaug
    for s, (LR, HR) in batches:
        plain.feed_data({"LR": LR, "HR": HR})
        plain.optimize_parameters(s)
    plain.get_current_log()
    assert calls == []
    model = _engine_sr_model(fxs, tmp_path / "da")
    for s, (LR, HR) in batches:
        del calls[:]
        model.feed_data({"LR": LR, "HR": HR})
        model.optimize_parameters(s)
        assert sorted(calls) == ["diffaug_bwd@bwd"] + ["diffaug_fwd@fwd"] * 4 + ["diffaug_mean@bwd"] + ["diffaug_mean@fwd"] * 4, calls
        # every application: the reduction, then the fused launch
        fwd = [c for c in calls if c.endswith("@fwd")]
        assert fwd == ["diffaug_mean@fwd", "diffaug_fwd@fwd"] * 4
        assert [c for c in calls if c.endswith("@bwd")] == ["diffaug_mean@bwd", "diffaug_bwd@bwd"]
    log = model.get_current_log()
    assert all(v == v and abs(v) != float("inf") for v in log.values()), log


def test_policy_without_colour_is_one_launch_each_way(fx, monkeypatch):
    calls = _count_ops(monkeypatch)
    x, m, prm, _, _ = reference(fx, "sq32", "transl-max")
    engine_run(x, prm, "translation", m, "nchw")
    assert calls == ["diffaug_fwd@fwd", "diffaug_bwd@bwd"]


def diffaug_recipe_edit(tree):
    """The shipped recipe with its two commented DiffAugment lines switched on, nothing else changed."""
    tree["train"].update({"diffaug": True, "dapolicy": "color,transl_zoom,flip,rotate,cutout"})


def test_shipped_recipe_with_diffaug_steps_under_amp(tmp_path, monkeypatch):
    """The shipped SR recipe (RRDBNet-23, batch 8, crop 128, use_amp: true) with diffaug / dapolicy uncommented parses, constructs and
    steps once; every log entry is finite."""
    import test_gpu_step as TS
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml, _ = TS.shipped_recipe(tmp_path, monkeypatch)
    assert FX.write_recipe("sr/train_sr.yml", str(tmp_path), diffaug_recipe_edit) == yml
    opt = options.parse(yml, is_train=True)
    assert opt["use_amp"] is True and opt["train"]["diffaug"] is True
    torch.manual_seed(opt["train"]["manual_seed"])
    model = create_model(opt, verbose=False)
    assert model.adversarial.diffaug and model.adversarial.dapolicy == "color,transl_zoom,flip,rotate,cutout"
    ds = opt["datasets"]["train"]
    LR, HR = detrand.synthetic_pair(ds["batch_size"], ds["crop_size"], 501)
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert set(log) >= {"pix-l1", "fea-vgg19-l1", "l_g_gan", "l_d_real", "l_d_fake"}
    assert all(v == v and abs(v) != float("inf") for v in log.values()), log


@pytest.mark.parametrize("recipe", ["i2i/train_pix2pix.yml", "i2i/train_cyclegan.yml"])
def test_shipped_i2i_recipes_construct_with_diffaug(recipe, tmp_path):
    """options/i2i/train_pix2pix.yml and train_cyclegan.yml with the two lines uncommented parse and construct."""
    import test_gpu_i2i as TI
    opt, model, _ = TI._shipped_i2i_recipe(tmp_path, recipe, diffaug_recipe_edit)
    assert opt["train"]["diffaug"] is True
    assert model.adversarial.diffaug and model.adversarial.dapolicy == "color,transl_zoom,flip,rotate,cutout"
