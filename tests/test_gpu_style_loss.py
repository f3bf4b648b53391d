"""Style loss and multi-layer perceptual taps on the GPU (-m gpu): the Gram kernels (csrc/gram.hip) against the fp64 restatement of
tools/make_golden_style.py, the multi-tap FeatureExtractor against the fp64 run, and two engine steps against the reference's SRModel
(tests/golden/style_loss.pt).

Tolerances.  In the f32 arithmetic a value or gradient lies within 4 x the reference's own fp32-vs-fp64 deviation of the same quantity
(`e32_*` of the fixture): the project's factor for "a different, equally fp32, summation order".  In bf16x3 the rule of
test_gpu_kernels.py::test_bf16x3_split_operand_mode applies: error <= 1.5 x the f32 matrix-core path's on the same inputs + 2e-7 x the
output scale.  Every figure is printed before it is asserted.

The L1 kink on the Gram difference is handled in three parts, so that no element needs leaving out: (a) the Gram matrices the forward
produces, (b) the backward kernel on a GIVEN S, (c) the module's gradient bit-identical to (b) applied to the L1 kernel's own
gradient map of (a)."""
import os

import pytest
import torch

from oracle import fixtures as FX, ref_harness
from tools import make_golden_style as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLICE_CASE = (64, 5, 7, 2)          # also run as channels [64, 128) of a 128-channel buffer


@pytest.fixture(scope="module")
def fx():
    return FX.load("style_loss")


@pytest.fixture(scope="module")
def gram_refs():
    """fp64 restatement per Gram case, computed once: (x, S, G, dx)."""
    out = {}
    for case in T.GRAM_CASES:
        x, S = T.gram_inputs(case)
        out[case] = (x, S, T.gram(x.double()), T.gram_grad(x.double(), S.double()))
    return out


def _mods():
    from trainner_amd import hip, ops
    return hip, ops


def _nhwc(x, ctot=None, coff=0, fill=7.5):
    """logical NCHW fp32 -> device NHWC buffer [N, H, W, ctot] holding x at channels [coff, coff + C)."""
    N, C, H, W = x.shape
    buf = torch.full((N, H, W, ctot or C), fill, dtype=torch.float32, device=DEV)
    buf[..., coff:coff + C] = x.permute(0, 2, 3, 1).to(DEV)
    return buf


def _gram_fwd(ops, x, ctot=None, coff=0):
    N, C, H, W = x.shape
    G = torch.full((N, C, C), float("nan"), device=DEV)
    ops.gram_fwd(ops.View(_nhwc(x, ctot, coff), coff, C), 1.0 / (C * H * W), G)
    return G


def _gram_bwd(ops, x, S, ctot=None, coff=0, prefill=None):
    """-> dx as logical NCHW (CPU fp32) and the whole gradient buffer."""
    N, C, H, W = x.shape
    dbuf = torch.full((N, H, W, ctot or C), float("nan") if prefill is None else 0.0, device=DEV)
    if prefill is not None:
        dbuf[..., coff:coff + C] = prefill.permute(0, 2, 3, 1).to(DEV)
        if ctot:
            dbuf[..., :coff] = 3.25
            dbuf[..., coff + C:] = 3.25
    ops.gram_bwd(ops.View(_nhwc(x, ctot, coff), coff, C), S.to(DEV).contiguous(), 1.0 / (C * H * W), ops.View(dbuf, coff, C),
                 accumulate=prefill is not None)
    return dbuf[..., coff:coff + C].permute(0, 3, 1, 2).cpu(), dbuf


def _both_modes(monkeypatch, launch):
    """launch() in the f32 and in the bf16x3 arithmetic -> {mode: result}; the test's own mode is restored by monkeypatch."""
    hip, ops = _mods()
    out = {}
    for name, code in (("f32", hip.MMA_F32), ("bf16x3", hip.MMA_BF16X3)):
        monkeypatch.setattr(ops, "FP32_MMA", code)
        out[name] = launch()
    return out


def _check(what, mode, got, ref64, e32):
    """The tolerance rule of the module docstring for the test's arithmetic `mode`; got: {mode: tensor}; ref64: one fp64 tensor, or one
    per mode where the reference depends on the run (see test_multi_tap_extractor_against_fp64_run)."""
    refs = ref64 if isinstance(ref64, dict) else {m: ref64 for m in got}
    scale = refs[mode].abs().max().item()
    err = {m: (t.double().cpu() - refs[m]).abs().max().item() for m, t in got.items()}
    print("\n%s [%s]: err f32 %.3e bf16x3 %.3e | e32 %.3e (f32 / e32 = %.2f) | scale %.3e | bf16x3 bound %.3e" % (
        what, mode, err["f32"], err["bf16x3"], e32, err["f32"] / max(e32, 1e-300), scale, 1.5 * err["f32"] + 2e-7 * scale))
    if mode == "f32":
        assert err["f32"] <= 4 * e32, (what, err, e32)
    else:
        assert err["bf16x3"] <= 1.5 * err["f32"] + 2e-7 * scale, (what, err, scale)


@pytest.mark.parametrize("case", T.GRAM_CASES + ("slice",))
def test_gram_forward_and_backward_against_fp64_restatement(fx, gram_refs, case, mma_mode, monkeypatch):
    hip, ops = _mods()
    ctot, coff = (128, 64) if case == "slice" else (None, 0)
    case = SLICE_CASE if case == "slice" else case
    x, S, G64, dx64 = gram_refs[case]
    rec = fx["gram"][case]
    G = _both_modes(monkeypatch, lambda: _gram_fwd(ops, x, ctot, coff))
    monkeypatch.setattr(ops, "FP32_MMA", {"f32": hip.MMA_F32, "bf16x3": hip.MMA_BF16X3}[mma_mode])
    mine = G[mma_mode]
    assert torch.equal(mine, mine.transpose(1, 2)), "G is not bit-exactly symmetric"
    assert torch.equal(mine, _gram_fwd(ops, x, ctot, coff)), "two runs differ"
    _check("G %s" % (case,), mma_mode, G, G64, rec["e32_G"])

    dx = _both_modes(monkeypatch, lambda: _gram_bwd(ops, x, S, ctot, coff)[0])
    _check("dx %s" % (case,), mma_mode, dx, dx64, rec["e32_dx"])
    monkeypatch.setattr(ops, "FP32_MMA", {"f32": hip.MMA_F32, "bf16x3": hip.MMA_BF16X3}[mma_mode])
    plain, _ = _gram_bwd(ops, x, S, ctot, coff)
    assert torch.equal(plain, dx[mma_mode]), "two runs differ"
    # accumulate: the pre-filled values survive -- exactly one fp32 addition per element on top of the plain result
    pre = T.seeded(tuple(x.shape), 9901) * rec["dx_absmax"]
    acc, dbuf = _gram_bwd(ops, x, S, ctot, coff, prefill=pre)
    assert torch.equal(acc, plain + pre)
    if ctot:
        assert (dbuf[..., :coff] == 3.25).all() and (dbuf[..., coff + x.shape[1]:] == 3.25).all(), "wrote outside the channel slice"


def test_gram_backward_does_not_assume_a_symmetric_s(gram_refs, mma_mode):
    """S and S^T give the same gradient bit for bit (the stager forms S + S^T), and an antisymmetric S gives exactly zero."""
    hip, ops = _mods()
    x, S, _, _ = gram_refs[(128, 16, 16, 2)]
    a, _ = _gram_bwd(ops, x, S)
    b, _ = _gram_bwd(ops, x, S.transpose(1, 2).contiguous())
    assert torch.equal(a, b)
    z, _ = _gram_bwd(ops, x, S - S.transpose(1, 2))
    assert (z == 0).all()


def test_style_module_gradient_is_the_backward_kernel_on_the_l1_map(fx, gram_refs, mma_mode, monkeypatch):
    """Parts (a) and (c) of the kink handling, through _GramFn and the L1 criterion as PerceptualLoss uses them."""
    hip, ops = _mods()
    from trainner_amd.models import losses as L
    case = (128, 16, 16, 2)
    x, _, G64, _ = gram_refs[case]
    y = T.seeded(tuple(x.shape), 9917)
    N, C, H, W = x.shape
    fx_ = _nhwc(x).permute(0, 3, 1, 2).requires_grad_(True)           # logical NCHW over NHWC storage, like a FeatureExtractor tap
    fy_ = _nhwc(y).permute(0, 3, 1, 2)
    gx = L._GramFn.apply(fx_)
    with torch.no_grad():
        gy = L._GramFn.apply(fy_)
    # (a)
    both = _both_modes(monkeypatch, lambda: L._GramFn.apply(fx_.detach()))
    monkeypatch.setattr(ops, "FP32_MMA", {"f32": hip.MMA_F32, "bf16x3": hip.MMA_BF16X3}[mma_mode])
    assert torch.equal(both[mma_mode], gx.detach())
    _check("G via _GramFn", mma_mode, both, G64, fx["gram"][case]["e32_G"])
    loss = L.L1Loss()(gx, gy) * 3.0
    loss.backward()
    # (c): S = the L1 kernel's own gradient map of (a) at the incoming scale 3, then the backward kernel
    S = torch.empty_like(gx)
    ops.l1_mean_bwd(gx.detach(), gy, 1.0, torch.full((1,), 3.0, device=DEV), S)
    assert S.abs().max().item() > 0
    want = torch.empty((N, H, W, C), device=DEV)
    ops.gram_bwd(ops.View(fx_.detach().permute(0, 2, 3, 1)), S, 1.0 / (C * H * W), ops.View(want))
    assert torch.equal(fx_.grad.permute(0, 2, 3, 1), want)
    ref = (T.gram(x.double()) - T.gram(y.double())).abs().mean().item() * 3.0
    print("\nstyle L1: engine %.9g fp64 %.9g" % (loss.item(), ref))
    assert abs(loss.item() - ref) <= 1e-5 * ref


# ------------------------------------------------------------------------------------------------ multi-tap extractor
def _engine_extractor(taps, keys, seed=T.VGG_FILL_SEED):
    from trainner_amd.models.modules.architectures.perceptual import FeatureExtractor
    net = FeatureExtractor(listen_list=list(taps), allow_random_init=True)
    sd = net.state_dict()
    sd.update({k: v for k, v in FX.initial_state(keys, seed, gain=1.0, bias_amp=0.05).items() if k in sd})      # a shorter network owns fewer
    net.load_state_dict(sd)
    return net.to(DEV)


@pytest.fixture(scope="module")
def extractor_refs(fx):
    """fp64 restatement per extractor case, computed once: (x, feats, maps, input gradient)."""
    sd = FX.initial_state(fx["extractor_keys"], T.VGG_FILL_SEED, gain=1.0, bias_amp=0.05)
    out = {}
    for name in T.EXTRACTOR_CASES:
        x, _ = T.extractor_inputs(name)
        xx = x.double().requires_grad_(True)
        feats = T.extract(xx, sd, T.TAPS)
        maps = T.tap_maps(feats)
        sum((feats[k] * maps[k].double()).sum() for k in feats).backward()
        out[name] = (x, {k: v.detach() for k, v in feats.items()}, maps, xx.grad.detach())
    return out


def _relu_layers(taps):
    """The convolutions of the truncated network that a ReLU follows."""
    from trainner_amd.models.modules.architectures.perceptual import vgg_layer_names
    names = vgg_layer_names("vgg19")
    names = names[:max(names.index(t) for t in taps) + 1]
    return [n for i, n in enumerate(names) if n.startswith("conv") and i + 1 < len(names)]


def _grad_under_pattern(x, sd, maps, pattern):
    """fp64 input gradient of sum_k sum(fea_k * m_k) with every ReLU's derivative taken from `pattern` (conv name -> bool map of the
    units that pass) instead of from the fp64 pre-activation: T.extract with relu(v) written as v * pattern."""
    import torch.nn.functional as F
    from trainner_amd.models.modules.architectures.perceptual import vgg_layer_names
    xx = x.double().requires_grad_(True)
    mean = torch.tensor([0.485, 0.456, 0.406]).double().view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).double().view(1, 3, 1, 1)
    v, total, last = (xx - mean) / std, 0.0, None
    names = vgg_layer_names("vgg19")
    for n in names[:max(names.index(t) for t in T.TAPS) + 1]:
        if n.startswith("conv"):
            v, last = F.conv2d(v, sd["feature_net.%s.weight" % n].double(), sd["feature_net.%s.bias" % n].double(), padding=1), n
        elif n.startswith("relu"):
            v = v * pattern[last].double()
        else:
            v = F.max_pool2d(v, 2, 2)
        if n in T.TAPS:
            total = total + (v * maps[n].double()).sum()
    total.backward()
    return xx.grad.detach()


@pytest.mark.parametrize("name", sorted(T.EXTRACTOR_CASES))
def test_multi_tap_extractor_against_fp64_run(fx, extractor_refs, name, mma_mode, monkeypatch):
    """Every tap and the input gradient of the seeded linear functional of all taps, and no convolution launched twice.

    The ReLU kinks are handled like the L1 kink above, in three parts, so that no element needs leaving out.  An input gradient is
    only defined up to the sign of every ReLU input, and among the ~5e5 ReLU inputs of a case some lie closer to zero than any fp32
    evaluation resolves (b2_32: one conv1_1 unit at 2.5e-8, three conv2_2 units below 4e-5): a run that rounds such a unit to the
    other side has, correctly, another gradient (1.4 on a scale of 100 for that one conv1_1 unit).  So
      (a) every tap against the fp64 run;
      (b) the run's own ReLU pattern -- read from an extractor that listens to every convolution, same weights, input and
          arithmetic -- differs from the fp64 pattern only at units whose fp64 input lies within 4 x e32 of zero, e32 = the
          largest fp32-vs-fp64 deviation of the case's taps (the deepest tap's: the deviation grows with depth);
      (c) the input gradient against the fp64 gradient UNDER THAT PATTERN, with the bounds of the module docstring."""
    hip, ops = _mods()
    x, feats64, maps, grad64 = extractor_refs[name]
    rec = fx["extractor"][name]
    sd = FX.initial_state(fx["extractor_keys"], T.VGG_FILL_SEED, gain=1.0, bias_amp=0.05)
    net = _engine_extractor(T.TAPS, fx["extractor_keys"])
    relu_layers = _relu_layers(T.TAPS)
    probe_net = _engine_extractor(relu_layers, fx["extractor_keys"])
    pre64 = T.extract(x.double(), sd, relu_layers)
    launches = []
    from trainner_amd.engine import ConvOp
    orig = ConvOp.fwd
    counted = lambda self, *a, **k: (launches.append(1), orig(self, *a, **k))[1]      # noqa: E731

    def run():
        monkeypatch.setattr(ops, "MMA", ops.FP32_MMA)              # the convolutions follow the arithmetic under test
        monkeypatch.setattr(ConvOp, "fwd", counted)
        xd = x.to(DEV).requires_grad_(True)
        feats = net(xd)
        sum((feats[k] * maps[k].to(DEV)).sum() for k in feats).backward()
        monkeypatch.setattr(ConvOp, "fwd", orig)
        with torch.no_grad():
            pattern = {k: (v > 0).cpu() for k, v in probe_net(x.to(DEV)).items()}
        return feats, xd.grad, pattern

    res = _both_modes(monkeypatch, run)
    n_convs = sum(1 for n in net.names if n.startswith("conv"))
    assert len(launches) == 2 * n_convs, "a convolution was launched twice"
    assert list(res[mma_mode][0]) == list(T.TAPS)
    # (a)
    for k in T.TAPS:
        assert tuple(res[mma_mode][0][k].shape) == rec["taps"][k]["shape"]
        _check("%s %s" % (name, k), mma_mode, {m: r[0][k].detach() for m, r in res.items()}, feats64[k], rec["taps"][k]["e32"])
    # (b)
    e32 = max(rec["taps"][k]["e32"] for k in T.TAPS)
    for m, r in res.items():
        for k in relu_layers:
            flipped = r[2][k] != (pre64[k] > 0)
            worst = pre64[k][flipped].abs().max().item() if flipped.any() else 0.0
            print("%s [%s] %s: %d of %d ReLU inputs on the other side, the farthest at %.3e (4 x e32 = %.3e)" % (
                name, m, k, int(flipped.sum()), flipped.numel(), worst, 4 * e32))
            assert worst <= 4 * e32, (name, m, k, worst)
    # (c)
    refs = {m: _grad_under_pattern(x, sd, maps, r[2]) for m, r in res.items()}
    print("%s: fp64 gradient under the run's pattern vs under its own: f32 %.3e bf16x3 %.3e" % (
        name, (refs["f32"] - grad64).abs().max().item(), (refs["bf16x3"] - grad64).abs().max().item()))
    _check("%s input gradient" % name, mma_mode, {m: r[1] for m, r in res.items()}, refs, rec["e32_grad"])


def test_absent_tap_gradients_are_skipped(fx, mma_mode):
    """A functional of ONE mid-network tap: the layers above it run no backward, and the gradient equals that of an extractor
    that listens to this tap alone, bit for bit."""
    x, _ = T.extractor_inputs("b2_32")
    m = T.seeded((2, 128, 16, 16), 9931).to(DEV)
    grads = []
    for taps in (T.TAPS, ("relu2_2",)):
        net = _engine_extractor(taps, [k for k in fx["extractor_keys"] if taps == T.TAPS or int(k[0].split("conv")[1][0]) <= 2])
        xd = x.to(DEV).requires_grad_(True)
        (net(xd)["relu2_2"] * m).sum().backward()
        grads.append(xd.grad)
    assert torch.equal(grads[0], grads[1])


def test_single_conv5_4_tap_is_bit_identical_to_the_single_output_node(mma_mode):
    """One conv tap that is also the last layer keeps its single-output node; the multi-tap sweep on the same network gives the same
    bits, output and input gradient."""
    from trainner_amd.models.modules.architectures.perceptual import FeatureExtractor
    net = FeatureExtractor(listen_list=["conv5_4"], allow_random_init=True)
    assert net._single
    keys = [(k, tuple(v.shape)) for k, v in net.state_dict().items() if k.startswith("feature_net")]
    sd = net.state_dict()
    sd.update(FX.initial_state(keys, T.VGG_FILL_SEED, gain=1.0, bias_amp=0.05))
    net.load_state_dict(sd)
    net = net.to(DEV)
    x, _ = T.extractor_inputs("b2_32")
    m = T.seeded((2, 512, 2, 2), 9941).to(DEV)
    out = []
    for single in (True, False):
        net._single = single
        xd = x.to(DEV).requires_grad_(True)
        f = net(xd)
        assert list(f) == ["conv5_4"]
        (f["conv5_4"] * m).sum().backward()
        out.append((f["conv5_4"].detach().clone(), xd.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------------------ the step record
def _engine_sr_model(fxs, tmp_path):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = ref_harness.esrgan_yaml(name="engine_style", out_root=str(tmp_path), gpu_ids="[0]", **fxs["spec"]["yaml"])
    T.style_yaml(yml, fxs["extra"])
    opt = options.parse(yml, is_train=True)
    model = create_model(opt, verbose=False)
    g, d, f = FX.initial_states(fxs)
    model.netG.load_state_dict(g)
    model.netD.load_state_dict(d)
    netF = [l["function"].network for l in model.generatorlosses.loss_list if "fea" in l["name"]][0]
    sd = netF.state_dict()
    sd.update(f)
    netF.load_state_dict(sd)
    return model, netF


def test_sr_step_with_style_and_multi_layer_taps_matches_reference_record(fx, tmp_path, mma_mode):
    """create_model -> feed_data -> optimize_parameters -> get_current_log with style_weight and a multi-layer perceptual_opt against the
    real reference's SRModel, two steps, with the bounds tests/test_gpu_step.py uses."""
    import test_gpu_step as TS
    fxs = fx["steps"]["style"]
    tol = TS.DEFAULT_TOL
    model, netF = _engine_sr_model(fxs, tmp_path)
    assert [l["name"] for l in model.generatorlosses.loss_list] == fxs["loss_names"]
    assert netF.taps == ["conv1_2", "relu2_2", "conv3_4", "relu4_2", "conv5_4"]
    for (s, (LR, HR)), ref_log in zip(FX.batches(fxs), fxs["logs"]):
        model.feed_data({"LR": LR, "HR": HR})
        model.optimize_parameters(s)
        log = model.get_current_log()
        print("\nstep", s, {k: (round(log[k], 7), round(v, 7)) for k, v in ref_log.items()})
        assert "fea-vgg19-l1" in log
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
