"""Contextual loss on the GPU (-m gpu): the kernels of csrc/contextual.hip against the fp64 restatements of
tools/make_golden_contextual.py, the Contextual_Loss module against the reference's fixture and two engine steps against the reference's
SRModel (tests/golden/contextual.pt).

Tolerances: the rule of tests/test_gpu_style_loss.py.  In the f32 arithmetic a quantity lies within 4 x the reference's own fp32-vs-fp64
deviation of the same quantity (`e32_*` of the fixture; never less than half an fp32 ulp of the quantity, see the tool's e32); in bf16x3
error <= 1.5 x the f32 run's error on the same inputs + 2e-7 x the output scale.  Every figure is printed before it is asserted.

The loss has three kinds of kink -- the column argmax, the row argmin, the clamp of d at 0 -- handled in three parts so that no element
needs leaving out: (a) the forward quantities d, row minima, column maxima, CS and the loss against fp64; (b) the run's own argmax /
argmin arrays, which the ops return, differ from the fp64 ones only where fp64's gap between the run's choice and the extremum is within
4 x e32 of that quantity; (c) dX against the fp64 gradient UNDER THE RUN'S PATTERN (tools.make_golden_contextual.grad_under_pattern).

One kernel case departs from the fixture's gradient floor max|dX| >= 1e-4: (512, 24, 24, 2, uncorrelated) has max|dX| = 7.0e-5 for
every seed, because the normalisation's backward divides by ||X - mu|| ~ 13 at C = 512 (tools/make_golden_contextual.py GRAD_FLOOR)."""
import math

import pytest
import torch

from oracle import fixtures as FX, ref_harness
from tools import make_golden_contextual as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLICE_CASE = T.KERNEL_CASES[1]          # also run as channels [64, 128) of a 128-channel buffer
SENTINEL = 3.25


@pytest.fixture(scope="module")
def fx():
    return FX.load("contextual")


@pytest.fixture(scope="module")
def refs(fx):
    """fp64 restatement per case, computed once: (X, Y, idx, forward quantities, gradient)."""
    out = {}
    for case in T.KERNEL_CASES + (T.POOLED_CASE,):
        rec = fx["cases"][case]
        X, Y = T.case_inputs(case, rec["seed"])
        idx = (rec["idx_x"], rec["idx_y"]) if case == T.POOLED_CASE else None
        f, g = T.own_gradient(X.double(), Y.double(), *(idx or (None, None)))
        out[case] = (X, Y, idx, f, g)
    return out


def _mods():
    from trainner_amd import hip, ops
    return hip, ops


def _nhwc(x, ctot=None, coff=0, fill=7.5):
    N, C, H, W = x.shape
    buf = torch.full((N, H, W, ctot or C), fill, dtype=torch.float32, device=DEV)
    buf[..., coff:coff + C] = x.permute(0, 2, 3, 1).to(DEV)
    return buf


def _run(ops, X, Y, ctot=None, coff=0, idx=None, grad=True, group=None):
    """ops.cx_layer on NHWC views of X, Y -> every returned array on the CPU, the distance matrix, dX as logical NCHW and the gradient
    buffer."""
    N, C, H, W = X.shape
    dbuf = torch.full((N, H, W, ctot or C), SENTINEL, device=DEV) if grad else None
    ix = iy = inv = None
    if idx is not None:
        ix, iy = (i.to(torch.int32).to(DEV) for i in idx)
        inv = torch.full((H * W,), -1, dtype=torch.int32)
        inv[idx[0]] = torch.arange(idx[0].numel(), dtype=torch.int32)
        inv = inv.to(DEV)
    probe = {}
    out = ops.cx_layer(ops.View(_nhwc(X, ctot, coff), coff, C), ops.View(_nhwc(Y, ctot, coff), coff, C), ix, iy, inv, b=T.B, h=T.BAND,
                       dx=None if dbuf is None else ops.View(dbuf, coff, C), probe=probe, group=group)
    res = {k: v.cpu() for k, v in out.items()}
    res["d"] = probe["d"].cpu()
    if grad:
        res["dx"], res["dbuf"] = dbuf[..., coff:coff + C].permute(0, 3, 1, 2).contiguous().cpu(), dbuf
    return res


def _both_modes(monkeypatch, launch):
    hip, ops = _mods()
    out = {}
    for name, code in (("f32", hip.MMA_F32), ("bf16x3", hip.MMA_BF16X3)):
        monkeypatch.setattr(ops, "FP32_MMA", code)
        monkeypatch.setattr(ops, "MMA", code)
        out[name] = launch()
    return out


def _set_mode(monkeypatch, mma_mode):
    hip, ops = _mods()
    code = {"f32": hip.MMA_F32, "bf16x3": hip.MMA_BF16X3}[mma_mode]
    monkeypatch.setattr(ops, "FP32_MMA", code)
    monkeypatch.setattr(ops, "MMA", code)


def _check(what, mode, got, ref64, e32):
    """The tolerance rule of the module docstring; got: {mode: tensor}; ref64: one fp64 tensor, or one per mode where the reference depends
    on the run's pattern."""
    refs = ref64 if isinstance(ref64, dict) else {m: ref64 for m in got}
    scale = refs[mode].abs().max().item()
    err = {m: (torch.as_tensor(t).double().cpu() - refs[m]).abs().max().item() for m, t in got.items()}
    print("\n%s [%s]: err f32 %.3e bf16x3 %.3e | e32 %.3e (f32 / e32 = %.2f) | scale %.3e | bf16x3 bound %.3e" % (
        what, mode, err["f32"], err["bf16x3"], e32, err["f32"] / max(e32, 1e-300), scale, 1.5 * err["f32"] + 2e-7 * scale))
    if mode == "f32":
        assert err["f32"] <= 4 * e32, (what, err, e32)
    else:
        assert err["bf16x3"] <= 1.5 * err["f32"] + 2e-7 * scale, (what, err, scale)


def _check_pattern(what, run, f64, rec):
    """Part (b): where the run's argmin / argmax differs from fp64's, fp64's value at the run's choice is within 4 x e32 of the extremum."""
    d64, cx64 = f64["d"], f64["cx"]
    at_min = d64.gather(2, run["argmin"].long().unsqueeze(2)).squeeze(2)
    gap_min = (at_min - f64["rowmin"]).max().item()
    at_max = cx64.gather(1, run["argmax"].long().unsqueeze(1)).squeeze(1)
    gap_max = (f64["colmax"] - at_max).max().item()
    print("%s: argmin differs at %d of %d rows (largest fp64 gap %.3e, 4 x e32 = %.3e); argmax at %d of %d columns (gap %.3e, 4 x e32 = %.3e)" % (
        what, int((run["argmin"].long() != f64["argmin"]).sum()), f64["argmin"].numel(), gap_min, 4 * rec["e32_rowmin"],
        int((run["argmax"].long() != f64["argmax"]).sum()), f64["argmax"].numel(), gap_max, 4 * rec["e32_colmax"]))
    assert run["argmin"].min() >= 0 and run["argmin"].max() < d64.shape[2] and run["argmax"].min() >= 0 and run["argmax"].max() < d64.shape[1]
    assert gap_min <= 4 * rec["e32_rowmin"], (what, "argmin", gap_min)
    assert gap_max <= 4 * rec["e32_colmax"], (what, "argmax", gap_max)


def _pattern_grad(X, Y, run, idx=None):
    return T.grad_under_pattern(X, Y, run["argmax"], run["argmin"], run["d"] > 0, *(idx or (None, None)))


def _three_parts(name, mode, runs, X, Y, idx, f64, rec):
    for k in ("d", "rowmin", "colmax", "CS", "loss"):                                    # (a)
        _check("%s %s" % (name, k), mode, {m: r[k] for m, r in runs.items()}, f64[k], rec["e32_" + k])
    for m, r in runs.items():                                                            # (b)
        _check_pattern("%s [%s]" % (name, m), r, f64, rec)
    grefs = {m: _pattern_grad(X, Y, r, idx) for m, r in runs.items()}                    # (c)
    _check("%s dX" % name, mode, {m: r["dx"] for m, r in runs.items()}, grefs, rec["e32_dx"])


@pytest.mark.parametrize("case", T.KERNEL_CASES + ("slice",), ids=lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else c)
def test_kernels_against_fp64_restatement(fx, refs, case, mma_mode, monkeypatch):
    """Parts (a), (b), (c); two runs bit-identical; a run without a gradient view gives the same forward bits and launches no gradient
    kernel; the slice case writes nothing outside its channels."""
    hip, ops = _mods()
    ctot, coff = (128, 64) if case == "slice" else (None, 0)
    case = SLICE_CASE if case == "slice" else case
    X, Y, _, f64, g64 = refs[case]
    rec = fx["cases"][case]
    P = case[1] * case[2]
    assert 0.05 <= rec["loss"] <= math.log(P) + 0.05 and rec["dx_absmax"] >= T.GRAD_FLOOR.get(case, 1e-4)
    runs = _both_modes(monkeypatch, lambda: _run(ops, X, Y, ctot, coff))
    _set_mode(monkeypatch, mma_mode)
    _three_parts(str(case), mma_mode, runs, X, Y, None, f64, rec)
    mine = runs[mma_mode]
    again = _run(ops, X, Y, ctot, coff)
    for k in ("d", "rowmin", "argmin", "colmax", "argmax", "CS", "loss", "dx"):
        assert torch.equal(mine[k], again[k]), "two runs differ in %s" % k
    calls = []
    orig = ops.cx_grad
    monkeypatch.setattr(ops, "cx_grad", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    fwd = _run(ops, X, Y, ctot, coff, grad=False)
    assert not calls, "the gradient kernels ran without a gradient view"
    for k in ("d", "rowmin", "argmin", "colmax", "argmax", "CS", "loss"):
        assert torch.equal(mine[k], fwd[k]), "the forward-only run differs in %s" % k
    _run(ops, X, Y, ctot, coff)
    assert len(calls) == 1
    if ctot:
        dbuf = mine["dbuf"]
        assert (dbuf[..., :coff] == SENTINEL).all() and (dbuf[..., coff + X.shape[1]:] == SENTINEL).all(), "wrote outside the channel slice"
        assert torch.equal(mine["dx"], _run(ops, X, Y)["dx"]), "the slice run differs from the dense run"


def test_pooled_operands(fx, refs, mma_mode, monkeypatch):
    """64 of 144 positions, different lists for X and Y: the three parts on the gathered operands, and a gradient that is exactly zero
    at the positions that were not sampled."""
    hip, ops = _mods()
    X, Y, idx, f64, g64 = refs[T.POOLED_CASE]
    rec = fx["cases"][T.POOLED_CASE]
    assert not torch.equal(idx[0], idx[1])
    runs = _both_modes(monkeypatch, lambda: _run(ops, X, Y, idx=idx))
    _set_mode(monkeypatch, mma_mode)
    _three_parts("pooled", mma_mode, runs, X, Y, idx, f64, rec)
    N, C, H, W = X.shape
    dx = runs[mma_mode]["dx"].reshape(N, C, H * W)
    unsampled = torch.ones(H * W, dtype=torch.bool)
    unsampled[idx[0]] = False
    assert unsampled.sum() == H * W - T.POOLED_KEEP
    assert (dx[:, :, unsampled] == 0).all(), "a position that was not sampled has a gradient"
    assert (dx[:, :, idx[0]] != 0).any()


def test_identical_operands(mma_mode):
    """X = Y: every row's minimum is a clamped (or nearly clamped) zero -- the clamp and the m_i = 0 path."""
    hip, ops = _mods()
    X = T.seeded((1, 64, 8, 8), 9973)
    r = _run(ops, X, X.clone())
    print("\nidentical: loss %.3e, min d %.3e, rows whose minimum is exactly 0: %d of 64, max|dX| %.3e" % (
        r["loss"].item(), r["d"].min().item(), int((r["rowmin"] == 0).sum()), r["dx"].abs().max().item()))
    assert torch.isfinite(r["loss"]) and r["loss"].item() <= 1e-5
    assert torch.isfinite(r["dx"]).all()
    assert torch.equal(r["argmin"][0].long(), torch.arange(64)) and torch.equal(r["argmax"][0].long(), torch.arange(64))


class _SumsGroup:
    """world_size 2 in one process: all_reduce_sum adds what the other 'rank' would contribute (None: records only)."""
    world_size, active = 2, True

    def __init__(self, other=None):
        self.other, self.seen = other, None

    def all_reduce_sum(self, t):
        self.seen = t.clone()
        if self.other is not None:
            t.add_(self.other)


def test_data_parallel_shards_share_the_channel_mean(fx, refs, mma_mode, monkeypatch):
    """Each one-image 'rank' of the two-image case reproduces its image's -log CS, and its gradient is world x the full-batch gradient of
    its image (the ranks' gradients are averaged afterwards), under the bounds of the full-batch case."""
    hip, ops = _mods()
    case = SLICE_CASE
    X, Y, _, f64, _ = refs[case]
    rec = fx["cases"][case]
    recorders = [_SumsGroup(), _SumsGroup()]
    for r in range(2):
        _run(ops, X[r:r + 1], Y[r:r + 1], grad=False, group=recorders[r])
        assert recorders[r].seen.numel() == case[0] + 1 and recorders[r].seen[-1].item() == case[1] * case[2]

    for r in range(2):
        runs = _both_modes(monkeypatch, lambda: _run(ops, X[r:r + 1], Y[r:r + 1], group=_SumsGroup(recorders[1 - r].seen)))
        _set_mode(monkeypatch, mma_mode)
        loss64 = -torch.log(f64["CS"][r])
        _check("rank %d loss" % r, mma_mode, {m: v["loss"] for m, v in runs.items()}, loss64, rec["e32_loss"])
        _check("rank %d CS" % r, mma_mode, {m: v["CS"][0] for m, v in runs.items()}, f64["CS"][r], rec["e32_CS"])
        grefs = {}
        for m, v in runs.items():
            pat = {k: f64[k].clone() for k in ("argmax", "argmin")}
            passes = f64["d"] > 0
            pat["argmax"][r], pat["argmin"][r], passes[r] = v["argmax"][0].long(), v["argmin"][0].long(), v["d"][0] > 0
            grefs[m] = 2.0 * T.grad_under_pattern(X, Y, pat["argmax"], pat["argmin"], passes)[r:r + 1]
        _check("rank %d dX" % r, mma_mode, {m: v["dx"] for m, v in runs.items()}, grefs, 2.0 * rec["e32_dx"])


# ------------------------------------------------------------------------------------------------ the module
def _engine_loss(fxm, max_1d_size=64):
    from trainner_amd.models.modules.contextual import Contextual_Loss
    cl = Contextual_Loss(dict(fxm["layers"]), max_1d_size=max_1d_size, distance_type="cosine", calc_type="regular", allow_random_init=True)
    _load_vgg(cl.vgg_model, fxm["keys"], T.VGG_FILL_SEED)
    return cl.to(DEV)


def _load_vgg(net, keys, seed):
    sd = net.state_dict()
    sd.update({k: v for k, v in FX.initial_state(keys, seed, gain=1.0, bias_amp=0.05).items() if k in sd})
    net.load_state_dict(sd)


def test_module_against_the_reference_fixture(fx, mma_mode, monkeypatch):
    """Contextual_Loss with seeded VGG weights on a 2 x 3 x 32 x 32 pair, layers {conv_3_2: 1, conv_4_2: 0.5}: the loss against the
    reference's, the input gradient against the fp64 gradient under the run's own pattern -- the contextual kinks of each layer (from
    the module's record) and the ReLU pattern of the VGG below the taps (read from an extractor that listens to every convolution, same
    weights, input and arithmetic), as tests/test_gpu_style_loss.py does for its extractor."""
    from trainner_amd.models.modules.architectures.perceptual import FeatureExtractor
    hip, ops = _mods()
    fxm = fx["module"]
    sd = FX.initial_state(fxm["keys"], T.VGG_FILL_SEED, gain=1.0, bias_amp=0.05)
    x, y = T.module_inputs()
    cl = _engine_loss(fxm)
    assert cl.vgg_model.taps == list(T.MODULE_TAPS) and cl.layers_weights == {"conv3_2": 1, "conv4_2": 0.5}
    relu_convs = T.relu_convs()
    probe_net = FeatureExtractor(listen_list=relu_convs, allow_random_init=True)
    _load_vgg(probe_net, fxm["keys"], T.VGG_FILL_SEED)
    probe_net = probe_net.to(DEV)

    def run():
        cl.record = []
        xd = x.to(DEV).requires_grad_(True)
        loss = cl(xd, y.to(DEV))
        loss.backward()
        with torch.no_grad():
            relu = {k: (v > 0).cpu() for k, v in probe_net(x.to(DEV)).items()}
            quiet = cl(x.to(DEV), y.to(DEV))
        assert torch.equal(quiet, loss.detach()), "the no_grad forward differs"
        return loss.detach().cpu(), xd.grad.cpu(), [{k: v.cpu() for k, v in r.items()} for r in cl.record[:2]], relu

    calls = []
    orig = ops.cx_grad
    monkeypatch.setattr(ops, "cx_grad", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    res = _both_modes(monkeypatch, run)
    _set_mode(monkeypatch, mma_mode)
    assert len(calls) == 2 * 2, "gradient kernels: once per layer and graph run, never under no_grad"
    _check("module loss", mma_mode, {m: r[0] for m, r in res.items()}, torch.tensor(fxm["loss"], dtype=torch.float64), fxm["e32_loss"])
    pre64 = T.S.extract(x.double(), sd, relu_convs)
    fy = T.S.extract(y.double(), sd, T.MODULE_TAPS)
    grefs = {}
    for m, (_, _, recs, relu) in res.items():
        flipped = sum(int((relu[k] != (pre64[k] > 0)).sum()) for k in relu_convs)
        xx = x.double().requires_grad_(True)
        fxp = T.extract_under_pattern(xx, sd, T.MODULE_TAPS, relu)
        total = 0
        for (k, w), r in zip(cl.layers_weights.items(), recs):
            assert (r["rowmin"] > 0).all()          # no clamped entry: the clamp pattern is 'all pass'
            passes = torch.ones((x.shape[0], r["argmax"].shape[1], r["argmax"].shape[1]), dtype=torch.bool)
            total = total + w * T.cx_loss_under_pattern(fxp[k], fy[k], r["argmax"], r["argmin"], passes)
        total.backward()
        grefs[m] = xx.grad.detach()
        print("module [%s]: %d ReLU inputs on the other side of zero; fp64 loss under the run's pattern %.9f (fixture %.9f)" % (
            m, flipped, total.item(), fxm["loss"]))
    _check("module input gradient", mma_mode, {m: r[1] for m, r in res.items()}, grefs, fxm["e32_grad"])


def test_module_pooling_draws_like_the_reference(fx, mma_mode):
    """max_1d_size = 3 after torch.manual_seed: the indices are the reference's recorded ones, and the CPU generator is left where two
    plain randperm draws per pooled layer leave it."""
    fxm = fx["module"]
    pooled = fxm["pooled"]
    cl = _engine_loss(fxm, max_1d_size=pooled["max_1d_size"])
    x, y = T.module_inputs()
    torch.manual_seed(pooled["seed"])
    xd = x.to(DEV).requires_grad_(True)
    loss = cl(xd, y.to(DEV))
    state = torch.get_rng_state()
    loss.backward()
    assert list(cl.last_indices) == list(T.MODULE_TAPS)
    for k in T.MODULE_TAPS:
        for got, want in zip(cl.last_indices[k], pooled["indices"][k]):
            assert torch.equal(got, want), k
    torch.manual_seed(pooled["seed"])
    for s in (64, 64, 16, 16):
        torch.randperm(s)
    assert torch.equal(state, torch.get_rng_state())
    print("\npooled module run: loss %.9g, reference fp64 %.9g; max|grad| %.3e (reference %.3e)" % (
        loss.item(), pooled["loss"], xd.grad.abs().max().item(), pooled["grad_absmax"]))
    assert abs(loss.item() - pooled["loss"]) <= 1e-5 * pooled["loss"]
    assert torch.isfinite(xd.grad).all() and xd.grad.abs().max().item() > 0


# ------------------------------------------------------------------------------------------------ the step record
def _engine_sr_model(fxs, tmp_path):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = ref_harness.esrgan_yaml(name="engine_contextual", out_root=str(tmp_path), gpu_ids="[0]", **fxs["spec"]["yaml"])
    T.cx_yaml(yml, fxs["extra"])
    opt = options.parse(yml, is_train=True)
    model = create_model(opt, verbose=False)
    g, d, f = FX.initial_states(fxs)
    model.netG.load_state_dict(g)
    model.netD.load_state_dict(d)
    netF = [l["function"].network for l in model.generatorlosses.loss_list if "fea" in l["name"]][0]
    sd = netF.state_dict()
    sd.update(f)
    netF.load_state_dict(sd)
    cl = [l for l in model.generatorlosses.loss_list if l["name"] == "contextual"][0]
    _load_vgg(cl["function"].vgg_model, fxs["cx_keys"], fxs["seeds"]["CXF"])
    return model, cl


def test_sr_step_with_the_contextual_loss_matches_reference_record(fx, tmp_path, mma_mode):
    """create_model -> feed_data -> optimize_parameters -> get_current_log with the recipe's three cx lines against the real reference's
    SRModel, two steps, with the bounds tests/test_gpu_step.py uses."""
    import test_gpu_step as TS
    fxs = fx["steps"]["contextual"]
    tol = TS.DEFAULT_TOL
    model, cl = _engine_sr_model(fxs, tmp_path)
    assert [l["name"] for l in model.generatorlosses.loss_list] == fxs["loss_names"] == ["pix-l1", "contextual", "fea-vgg19-l1"]
    assert cl["weight"] == T.CX_WEIGHT and cl["function"].vgg_model.taps == ["conv3_2", "conv4_2"] and cl["function"].max_1d_size == 64
    for (s, (LR, HR)), ref_log in zip(FX.batches(fxs), fxs["logs"]):
        model.feed_data({"LR": LR, "HR": HR})
        model.optimize_parameters(s)
        log = model.get_current_log()
        print("\nstep", s, {k: (round(log[k], 7), round(v, 7)) for k, v in ref_log.items()})
        assert "contextual" in log
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
