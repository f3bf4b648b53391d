"""Colour, average and multi-scale pixel losses on the device (-m gpu): csrc/pooled_losses.hip through the C ABI (ops.pool_loss_* /
multiscale_loss_*, the modules of models/modules/pooled_losses.py, GeneratorLoss, SRModel) against tests/golden/pooled_losses.pt (the
REAL reference's fp64 runs, tools/make_golden_pooled_losses.py) and against the tool's fp64 restatement, which the tool pinned to the
reference to 1e-12 and tests/test_cpu_pooled_losses.py pins to the fixture again.

Tolerances are measured on the reference, never on the engine (the fixture's e32_* entries are the reference's own fp32-vs-fp64
deviations), and every figure is printed before it is asserted (`pytest -s`):
    value     |v - v64| <= max(4 x the case's e32_val, 4 fp32 ulps of the value)
    gradient  max error over every compared element <= 4 x e32_grad.  Every element is compared for l2 and for cells of one pixel
              (the sign of an fp32 subtraction is exact).  For the criteria with a kink at 0 the sign of a POOLED difference is not
              exact in fp32: the footprint of the cells with 0 < |d64| <= 4 x e32_resp is left out (tools' `kept_mask`, which the tool
              also applied to e32_grad), and at most 1 % of a case's cells may be.
The factor 4 allows a different, equally fp32, summation order; a ratio above 1 is a cause to be found, not a factor to raise.
"""
import os

import pytest
import torch

from oracle import fixtures as FX, ref_harness
from tools import make_golden_pooled_losses as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pooled_losses.pt")
CRIT = {"l1": 0, "l2": 1, "cb": 2, "elastic": 3, "clipl1": 4, "l1cosinesim": 5}


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


_REF = {}


def reference(case, name):
    """(sr, hr, fp64 value, full fp64 gradient) of the restatement, computed once per case and name and never modified."""
    if (case, name) not in _REF:
        sr, hr = T.make_inputs(case)
        v, g = T.restate_with_grad(sr, hr, name, T.CASES[case][1])
        _REF[(case, name)] = (sr, hr, v.item(), g)
    return _REF[(case, name)]


def loss_fn(name, k):
    from trainner_amd.models import losses
    entry = losses.get_loss_fn(name, 1, device=DEV, opt={"scale": k})
    assert entry["name"] == T.built_name(name)
    return entry["function"]


def value_bound(t):
    v = abs(t["value"])
    ulp = torch.finfo(torch.float32).eps * 2.0 ** torch.tensor(max(v, 1e-30)).log2().floor().item()
    return max(4 * t["e32_val"], 4 * ulp)


def to_dev(t, layout):
    return t.to(DEV).contiguous(memory_format=torch.channels_last if layout == "cl" else torch.contiguous_format)


def engine_run(name, k, sr, hr, layout="nchw"):
    """-> (value as a Python float, d value / d sr on the CPU in fp64) of the built loss function on the device."""
    x, y = to_dev(sr, layout).requires_grad_(True), to_dev(hr, layout)
    v = loss_fn(name, k)(x, y)
    assert v.dtype == torch.float32 and v.dim() == 0
    v.backward()
    assert x.grad.stride() == x.stride()
    return v.item(), x.grad.detach().cpu().contiguous().double()


def raw(name, k, x, y, gs=None, gx=None, accumulate=False):
    """The two launches through ops -> (value on the CPU, gx); gx starts as NaN unless given."""
    from trainner_amd import ops
    layout = 0 if x.is_contiguous() else 1
    loss = torch.full((), float("nan"), device=DEV)
    if gx is None:
        gx = torch.full_like(x, float("nan"))
    crit = CRIT[T.crit_of(name)]
    if T.kind_of(name) == "multiscale":
        ops.multiscale_loss_fwd(x, y, layout, crit, loss)
        ops.multiscale_loss_bwd(x, y, layout, crit, gs, gx, accumulate=accumulate)
    else:
        uv = T.kind_of(name) == "color"
        ops.pool_loss_fwd(x, y, layout, k, uv, crit, loss)
        ops.pool_loss_bwd(x, y, layout, k, uv, crit, gs, gx, accumulate=accumulate)
    return loss.item(), gx


def compare(fx, case, name, value, grad, tag):
    """-> (report line, ok) of an engine value and gradient (fp64, CPU, NCHW) against the fixture and the restatement."""
    rec = fx["cases"][case]
    t = rec["names"][name]
    sr, hr, vref, gref = reference(case, name)
    assert abs(vref - t["value"]) <= 1e-12 * max(1.0, abs(t["value"]))
    assert T.probe_error(gref, t["grad"])[0] <= 1e-12 * max(1.0, t["grad_absmax"])
    keep, share = T.kept_mask(sr, hr, name, rec["k"], t["e32_resp"])
    ev, bv = abs(value - t["value"]), value_bound(t)
    eg, bg = (grad - gref)[keep].abs().max().item(), 4 * t["e32_grad"]
    line = "%s %s %s: value err %.3e (bound %.3e, ratio %.3f)  grad err %.3e (bound %.3e, ratio %.3f; max|g| %.3e)  left out %.4f of the cells" % (
        case, name, tag, ev, bv, ev / bv, eg, bg, eg / bg, t["grad_absmax"], share)
    return line, ev <= bv and eg <= bg and share <= 0.01 and bool(torch.isfinite(grad).all())


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("case", list(T.CASES))
def test_golden_value_and_gradient(fx, case, layout):
    rec = fx["cases"][case]
    failures = []
    for name in T.names_for(case):
        sr, hr, _, _ = reference(case, name)
        for t_, pr in ((sr, rec["sr"]), (hr, rec["hr"])):
            assert T.probe_error(t_, pr)[0] <= 1e-6, "make_inputs no longer rebuilds the fixture's pair"
        value, grad = engine_run(name, rec["k"], sr, hr, layout)
        line, ok = compare(fx, case, name, value, grad, layout)
        print("\n" + line, end="")
        if not ok:
            failures.append(line)
    assert not failures, failures


CUT = [("avg_k4", "avg-l1"), ("avg_k4", "avg-l1cosinesim"), ("col_k4", "color-l1cosinesim"), ("avg_k4_vec", "avg-l1"), ("avg_k3", "avg-l1"),
       ("avg_k2", "avg-l2"), ("avg_c2", "avg-l1")]


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("case, name", CUT)
def test_dropped_rows_and_columns_get_exactly_zero(case, name, layout):
    """The trailing H % k rows and W % k columns belong to no cell: their gradient is exactly 0, everything else is not."""
    sr, hr, _, _ = reference(case, name)
    k = T.CASES[case][1]
    H, W = sr.shape[2:]
    hk, wk = H // k * k, W // k * k
    assert hk < H or wk < W
    _, gx = raw(name, k, to_dev(sr, layout), to_dev(hr, layout))
    cut = torch.ones(H, W, dtype=torch.bool, device=DEV)
    cut[:hk, :wk] = False
    worst = gx[:, :, cut].abs().max().item()
    inside = (gx[:, :, :hk, :wk] != 0).double().mean().item()
    print("\n%s %s %s: max |gx| on the %d cut pixels %.3e, non-zero share inside %.4f" % (case, name, layout, int(cut.sum()), worst, inside), end="")
    assert worst == 0.0
    assert inside == 1.0


def test_multiscale_rows_beyond_a_levels_floor_take_that_level_out(fx):
    """40 x 52: rows 32 .. 39 lie in no cell of level 4 and columns 48 .. 51 in none of levels 3 and 4.  With x = y + c every cell's
    derivative is +1, so the gradient is the sum of weight / (count 4^i) over the levels that hold the pixel, exactly known."""
    y = T.make_inputs("ms40x52")[1].to(DEV)
    x = y + 0.25
    v, gx = raw("multiscale-l1", 1, x, y)
    n = [2 * 3 * (40 >> i) * (52 >> i) for i in range(5)]
    term = [w / (n[i] * 4 ** i) for i, w in enumerate(T.MS_WEIGHTS)]
    want = torch.full((40, 52), sum(term), dtype=torch.float64)
    want[32:, :] -= term[4]
    want[:, 48:] -= term[3]
    want[:32, 48:] -= term[4]
    err = (gx.cpu().double() - want).abs().max().item()
    print("\nmulti-scale floors: value %.9f (want 0.5 within the rounding of y + 0.25), grad err %.3e of %.3e" % (v, err, sum(term)), end="")
    assert abs(v - 0.5) <= 1e-6
    assert err <= 4 * torch.finfo(torch.float32).eps * sum(term)


FULL = [("ms37x45", "multiscale-l1"), ("ms80x144", "multiscale-l1cosinesim"), ("ms_c4", "multiscale-elastic"), ("avg_k4", "avg-cb"),
        ("avg_k8", "avg-l1"), ("avg_k1", "avg-l1cosinesim"), ("col_k4", "color-l1"), ("recipe64x48", "color-l1cosinesim"),
        ("avg_k4_vec", "avg-l1cosinesim")]


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("case, name", FULL)
def test_gx_is_written_in_full(case, name, layout):
    """gx starts as NaN: the backward writes every element, the ones no cell covers included."""
    sr, hr, _, _ = reference(case, name)
    v, gx = raw(name, T.CASES[case][1], to_dev(sr, layout), to_dev(hr, layout))
    bad = int((~torch.isfinite(gx)).sum())
    print("\n%s %s %s: %d of %d elements not finite, value %.6e" % (case, name, layout, bad, gx.numel(), v), end="")
    assert bad == 0
    assert v == v and abs(v) != float("inf")


@pytest.mark.parametrize("case, name", [("avg_k4", "avg-l1cosinesim"), ("recipe64x48", "color-l1cosinesim"), ("recipe64x48", "avg-l1"),
                                        ("ms40x52", "multiscale-l1cosinesim"), ("recipe64x48", "multiscale-l1")])
def test_accumulate_adds_to_gx_and_gscale_scales(case, name):
    sr, hr, _, _ = reference(case, name)
    k = T.CASES[case][1]
    x, y = sr.to(DEV), hr.to(DEV)
    _, unit = raw(name, k, x, y)
    half = torch.tensor([0.5], device=DEV)
    _, fresh = raw(name, k, x, y, gs=half)
    base = torch.randn_like(x)
    acc = base.clone()
    raw(name, k, x, y, gs=half, gx=acc, accumulate=True)
    d_acc = (acc - (base + fresh)).abs().max().item()
    d_half = (unit - 2 * fresh).abs().max().item()
    print("\n%s %s: accumulate vs base + fresh %.3e, unit vs 2 x half %.3e" % (case, name, d_acc, d_half), end="")
    assert torch.equal(acc, base + fresh)          # the cut pixels keep `base` exactly: + 0
    assert torch.equal(unit, 2 * fresh)            # halving is exact in binary floating point; a NULL gscale is 1


@pytest.mark.parametrize("case, name", [("recipe64x48", "color-l1cosinesim"), ("recipe64x48", "avg-l1"), ("recipe64x48", "multiscale-l1"),
                                        ("avg_k8", "avg-elastic"), ("ms37x45", "multiscale-l2"), ("avg_k4", "avg-l1")])
def test_offset_view_takes_the_scalar_path_and_matches(fx, case, name):
    """A pointer 4 bytes past a 16-byte boundary: both images and gx are dense views of larger buffers."""
    sr, hr, _, _ = reference(case, name)

    def shifted(t):
        buf = torch.zeros(t.numel() + 1, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    value, gx = raw(name, T.CASES[case][1], shifted(sr), shifted(hr), gx=shifted(torch.full_like(sr, float("nan"))))
    line, ok = compare(fx, case, name, value, gx.cpu().double(), "offset view")
    print("\n" + line, end="")
    assert ok, line


@pytest.mark.parametrize("name", T.RECIPE)
def test_channels_last_gradient_keeps_the_strides_and_two_runs_are_bit_identical(name):
    sr, hr, _, _ = reference("recipe64x48", name)
    for layout in ("nchw", "cl"):
        x, y = to_dev(sr, layout).requires_grad_(True), to_dev(hr, layout)
        loss_fn(name, 4)(x, y).backward()
        print("\n%s %s: x strides %s, gradient strides %s" % (name, layout, x.stride(), x.grad.stride()), end="")
        assert x.grad.stride() == x.stride()
        assert x.grad.is_contiguous(memory_format=torch.channels_last if layout == "cl" else torch.contiguous_format)
    v1, g1 = engine_run(name, 4, sr, hr)
    v2, g2 = engine_run(name, 4, sr, hr)
    assert v1 == v2 and torch.equal(g1, g2)


def test_generator_loss_logs_the_three_recipe_terms(fx):
    """GeneratorLoss with the recipe's six lines on the device: names, order and weight x value of the 64 x 48 pair, in both precisions
    of the incoming images (the operands are promoted to fp32)."""
    from trainner_amd.models import losses
    rec = fx["cases"]["recipe64x48"]
    train = {"color_criterion": "color-l1cosinesim", "color_weight": 1, "avg_criterion": "avg-l1", "avg_weight": 5,
             "ms_criterion": "multiscale-l1", "ms_weight": 1e-2}
    gl = losses.GeneratorLoss({"train": train, "scale": 4}, device=DEV)
    sr, hr = T.make_inputs("recipe64x48")
    x = sr.to(DEV).requires_grad_(True)
    results, log = gl(x, hr.to(DEV), {})
    assert list(log) == ["color-l1cosinesim", "avg-l1", "pix-multiscale-l1"]
    for (built, wkey), name, r in zip(T.STEP_TERMS.items(), T.RECIPE, results):
        t, w = rec["names"][name], train[wkey]
        err, bound = abs(log[built].item() - w * t["value"]), w * value_bound(t) + 2 * torch.finfo(torch.float32).eps * w * abs(t["value"])
        print("\n%s: logged %.9e, weight x fixture %.9e, err %.3e (bound %.3e)" % (built, log[built].item(), w * t["value"], err, bound), end="")
        assert r.item() == log[built].item()
        assert err <= bound
    sum(results).backward()
    want = sum(train[wkey] * reference("recipe64x48", name)[3] for (_, wkey), name in zip(T.STEP_TERMS.items(), T.RECIPE))
    err = (x.grad.cpu().double() - want).abs().max().item()
    bound = sum(train[wkey] * 4 * rec["names"][name]["e32_grad"] for (_, wkey), name in zip(T.STEP_TERMS.items(), T.RECIPE)) + \
        2 * torch.finfo(torch.float32).eps * want.abs().max().item()          # + the rounding of the two additions of autograd
    print("\nsummed gradient err %.3e (bound %.3e; max|g| %.3e)" % (err, bound, want.abs().max().item()), end="")
    assert err <= bound
    # half-precision images are promoted: the losses see exactly the fp32 images of the rounded values
    results16, _ = gl(sr.half().to(DEV), hr.half().to(DEV), {})
    results32, _ = gl(sr.half().float().to(DEV), hr.half().float().to(DEV), {})
    assert [r.item() for r in results16] == [r.item() for r in results32]


def _engine_model(fxs, tmp_path, weights, extra=""):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = ref_harness.esrgan_yaml(name="engine_pooled", out_root=str(tmp_path), gpu_ids="[0]", **fxs["spec"]["yaml"])
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
    """optimize_parameters with the recipe's six lines (its weights) against the real reference's SRModel, two steps at nb 1, crop 64,
    with the bounds tests/test_gpu_step.py uses (DEFAULT_TOL)."""
    import test_gpu_step as TS
    fxs = fx["steps"]["recipe"]
    tol = TS.DEFAULT_TOL
    model = _engine_model(fxs, tmp_path, fxs["weights"])
    assert [l["name"] for l in model.generatorlosses.loss_list] == ["pix-l1", "fea-vgg19-l1"] + list(T.STEP_TERMS)
    assert model.generatorlosses.precise_loss_list == []
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


def test_step_without_the_new_keys_issues_none_of_the_new_launches_and_fs_steps(fx, tmp_path, monkeypatch):
    from trainner_amd import ops
    names = ("pool_loss_fwd", "pool_loss_bwd", "multiscale_loss_fwd", "multiscale_loss_bwd")
    calls = []
    for n in names:
        real = getattr(ops, n)
        monkeypatch.setattr(ops, n, lambda *a, _real=real, _n=n, **k: (calls.append(_n), _real(*a, **k))[1])
    fxs = fx["steps"]["recipe"]
    model = _engine_model(fxs, tmp_path / "plain", None)
    assert [l["name"] for l in model.generatorlosses.loss_list] == ["pix-l1", "fea-vgg19-l1"]
    s, (LR, HR) = next(iter(FX.batches(fxs)))
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(s)
    assert not set(T.STEP_TERMS) & set(model.get_current_log())
    assert calls == []
    # one step with fs: true and the three terms: they run (one forward and one backward each) and log finite, positive values
    model = _engine_model(fxs, tmp_path / "fs", fxs["weights"], extra="\n  fs: true\n  lpf_type: average\n  hpf_type: average")
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(s)
    log = model.get_current_log()
    print("\nfs step", {k: log[k] for k in ("pix-l1",) + tuple(T.STEP_TERMS)}, end="")
    assert sorted(calls) == ["multiscale_loss_bwd", "multiscale_loss_fwd", "pool_loss_bwd", "pool_loss_bwd", "pool_loss_fwd", "pool_loss_fwd"]
    for k in T.STEP_TERMS:
        assert k in log and 0 < log[k] < float("inf")


# ------------------------------------------------------------------------------------------------ the multi-band / multi-cell paths
# The forwards launch at most 256 (pool) and 1024 (multi-scale) blocks and the pool backward at most 4096: beyond that a block takes
# several cells, or several bands through one LDS pyramid.  No fixture case is that large, so this shape is held against the fp64
# restatement alone (pinned to the reference by the tool and by tests/test_cpu_pooled_losses.py), with the yardsticks taken from the
# restatement's own fp32 run.  1 x 3 x 1048 x 1092: 66 x 18 = 1188 bands (H % 16 = 8, W % 64 = 4); 1.14 M cells at k = 1 (more than
# the 1 M threads of the capped backward grid) and 262 x 273 = 71526 at k = 4 (more than the forward's 65536).
BIG_SHAPE, BIG_SEED = (1, 3, 1048, 1092), 71
BIG = [("avg-l1cosinesim", 1), ("avg-l1", 4), ("color-l1cosinesim", 4), ("multiscale-l1", 1), ("multiscale-l1cosinesim", 1)]
_BIG = {}


def big_reference(name, k):
    """(sr, hr, yardsticks like a fixture entry, fp64 gradient, kept mask, share left out), computed once per name."""
    if (name, k) not in _BIG:
        sr, hr = T.make_pair(BIG_SHAPE, BIG_SEED)
        v64, g64 = T.restate_with_grad(sr, hr, name, k)
        v32, g32 = T.restate_with_grad(sr, hr, name, k, dtype=torch.float32)
        e32_resp = [(a.double() - b).abs().max().item() for a, b in zip(T.responses(sr, hr, name, k), T.responses(sr.double(), hr.double(), name, k))]
        keep, share = T.kept_mask(sr, hr, name, k, e32_resp)
        t = {"value": v64.item(), "e32_val": abs(v32.double().item() - v64.item()), "e32_grad": (g32.double() - g64)[keep].abs().max().item(),
             "grad_absmax": g64.abs().max().item()}
        _BIG[(name, k)] = (sr, hr, t, g64, keep, share)
    return _BIG[(name, k)]


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("name, k", BIG)
def test_shape_above_the_block_caps(name, k, layout):
    sr, hr, t, g64, keep, share = big_reference(name, k)
    bands = -(-BIG_SHAPE[2] // 16) * -(-BIG_SHAPE[3] // 64)
    cells = (BIG_SHAPE[2] // k) * (BIG_SHAPE[3] // k)
    assert bands > 1024 and (k != 1 or cells > 4096 * 256) and cells > 256 * 256
    value, gx = raw(name, k, to_dev(sr, layout), to_dev(hr, layout))
    grad = gx.cpu().contiguous().double()
    ev, bv = abs(value - t["value"]), value_bound(t)
    eg, bg = (grad - g64)[keep].abs().max().item(), 4 * t["e32_grad"]
    print("\n%s k %d %s: value err %.3e (bound %.3e, ratio %.3f)  grad err %.3e (bound %.3e, ratio %.3f; max|g| %.3e)  left out %.5f of the cells" % (
        name, k, layout, ev, bv, ev / bv, eg, bg, eg / bg, t["grad_absmax"], share), end="")
    assert share <= 0.01
    assert bool(torch.isfinite(gx).all())
    assert ev <= bv
    assert eg <= bg


@pytest.mark.parametrize("case, name", [("ms80x144", "multiscale-l1"), ("ms80x144", "multiscale-l1cosinesim"), ("ms40x52", "multiscale-cb"),
                                        ("recipe64x48", "color-l1cosinesim"), ("recipe64x48", "avg-l1"), ("avg_k2", "avg-l2")])
def test_few_blocks_take_many_bands_and_cells(fx, case, name):
    """The forwards held to 3 (multi-scale) and 1 (pool) blocks: ms80x144's 15 bands go 5 to a block through one LDS pyramid, and one
    block takes every cell; against the fixture with its bounds, and bit-identical with the default grid's gradient."""
    from trainner_amd import ops
    sr, hr, _, _ = reference(case, name)
    x, y = sr.to(DEV), hr.to(DEV)
    v_default, g_default = raw(name, T.CASES[case][1], x, y)
    try:
        ops.pooled_forward_blocks(1, 3)
        value, gx = raw(name, T.CASES[case][1], x, y)
    finally:
        ops.pooled_forward_blocks(0, 0)
    line, ok = compare(fx, case, name, value, gx.cpu().double(), "few blocks")
    print("\n" + line + "  (default grid: value %.9e, few blocks: %.9e)" % (v_default, value), end="")
    assert ok, line
    assert torch.equal(gx, g_default)
