"""HFEN, image-gradient, total-variation and difference-only pixel losses on the device (-m gpu): csrc/image_losses.hip through the
C ABI (ops.filter_loss_* / fd_loss_* / pointwise_loss_*, the modules of models/modules/image_losses.py, GeneratorLoss) against
tests/golden/image_losses.pt (the REAL reference's fp64 runs, tools/make_golden_image_losses.py) and against the tool's fp64
restatement, which the tool pinned to the reference to 1e-12 and tests/test_cpu_image_losses.py pins to the fixture again.

Tolerances are measured on the reference, never on the engine (the fixture's e32_* entries are the reference's own fp32-vs-fp64
deviations), and every figure is printed before it is asserted (`pytest -s`):
    value     |v - v64| <= max(4 x the case's e32_val, 4 fp32 ulps of the value)
    gradient  max error <= 4 x e32_grad for the kink-free names (*-l2, tv-*, dtv-*) and for the pixel criteria (the sign of a first
              difference of two fp32 numbers is exact); for grad-*-l1 / -cb the same outside the 3 x 3 reach of a response with
              0 < |e64| <= 4 x e32_resp (tools/make_golden_image_losses.near_zero_mask states why an exact 0 excludes nothing)
    HFEN with a kinked criterion (l1, cb, elastic) in three parts: (a) the rho'(e) map the forward emits, (b) the adjoint stencil on a
              given map, (c) the module's gradient bit-identical to (b) on the map of (a)
The factor 4 allows a different, equally fp32, summation order; a ratio above 1 is a cause to be found, not a factor to raise.
"""
import os

import pytest
import torch

from oracle import detrand, fixtures as FX, ref_harness
from tools import make_golden_image_losses as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_losses.pt")
KINKFREE = tuple(n for n in T.NAMES if n.endswith("-l2") or n.split("-")[0] in ("tv", "dtv", "pix"))
HFEN_KINKED = ("hfen-l1", "hfen-cb", "hfen-elastic")
GRAD_KINKED = ("grad-2d-l1", "grad-4d-l1", "grad-4d-cb")
CRIT = {"l1": 0, "l2": 1, "cb": 2, "elastic": 3, "clipl1": 4}


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


def loss_fn(name):
    from trainner_amd.models import losses
    return losses.get_loss_fn(T.builder_type(name), 1, device=DEV)["function"]


def value_bound(t):
    v = abs(t["value"]) if isinstance(t, dict) else abs(t)
    e32 = t["e32_val"] if isinstance(t, dict) else 0.0
    ulp = torch.finfo(torch.float32).eps * 2.0 ** torch.tensor(max(v, 1e-30)).log2().floor().item()
    return max(4 * e32, 4 * ulp)


def to_dev(t, layout):
    return t.to(DEV).contiguous(memory_format=torch.channels_last if layout == "cl" else torch.contiguous_format)


def engine_run(name, sr, hr, layout="nchw"):
    """-> (value as a Python float, d value / d sr on the CPU in fp64) of the built loss function on the device."""
    x, y = to_dev(sr, layout).requires_grad_(True), to_dev(hr, layout)
    f = loss_fn(name)
    v = f(x) if "tv" in name else f(x, y)
    assert v.dtype == torch.float32 and v.dim() == 0
    v.backward()
    assert x.grad.stride() == x.stride()
    return v.item(), x.grad.detach().cpu().contiguous().double()


def hfen_scale(name, numel):
    return 1.0 / numel if name.split("-")[1] in ("cb", "clipl1") else 1.0


def hfen_forward_map(name, sr, hr, layout="nchw"):
    """The engine's rho'(e) map (CPU, fp32, NCHW order) and value for an hfen name, through the ops wrapper."""
    from trainner_amd import ops
    x, y = to_dev(sr, layout), to_dev(hr, layout)
    taps = tuple(float(v) for v in T.log_taps().flatten())
    out = torch.empty((), dtype=torch.float32, device=DEV)
    dmap = torch.full_like(x, float("nan"))
    ops.filter_loss_fwd(x, y, 1 if layout == "cl" else 0, taps, 15, CRIT[name.split("-")[1]], hfen_scale(name, x.numel()), out, dmap)
    return dmap, out.item(), taps


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("case", T.CASES)
def test_golden_value_and_gradient(fx, case, layout):
    rec = fx["cases"][case]
    sr, hr = T.make_inputs(case)
    for t_, pr in ((sr, rec["sr"]), (hr, rec["hr"])):
        assert T.probe_error(t_, pr)[0] <= 1e-6, "make_inputs no longer rebuilds the fixture's pair"
    failures = []
    for name in T.names_for(case):
        t = rec["names"][name]
        _, gref = T.restate_with_grad(sr, hr, name)
        assert T.probe_error(gref, t["grad"])[0] <= 1e-12 * max(1.0, t["grad_absmax"])
        value, grad = engine_run(name, sr, hr, layout)
        ev, bv = abs(value - t["value"]), value_bound(t)
        line = "%s %s %s: value err %.3e (bound %.3e, ratio %.3f)" % (case, name, layout, ev, bv, ev / bv)
        ok = ev <= bv
        if name in KINKFREE or name in GRAD_KINKED:
            err = (grad - gref).abs()
            left_out = 0.0
            if name in GRAD_KINKED:
                mask = T.near_zero_mask(sr, hr, name, t["e32_resp"])
                left_out = mask.double().mean().item()
                assert left_out <= 1e-3
                err = err[~mask]
            eg, bg = err.max().item(), 4 * t["e32_grad"]
            line += "  grad err %.3e (bound %.3e, ratio %.3f; max|g| %.3e, left out %.2e)" % (eg, bg, eg / bg, t["grad_absmax"], left_out)
            ok = ok and eg <= bg
        else:
            assert name in HFEN_KINKED
            assert torch.isfinite(grad).all()
        print("\n" + line, end="")
        if not ok:
            failures.append(line)
    assert not failures, failures


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("name", HFEN_KINKED)
@pytest.mark.parametrize("case", [c for c in T.CASES if c != "gray72"])
def test_hfen_kinked_map_adjoint_and_module(fx, case, name, layout):
    from trainner_amd import ops
    t = fx["cases"][case]["names"][name]
    crit = name.split("-")[1]
    sr, hr = T.make_inputs(case)
    taps32 = T.log_taps()
    e64 = T.hfen_response(sr.double(), hr.double(), taps32)
    m64 = T.drho(e64, crit)
    kappa = 4 * t["e32_resp"]
    far = e64.abs() > kappa
    near_share = 1.0 - far.double().mean().item()
    assert near_share <= 1e-3
    # (a) the map the forward emits
    dmap, value, taps = hfen_forward_map(name, sr, hr, layout)
    m = dmap.cpu().contiguous().double()
    assert torch.isfinite(m).all()
    ea = (m - m64)[far].abs().max().item()
    ba = 4 * t["e32_map"]
    flips = int((torch.sign(m) != torch.sign(m64))[far].sum())
    rho_max = {"l1": 1.0, "cb": 1.0, "elastic": 0.8 + 0.4 * kappa}[crit]
    over = int((m[~far].abs() > rho_max).sum())
    ev, bv = abs(value - t["value"]), value_bound(t)
    print("\n%s %s %s: value err %.3e (bound %.3e)  (a) near share %.2e, flipped signs away from 0: %d, map err %.3e (bound %.3e), "
          "near-zero entries beyond rho'max: %d" % (case, name, layout, ev, bv, near_share, flips, ea, ba, over), end="")
    # (b) the adjoint stencil on a given map: the fetched one and a seeded random one
    results = []
    for tag, given, key in (("fetched", dmap, "e32_adj"), ("random", to_dev(T.random_map(tuple(sr.shape)), layout), "e32_adj_rand")):
        gx = torch.full_like(given, float("nan"))
        ops.filter_loss_bwd(given, 1 if layout == "cl" else 0, taps, 15, 1.0, None, gx)
        want = T.adjoint(given.cpu().contiguous().double(), taps32)
        eb, bb = (gx.cpu().contiguous().double() - want).abs().max().item(), 4 * t[key]
        print("  (b) %s map: adjoint err %.3e (bound %.3e, ratio %.3f)" % (tag, eb, bb, eb / bb), end="")
        results.append((eb, bb))
    # (c) the module's gradient is the backward kernel on the map its own forward emitted, times the weight
    weight = 0.37
    x, y = to_dev(sr, layout).requires_grad_(True), to_dev(hr, layout)
    (weight * loss_fn(name)(x, y)).backward()
    gx = torch.empty_like(dmap)
    ops.filter_loss_bwd(dmap, 1 if layout == "cl" else 0, taps, 15, hfen_scale(name, x.numel()), torch.tensor([weight], device=DEV), gx)
    assert ev <= bv
    assert flips == 0 and ea <= ba and over == 0, (flips, ea, ba, over)
    for eb, bb in results:
        assert eb <= bb, (eb, bb)
    assert torch.equal(x.grad, gx)


class StubGroup:
    """world_size 2 in one process: mean_scalar records what each 'rank' logs and hands it back."""
    world_size, active = 2, True

    def __init__(self):
        self.seen = []

    def mean_scalar(self, t):
        self.seen.append(t.detach().clone())
        return t.detach()


@pytest.mark.parametrize("train", [{"hfen_criterion": "l1", "hfen_weight": 1e-3}, {"hfen_criterion": "l2", "hfen_weight": 1e-3},
                                   {"hfen_criterion": "elastic", "hfen_weight": 1e-3}, {"hfen_criterion": "cb", "hfen_weight": 1},
                                   {"tv_type": "normal", "tv_norm": 1, "tv_weight": 1}, {"pixel_criterion": "l2", "pixel_weight": 1},
                                   {"grad_type": "grad-4d-l1", "grad_weight": 1}], ids=lambda d: "-".join(str(v) for v in d.values()))
def test_two_half_batches_log_and_back_propagate_what_the_whole_batch_does(fx, train):
    """Data parallelism with a stub group: the two half-batches must log what the whole batch logs, and the mean of their two `sr`
    gradients must be the whole batch's gradient (the sum-reduced HFEN terms are multiplied by the world size for that)."""
    from trainner_amd.models import losses
    sr, hr = T.make_inputs("sq72")
    precise = "grad_type" in train

    def run(gl, a, b):
        x = a.to(DEV).requires_grad_(True)
        res, log = gl(x, b.to(DEV), {}, precise=precise)
        assert len(res) == 1 and len(log) == 1
        res[0].backward()
        return list(log.values())[0].item(), x.grad.cpu().double(), list(log)[0]

    whole_v, whole_g, name = run(losses.GeneratorLoss({"train": train}, device=DEV), sr, hr)
    gl = losses.GeneratorLoss({"train": train}, device=DEV)
    gl.dp_group = StubGroup()
    halves = [run(gl, sr[i:i + 1], hr[i:i + 1]) for i in range(2)]
    assert len(gl.dp_group.seen) == 2
    logged = sum(t.item() for t in gl.dp_group.seen) / 2          # what a real group's mean_scalar hands to the log
    mean_g = torch.cat([h[1] for h in halves]) / 2                # what the gradient averaging over the ranks leaves
    t = fx["cases"]["sq72"]["names"][name]
    w = (gl.loss_list + gl.precise_loss_list)[0]["weight"]
    # each side against the reference's fp64 result for the WHOLE batch, at the bounds of the golden test (times the weight)
    v64, g64 = T.restate_with_grad(sr, hr, name)
    v64, g64 = w * v64.item(), w * g64
    assert abs(v64 - w * t["value"]) <= 1e-12 * max(1.0, abs(v64))
    bv = max(w * 4 * t["e32_val"], value_bound(v64))
    evw, evh = abs(whole_v - v64), abs(logged - v64)
    line = "%s: fp64 %.9e whole %.9e halves %.9e: value errs %.3e / %.3e (bound %.3e)" % (name, v64, whole_v, logged, evw, evh, bv)
    ok = evw <= bv and evh <= bv
    if name in HFEN_KINKED:
        # the rho'(e) map of an image does not depend on its batch; the factors (world size, 1 / numel of half the batch) are powers
        # of two: the averaged gradient of the halves must be the whole batch's bit for bit
        same = torch.equal(mean_g, whole_g)
        line += "  kinked HFEN: averaged gradient bit-identical to the whole batch's: %s" % same
        ok = ok and same
    else:
        keep = ~T.near_zero_mask(sr, hr, name, t["e32_resp"]) if name in GRAD_KINKED else torch.ones_like(g64, dtype=torch.bool)
        bg = w * 4 * t["e32_grad"]
        egw, egh = (whole_g - g64)[keep].abs().max().item(), (mean_g - g64)[keep].abs().max().item()
        line += "  grad errs %.3e / %.3e (bound %.3e)" % (egw, egh, bg)
        ok = ok and egw <= bg and egh <= bg
    print("\n" + line, end="")
    assert ok, line


@pytest.mark.parametrize("name", ["pix-elastic", "hfen-l1", "hfen-cb", "grad-4d-l1", "dtv-l1"])
def test_two_runs_are_bit_identical(name):
    sr, hr = T.make_inputs("odd99x117")
    v1, g1 = engine_run(name, sr, hr)
    v2, g2 = engine_run(name, sr, hr)
    assert v1 == v2 and torch.equal(g1, g2)


def test_accumulate_adds_exactly_and_a_null_gscale_is_one():
    from trainner_amd import ops
    sr, hr = T.make_inputs("odd99x117")
    x, y = sr.to(DEV), hr.to(DEV)
    dmap, _, taps = hfen_forward_map("hfen-l1", sr, hr)
    gscale = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    calls = {"filter": lambda gs, out, acc: ops.filter_loss_bwd(dmap, 0, taps, 15, 1.0, gs, out, accumulate=acc),
             "fd": lambda gs, out, acc: ops.fd_loss_bwd(x, y, 0, 4, 0, 1.0, gs, out, accumulate=acc),
             "tv": lambda gs, out, acc: ops.fd_loss_bwd(x, None, 0, 2, 1, 1.0, gs, out, accumulate=acc),
             "point": lambda gs, out, acc: ops.pointwise_loss_bwd(x, y, 3, 1.0, gs, out, accumulate=acc)}
    for tag, call in calls.items():
        fresh = torch.full_like(x, float("nan"))
        call(gscale, fresh, False)
        assert torch.isfinite(fresh).all(), tag
        base = torch.randn_like(x)
        acc = base.clone()
        call(gscale, acc, True)
        assert torch.equal(acc, base + fresh), tag
        unit = torch.empty_like(x)
        call(None, unit, False)
        assert torch.equal(unit, 2 * fresh), tag          # halving is exact in binary floating point


ZERO_CRITS = ("l1", "l2", "elastic", "clipl1")


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("name", ["pix-" + c for c in ZERO_CRITS] + ["hfen-" + c for c in ZERO_CRITS]
                         + ["grad-%s-%s" % (d, c) for d in ("2d", "4d") for c in ZERO_CRITS])
def test_identical_images_give_exactly_zero(name, layout):
    """sr == hr: value exactly 0 for l1 / l2 / elastic / clipl1 under pix, hfen and grad, and a finite (here: zero) gradient."""
    _, hr = T.make_inputs("odd99x117")
    value, grad = engine_run(name, hr, hr, layout)
    assert value == 0.0
    assert torch.isfinite(grad).all()
    assert grad.abs().max().item() == 0.0          # rho'(0) = 0 for each of these criteria


def test_hfen_refuses_other_channel_counts():
    x = torch.rand(2, 1, 32, 32, device=DEV)
    with pytest.raises(RuntimeError, match="3 channels"):
        loss_fn("hfen-l1")(x, x)


def _engine_model(fxs, tmp_path, weights):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = ref_harness.esrgan_yaml(name="engine_imgloss", out_root=str(tmp_path), gpu_ids="[0]", **fxs["spec"]["yaml"])
    if weights:
        T.losses_yaml(yml, weights)
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
    """optimize_parameters with hfen-l1, grad-4d-l1 and tv-l1 on (weights of the record: each term within 0.1 x .. 10 x of pix-l1 in
    the reference's log) against the real reference's SRModel, two steps, with the bounds tests/test_gpu_step.py uses (DEFAULT_TOL)."""
    import test_gpu_step as TS
    fxs = fx["steps"]["recipe_terms"]
    tol = TS.DEFAULT_TOL
    model = _engine_model(fxs, tmp_path, fxs["weights"])
    assert [l["name"] for l in model.generatorlosses.loss_list] == ["pix-l1", "hfen-l1", "tv-l1", "fea-vgg19-l1"]
    assert [l["name"] for l in model.generatorlosses.precise_loss_list] == ["grad-4d-l1"]
    for (s, (LR, HR)), ref_log in zip(FX.batches(fxs), fxs["logs"]):
        model.feed_data({"LR": LR, "HR": HR})
        model.optimize_parameters(s)
        log = model.get_current_log()
        print("\nstep", s, {k: (round(log[k], 7), round(v, 7)) for k, v in ref_log.items()})
        for k in T.STEP_TERMS:
            assert k in ref_log and 0.1 <= ref_log[k] / ref_log["pix-l1"] <= 10.0
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


def test_step_without_the_new_keys_issues_none_of_the_new_launches(fx, tmp_path, monkeypatch):
    from trainner_amd import ops
    names = ("filter_loss_fwd", "filter_loss_bwd", "fd_loss_fwd", "fd_loss_bwd", "pointwise_loss_fwd", "pointwise_loss_bwd")
    calls = []
    for n in names:
        real = getattr(ops, n)
        monkeypatch.setattr(ops, n, lambda *a, _real=real, _n=n, **k: (calls.append(_n), _real(*a, **k))[1])
    fxs = fx["steps"]["recipe_terms"]
    model = _engine_model(fxs, tmp_path / "plain", None)
    assert [l["name"] for l in model.generatorlosses.loss_list] == ["pix-l1", "fea-vgg19-l1"]
    assert model.generatorlosses.precise_loss_list == []
    s, (LR, HR) = next(iter(FX.batches(fxs)))
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(s)
    assert not set(T.STEP_TERMS) & set(model.get_current_log())
    assert calls == []
    # ... and with the options: HFEN one forward and one backward, tv and grad one forward and one backward each
    model = _engine_model(fxs, tmp_path / "terms", fxs["weights"])
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(s)
    assert sorted(calls) == ["fd_loss_bwd", "fd_loss_bwd", "fd_loss_fwd", "fd_loss_fwd", "filter_loss_bwd", "filter_loss_fwd"]


def test_shipped_recipe_with_the_three_terms_steps_under_amp(tmp_path, monkeypatch):
    """options/sr/train_sr.yml with its lines 114-120 uncommented (nothing else changed: RRDBNet-23, batch 8, crop 128,
    use_amp: true) parses, constructs and steps; the new terms run their fp32 kernels."""
    import test_gpu_step as TS
    from test_cpu_image_losses import recipe_edit
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml, _ = TS.shipped_recipe(tmp_path, monkeypatch)
    assert FX.write_recipe("sr/train_sr.yml", str(tmp_path), recipe_edit) == yml
    opt = options.parse(yml, is_train=True)
    assert opt["use_amp"] is True
    torch.manual_seed(opt["train"]["manual_seed"])
    model = create_model(opt, verbose=False)
    ds = opt["datasets"]["train"]
    LR, HR = detrand.synthetic_pair(ds["batch_size"], ds["crop_size"], 501)
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert set(log) >= {"pix-l1", "fea-vgg19-l1", "l_g_gan", "hfen-l1", "grad-4d-l1", "tv-l1"}
    assert all(v == v and abs(v) != float("inf") for v in log.values()), log
    assert log["hfen-l1"] > 0 and log["grad-4d-l1"] > 0 and log["tv-l1"] > 0


@pytest.mark.parametrize("name", ["hfen-l2", "hfen-l1", "grad-4d-l1", "tv-l1"])
def test_bench_batch_against_chunked_restatement(fx, name):
    """16 x 3 x 512 x 512 once per family, against the fp64 restatement evaluated image by image on the CPU.  The pair is not a fixture
    case, so the bounds are derived, not stored: 4 x the largest relative deviation (e32_val / |value|, e32_grad / max|g|) the
    reference shows over the fixture's cases of this name, times this pair's value / max |g|.  hfen-l1 (kinked) is held to its value
    and to parts (b) and (c) of test_hfen_kinked_map_adjoint_and_module on this batch (adjoint bound: the fixture's largest
    e32_adj / max|g|, times this map's max |A m|)."""
    N, C, H, W = 16, 3, 512, 512
    low = detrand.uniform01(N * C * (H // 4) * (W // 4), 31).double().reshape(N, C, H // 4, W // 4)
    hr = torch.nn.functional.interpolate(low, scale_factor=4, mode="bicubic", align_corners=False)
    hr = (hr + 0.05 * (detrand.uniform01(N * C * H * W, 32).double().reshape(N, C, H, W) - 0.5)).clamp(0, 1).float()
    sr = (hr.double() + 0.16 * (detrand.uniform01(N * C * H * W, 33).double().reshape(N, C, H, W) - 0.5)).clamp(-0.1, 1.1).float()
    batch_sum = name in ("hfen-l1", "hfen-l2")
    vref, gref = 0.0, torch.empty(N, C, H, W, dtype=torch.float64)
    for n in range(N):
        v, g = T.restate_with_grad(sr[n:n + 1], hr[n:n + 1], name)
        vref += v.item() if batch_sum else v.item() / N
        gref[n] = g[0] if batch_sum else g[0] / N
    value, grad = engine_run(name, sr, hr)
    recs = [c["names"][name] for c in fx["cases"].values() if name in c["names"]]
    rel_v = max(t["e32_val"] / abs(t["value"]) for t in recs)
    rel_g = max(t["e32_grad"] / t["grad_absmax"] for t in recs)
    ev, bv = abs(value - vref), max(4 * rel_v * abs(vref), value_bound(vref))
    line = "16x3x512x512 %s: value %.9e err %.3e (bound %.3e)" % (name, value, ev, bv)
    ok = ev <= bv
    if name != "hfen-l1":
        err = (grad - gref).abs()
        if name == "grad-4d-l1":
            mask = T.near_zero_mask(sr, hr, name, max(t["e32_resp"] for t in recs))
            assert mask.double().mean().item() <= 1e-3
            err = err[~mask]
        eg, bg = err.max().item(), 4 * rel_g * gref.abs().max().item()
        line += "  grad err %.3e (bound %.3e, max|g| %.3e)" % (eg, bg, gref.abs().max().item())
        ok = ok and eg <= bg
    else:
        # the kinked path at bench size (8 x 32 tiles per plane): parts (b) and (c) of the triple on this batch
        from trainner_amd import ops
        dmap, _, taps = hfen_forward_map(name, sr, hr)
        gx = torch.full_like(dmap, float("nan"))
        ops.filter_loss_bwd(dmap, 0, taps, 15, 1.0, None, gx)
        want = T.adjoint(dmap.cpu().double(), T.log_taps())
        rel_a = max(t["e32_adj"] / t["grad_absmax"] for t in recs)          # hfen-l1's gradient IS the adjoint of its map
        eb, bb = (gx.cpu().double() - want).abs().max().item(), 4 * rel_a * want.abs().max().item()
        x = sr.to(DEV).requires_grad_(True)
        (0.37 * loss_fn(name)(x, hr.to(DEV))).backward()
        ops.filter_loss_bwd(dmap, 0, taps, 15, 1.0, torch.tensor([0.37], device=DEV), gx)
        same = torch.equal(x.grad, gx)
        line += "  (b) adjoint err %.3e (bound %.3e)  (c) module gradient bit-identical: %s" % (eb, bb, same)
        ok = ok and eb <= bb and same
    print("\n" + line, end="")
    assert ok, line
