"""Colour, average and multi-scale pixel losses, the parts that need no device: the fp64 restatement of
tools/make_golden_pooled_losses.py against tests/golden/pooled_losses.pt (the REAL reference's fp64 runs), the formulas by hand, the
option surface of GeneratorLoss (names, order, refusals, routing under frequency separation) in the SR, Pix2Pix and CycleGAN models'
loss builder, and header <-> library <-> binding agreement."""
import os
import re

import pytest
import torch
import torch.nn as nn

from tools import make_golden_pooled_losses as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "pooled_losses.pt")
NEW_EXPORTS = {"tnr_pooled_workspace_bytes", "tnr_pooled_forward_blocks", "tnr_pool_loss_fwd", "tnr_pool_loss_bwd", "tnr_multiscale_loss_fwd",
               "tnr_multiscale_loss_bwd"}
RECIPE = {"color_criterion": "color-l1cosinesim", "color_weight": 1, "avg_criterion": "avg-l1", "avg_weight": 5,
          "ms_criterion": "multiscale-l1", "ms_weight": 1e-2}


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


def test_fixture_is_small_and_complete(fx):
    assert os.path.getsize(FIXTURE) < 1 << 19
    assert set(fx["cases"]) == set(T.CASES)
    seen = {kind: set() for kind in ("color", "avg", "multiscale")}
    for case, (shape, k, names, _, _) in T.CASES.items():
        rec = fx["cases"][case]
        assert rec["shape"] == tuple(shape) and rec["k"] == k and set(rec["names"]) == set(names)
        for name in names:
            seen[T.kind_of(name)].add(T.crit_of(name))
            t = rec["names"][name]
            assert t["ambiguous"] <= 0.01 and len(t["e32_resp"]) == (5 if T.kind_of(name) == "multiscale" else 1)
        # the recipe's criterion on every case of its loss
        for recipe in T.RECIPE:
            if any(T.kind_of(n) == T.kind_of(recipe) for n in names):
                assert recipe in names, (case, recipe)
    assert all(crits == set(T.CRITERIA) for crits in seen.values()), seen
    assert set(T.RECIPE) <= set(T.names_for("recipe64x48"))
    blacks = [c for c, spec in T.CASES.items() if spec[4] is not None and any(T.crit_of(n) == "l1cosinesim" for n in spec[2])]
    assert blacks
    for c in blacks:
        for name in T.names_for(c):
            if T.crit_of(name) == "l1cosinesim":
                assert fx["cases"][c]["names"][name]["black_grad_absmax"] < 10          # a zero-norm hr pixel: a finite gradient
    step = fx["steps"]["recipe"]
    assert step["weights"] == T.STEP_WEIGHTS
    for log in step["logs"]:
        assert all(log[n] > 0 for n in T.STEP_TERMS)


@pytest.mark.parametrize("case", list(T.CASES))
def test_restatement_matches_the_reference_record(fx, case):
    rec = fx["cases"][case]
    sr, hr = T.make_inputs(case)
    assert (sr < 0).any() and (sr > 1).any()
    for t, pr in ((sr, rec["sr"]), (hr, rec["hr"])):
        assert T.probe_error(t, pr)[0] <= 1e-6
    for name in T.names_for(case):
        t = rec["names"][name]
        v, g = T.restate_with_grad(sr, hr, name, rec["k"])
        assert abs(v.item() - t["value"]) <= 1e-12 * max(1.0, abs(t["value"])), (name, v.item(), t["value"])
        es, _ = T.probe_error(g, t["grad"])
        assert es <= 1e-12 * max(1.0, t["grad_absmax"]), (name, es)
        keep, share = T.kept_mask(sr, hr, name, rec["k"], t["e32_resp"])
        assert share == t["ambiguous"] and keep.shape == sr.shape


def test_formulas_by_hand():
    # floor mode: at 10 x 11 with k = 4 rows 8, 9 and columns 8 .. 10 belong to no cell and take exactly no gradient
    x = torch.rand(1, 3, 10, 11, dtype=torch.float64).requires_grad_(True)
    y = torch.rand(1, 3, 10, 11, dtype=torch.float64)
    assert T.box(x, 4).shape == (1, 3, 2, 2)
    assert torch.equal(T.box(x, 4), nn.functional.avg_pool2d(x, 4)) or (T.box(x, 4) - nn.functional.avg_pool2d(x, 4)).abs().max() < 1e-15
    T.restate(x, y, "avg-l1", 4).backward()
    assert x.grad[..., 8:, :].abs().max() == 0 and x.grad[..., :, 8:].abs().max() == 0 and (x.grad[..., :8, :8] != 0).all()
    assert torch.equal(T.box(y, 1), y)                   # k = 1 is the identity
    # UV of white and of black is (.5, .5); of pure red (r - y) * .877 + .5 with y = .299
    uv = T.rgb_to_uv(torch.tensor([[1., 1., 1.], [0., 0., 0.], [1., 0., 0.]], dtype=torch.float64).reshape(3, 3, 1, 1)).reshape(3, 2)
    want = torch.tensor([[.5, .5], [.5, .5], [(0 - .299) * .493 + .5, (1 - .299) * .877 + .5]], dtype=torch.float64)
    assert (uv - want).abs().max() < 1e-15
    # l1cosinesim of one pixel pair: mean |a - b| + 5 (1 - cos)
    a = torch.tensor([3., 0., 4.], dtype=torch.float64).reshape(1, 3, 1, 1)
    b = torch.tensor([0., 0., 2.], dtype=torch.float64).reshape(1, 3, 1, 1)
    assert abs(T.criterion(a, b, "l1cosinesim").item() - ((3 + 0 + 2) / 3 + 5 * (1 - 8 / (5 * 2)))) < 1e-15
    # a zero-norm second operand: cos = 0, and the gradient of the cosine term is exactly 0
    ag = a.clone().requires_grad_(True)
    v = T.criterion(ag, torch.zeros_like(b), "l1cosinesim")
    v.backward()
    assert abs(v.item() - (7 / 3 + 5)) < 1e-15 and torch.equal(ag.grad.flatten(), torch.tensor([1 / 3, 0., 1 / 3], dtype=torch.float64))
    # multi-scale: a constant difference c gives c * (1 + .5 + .25 + .125 + .125) whatever the shape; rows 32 .. 39 of a 40 x 52 image
    # belong to no cell of level 4 (40 >> 4 = 2 cells of 16 rows)
    y = torch.rand(2, 3, 40, 52, dtype=torch.float64)
    x = (y + 0.25).requires_grad_(True)
    v = T.restate(x, y, "multiscale-l1", 1)
    assert abs(v.item() - 0.25 * 2) < 1e-12
    v.backward()
    n = [2 * 3 * (40 >> i) * (52 >> i) for i in range(5)]
    full = sum(w / (n[i] * 4 ** i) for i, w in enumerate(T.MS_WEIGHTS))
    assert abs(x.grad[0, 0, 0, 0].item() - full) < 1e-15
    assert abs(x.grad[0, 0, 35, 0].item() - (full - T.MS_WEIGHTS[4] / (n[4] * 4 ** 4))) < 1e-15
    assert abs(x.grad[0, 0, 0, 51].item() - (full - sum(T.MS_WEIGHTS[i] / (n[i] * 4 ** i) for i in (3, 4)))) < 1e-15
    with pytest.raises(ValueError):
        T.restate(torch.rand(1, 3, 15, 40), torch.rand(1, 3, 15, 40), "multiscale-l1", 1)


def test_data_parallel_shards_average_to_the_global_batch():
    """The claim of GeneratorLoss._log: each loss is a batch mean over equal shards (the cosine term of l1cosinesim included), so the
    mean of two half-batch values is the whole-batch value and the ranks' averaged gradient is the global one."""
    sr, hr = T.make_inputs("recipe64x48")
    sr, hr = sr.double(), hr.double()
    for name in T.RECIPE + ("multiscale-l1cosinesim", "avg-l1cosinesim"):
        whole = T.restate(sr, hr, name, 4).item()
        halves = [T.restate(sr[i:i + 1], hr[i:i + 1], name, 4).item() for i in range(2)]
        assert abs(whole - sum(halves) / 2) <= 1e-14, (name, whole, halves)


def _opt(train, scale=4):
    return {"train": train, "scale": scale, "datasets": {"train": {"znorm": False}}}


def test_recipe_line_builds_one_entry():
    """Fails before this feature: `color_weight` used to raise NotImplementedError."""
    from trainner_amd.models import losses
    from trainner_amd.models.modules import pooled_losses as PL
    gl = losses.GeneratorLoss(_opt({"color_criterion": "color-l1cosinesim", "color_weight": 1}), device="cpu")
    assert [(l["name"], l["weight"]) for l in gl.loss_list] == [("color-l1cosinesim", 1)] and gl.precise_loss_list == []
    f = gl.loss_list[0]["function"]
    assert isinstance(f, PL.ColorLoss) and f.k == 4 and f.uv and isinstance(f.criterion, PL.L1CosineSim) and f.criterion.loss_lambda == 5


def test_generator_loss_builds_the_terms_in_the_references_position():
    from trainner_amd import ops
    from trainner_amd.models import losses
    from trainner_amd.models.modules import pooled_losses as PL
    train = dict(RECIPE, pixel_criterion="l1", pixel_weight=1e-2, of_type="overflow", of_weight=0.2, spl_type="gpl", spl_weight=1e-3,
                 grad_type="grad-4d-l1", grad_weight=4e-1)
    gl = losses.GeneratorLoss(_opt(train), device="cpu")
    assert [(l["name"], l["weight"]) for l in gl.loss_list] == [("pix-l1", 1e-2), ("gpl", 1e-3), ("overflow", 0.2), ("color-l1cosinesim", 1),
                                                                ("avg-l1", 5), ("pix-multiscale-l1", 1e-2)]
    assert [l["name"] for l in gl.precise_loss_list] == ["grad-4d-l1"]
    by_name = {l["name"]: l["function"] for l in gl.loss_list}
    avg, ms = by_name["avg-l1"], by_name["pix-multiscale-l1"]
    assert isinstance(avg, PL.AverageLoss) and avg.k == 4 and not avg.uv and avg.crit == ops.CRIT_L1
    assert isinstance(ms, PL.MultiscalePixelLoss) and ms.crit == ops.CRIT_L1 and ms.weights == [1, 0.5, 0.25, 0.125, 0.125]
    # every criterion under every loss, by name
    crits = {"l1": ops.CRIT_L1, "l2": ops.CRIT_L2, "cb": ops.CRIT_CB, "elastic": ops.CRIT_ELASTIC, "clipl1": ops.CRIT_CLIPL1,
             "l1cosinesim": ops.CRIT_L1COS}
    for kind, built in (("color", "color-%s"), ("avg", "avg-%s"), ("multiscale", "pix-multiscale-%s")):
        for c, code in crits.items():
            entry = losses.get_loss_fn("%s-%s" % (kind, c), 3, device="cpu", opt={"scale": 2})
            assert entry["name"] == built % c and entry["weight"] == 3 and entry["function"].crit == code
            if kind != "multiscale":
                assert entry["function"].k == 2
    assert not {"color_weight", "avg_weight", "ms_weight"} & set(losses.GeneratorLoss._UNSUPPORTED)
    assert set(losses.GeneratorLoss._UNSUPPORTED) == {"lpips_weight", "fft_weight", "fdpl_weight", "range_weight"}


def test_what_builds_nothing_and_the_pinned_refusals():
    from trainner_amd.models import losses
    # a criterion without a weight builds nothing, as in the reference
    for train in ({"color_criterion": "color-l1"}, {"avg_criterion": "avg-l1", "avg_weight": 0}, {"ms_criterion": "multiscale-l1"}):
        gl = losses.GeneratorLoss(_opt(train), device="cpu")
        assert gl.loss_list == [] and gl.precise_loss_list == [], train
    # a weight without its criterion is refused by name (tests/test_cpu_spl.py pins this)
    for wkey, ckey in (("color_weight", "color_criterion"), ("avg_weight", "avg_criterion"), ("ms_weight", "ms_criterion")):
        with pytest.raises(NotImplementedError, match="'%s' is set but '%s' is not" % (wkey, ckey)):
            losses.GeneratorLoss({"train": {wkey: 1}}, device="cpu")
    # the new criterion stays out of the pixel, HFEN and image-gradient losses (tests/test_cpu_image_losses.py pins this)
    for crit in ("l1cosinesim", "multiscale-l1"):
        with pytest.raises(NotImplementedError, match=re.escape(crit)):
            losses.GeneratorLoss({"train": {"pixel_criterion": crit, "pixel_weight": 1}}, device="cpu")
    with pytest.raises(NotImplementedError, match="l1cosinesim"):
        losses.GeneratorLoss({"train": {"hfen_criterion": "l1cosinesim", "hfen_weight": 1}}, device="cpu")
    with pytest.raises(NotImplementedError, match="l1cosinesim"):
        losses.GeneratorLoss({"train": {"grad_type": "grad-2d-l1cosinesim", "grad_weight": 1}}, device="cpu")
    # the remaining refusals
    for k in ("fft_weight", "fdpl_weight", "range_weight", "lpips_weight"):
        with pytest.raises(NotImplementedError, match=k):
            losses.GeneratorLoss({"train": {k: 1}}, device="cpu")


def test_refused_option_values_are_named():
    from trainner_amd.models import losses
    from trainner_amd.models.modules import image_losses as IL
    from trainner_amd.models.modules import pooled_losses as PL
    l1 = IL.criterion("l1")
    for kind in ("color", "avg", "multiscale"):
        for crit in ("relativel1", "fro"):
            with pytest.raises(NotImplementedError, match=crit):
                losses.get_loss_fn("%s-%s" % (kind, crit), 1, device="cpu", opt={"scale": 4})
    with pytest.raises(NotImplementedError, match="color-l1-extra"):
        losses.get_loss_fn("color-l1-extra", 1, device="cpu", opt={"scale": 4})
    with pytest.raises(NotImplementedError, match=r"color_criterion \[l1\]"):
        losses.GeneratorLoss(_opt({"color_criterion": "l1", "color_weight": 1}), device="cpu")
    with pytest.raises(ValueError, match="scale"):
        losses.get_loss_fn("avg-l1", 1, device="cpu", opt={})
    for cls in (PL.ColorLoss, PL.AverageLoss):
        for ds_f in (None, nn.MaxPool2d(4), nn.AvgPool2d(4, stride=2), nn.AvgPool2d((4, 2)), nn.AvgPool2d(4, padding=1),
                     nn.AvgPool2d(4, ceil_mode=True), nn.AvgPool2d(4, divisor_override=3)):
            with pytest.raises(NotImplementedError, match="ds_f="):
                cls(loss_f=l1, ds_f=ds_f)
        with pytest.raises(NotImplementedError, match="kernel_size 9 > 8"):
            cls(loss_f=l1, ds_f=nn.AvgPool2d(9))
        assert cls(loss_f=l1, ds_f=nn.AvgPool2d((8, 8), stride=8)).k == 8
        for bad in (None, nn.L1Loss(), IL.criterion("l1", "sum")):
            with pytest.raises(NotImplementedError, match="loss_f"):
                cls(loss_f=bad, ds_f=nn.AvgPool2d(4))
    with pytest.raises(NotImplementedError, match="scale=4"):
        PL.MultiscalePixelLoss(loss_f=l1, scale=4)
    with pytest.raises(NotImplementedError, match="loss_f"):
        PL.MultiscalePixelLoss(loss_f=nn.L1Loss())
    with pytest.raises(NotImplementedError, match="loss_lambda=3"):
        PL.L1CosineSim(loss_lambda=3)
    with pytest.raises(NotImplementedError, match="reduction='sum'"):
        PL.L1CosineSim(reduction="sum")
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="mask"):
        PL.MultiscalePixelLoss(loss_f=l1)(x, x, mask=torch.ones(1, 1, 32, 32))
    with pytest.raises(ValueError, match="reference fails there too"):
        PL.MultiscalePixelLoss(loss_f=l1)(torch.rand(1, 3, 15, 40), torch.rand(1, 3, 15, 40))
    with pytest.raises(NotImplementedError, match="3 x H x W"):
        PL.ColorLoss(loss_f=l1, ds_f=nn.AvgPool2d(4))(torch.rand(1, 4, 16, 16), torch.rand(1, 4, 16, 16))
    for f in (PL.AverageLoss(loss_f=l1, ds_f=nn.AvgPool2d(4)), PL.MultiscalePixelLoss(loss_f=l1), PL.L1CosineSim()):
        with pytest.raises(NotImplementedError, match=r"\(1\.\.4\)"):
            f(torch.rand(1, 5, 16, 16), torch.rand(1, 5, 16, 16))


class _Recorder:
    def __init__(self, calls, name):
        self.calls, self.name = calls, name

    def __call__(self, *args):
        self.calls.append((self.name, args))
        return torch.tensor(1.0)


def test_regular_and_frequency_separated_routing():
    """Under fs the multi-scale term (a `pix-` name) sees the low-passed pair, the colour and average terms the unfiltered one
    (calc_losses_fs); all three get fp32 operands whatever the incoming precision."""
    from trainner_amd.dataops import filters
    from trainner_amd.models import losses

    filtered = []

    class StubLow(filters.FilterLow):
        def forward(self, t):
            assert t.dtype == torch.float32
            filtered.append(t)
            return t * 0.5

    gl = losses.GeneratorLoss(_opt(dict(RECIPE, ms_weight=0.25, of_type="overflow", of_weight=3.0)), device="cpu")
    calls = []
    for l in gl.loss_list:
        l["function"] = _Recorder(calls, l["name"])
    names = ["overflow", "color-l1cosinesim", "avg-l1", "pix-multiscale-l1"]
    sr, hr = torch.rand(1, 3, 16, 16).half(), torch.rand(1, 3, 16, 16).half()
    results, log = gl(sr, hr, {})
    assert [c[0] for c in calls] == names and list(log) == names
    assert [r.item() for r in results] == [3.0, 1.0, 5.0, 0.25]
    for name, args in calls[1:]:
        assert len(args) == 2 and all(a.dtype == torch.float32 for a in args)
        assert torch.equal(args[0], sr.float()) and torch.equal(args[1], hr.float())
    del calls[:]
    results, log = gl(sr, hr, {}, fsfilter=StubLow())
    assert [c[0] for c in calls] == names and list(log) == names
    assert [r.item() for r in results] == [3.0, 1.0, 5.0, 0.25]
    by_name = dict(calls)
    for name in ("color-l1cosinesim", "avg-l1"):
        assert torch.equal(by_name[name][0], sr.float()) and torch.equal(by_name[name][1], hr.float())
    assert torch.equal(by_name["pix-multiscale-l1"][0], sr.float() * 0.5) and torch.equal(by_name["pix-multiscale-l1"][1], hr.float() * 0.5)
    assert len(filtered) == 2                              # sr and hr once each: overflow and multi-scale share the memo


@pytest.mark.parametrize("model", ["pix2pix", "cyclegan"])
def test_image_to_image_models_construct_with_the_three_terms(model, tmp_path):
    """The Pix2Pix and CycleGAN models use the same GeneratorLoss; their recipes have scale 1, so the pool is the identity."""
    from oracle import ref_harness
    from trainner_amd.models import losses
    from trainner_amd.options import options
    yml = ref_harness.i2i_yaml(name="cpu_pooled_" + model, model=model, out_root=str(tmp_path))
    with open(yml) as fh:
        txt = fh.read()
    assert txt.count("\n  manual_seed:") == 1
    lines = "".join("\n  %s: %s" % kv for kv in RECIPE.items())
    with open(yml, "w") as fh:
        fh.write(txt.replace("\n  manual_seed:", lines + "\n  manual_seed:"))
    opt = options.parse(yml, is_train=True)
    gl = losses.GeneratorLoss(opt, device="cpu")
    assert [(l["name"], l["weight"]) for l in gl.loss_list] == [("pix-l1", opt["train"]["pixel_weight"]), ("color-l1cosinesim", 1),
                                                                ("avg-l1", 5), ("pix-multiscale-l1", 1e-2)]
    assert gl.loss_list[1]["function"].k == 1 and gl.loss_list[2]["function"].k == 1


def test_shipped_sr_recipe_with_the_six_lines_parses_and_constructs(tmp_path):
    """options/sr/train_sr.yml with its six colour / average / multi-scale lines uncommented."""
    from oracle import fixtures as FX
    from trainner_amd.models import losses
    from trainner_amd.options import options
    opt = options.parse(FX.write_recipe("sr/train_sr.yml", str(tmp_path), lambda tree: tree["train"].update(RECIPE)), is_train=True)
    assert opt["scale"] == 4
    train = {k: v for k, v in opt["train"].items() if k not in ("feature_weight", "feature_criterion")}   # (no VGG on the CPU)
    gl = losses.GeneratorLoss(dict(opt, train=train), device="cpu")
    assert [(l["name"], l["weight"]) for l in gl.loss_list] == [("pix-l1", 1e-2), ("color-l1cosinesim", 1), ("avg-l1", 5),
                                                                ("pix-multiscale-l1", 1e-2)]
    assert gl.loss_list[1]["function"].k == 4 and gl.loss_list[2]["function"].k == 4


def test_header_and_exports_declare_the_new_entry_points():
    from trainner_amd import hip, ops
    with open(os.path.join(ROOT, "include", "trainner_hip.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"\b(tnr_\w+)\s*\(", text))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(hip.EXPORTS)
    assert re.search(r"TNR_CRIT_L1COS\s*=\s*%d\b" % ops.CRIT_L1COS, text)
    lib = hip.load()          # types every export: a symbol the library lacks raises here
    assert lib.tnr_version() == hip.ABI_VERSION          # no descriptor changed
    # the ticket's 16 bytes, then one fp64 slot per block of the multi-scale forward (two per block of the pool forward), up to the
    # largest grid an override may ask for
    assert lib.tnr_pooled_workspace_bytes() == 16 + 4096 * 8
    assert lib.tnr_pooled_forward_blocks(2049, 0) != 0 and lib.tnr_pooled_forward_blocks(0, 4097) != 0
    assert lib.tnr_pooled_forward_blocks(2048, 4096) == 0 and lib.tnr_pooled_forward_blocks(0, 0) == 0


def test_library_refuses_what_the_kernels_do_not_implement():
    """Argument checks run before any launch, so they need no device.  The pointers are those of real tensors, large enough for every
    shape below and on the device where one is visible: should a check ever regress there, the launch it lets through stays in bounds."""
    from trainner_amd import hip
    lib = hip.load()
    buf = torch.zeros(1 << 16, device="cuda" if torch.cuda.is_available() else "cpu")
    ws = torch.zeros(1 << 13, dtype=torch.float64, device=buf.device)
    p, q, w = buf.data_ptr(), buf.data_ptr() + (1 << 17), ws.data_ptr()

    def refused(rc, word):
        msg = lib.tnr_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)

    n = ws.numel() * 8
    refused(lib.tnr_pool_loss_fwd(p, p, 1, 3, 32, 32, 0, 9, 0, 0, w, w, n, None), "pool k")
    refused(lib.tnr_pool_loss_fwd(p, p, 1, 3, 32, 32, 0, 0, 0, 0, w, w, n, None), "pool k")
    refused(lib.tnr_pool_loss_fwd(p, p, 1, 4, 32, 32, 0, 4, 1, 0, w, w, n, None), "UV map needs 3 channels")
    refused(lib.tnr_pool_loss_fwd(p, p, 1, 5, 32, 32, 0, 4, 0, 0, w, w, n, None), "at most 4 channels")
    refused(lib.tnr_pool_loss_fwd(p, p, 1, 3, 32, 32, 0, 4, 0, 6, w, w, n, None), "unknown criterion")
    refused(lib.tnr_pool_loss_fwd(p, p, 1, 3, 3, 32, 0, 4, 0, 0, w, w, n, None), "no 4 x 4 cell")
    refused(lib.tnr_pool_loss_fwd(p, p, 1, 3, 32, 32, 0, 4, 0, 0, w, w, 8, None), "workspace")
    refused(lib.tnr_pool_loss_bwd(p, p, 1, 3, 32, 32, 0, 4, 0, 0, None, p, 0, None), "aliased")
    refused(lib.tnr_multiscale_loss_fwd(p, p, 1, 3, 15, 32, 0, 0, w, w, n, None), "min(H, W) >= 16")
    refused(lib.tnr_multiscale_loss_bwd(p, p, 1, 5, 32, 32, 0, 0, None, q, 0, None), "at most 4 channels")
    refused(lib.tnr_multiscale_loss_bwd(p, p, 1, 3, 32, 32, 2, 0, None, q, 0, None), "layout")


def test_no_device_no_fallback():
    """Without a HIP device the modules raise; they never compute in eager PyTorch."""
    from trainner_amd import hip
    from trainner_amd.models import losses
    if torch.cuda.is_available():
        pytest.skip("a device is visible: the device path is covered by tests/test_gpu_pooled_losses.py")
    x = torch.rand(2, 3, 40, 40)
    for name in T.RECIPE:
        f = losses.get_loss_fn(name, 1, device="cpu", opt={"scale": 4})["function"]
        with pytest.raises(hip.HipEngineError):
            f(x, x)
