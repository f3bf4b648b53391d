"""Contextual loss, the parts that need no GPU: the fp64 restatements of tools/make_golden_contextual.py against the fixture made from the
real reference (tests/golden/contextual.pt), GeneratorLoss's `contextual` entry (name, weight, position, the reference's conditions),
the shipped recipe with its three cx lines uncommented, the constructor options that stay refused, the reference's layer-name mapping and
the operands frequency separation hands the term."""
import math

import pytest
import torch

from oracle import fixtures as FX
from tools import make_golden_contextual as T
from trainner_amd.models import losses as L
from trainner_amd.models.modules.contextual import Contextual_Loss, alt_layers_names

CX = {"cx_type": "contextual", "cx_weight": 0.5, "cx_vgg_layers": {"conv_3_2": 1, "conv_4_2": 1}}


@pytest.fixture(scope="module")
def fx():
    return FX.load("contextual")


def _probe_close(t, pr, tol=1e-12):
    s = t.detach().contiguous().flatten().double()
    assert s.numel() == pr["numel"]
    scale = max(1.0, pr["samples"].abs().max().item())
    assert (s[::pr["stride"]][:len(pr["samples"])] - pr["samples"]).abs().max().item() <= tol * scale
    assert abs(s.norm().item() - pr["l2"]) <= 1e-10 * max(1.0, pr["l2"])


@pytest.mark.parametrize("case", T.KERNEL_CASES + (T.POOLED_CASE,), ids=lambda c: "-".join(map(str, c)))
def test_restatements_match_the_reference_fixture(fx, case):
    rec = fx["cases"][case]
    X, Y = T.case_inputs(case, rec["seed"])
    idx = (rec["idx_x"], rec["idx_y"]) if case == T.POOLED_CASE else (None, None)
    if case == T.POOLED_CASE:
        assert all(torch.equal(a, b) for a, b in zip(idx, T.pooled_indices()))
    f, g = T.own_gradient(X.double(), Y.double(), *idx)
    assert abs(f["loss"].item() - rec["loss"]) <= 1e-12 * max(1.0, abs(rec["loss"]))
    assert (f["CS"] - rec["CS"]).abs().max().item() <= 1e-12
    for k in ("d", "rowmin", "colmax"):
        _probe_close(f[k], rec[k])
    _probe_close(g, rec["dx"])
    # the restatement that takes the pattern as inputs, on the fp64 run's own pattern, is the same gradient
    gp = T.grad_under_pattern(X, Y, f["argmax"], f["argmin"], f["passes"], *idx)
    assert (gp - g).abs().max().item() <= 1e-12 * max(1.0, rec["dx_absmax"])
    P = idx[0].numel() if idx[0] is not None else case[1] * case[2]
    assert 0.05 <= rec["loss"] <= math.log(P) + 0.05 and rec["dx_absmax"] >= T.GRAD_FLOOR.get(case, 1e-4)
    assert rec["e32_CS"] >= 2.0 ** -24 * rec["CS_absmax"] and rec["e32_loss"] >= 2.0 ** -24 * rec["loss_absmax"]


def test_module_restatement_matches_the_reference_fixture(fx):
    rec = fx["module"]
    sd = FX.initial_state(rec["keys"], T.VGG_FILL_SEED, gain=1.0, bias_amp=0.05)
    x, y = T.module_inputs()
    for indices, want in ((None, rec), (rec["pooled"]["indices"], rec["pooled"])):
        xx = x.double().requires_grad_(True)
        loss = T.module_restatement(xx, y.double(), sd, rec["layers"], indices)
        loss.backward()
        assert abs(loss.item() - want["loss"]) <= 1e-12 * max(1.0, abs(want["loss"]))
        _probe_close(xx.grad, want["grad"])
    # with every ReLU resolved by the fp64 run's own pattern the under-pattern extractor is the extractor
    pattern = {k: v > 0 for k, v in T.S.extract(x.double(), sd, T.relu_convs()).items()}
    a, b = T.extract_under_pattern(x.double(), sd, T.MODULE_TAPS, pattern), T.S.extract(x.double(), sd, T.MODULE_TAPS)
    assert all(torch.equal(a[k], b[k]) for k in T.MODULE_TAPS)


def _opt(train):
    base = {"pixel_criterion": "l1", "pixel_weight": 1e-2, "perceptual_allow_random_init": True}
    base.update(train)
    return {"train": base, "datasets": {"train": {"znorm": False}}}


def test_generator_loss_builds_the_contextual_entry():
    gl = L.GeneratorLoss(_opt(dict(CX, tv_type="normal", tv_norm=1, tv_weight=1e-5, feature_criterion="l1", feature_weight=1)), device="cpu")
    assert [(l["name"], l["weight"]) for l in gl.loss_list] == [("pix-l1", 1e-2), ("tv-l1", 1e-5), ("contextual", 0.5), ("fea-vgg19-l1", 1)]
    cl = gl.loss_list[2]["function"]
    assert isinstance(cl, Contextual_Loss)
    assert cl.layers_weights == {"conv3_2": 1, "conv4_2": 1} and cl.max_1d_size == 64 and (cl.b, cl.band_width) == (1.0, 0.5)
    assert cl.vgg_model.taps == ["conv3_2", "conv4_2"] and cl.vgg_model.names[-1] == "conv4_2"
    assert cl.vgg_model is not gl.loss_list[3]["function"].network          # its own extractor, as in the reference


def test_generator_loss_builds_nothing_without_feature_networks_weight_or_type():
    names = lambda gl: [l["name"] for l in gl.loss_list]          # noqa: E731
    assert names(L.GeneratorLoss(_opt(CX), device="cpu", allow_featnets=False)) == ["pix-l1"]
    assert names(L.GeneratorLoss(_opt(dict(CX, cx_weight=0)), device="cpu")) == ["pix-l1"]
    assert names(L.GeneratorLoss(_opt({k: v for k, v in CX.items() if k != "cx_weight"}), device="cpu")) == ["pix-l1"]
    assert names(L.GeneratorLoss(_opt({k: v for k, v in CX.items() if k != "cx_type"}), device="cpu")) == ["pix-l1"]


def recipe_edit(tree):
    tree["train"].update(CX)
    tree["train"]["perceptual_allow_random_init"] = True          # (no ImageNet file here)


def test_shipped_recipe_with_the_cx_lines_parses_and_constructs(tmp_path):
    """options/sr/train_sr.yml with the first three lines of its optional block uncommented."""
    from trainner_amd.options import options
    opt = options.parse(FX.write_recipe("sr/train_sr.yml", str(tmp_path), recipe_edit), is_train=True)
    gl = L.GeneratorLoss(opt, device="cpu")
    names = [l["name"] for l in gl.loss_list]
    assert names == ["pix-l1", "contextual", "fea-vgg19-l1"]
    assert gl.loss_list[1]["weight"] == 0.5 and gl.loss_list[1]["function"].vgg_model.taps == ["conv3_2", "conv4_2"]


@pytest.mark.parametrize("kw, name", [({"distance_type": "l1"}, "distance_type"), ({"distance_type": "l2"}, "distance_type"),
                                      ({"calc_type": "bilateral"}, "calc_type"), ({"calc_type": "symetric"}, "calc_type"),
                                      ({"crop_quarter": True}, "crop_quarter"), ({"use_vgg": False}, "use_vgg"), ({"z_norm": True}, "z_norm"),
                                      ({"b": 0.0}, "'b'")])
def test_refused_constructor_options_name_themselves(kw, name):
    with pytest.raises(NotImplementedError, match=name):
        Contextual_Loss({"conv_3_2": 1}, allow_random_init=True, **kw)


def test_band_width_and_distance_type_fail_as_in_the_reference():
    with pytest.raises(AssertionError, match="band_width"):
        Contextual_Loss({"conv_3_2": 1}, band_width=0.0, allow_random_init=True)
    with pytest.raises(AssertionError, match="distance type"):
        Contextual_Loss({"conv_3_2": 1}, distance_type="chebyshev", allow_random_init=True)


def test_layer_names_go_through_the_reference_mapping():
    assert alt_layers_names({"conv_3_2": 1, "conv_4_2": 0.5, "conv3_2": 7, "relu_1_1": 2}) == {"conv3_2": 1, "conv4_2": 0.5, "relu1_1": 2}
    with pytest.raises(ValueError, match="conv_3_2"):
        Contextual_Loss({"conv3_2": 1}, allow_random_init=True)
    with pytest.raises(ValueError, match="conv_3_2"):          # the reference's own default, which its mapping empties
        L.GeneratorLoss(_opt({"cx_type": "contextual", "cx_weight": 0.5}), device="cpu")


def test_frequency_separation_hands_the_term_the_unfiltered_pair(monkeypatch):
    from trainner_amd.dataops import filters
    gl = L.GeneratorLoss(_opt(CX), device="cpu")
    seen = []
    cl = gl.loss_list[1]["function"]
    monkeypatch.setattr(type(cl), "forward", lambda self, a, b: (seen.append((a, b)), torch.tensor(2.0))[1])
    pix = gl.loss_list[0]["function"]
    monkeypatch.setattr(type(pix), "forward", lambda self, a, b: torch.tensor(1.0))

    class Low(filters.FilterLow):
        def __init__(self):
            torch.nn.Module.__init__(self)

        def forward(self, t):
            return t + 100.0

    sr, hr = torch.zeros(1, 3, 8, 8), torch.ones(1, 3, 8, 8)
    log = {}
    results, log = gl(sr, hr, log, fsfilter=Low())
    assert len(seen) == 1 and seen[0][0] is sr and seen[0][1] is hr
    assert results[1].item() == 1.0 and log["contextual"].item() == 1.0          # weight 0.5 x 2.0
    seen.clear()
    results, log = gl(sr, hr, {})
    assert len(seen) == 1 and seen[0][0] is sr and seen[0][1] is hr and log["contextual"].item() == 1.0
