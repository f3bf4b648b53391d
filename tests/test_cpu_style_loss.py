"""Style loss and multi-layer perceptual taps, the parts that need no GPU: the fp64 restatements of tools/make_golden_style.py against
the fixture made from the real reference (tests/golden/style_loss.pt), construction of the multi-tap FeatureExtractor with the
reference's truncation and state_dict keys, PerceptualLoss's resolution of the two layer dictionaries (losses.py:265-293),
GeneratorLoss's `fea` entry for a style-only config, and the options that stay refused."""
import pytest
import torch

from oracle import fixtures as FX
from tools import make_golden_style as T
from trainner_amd.models import losses as L
from trainner_amd.models.modules.architectures.perceptual import FeatureExtractor, vgg_layer_names


@pytest.fixture(scope="module")
def fx():
    return FX.load("style_loss")


def _probe_close(t, pr, tol=1e-12):
    s = t.detach().contiguous().flatten().double()
    assert s.numel() == pr["numel"]
    scale = max(1.0, pr["samples"].abs().max().item())
    assert (s[::pr["stride"]][:len(pr["samples"])] - pr["samples"]).abs().max().item() <= tol * scale
    assert abs(s.norm().item() - pr["l2"]) <= 1e-10 * max(1.0, pr["l2"])


@pytest.mark.parametrize("case", T.GRAM_CASES)
def test_gram_restatement_matches_reference_fixture(fx, case):
    x, S = T.gram_inputs(case)
    rec = fx["gram"][case]
    _probe_close(T.gram(x.double()), rec["G"])
    _probe_close(T.gram_grad(x.double(), S.double()), rec["dx"])


@pytest.mark.parametrize("name", sorted(T.EXTRACTOR_CASES))
def test_extractor_restatement_matches_reference_fixture(fx, name):
    sd = FX.initial_state(fx["extractor_keys"], T.VGG_FILL_SEED, gain=1.0, bias_amp=0.05)
    x, _ = T.extractor_inputs(name)
    x = x.double().requires_grad_(True)
    feats = T.extract(x, sd, T.TAPS)
    assert list(feats) == list(T.TAPS)
    maps = T.tap_maps(feats)
    sum((feats[k] * maps[k].double()).sum() for k in feats).backward()
    rec = fx["extractor"][name]
    for k in T.TAPS:
        assert tuple(feats[k].shape) == rec["taps"][k]["shape"]
        _probe_close(feats[k], rec["taps"][k]["fea"])
    _probe_close(x.grad, rec["grad"])


def test_perceptual_restatement_matches_reference_fixture(fx):
    rec = fx["perceptual"]
    sd = FX.initial_state(rec["keys"], T.VGG_FILL_SEED, gain=1.0, bias_amp=0.05)
    listen = list(dict(T.PERC_LAYERS, **T.STYLE_LAYERS))
    x, y = T.extractor_inputs("b2_32")
    x = x.double().requires_grad_(True)
    p, s = T.perceptual_terms(T.extract(x, sd, listen), T.extract(y.double(), sd, listen), T.PERC_LAYERS, T.STYLE_LAYERS, 1.0, 2.0)
    (p + s).backward()
    assert abs(p.item() - rec["percep"]) <= 1e-12 and abs(s.item() - rec["style"]) <= 1e-12
    _probe_close(x.grad, rec["grad"])


@pytest.mark.parametrize("listen", [["conv1_2", "relu2_2", "pool2", "conv3_4"], ["relu1_1", "relu2_1", "relu3_1"], ["pool5", "conv1_1"],
                                    ["conv5_4"]])
def test_feature_extractor_constructs_with_reference_truncation_and_keys(listen):
    net = FeatureExtractor(listen_list=listen, allow_random_init=True)
    names = vgg_layer_names("vgg19")
    last = max(names.index(v) for v in listen)
    assert net.names == names[:last + 1]                                   # perceptual.py:129-144
    assert net.listen_list == set(listen)
    assert net.taps == [n for n in names if n in listen]                   # network order
    convs = [n for n in names[:last + 1] if n.startswith("conv")]
    want = [k for n in convs for k in ("feature_net.%s.weight" % n, "feature_net.%s.bias" % n)] + ["mean", "std"]
    assert sorted(net.state_dict().keys()) == sorted(want)
    assert all(not p.requires_grad for p in net.parameters())


def test_extractor_fixture_keys_are_the_engine_keys(fx):
    net = FeatureExtractor(listen_list=list(T.TAPS), allow_random_init=True)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items() if k.startswith("feature_net")] == fx["extractor_keys"]


def test_feature_extractor_rejects_an_unknown_layer():
    with pytest.raises(ValueError, match="conv9_9"):
        FeatureExtractor(listen_list=["conv1_1", "conv9_9"], allow_random_init=True)


@pytest.mark.parametrize("option", ["remove_pooling", "change_padding", "requires_grad", "z_norm"])
def test_refused_extractor_options_name_themselves(option):
    with pytest.raises(NotImplementedError, match=option):
        FeatureExtractor(listen_list=["conv1_2", "relu2_2"], allow_random_init=True, **{option: True})


@pytest.mark.parametrize("option", ["rotations", "flips"])
def test_refused_perceptual_options_name_themselves(option):
    opt = {"train": {"feature_weight": 1, "style_weight": 1, "perceptual_opt": {"perceptual_layers": {"conv1_2": 1}, option: True}}}
    with pytest.raises(NotImplementedError, match=option):
        L.PerceptualLoss(criterion=None, network=None, opt=opt)


P, S = {"conv1_2": 0.1, "conv3_4": 1}, {"relu2_2": 1, "relu4_2": 2}


@pytest.mark.parametrize("layers_p, layers_s, want_p, want_s", [
    (P, S, P, S),
    (P, {}, P, P),               # empty style_layers: the style term uses the perceptual layers
    ({}, S, S, S),               # empty perceptual layers: the perceptual term uses the style layers
    ({}, {}, {}, {}),
])
def test_perceptual_loss_resolves_the_layer_dictionaries_like_the_reference(layers_p, layers_s, want_p, want_s):
    opt = {"train": {"feature_weight": 0.5, "style_weight": 3.0,
                     "perceptual_opt": {"perceptual_layers": dict(layers_p), "style_layers": dict(layers_s)}}}
    pl = L.PerceptualLoss(criterion=None, network=None, opt=opt)
    assert (pl.perceptual_weight, pl.style_weight) == (0.5, 3.0)
    assert pl.w_l_p == want_p and pl.w_l_s == want_s


def test_perceptual_loss_defaults():
    pl = L.PerceptualLoss(criterion=None, network=None, opt=None)
    assert (pl.perceptual_weight, pl.style_weight, pl.w_l_p) == (1.0, 0.0, {"conv5_4": 1}) and not hasattr(pl, "w_l_s")
    pl = L.PerceptualLoss(criterion=None, network=None, opt={"train": {"feature_weight": 1, "style_weight": 2}})
    assert pl.w_l_p == {"conv5_4": 1} and pl.w_l_s == {"conv5_4": 1}
    pl = L.PerceptualLoss(criterion=None, network=None, opt={"train": {"style_weight": 2, "perceptual_opt": {"style_layers": {"relu1_1": 1}}}})
    assert pl.perceptual_weight == 0 and not hasattr(pl, "w_l_p") and pl.w_l_s == {"relu1_1": 1}


def _opt(train):
    base = {"pixel_criterion": "l1", "pixel_weight": 1e-2, "feature_criterion": "l1", "perceptual_allow_random_init": True}
    base.update(train)
    return {"train": base, "datasets": {"train": {"znorm": False}}}


def test_generator_loss_builds_the_fea_entry_for_a_style_only_config():
    gl = L.GeneratorLoss(_opt({"style_weight": 5.0, "perceptual_opt": {"perceptual_layers": {}, "style_layers": {"relu1_2": 1, "relu3_3": 1}}}),
                         device="cpu")
    assert [l["name"] for l in gl.loss_list] == ["pix-l1", "fea-vgg19-l1"] and gl.cri_fea
    fea = gl.loss_list[1]
    assert fea["weight"] == 1
    pl = fea["function"]
    assert pl.perceptual_weight == 0 and pl.style_weight == 5.0 and pl.w_l_s == {"relu1_2": 1, "relu3_3": 1}
    assert pl.network.taps == ["relu1_2", "relu3_3"] and pl.network.names[-1] == "relu3_3"


def test_style_only_config_without_perceptual_layers_still_listens_to_conv5_4_like_the_reference():
    """networks.py:328: define_F's default for a missing `perceptual_layers` is {conv5_4: 1}, whatever the weights."""
    gl = L.GeneratorLoss(_opt({"style_weight": 5.0, "perceptual_opt": {"style_layers": {"relu1_2": 1}}}), device="cpu")
    assert gl.loss_list[1]["function"].network.taps == ["relu1_2", "conv5_4"]


def test_generator_loss_listens_to_the_union_of_both_dictionaries():
    gl = L.GeneratorLoss(_opt({"feature_weight": 1, "style_weight": 30.0,
                               "perceptual_opt": {"perceptual_layers": {"conv1_2": 0.1, "conv3_4": 1, "conv5_4": 1},
                                                  "style_layers": {"relu2_2": 1, "relu4_2": 1}}}), device="cpu")
    net = gl.loss_list[1]["function"].network
    assert net.taps == ["conv1_2", "relu2_2", "conv3_4", "relu4_2", "conv5_4"] and net.names[-1] == "conv5_4"


def test_fea_effective_skips_a_none_term():
    l = {"weight": 2.0}
    a, b = torch.tensor(3.0), torch.tensor(0.5)
    assert L.GeneratorLoss._fea_effective(l, a, None).item() == 6.0
    assert L.GeneratorLoss._fea_effective(l, None, b).item() == 1.0
    assert L.GeneratorLoss._fea_effective(l, a, b).item() == 7.0
