"""LPIPS metric (net-lin / squeeze / v0.1) without kernels: parameter layout against the reference PNetLin's (tests/golden/lpips_squeeze.pt,
tools/make_golden_lpips.py), torchvision key mapping, weight resolution, the fp64 restatement the GPU tests compare with, and that
restatement's ability to see the two likely mistakes (floor-mode pooling, a dropped layer)."""
import os

import pytest
import torch

from oracle import ref_harness
from tools import make_golden_lpips as G

FX = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_squeeze.pt"), weights_only=False)


def bound(ref):
    return 1e-4 * abs(ref) + 1e-6


def test_state_dict_matches_reference_pnetlin():
    from trainner_amd.models.modules.LPIPS.perceptual_loss import PerceptualLoss
    m = PerceptualLoss(allow_random_init=True)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == FX["pnet_keys"]
    assert m.weights_source == {"net": "random-init", "lin": "random-init"}


def test_torchvision_key_mapping():
    from trainner_amd.models.modules.LPIPS.networks_basic import torchvision_to_slices
    from trainner_amd.models.modules.LPIPS.perceptual_loss import PerceptualLoss
    tv = G.seeded_backbone_state(FX["seed"], FX["gain"])
    assert [(k, tuple(v.shape)) for k, v in tv.items()] == FX["tv_keys"]
    mapped = torchvision_to_slices(dict(tv, **{"classifier.1.weight": torch.zeros(1000, 512, 1, 1)}))
    assert mapped["net.slice1.0.weight"] is tv["features.0.weight"]
    assert mapped["net.slice2.4.expand3x3.bias"] is tv["features.4.expand3x3.bias"]
    assert mapped["net.slice7.12.squeeze.weight"] is tv["features.12.squeeze.weight"]
    assert len(mapped) == len(tv) and not any("classifier" in k for k in mapped)
    m = PerceptualLoss(allow_random_init=True)
    m.load_torchvision_state(tv)
    m.load_heads(FX["lin"])
    sd = m.state_dict()
    for k, v in mapped.items():
        assert torch.equal(sd[k], v), k
    for k, v in FX["lin"].items():
        assert torch.equal(sd[k], v), k
    with pytest.raises(KeyError):
        m.load_torchvision_state({"features.0.weight": tv["features.0.weight"]})


def test_weight_resolution(tmp_path, monkeypatch):
    from trainner_amd.models.modules.LPIPS.perceptual_loss import LPIPSWeightsUnavailable, PerceptualLoss
    from trainner_amd.utils.metrics import MetricsDict
    hub = tmp_path / "torch_home"
    lp = tmp_path / "lpips_weights"
    monkeypatch.setenv("TORCH_HOME", str(hub))
    monkeypatch.setenv("TNR_LPIPS_WEIGHTS", str(lp))
    bpath = os.path.join(str(hub), "hub", "checkpoints", "squeezenet1_1-b8a52dc0.pth")
    lpath = os.path.join(str(lp), "v0.1", "squeeze.pth")
    with pytest.raises(LPIPSWeightsUnavailable) as e:
        PerceptualLoss()
    assert isinstance(e.value, NotImplementedError) and bpath in str(e.value) and lpath in str(e.value)
    with pytest.raises(NotImplementedError):
        MetricsDict("psnr,lpips")
    os.makedirs(os.path.dirname(bpath))
    torch.save(G.seeded_backbone_state(FX["seed"], FX["gain"]), bpath)
    with pytest.raises(LPIPSWeightsUnavailable):                 # the heads are still missing
        PerceptualLoss()
    os.makedirs(os.path.dirname(lpath))
    torch.save(FX["lin"], lpath)
    m = PerceptualLoss()
    assert m.weights_source == {"net": bpath, "lin": lpath}
    assert torch.equal(m.state_dict()["lin3.model.1.weight"], FX["lin"]["lin3.model.1.weight"])
    assert MetricsDict("psnr,ssim,lpips").lpips_model.weights_source == m.weights_source
    os.remove(bpath)
    with pytest.raises(LPIPSWeightsUnavailable):
        PerceptualLoss()


def test_unsupported_options_raise():
    from trainner_amd.models.modules.LPIPS.perceptual_loss import PerceptualLoss
    for kw in (dict(net="alex"), dict(net="vgg"), dict(spatial=True), dict(version="0.0"), dict(model="net")):
        with pytest.raises(NotImplementedError):
            PerceptualLoss(allow_random_init=True, **kw)


def test_restatement_matches_reference_and_sees_mistakes():
    tv = G.seeded_backbone_state(FX["seed"], FX["gain"])
    for p in FX["pairs"]:
        ref = p["total"]
        t, per_layer = G.restate(tv, FX["lin"], p["img1"], p["img2"], crop=p["crop"])
        assert abs(t - ref) <= bound(ref), (p["name"], t, ref)
        for got, want in zip(per_layer, p["per_layer"]):
            assert abs(got - want) <= bound(want), (p["name"], per_layer, p["per_layer"])
        if p["name"] in ("same", "pm1"):
            continue
        for drop in range(7):
            t_drop, _ = G.restate(tv, FX["lin"], p["img1"], p["img2"], crop=p["crop"], drop_layer=drop)
            assert abs(t_drop - ref) > 10 * bound(ref), (p["name"], drop)
        if p["name"] in ("even66", "odd35x50"):            # sizes where ceil-mode pooling changes the output grid
            t_floor, _ = G.restate(tv, FX["lin"], p["img1"], p["img2"], crop=p["crop"], ceil_mode=False)
            assert abs(t_floor - ref) > 10 * bound(ref), p["name"]
    assert FX["pairs"][3]["name"] == "same" and FX["pairs"][3]["total"] == 0.0
    assert abs(FX["average"] - sum(p["total"] for p in FX["pairs"]) / len(FX["pairs"])) < 1e-12


@pytest.mark.skipif(not ref_harness.reference_available(), reason="needs the reference tree (build container only)")
def test_golden_regenerates():
    fx = G.build_fixture()
    assert fx["seed"] == FX["seed"] and fx["gain"] == FX["gain"] and fx["tv_keys"] == FX["tv_keys"] and fx["pnet_keys"] == FX["pnet_keys"]
    assert fx["average"] == FX["average"]
    for k, v in FX["lin"].items():
        assert torch.equal(fx["lin"][k], v)
    for a, b in zip(fx["pairs"], FX["pairs"]):
        assert a["name"] == b["name"] and torch.equal(a["img1"], b["img1"]) and torch.equal(a["img2"], b["img2"])
        assert a["total"] == b["total"] and a["per_layer"] == b["per_layer"]
