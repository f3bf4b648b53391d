"""SSIM / MS-SSIM training losses, CPU side (-m "not gpu"): the fixture against the fp64 restatement the GPU tests compare the
engine with, the option plumbing (`ssim_type` / `ssim_weight` -> GeneratorLoss.precise_loss_list), the host-side level geometry,
and the C ABI's declarations."""
import os
import re

import pytest
import torch

from tools import make_golden_ssim as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ssim_loss.pt")
SSIM_EXPORTS = {"tnr_ssim_workspace_bytes", "tnr_ssim_fwd", "tnr_ssim_bwd", "tnr_avgpool2_pad_dims", "tnr_avgpool2_pad_fwd",
                "tnr_avgpool2_pad_bwd", "tnr_msssim_combine"}


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


def test_fixture_holds_data_only_and_is_small(fx):
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert set(fx["cases"]) == set(G.REGULAR) | set(G.BRANCH) and set(fx["steps"]) == set(G.TYPES)


@pytest.mark.parametrize("kind", G.TYPES)
@pytest.mark.parametrize("name", list(G.REGULAR) + list(G.BRANCH))
def test_fixture_equals_restatement_in_fp64(fx, name, kind):
    rec = fx["cases"][name]
    t = rec["types"][kind]
    sr, hr = G.make_inputs(name)
    assert tuple(sr.shape) == rec["shape"] and sr.is_contiguous(memory_format=torch.channels_last) == (rec["channels_last"] or sr.shape[1] == 1)
    for ten, pr in ((sr, rec["sr"]), (hr, rec["hr"])):
        assert G.probe_error(ten, pr)[0] <= 1e-6
    v, g, detail = G.restate_with_grad(sr, hr, kind)
    assert abs(v.item() - t["value"]) <= 1e-12
    if rec["regular"]:
        es, esum = G.probe_error(g, t["grad"])
        assert es <= 1e-12 and esum <= 1e-10, (es, esum)
        assert abs(g.abs().max().item() - t["grad_absmax"]) <= 1e-12
        # the condition the regular cases were built under: neither branch of the definition is near
        assert detail["clamped"] == 0 and t["clamped32"] == 0 and t["clamped64"] == 0 and t["min_level_value"] > 0.5
        assert 0 < t["e32_grad"] < 1e-3 * t["grad_absmax"] and t["e32_val"] < 1e-5


def test_branch_cases_do_reach_their_branch(fx):
    assert fx["cases"]["clamp_patch"]["types"]["ssim"]["clamped32"] > 0
    assert fx["cases"]["relu_negated"]["types"]["ms-ssim"]["relu_images"] == [1]
    sr, hr = G.make_inputs("relu_negated")
    detail = {}
    G.restate(sr.double(), hr.double(), "ms-ssim", detail=detail)
    assert min(cs[1].item() for _, cs in detail["levels"][:-1]) < 0


@pytest.mark.parametrize("kind", G.TYPES)
def test_half_batch_means_average_to_the_whole_batch_value(kind):
    """Both losses are batch means of per-image terms: the mean of the values of two equal shards is the value of the whole batch,
    which is why the data-parallel gradient needs no collective beyond the gradient averaging (losses.GeneratorLoss._log)."""
    sr, hr = G.make_inputs("sq72")
    sr, hr = sr.double(), hr.double()
    whole = G.restate(sr, hr, kind).item()
    halves = [G.restate(sr[i:i + 1], hr[i:i + 1], kind).item() for i in range(2)]
    assert abs(sum(halves) / 2 - whole) <= 1e-14


def test_generator_loss_builds_the_precise_list_from_options():
    """Fails before this feature: `ssim_weight` used to raise NotImplementedError."""
    from trainner_amd.models import losses
    from trainner_amd.models.modules.ssim import MS_SSIM, SSIM
    gl = losses.GeneratorLoss({"train": {"ssim_type": "ms-ssim", "ssim_weight": 0.5}}, device="cpu")
    assert gl.loss_list == [] and len(gl.precise_loss_list) == 1
    entry = gl.precise_loss_list[0]
    assert entry["name"] == "ms-ssim" and entry["weight"] == 0.5 and isinstance(entry["function"], MS_SSIM)
    assert entry["function"].channels == 3 and entry["function"].normalize == "relu" and entry["function"].data_range == 1.0
    gl = losses.GeneratorLoss({"train": {"ssim_type": "ssim", "ssim_weight": 1, "image_channels": 1}}, device="cpu")
    assert gl.precise_loss_list[0]["name"] == "ssim" and isinstance(gl.precise_loss_list[0]["function"], SSIM)
    assert gl.precise_loss_list[0]["function"].channels == 1
    assert losses.GeneratorLoss({"train": {"ssim_type": "ssim", "ssim_weight": 1}}, device="cpu",
                                allow_featnets=False).precise_loss_list[0]["function"].channels == 1
    # no weight, or no type: nothing is built (losses.py:798)
    assert losses.GeneratorLoss({"train": {"ssim_type": "ssim"}}, device="cpu").precise_loss_list == []
    assert losses.GeneratorLoss({"train": {"ssim_weight": 1}}, device="cpu").precise_loss_list == []
    # the other precise terms stay refused
    for key in ("grad_weight", "fft_weight", "fdpl_weight", "range_weight"):
        with pytest.raises(NotImplementedError):
            losses.GeneratorLoss({"train": {key: 1}}, device="cpu")
    with pytest.raises(NotImplementedError):
        losses.get_loss_fn("ssim-unknown", 1, device="cpu")


def test_shipped_recipe_with_msssim_parses_and_constructs(tmp_path):
    from oracle import fixtures as FX
    from trainner_amd.models import losses
    from trainner_amd.options import options

    def edit(tree):
        tree["train"]["ssim_type"], tree["train"]["ssim_weight"] = "ms-ssim", 1

    opt = options.parse(FX.write_recipe("sr/train_sr.yml", str(tmp_path), edit), is_train=True)
    assert opt["train"]["ssim_type"] == "ms-ssim" and opt["train"]["ssim_weight"] == 1
    train = {k: v for k, v in opt["train"].items() if k not in ("feature_weight", "feature_criterion")}   # (no VGG on the CPU)
    gl = losses.GeneratorLoss({"train": train}, device="cpu")
    assert [(l["name"], l["weight"]) for l in gl.precise_loss_list] == [("ms-ssim", 1)]


def test_level_geometry():
    from trainner_amd.models.modules.ssim import gaussian_taps, msssim_levels, pooled_size
    taps = lambda hw: [(h, w, k) for h, w, k, _ in msssim_levels(hw[0] - 8, hw[1] - 8)]          # noqa: E731
    assert taps((192, 192)) == [(184, 184, 11), (92, 92, 11), (46, 46, 11), (23, 23, 11), (12, 12, 11)]
    assert taps((136, 136)) == [(128, 128, 11), (64, 64, 11), (32, 32, 11), (16, 16, 11), (8, 8, 7)]
    assert taps((72, 72)) == [(64, 64, 11), (32, 32, 11), (16, 16, 11), (8, 8, 7), (4, 4, 3)]
    assert taps((99, 117)) == [(91, 109, 11), (46, 55, 11), (23, 28, 11), (12, 14, 11), (6, 7, 5)]
    # the recipe's HR crop 128: level 5 is 8 x 8... of the 120 x 120 shaved image: 120, 60, 30, 15, 8 -> 7 taps, sigma 1.5 * 7 / 11
    lev = msssim_levels(120, 120)
    assert [l[:3] for l in lev][-1] == (8, 8, 7) and abs(lev[-1][3] - 0.9545454545) < 1e-9
    # sigma carries over: 7 taps at 1.5 * 7 / 11, then 3 taps at that * 3 / 7
    lev = msssim_levels(64, 64)
    assert abs(lev[3][3] - 1.5 * 7 / 11) < 1e-12 and abs(lev[4][3] - 1.5 * 7 / 11 * 3 / 7) < 1e-12 and abs(lev[4][3] - 0.409) < 1e-3
    for h, w in ((91, 109), (46, 55), (23, 28), (7, 7), (2, 3)):
        assert pooled_size(h, w) == tuple(torch.nn.functional.avg_pool2d(torch.zeros(1, 1, h, w), 2, padding=(h % 2, w % 2)).shape[2:])
    # the engine's geometry and taps are the restatement's
    for hw in ((184, 184), (64, 64), (91, 109), (120, 120)):
        assert [tuple(l) for l in msssim_levels(*hw)] == [tuple(l) for l in G.level_table(*hw)]
    for k, s in ((11, 1.5), (7, 1.5 * 7 / 11), (3, 0.409), (5, 0.68)):
        assert torch.equal(gaussian_taps(k, s), G.window(k, s))
    assert abs(gaussian_taps(11, 1.5).sum().item() - 1) < 1e-6
    with pytest.raises(ValueError):
        msssim_levels(3, 3)          # 3 -> 2 -> 1: a 1-pixel level cannot be pooled again, five levels are out of reach


def test_unsupported_options_raise():
    from trainner_amd.models.modules.ssim import MS_SSIM, SSIM
    for kw in (dict(size_average=False), dict(use_padding=True), dict(per_channel=True), dict(full=True), dict(compensation=0.9),
               dict(win=torch.ones(3, 1, 1, 11)), dict(window_size=13)):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            SSIM(data_range=1., **kw)
    for kw in (dict(size_average=False), dict(use_padding=True), dict(option=2), dict(normalize=False), dict(normalize=None),
               dict(levels=3), dict(weights=torch.ones(5)), dict(win=torch.ones(3, 1, 1, 11))):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            MS_SSIM(data_range=1., **({"normalize": "relu"} | kw))
    with pytest.raises(ValueError):
        SSIM(window_size=10)
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="nonnegative_ssim"):
        SSIM(data_range=1.)(x, x, nonnegative_ssim=True)
    for mod in (SSIM(data_range=1.), MS_SSIM(data_range=1., normalize="relu")):
        with pytest.raises(RuntimeError, match="channels"):
            mod(torch.zeros(2, 1, 32, 32), torch.zeros(2, 1, 32, 32))
        with pytest.raises(ValueError):
            mod(torch.zeros(2, 3, 8, 32), torch.zeros(2, 3, 8, 32))          # nothing left after the shave
        with pytest.raises(ValueError):
            mod(x, torch.zeros(2, 3, 32, 16))
        with pytest.raises(ValueError):
            mod(x[0], x[0])
    # the modules keep the reference's parameters (names and shapes)
    assert tuple(SSIM(channels=3).window.shape) == (3, 1, 1, 11) and tuple(MS_SSIM(normalize="relu").weights.shape) == (5,)


def test_header_and_exports_declare_the_ssim_entry_points():
    from trainner_amd import hip
    with open(os.path.join(ROOT, "include", "trainner_hip.h")) as fh:
        declared = set(re.findall(r"\b(tnr_\w+)\s*\(", fh.read()))
    assert SSIM_EXPORTS <= declared and SSIM_EXPORTS <= set(hip.EXPORTS)
    lib = hip.load()
    assert lib.tnr_version() == hip.ABI_VERSION == 3          # no descriptor changed
    # 16 x 3 x 512 x 512, shave 4, 11 taps: 494 x 494 maps in 16 x 16 tiles of 32 x 32, {ssim, cs} fp64 per tile
    assert lib.tnr_ssim_workspace_bytes(16, 3, 512, 512, 4, 11) == 16 * 3 * 16 * 16 * 2 * 8
    assert lib.tnr_ssim_workspace_bytes(1, 3, 8, 8, 4, 11) == 0
    import ctypes as C
    ho, wo = C.c_int32(), C.c_int32()
    assert lib.tnr_avgpool2_pad_dims(99, 117, 4, C.byref(ho), C.byref(wo)) == 0 and (ho.value, wo.value) == (46, 55)


def test_no_device_no_fallback():
    """Without a HIP device the modules raise; they never compute in eager PyTorch."""
    from trainner_amd import hip
    from trainner_amd.models.modules.ssim import MS_SSIM, SSIM
    if torch.cuda.is_available():
        return          # a device is visible: the device path is covered by tests/test_gpu_ssim_loss.py
    x = torch.rand(2, 3, 40, 40)
    for mod in (SSIM(data_range=1.), MS_SSIM(data_range=1., normalize="relu")):
        with pytest.raises(hip.HipEngineError):
            mod(x, x)
