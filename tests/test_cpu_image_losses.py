"""HFEN, image-gradient, total-variation and difference-only pixel losses, the parts that need no device: the fp64 restatement of
tools/make_golden_image_losses.py against tests/golden/image_losses.pt (the REAL reference's fp64 runs), the LoG taps bit for bit,
the finite-difference borders by hand, the option surface of GeneratorLoss, and header <-> library <-> binding agreement."""
import os
import re

import pytest
import torch

from tools import make_golden_image_losses as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "image_losses.pt")
NEW_EXPORTS = {"tnr_imgloss_workspace_bytes", "tnr_filter_loss_fwd", "tnr_filter_loss_bwd", "tnr_fd_loss_fwd", "tnr_fd_loss_bwd",
               "tnr_pointwise_loss_fwd", "tnr_pointwise_loss_bwd"}


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


def test_fixture_is_small_and_complete(fx):
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert set(fx["cases"]) == set(T.CASES)
    for case in T.CASES:
        assert set(fx["cases"][case]["names"]) == set(T.names_for(case))
    assert not any(n.startswith("hfen") for n in fx["cases"]["gray72"]["names"])


@pytest.mark.parametrize("case", T.CASES)
def test_restatement_matches_the_reference_record(fx, case):
    rec = fx["cases"][case]
    sr, hr = T.make_inputs(case)
    for t, pr in ((sr, rec["sr"]), (hr, rec["hr"])):
        assert T.probe_error(t, pr)[0] <= 1e-6
    for name in T.names_for(case):
        t = rec["names"][name]
        v, g = T.restate_with_grad(sr, hr, name)
        assert abs(v.item() - t["value"]) <= 1e-12 * max(1.0, abs(t["value"])), (name, v.item(), t["value"])
        es, esum = T.probe_error(g, t["grad"])
        assert es <= 1e-12 * max(1.0, t["grad_absmax"]), (name, es)


def test_log_taps_are_the_references_bit_for_bit(fx):
    from trainner_amd.models.modules.image_losses import HFENLoss, criterion, log_kernel_taps
    taps = log_kernel_taps(15, 2.5)
    assert taps.dtype == torch.float32 and tuple(taps.shape) == (15, 15)
    assert torch.equal(taps, fx["log_taps"])
    mod = HFENLoss(loss_f=criterion("l1", "sum"))
    assert torch.equal(mod.kernel, fx["log_taps"]) and len(mod.taps) == 225
    assert torch.equal(torch.tensor(mod.taps, dtype=torch.float32).reshape(15, 15), fx["log_taps"])


def test_finite_difference_borders_by_hand():
    """dx zeroed in the last column, dy and dp in the last row; dn is NOT zeroed (it is -x on the last row and column) and
    dp = right - bottom sees a zero `right` in the last column."""
    x = torch.tensor([[1., 2., 4.], [8., 16., 32.], [64., 128., 256.]], dtype=torch.float64).reshape(1, 1, 3, 3)
    dx, dy, dp, dn = T.fd_responses(x, True)
    assert dx[0, 0].tolist() == [[1., 2., 0.], [8., 16., 0.], [64., 128., 0.]]
    assert dy[0, 0].tolist() == [[7., 14., 28.], [56., 112., 224.], [0., 0., 0.]]
    assert dn[0, 0].tolist() == [[15., 30., -4.], [120., 240., -32.], [-64., -128., -256.]]
    assert dp[0, 0].tolist() == [[2. - 8., 4. - 16., 0. - 32.], [16. - 64., 32. - 128., 0. - 256.], [0., 0., 0.]]
    assert len(T.fd_responses(x, False)) == 2
    # total variation of this image by hand: (sum |dx| + sum |dy|) / 9 for one image
    assert abs(T.restate(x, x, "tv-l1").item() - (219. + 441.) / 9.) < 1e-12
    # the gradient loss of an image against itself is 0, cb keeps its 1e-6 floor at every position, zeroed ones included
    assert T.restate(x, x, "grad-4d-l1").item() == 0.0
    assert abs(T.restate(x, x, "grad-4d-cb").item() - 1e-6) < 1e-18


def test_generator_loss_builds_the_new_terms_from_options():
    """Fails before this feature: `hfen_weight` used to raise NotImplementedError."""
    from trainner_amd.models import losses
    from trainner_amd.models.modules import image_losses as IL
    train = {"pixel_criterion": "cb", "pixel_weight": 1e-2, "hfen_criterion": "l1", "hfen_weight": 1e-6, "tv_type": "normal",
             "tv_norm": 1, "tv_weight": 1e-5, "grad_type": "grad-4d-l1", "grad_weight": 4e-1, "ssim_type": "ssim", "ssim_weight": 1}
    gl = losses.GeneratorLoss({"train": train}, device="cpu")
    assert [(l["name"], l["weight"]) for l in gl.loss_list] == [("pix-cb", 1e-2), ("hfen-l1", 1e-6), ("tv-l1", 1e-5)]
    assert [(l["name"], l["weight"]) for l in gl.precise_loss_list] == [("grad-4d-l1", 4e-1), ("ssim", 1)]
    pix, hfen, tv = (l["function"] for l in gl.loss_list)
    assert isinstance(pix, IL.CharbonnierLoss) and pix.reduction == "mean"
    assert isinstance(hfen, IL.HFENLoss) and isinstance(hfen.criterion, IL.L1Loss) and hfen.criterion.reduction == "sum" and hfen.sum_reduced
    assert isinstance(tv, IL.TVLoss) and (tv.tv_type, tv.p, tv.dirs) == ("tv", 1, 2)
    grad = gl.precise_loss_list[0]["function"]
    assert isinstance(grad, IL.GradientLoss) and grad.dirs == 4 and isinstance(grad.criterion, IL.L1Loss) and grad.criterion.reduction == "mean"
    # names and reductions of every builder form (cb and clipl1 ignore HFEN's reduction='sum' and stay means)
    for crit, cls, red in (("l1", IL.L1Loss, "sum"), ("l2", IL.MSELoss, "sum"), ("cb", IL.CharbonnierLoss, "mean"),
                           ("elastic", IL.ElasticLoss, "sum"), ("clipl1", IL.ClipL1, "mean")):
        entry = losses.get_loss_fn("hfen-" + crit, 2, device="cpu")
        assert entry["name"] == "hfen-" + crit and entry["weight"] == 2 and isinstance(entry["function"].criterion, cls)
        assert entry["function"].criterion.reduction == red and entry["function"].sum_reduced == (red == "sum")
    for crit, name in (("l2", "pix-l2"), ("MSE", "pix-MSE"), ("cb", "pix-cb"), ("elastic", "pix-elastic"), ("clipl1", "pix-clipl1")):
        entry = losses.get_loss_fn(crit, 1, device="cpu")
        assert entry["name"] == name and entry["function"].reduction == "mean"
    assert losses.get_loss_fn("grad-2d-cb", 1, device="cpu")["function"].dirs == 2
    for name, dirs, p in (("tv-l1", 2, 1), ("tv-l2", 2, 2), ("dtv-l1", 4, 1), ("dtv-l2", 4, 2)):
        f = losses.get_loss_fn(name, 1, device="cpu")["function"]
        assert (f.dirs, f.p) == (dirs, p)
    # check_loss_names: the reference's spellings
    assert losses.check_loss_names(hfen_criterion="L2") == "hfen-l2" and losses.check_loss_names(hfen_criterion="rel_l1") == "hfen-relativel1"
    for tv_type, tv_norm, want in (("normal", 1, "tv-l1"), ("normal", "L2", "tv-l2"), ("4D", "L1", "dtv-l1"), ("4D", 2, "dtv-l2"),
                                   ("dtv", "l1", "dtv-l1")):
        assert losses.check_loss_names(tv_type=tv_type, tv_norm=tv_norm) == want
    assert losses.check_loss_names(tv_type="normal") is None
    # a tv_type without a tv_norm builds nothing, as in the reference; a weight alone builds nothing either
    assert losses.GeneratorLoss({"train": {"tv_type": "normal", "tv_weight": 1}}, device="cpu").loss_list == []
    assert losses.GeneratorLoss({"train": {"hfen_weight": 1}}, device="cpu").loss_list == []
    assert losses.GeneratorLoss({"train": {"grad_type": "grad-2d-l1"}}, device="cpu").precise_loss_list == []
    # the one place where the engine is stricter than the reference: a grad weight without a type is refused
    with pytest.raises(NotImplementedError, match="grad_type"):
        losses.GeneratorLoss({"train": {"grad_weight": 1}}, device="cpu")


def test_refused_kinds_raise():
    from trainner_amd.models import losses
    from trainner_amd.models.modules import image_losses as IL
    for crit in ("relativel1", "l1cosinesim", "fro", "multiscale-l1"):
        with pytest.raises(NotImplementedError):
            losses.GeneratorLoss({"train": {"pixel_criterion": crit, "pixel_weight": 1}}, device="cpu")
    for crit in ("rel_l1", "rel_l2", "relativel1", "l1cosinesim", "fro"):
        with pytest.raises(NotImplementedError):
            losses.GeneratorLoss({"train": {"hfen_criterion": crit, "hfen_weight": 1}}, device="cpu")
    for gtype in ("grad-2d-relativel1", "grad-4d-fro", "grad-2d"):
        with pytest.raises(NotImplementedError):
            losses.GeneratorLoss({"train": {"grad_type": gtype, "grad_weight": 1}}, device="cpu")
    with pytest.raises(NotImplementedError):
        losses.GeneratorLoss({"train": {"tv_type": "normal", "tv_norm": 3, "tv_weight": 1}}, device="cpu")
    with pytest.raises(NotImplementedError, match="kernel"):
        IL.HFENLoss(loss_f=IL.criterion("l1"), kernel="dog")
    with pytest.raises(NotImplementedError, match="norm"):
        IL.HFENLoss(loss_f=IL.criterion("l1"), norm=True)
    with pytest.raises(NotImplementedError):
        IL.HFENLoss(loss_f=torch.nn.L1Loss())
    with pytest.raises(NotImplementedError):
        IL.TVLoss(beta=1)
    with pytest.raises(NotImplementedError, match="feature criterion"):
        losses.get_loss_fn("fea-vgg19-l2", 1, device="cpu", opt={"train": {}})
    gl = losses.GeneratorLoss({"train": {"hfen_criterion": "l1", "hfen_weight": 1}}, device="cpu")
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(NotImplementedError):
        gl(x, x, {}, fsfilter=lambda t: t)
    with pytest.raises(NotImplementedError):
        gl(x, x, {}, selector=["pix"])
    with pytest.raises(RuntimeError, match="3 channels"):
        gl.loss_list[0]["function"](torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16))


def test_shipped_recipe_with_the_three_terms_parses_and_constructs(tmp_path):
    """options/sr/train_sr.yml with its lines 114-120 uncommented."""
    from oracle import fixtures as FX
    from trainner_amd.models import losses
    from trainner_amd.options import options
    opt = options.parse(FX.write_recipe("sr/train_sr.yml", str(tmp_path), recipe_edit), is_train=True)
    train = {k: v for k, v in opt["train"].items() if k not in ("feature_weight", "feature_criterion")}   # (no VGG on the CPU)
    gl = losses.GeneratorLoss({"train": train}, device="cpu")
    assert [(l["name"], l["weight"]) for l in gl.loss_list] == [("pix-l1", 1e-2), ("hfen-l1", 1e-6), ("tv-l1", 1e-5)]
    assert [(l["name"], l["weight"]) for l in gl.precise_loss_list] == [("grad-4d-l1", 4e-1)]


def recipe_edit(tree):
    tree["train"].update({"hfen_criterion": "l1", "hfen_weight": 1e-6, "grad_type": "grad-4d-l1", "grad_weight": 4e-1,
                          "tv_type": "normal", "tv_weight": 1e-5, "tv_norm": 1})


def test_sum_reduced_hfen_is_a_sum_over_the_batch():
    """hfen-l1 / -l2 / -elastic of a batch is the SUM of its images' terms (so under data parallelism the local term is multiplied by
    the world size); every other name is the mean of per-image terms over equal shards."""
    sr, hr = T.make_inputs("sq72")
    sr, hr = sr.double(), hr.double()
    for name in T.NAMES:
        whole = T.restate(sr, hr, name).item()
        halves = [T.restate(sr[i:i + 1], hr[i:i + 1], name).item() for i in range(2)]
        want = sum(halves) if name in ("hfen-l1", "hfen-l2", "hfen-elastic") else sum(halves) / 2
        assert abs(want - whole) <= 1e-12 * max(1.0, abs(whole)), name


def test_header_and_exports_declare_the_new_entry_points():
    from trainner_amd import hip
    with open(os.path.join(ROOT, "include", "trainner_hip.h")) as fh:
        declared = set(re.findall(r"\b(tnr_\w+)\s*\(", fh.read()))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(hip.EXPORTS)
    lib = hip.load()          # types every export: a symbol the library lacks raises here
    assert lib.tnr_version() == hip.ABI_VERSION == 3          # no descriptor changed
    # 16 x 3 x 512 x 512 in 64 x 16 tiles: one fp64 slot per tile
    assert lib.tnr_imgloss_workspace_bytes(16, 3, 512, 512) == 16 * 3 * 8 * 32 * 8
    assert lib.tnr_imgloss_workspace_bytes(2, 3, 99, 117) == 2 * 3 * 2 * 7 * 8
    assert lib.tnr_imgloss_workspace_bytes(0, 3, 8, 8) == 0


def test_no_device_no_fallback():
    """Without a HIP device the modules raise; they never compute in eager PyTorch."""
    from trainner_amd import hip
    from trainner_amd.models import losses
    if torch.cuda.is_available():
        return          # a device is visible: the device path is covered by tests/test_gpu_image_losses.py
    x = torch.rand(2, 3, 40, 40)
    for name in ("l2", "hfen-l1", "grad-4d-l1", "tv-l1"):
        f = losses.get_loss_fn(name, 1, device="cpu")["function"]
        with pytest.raises(hip.HipEngineError):
            f(x) if name == "tv-l1" else f(x, x)
