"""Spatial profile losses (cpl, gpl) and the overflow loss, the parts that need no device: the fp64 restatement of
tools/make_golden_spl.py against tests/golden/spl.pt (the REAL reference's fp64 runs), the formulas by hand, the option surface of
GeneratorLoss (names, order, refusals, routing under frequency separation) in the SR, Pix2Pix and CycleGAN models' loss builder, and
header <-> library <-> binding agreement."""
import os
import re

import pytest
import torch

from tools import make_golden_spl as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "spl.pt")
NEW_EXPORTS = {"tnr_spl_workspace_bytes", "tnr_spl_coef_bytes", "tnr_spl_loss_fwd", "tnr_spl_loss_bwd", "tnr_overflow_loss_fwd",
               "tnr_overflow_loss_bwd"}


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


def test_fixture_is_small_and_complete(fx):
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert set(fx["cases"]) == set(T.CASES)
    for case in T.CASES:
        assert set(fx["cases"][case]["names"]) == set(T.names_for(case))
        assert fx["cases"][case]["znorm"] == T.znorm_of(case)
    assert "cpl" not in fx["cases"]["gray72"]["names"]
    for name in ("cpl", "gpl"):
        t = fx["cases"]["blackrow72"]["names"][name]
        assert t["black_absmax"] > 1e9 and t["grad_absmax"] > 1e9 and 0 < t["black_rel32"] < 1e-5
    step = fx["steps"]["spl_overflow"]
    assert set(step["weights"]) == {"spl_weight", "of_weight"}
    for log in step["logs"]:
        assert log["overflow"] > 0 and 0.1 <= abs(log["cpl"]) / log["pix-l1"] <= 10 and 0.1 <= log["overflow"] / log["pix-l1"] <= 10
        assert abs(log["gpl"]) <= 10 * log["pix-l1"]


@pytest.mark.parametrize("case", T.CASES)
def test_restatement_matches_the_reference_record(fx, case):
    rec = fx["cases"][case]
    sr, hr = T.make_inputs(case)
    for t, pr in ((sr, rec["sr"]), (hr, rec["hr"])):
        assert T.probe_error(t, pr)[0] <= 1e-6
    for name in T.names_for(case):
        t = rec["names"][name]
        v, g = T.restate_with_grad(sr, hr, name, rec["znorm"])
        assert abs(v.item() - t["value"]) <= 1e-12 * max(1.0, abs(t["value"])), (name, v.item(), t["value"])
        es, _ = T.probe_error(g, t["grad"])
        assert es <= 1e-12 * max(1.0, t["grad_absmax"]), (name, es)


def test_case_inputs_cover_what_they_are_for():
    sr, hr = T.make_inputs("znorm99x117")
    for t in (sr, hr):
        assert (t < -1).any() and (t > 1).any() and ((t > -1) & (t < 1)).any()
    sr, _ = T.make_inputs("overflow99x117")
    assert min((sr < 0).double().mean(), (sr > 1).double().mean(), ((sr >= 0) & (sr <= 1)).double().mean()) >= 0.10
    sr, _ = T.make_inputs("blackrow72")
    assert sr[:, :, T.BLACK_ROW].abs().max() == 0 and sr[:, :, T.BLACK_ROW - 1].abs().min() >= 0 and sr[:, :, T.BLACK_ROW + 1].abs().max() > 0


def test_formulas_by_hand():
    """One 2 x 2 plane: SPLoss = -(column cosines + row cosines) / (H N); the eps branch; the overflow loss and its kinks."""
    x = torch.tensor([[3., 0.], [4., 0.]], dtype=torch.float64).reshape(1, 1, 2, 2)
    y = torch.tensor([[3., 1.], [4., 1.]], dtype=torch.float64).reshape(1, 1, 2, 2)
    # columns: (3, 4) . (3, 4) / 25 = 1 and the zero column: 0 / eps . y^ = 0; rows: (3, 0) . (3, 1) / (3 sqrt 10), (4, 0) . (4, 1) / (4 sqrt 17)
    want = -(1.0 + 0.0 + 3 / 10 ** 0.5 + 4 / 17 ** 0.5) / 2
    assert abs(T.spl_trace(x, y).item() - want) < 1e-12
    # the gradient on the zero column is y^ / eps from the column term (plus the rows' O(1) terms): 1 / (sqrt 2 eps) / (H N)
    xg = x.clone().requires_grad_(True)
    T.spl_trace(xg, y).backward()
    assert abs(xg.grad[0, 0, 0, 1].item() / (-(1 / 2 ** 0.5 / T.EPS) / 2) - 1) < 1e-9
    xe = x.clone().requires_grad_(True)
    T.spl_trace(xe, y, eps_only=True).backward()
    assert abs(xe.grad[0, 0, 0, 1].item() / (-(1 / 2 ** 0.5 / T.EPS) / 2) - 1) < 1e-12 and xe.grad[0, 0, 0, 0].item() == 0
    # differences: nothing flows through the zeroed last column / row
    dx, dy = T.differences(y)
    assert dx[0, 0].tolist() == [[-2., 0.], [-3., 0.]] and dy[0, 0].tolist() == [[1., 0.], [0., 0.]]
    # yuv of white is (1, .5, .5)
    yuv = T.rgb_to_yuv(torch.ones(1, 3, 1, 1, dtype=torch.float64))
    assert (yuv.flatten() - torch.tensor([1., .5, .5], dtype=torch.float64)).abs().max() < 1e-15
    # overflow: log(1 + distance to [0, 1]) / numel, derivative 0 on the closed interval
    o = torch.tensor([-1., 0., 0.5, 1., 3.], dtype=torch.float64).reshape(1, 1, 1, 5).requires_grad_(True)
    v = T.restate(o, None, "overflow")
    assert abs(v.item() - (torch.log(torch.tensor(2.)) + torch.log(torch.tensor(3.))).double().item() / 5) < 1e-7
    v.backward()
    assert (o.grad.flatten() * 5 - torch.tensor([-0.5, 0., 0., 0., 1 / 3], dtype=torch.float64)).abs().max() < 1e-15


def _train(**extra):
    train = {"pixel_criterion": "l1", "pixel_weight": 1e-2, "tv_type": "normal", "tv_norm": 1, "tv_weight": 1e-5,
             "grad_type": "grad-4d-l1", "grad_weight": 4e-1}
    train.update(extra)
    return train


@pytest.mark.parametrize("spl_type, names", [("spl", ["cpl", "gpl"]), ("cpl", ["cpl"]), ("gpl", ["gpl"])])
def test_generator_loss_builds_the_terms_in_the_references_position(spl_type, names):
    """Fails before this feature: `spl_weight` / `of_weight` used to raise NotImplementedError."""
    from trainner_amd.models import losses
    from trainner_amd.models.modules import spl as SPL
    opt = {"train": _train(spl_type=spl_type, spl_weight=1e-3, of_type="overflow", of_weight=0.2), "datasets": {"train": {"znorm": True}}}
    gl = losses.GeneratorLoss(opt, device="cpu")
    assert [(l["name"], l["weight"]) for l in gl.loss_list] == [("pix-l1", 1e-2), ("tv-l1", 1e-5)] + [(n, 1e-3) for n in names] + \
        [("overflow", 0.2)]
    assert [l["name"] for l in gl.precise_loss_list] == ["grad-4d-l1"]
    by_name = {l["name"]: l["function"] for l in gl.loss_list}
    if "cpl" in names:
        f = by_name["cpl"]
        assert isinstance(f, SPL.CPLoss) and f.spl_denorm and f.yuv_denorm and f.rgb and f.yuv and f.yuvgrad
    if "gpl" in names:
        assert isinstance(by_name["gpl"], SPL.GPLoss) and by_name["gpl"].spl_denorm
    assert isinstance(by_name["overflow"], SPL.OFLoss) and by_name["overflow"].legit_range == [0, 1]
    # without znorm (or without a datasets block at all) nothing is denormed
    gl = losses.GeneratorLoss({"train": _train(spl_type=spl_type, spl_weight=1)}, device="cpu")
    assert [l["name"] for l in gl.loss_list] == ["pix-l1", "tv-l1"] + names
    assert not any(l["function"].spl_denorm for l in gl.loss_list if l["name"] in ("cpl", "gpl"))


def test_builder_names_and_what_builds_nothing():
    from trainner_amd.models import losses
    for name in ("cpl", "gpl", "overflow"):
        entry = losses.get_loss_fn(name, 3, device="cpu", opt={"datasets": {"train": {}}})
        assert entry["name"] == name and entry["weight"] == 3
    # an unknown spl_type builds nothing, as in the reference; so does a type without a weight or a weight without a type
    for train in ({"spl_type": "trace", "spl_weight": 1}, {"spl_type": "spl"}, {"spl_weight": 1}, {"of_type": "overflow"}, {"of_weight": 1},
                  {"spl_type": "spl", "spl_weight": 0}):
        gl = losses.GeneratorLoss({"train": train}, device="cpu")
        assert gl.loss_list == [] and gl.precise_loss_list == [], train
    # of_type goes through get_loss_fn: anything but overflow meets its raise
    with pytest.raises(NotImplementedError, match=r"Loss type \[range\] is not implemented"):
        losses.GeneratorLoss({"train": {"of_type": "range", "of_weight": 1}}, device="cpu")
    # the still-refused experimental weights
    for k in ("color_weight", "avg_weight", "ms_weight", "fft_weight", "fdpl_weight", "range_weight", "lpips_weight"):
        with pytest.raises(NotImplementedError, match=k):
            losses.GeneratorLoss({"train": {k: 1}}, device="cpu")
    assert "spl_weight" not in losses.GeneratorLoss._UNSUPPORTED and "of_weight" not in losses.GeneratorLoss._UNSUPPORTED


def test_refused_option_values_are_named():
    from trainner_amd.models.modules import spl as SPL
    with pytest.raises(NotImplementedError, match="trace=True"):
        SPL.GPLoss(trace=True)
    with pytest.raises(NotImplementedError, match="trace=True"):
        SPL.CPLoss(trace=True)
    for k in ("rgb", "yuv", "yuvgrad"):
        with pytest.raises(NotImplementedError, match=k + "=False"):
            SPL.CPLoss(**{k: False})
    with pytest.raises(NotImplementedError, match="yuv_denorm=True"):
        SPL.CPLoss(spl_denorm=False, yuv_denorm=True)
    SPL.CPLoss(spl_denorm=True, yuv_denorm=False)          # one denorm before everything: what the kernels do
    with pytest.raises(NotImplementedError, match="legit_range"):
        SPL.OFLoss(legit_range=[-1, 1])
    with pytest.raises(NotImplementedError, match="out_norm"):
        SPL.OFLoss(out_norm="b")
    assert SPL.OFLoss(legit_range=[0, 1]).out_norm == "bci"
    with pytest.raises(NotImplementedError, match="3 x H x W"):
        SPL.CPLoss()(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    with pytest.raises(NotImplementedError):
        SPL.GPLoss()(torch.zeros(1, 5, 8, 8), torch.zeros(1, 5, 8, 8))
    with pytest.raises(NotImplementedError):
        SPL.OFLoss()(torch.zeros(8, 8))


class _Recorder:
    def __init__(self, calls, name):
        self.calls, self.name = calls, name

    def __call__(self, *args):
        self.calls.append((self.name, args))
        return torch.tensor(1.0)


def _stubbed(train):
    from trainner_amd.models import losses
    gl = losses.GeneratorLoss({"train": train}, device="cpu")
    calls = []
    for l in gl.loss_list + gl.precise_loss_list:
        l["function"] = _Recorder(calls, l["name"])
    return gl, calls


def test_regular_and_frequency_separated_routing():
    """overflow sees sr alone; under fs, cpl and gpl see the low-passed pair and overflow the low-passed sr (calc_losses_fs); all three
    get fp32 operands whatever the incoming precision."""
    from trainner_amd.dataops import filters

    class StubLow(filters.FilterLow):
        def forward(self, t):
            assert t.dtype == torch.float32
            return t * 0.5

    sr, hr = torch.rand(1, 3, 8, 8).half(), torch.rand(1, 3, 8, 8).half()
    gl, calls = _stubbed({"spl_type": "spl", "spl_weight": 2.0, "of_type": "overflow", "of_weight": 3.0})
    results, log = gl(sr, hr, {})
    assert [c[0] for c in calls] == ["cpl", "gpl", "overflow"] and list(log) == ["cpl", "gpl", "overflow"]
    assert [r.item() for r in results] == [2.0, 2.0, 3.0]
    for name, args in calls:
        assert all(a.dtype == torch.float32 for a in args)
        assert len(args) == (1 if name == "overflow" else 2) and torch.equal(args[0], sr.float())
        if name != "overflow":
            assert torch.equal(args[1], hr.float())
    del calls[:]
    results, log = gl(sr, hr, {}, fsfilter=StubLow())
    assert [c[0] for c in calls] == ["cpl", "gpl", "overflow"] and list(log) == ["cpl", "gpl", "overflow"]
    assert [r.item() for r in results] == [2.0, 2.0, 3.0]
    for name, args in calls:
        assert len(args) == (1 if name == "overflow" else 2) and torch.equal(args[0], sr.float() * 0.5)
        if name != "overflow":
            assert torch.equal(args[1], hr.float() * 0.5)
    # the precise list is untouched by the new names
    assert gl.precise_loss_list == []


@pytest.mark.parametrize("model", ["pix2pix", "cyclegan"])
def test_image_to_image_models_construct_with_gpl(model, tmp_path):
    """The Pix2Pix and CycleGAN models use the same GeneratorLoss: `spl_type: gpl` lands in their loss list."""
    from oracle import ref_harness
    from trainner_amd.models import losses
    from trainner_amd.options import options
    yml = ref_harness.i2i_yaml(name="cpu_spl_" + model, model=model, out_root=str(tmp_path))
    with open(yml) as fh:
        txt = fh.read()
    assert txt.count("\n  manual_seed:") == 1
    with open(yml, "w") as fh:
        fh.write(txt.replace("\n  manual_seed:", "\n  spl_type: gpl\n  spl_weight: 0.5\n  of_type: overflow\n  of_weight: 0.25\n  manual_seed:"))
    opt = options.parse(yml, is_train=True)
    assert opt["train"]["spl_type"] == "gpl" and opt["train"]["spl_weight"] == 0.5
    gl = losses.GeneratorLoss(opt, device="cpu")
    assert [(l["name"], l["weight"]) for l in gl.loss_list] == [("pix-l1", opt["train"]["pixel_weight"]), ("gpl", 0.5), ("overflow", 0.25)]


def test_header_and_exports_declare_the_new_entry_points():
    from trainner_amd import hip
    with open(os.path.join(ROOT, "include", "trainner_hip.h")) as fh:
        declared = set(re.findall(r"\b(tnr_\w+)\s*\(", fh.read()))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(hip.EXPORTS)
    lib = hip.load()          # types every export: a symbol the library lacks raises here
    assert lib.tnr_version() == hip.ABI_VERSION          # no descriptor changed
    # 2 x 3 x 99 x 117, cpl (12 planes): 2 x 7 tiles per image in 2 bands; row segments per tile column, column segments per band,
    # then 4 fp64 per finalize block over the 2 * 12 * (99 + 117) lines
    lines = 2 * 12 * (99 + 117)
    assert lib.tnr_spl_workspace_bytes(2, 3, 99, 117, 1 | 2 | 8) == ((2 * 12 * 99 * 2 + 2 * 12 * 2 * 117) * 3 + -(-lines // 256) * 4) * 8
    assert lib.tnr_spl_coef_bytes(2, 3, 99, 117, 1 | 2 | 8) == lines * 2 * 4
    assert lib.tnr_spl_coef_bytes(2, 1, 72, 72, 4) == 2 * 2 * 144 * 2 * 4
    # the YUV families need 3 channels; more than 4 channels and an empty mask are refused
    assert lib.tnr_spl_workspace_bytes(2, 1, 72, 72, 2) == 0 and lib.tnr_spl_workspace_bytes(2, 5, 72, 72, 4) == 0
    assert lib.tnr_spl_workspace_bytes(2, 3, 72, 72, 0) == 0


def test_no_device_no_fallback():
    """Without a HIP device the modules raise; they never compute in eager PyTorch."""
    from trainner_amd import hip
    from trainner_amd.models import losses
    if torch.cuda.is_available():
        pytest.skip("a device is visible: the device path is covered by tests/test_gpu_spl.py")
    x = torch.rand(2, 3, 40, 40)
    for name in ("cpl", "gpl", "overflow"):
        f = losses.get_loss_fn(name, 1, device="cpu", opt={})["function"]
        with pytest.raises(hip.HipEngineError):
            f(x) if name == "overflow" else f(x, x)
