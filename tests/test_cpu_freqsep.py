"""Frequency separation (fs / lpf_type / hpf_type), the parts that need no device: the fp64 restatement of tools/make_golden_freqsep.py
against tests/golden/freqsep.pt (the REAL reference's fp64 runs), the Gaussian taps bit for bit, the average filter's borders by hand,
the option surface of FilterLow / FilterHigh / setup_fs, the routing of GeneratorLoss and Adversarial by loss name (with recording
stand-ins), and header <-> library <-> binding agreement."""
import os
import re

import pytest
import torch

from tools import make_golden_freqsep as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "freqsep.pt")
EPS81 = 81 * 2.0 ** -52          # hand-worked fp64 cases: 81 products summed in some order
NEW_EXPORTS = {"tnr_freqsep_low", "tnr_freqsep_high_fwd", "tnr_freqsep_high_bwd"}


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


def test_fixture_is_small_and_complete(fx):
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert set(fx["cases"]) == set(T.CASES)
    for case in T.CASES:
        assert set(fx["cases"][case]["filters"]) == set(T.filters_for(case))
    assert set(fx["cases"]["gray72"]["filters"]) == {"low-average", "high-average"}
    assert set(fx["steps"]) == {"sr_average", "sr_gaussian", "pix2pix"}
    assert fx["clamp_scale"] == T.CLAMP_SCALE
    for case in T.CASES:
        for name, t in fx["cases"][case]["filters"].items():
            assert t["sep_dev"] <= t["e32_out"], (case, name)          # 9 + 9 taps cost less than the reference's own fp32 rounding
            if name.startswith("high"):
                assert t["near_share"] <= 1e-3 and t["grad_left_out"] <= 1e-3          # (both are 0 in this fixture)
    for name in ("high-average", "high-gaussian"):
        assert fx["cases"]["clamp72"]["filters"][name]["clamped_share"] >= 1e-2


@pytest.mark.parametrize("case", T.CASES)
def test_restatement_matches_the_reference_record(fx, case):
    rec = fx["cases"][case]
    x = T.make_input(case)
    m = T.seeded_map(tuple(x.shape))
    assert T.probe_error(x, rec["x"])[0] <= 1e-6 and T.probe_error(m, rec["m"])[0] == 0.0
    for name in T.filters_for(case):
        t = rec["filters"][name]
        out, grad = T.restate_with_grad(x, name, m)
        assert T.probe_error(out, t["out"])[0] <= 1e-12, name
        assert T.probe_error(grad, t["grad"])[0] <= 1e-12, name
        assert abs(out.abs().max().item() - t["out_absmax"]) <= 1e-12 and abs(grad.abs().max().item() - t["grad_absmax"]) <= 1e-12


def test_gaussian_taps_are_the_references_bit_for_bit(fx):
    from trainner_amd.dataops import filters as EF
    k1, k2 = EF.gaussian_taps1d(), EF.gaussian_taps2d()
    assert k1.dtype == torch.float32 and tuple(k1.shape) == (9,) and k2.dtype == torch.float32 and tuple(k2.shape) == (9, 9)
    assert torch.equal(k1, fx["gaussian_taps1d"]) and torch.equal(k2, fx["gaussian_taps2d"])
    mod = EF.FilterLow(filter_type="gaussian")
    assert torch.equal(mod.kernel, fx["gaussian_taps2d"])
    assert torch.equal(torch.tensor(mod.taps, dtype=torch.float32), fx["gaussian_taps1d"])
    assert EF.FilterHigh(filter_type="gaussian").taps == mod.taps
    avg = EF.FilterLow(filter_type="average")
    assert avg.taps == (float(torch.tensor(1.0 / 9.0, dtype=torch.float32)),) * 9 and not hasattr(avg, "kernel")


def test_average_borders_by_hand():
    """Zero padding counted: an all-ones 9 x 9 image gives 25 / 81 in a corner (5 x 5 of the window inside), 45 / 81 in the middle of an
    edge, 1 in the centre; the high-pass is (1 - that + 1) / 2.  The separable evaluation with the fp32 taps agrees to fp32's 1 / 9."""
    x = torch.ones(1, 1, 9, 9, dtype=torch.float64)
    lo = T.restate(x, "low-average")[0, 0]
    for (i, j), want in {(0, 0): 25, (0, 8): 25, (8, 8): 25, (0, 4): 45, (4, 0): 45, (4, 4): 81, (1, 1): 36, (3, 8): 8 * 5}.items():
        assert abs(lo[i, j].item() - want / 81.0) <= EPS81, (i, j)
    hi = T.restate(x, "high-average")[0, 0]
    assert abs(hi[0, 0].item() - (1 - 25 / 81.0 + 1) / 2) <= EPS81 and abs(hi[4, 4].item() - 0.5) <= EPS81
    sep = T.low_separable(x, "average")[0, 0]
    assert (sep - lo).abs().max().item() <= 4e-8
    # a 5 x 5 image lies inside every window: 25 / 81 everywhere
    assert (T.restate(torch.ones(1, 1, 5, 5, dtype=torch.float64), "low-average") - 25 / 81.0).abs().max().item() <= EPS81
    # the clamp: x - L x beyond +-1 saturates, and the gradient stops there
    x = torch.zeros(1, 1, 9, 9, dtype=torch.float64)
    x[0, 0, 4, 4] = 3.0
    x[0, 0, 0, 0] = -3.0
    m = torch.ones_like(x)
    out, grad = T.restate_with_grad(x, "high-average", m)
    assert out[0, 0, 4, 4].item() == 1.0 and out[0, 0, 0, 0].item() == 0.0
    # g' = 0.5 except at the two saturated pixels; gx = g' - L g'
    gp = torch.full_like(x, 0.5)
    gp[0, 0, 4, 4] = gp[0, 0, 0, 0] = 0.0
    assert (grad - (gp - T.low(gp, "average"))).abs().max().item() <= EPS81


def test_option_surface_and_defaults():
    """Fails before this feature: `fs: true` used to raise NotImplementedError in setup_fs."""
    from trainner_amd.dataops import filters as EF
    from trainner_amd.models.base_model import BaseModel

    def model_with(train):
        m = BaseModel.__new__(BaseModel)
        m.opt, m.device = {"train": train}, "cpu"
        m.setup_fs()
        return m

    m = model_with({})
    assert m.f_low is None and m.f_high is None and not m.fs
    m = model_with({"fs": True})
    assert isinstance(m.f_low, EF.FilterLow) and isinstance(m.f_high, EF.FilterHigh)
    assert m.f_low.filter_type == "average" and not m.f_low.gaussian and not m.f_high.gaussian and m.f_high.type == "separator"
    m = model_with({"fs": True, "lpf_type": "gaussian", "hpf_type": "gaussian"})
    assert m.f_low.gaussian and m.f_high.gaussian
    m = model_with({"fs": True, "lpf_type": "box", "hpf_type": "average"})          # any other low-pass type is the average
    assert not m.f_low.gaussian
    with pytest.raises(NotImplementedError, match="hpf_type"):
        model_with({"fs": True, "hpf_type": "sobel"})
    assert EF.FilterLow().taps == EF.FilterLow(filter_type="average").taps          # filter_type None: AvgPool2d
    for kw, word in (({"recursions": 2}, "recursions"), ({"kernel_size": 5}, "kernel_size"), ({"stride": 2}, "stride"),
                     ({"padding": False}, "padding"), ({"include_pad": False}, "include_pad"),
                     ({"filter_type": "gaussian", "image_channels": 1}, "image_channels")):
        with pytest.raises(NotImplementedError, match=word):
            EF.FilterLow(**kw)
    for kw, word in (({"recursions": 2}, "recursions"), ({"kernel_size": 5}, "kernel_size"), ({"stride": 2}, "stride"),
                     ({"include_pad": False}, "include_pad"), ({"normalize": False}, "normalize"),
                     ({"filter_type": "gaussian", "image_channels": 1}, "image_channels")):
        with pytest.raises(NotImplementedError, match=word):
            EF.FilterHigh(**dict({"filter_type": "average"}, **kw))
    for ftype in (None, "log", "sobel"):
        with pytest.raises(NotImplementedError, match="hpf_type"):
            EF.FilterHigh(filter_type=ftype)
    with pytest.raises(RuntimeError, match="3 channels"):
        EF.FilterLow(filter_type="gaussian")(torch.zeros(1, 1, 16, 16))


def test_options_map_use_frequency_separation_to_fs(tmp_path):
    from oracle import ref_harness
    from trainner_amd.options import options
    yml = T.fs_yaml(ref_harness.esrgan_yaml(name="fs_opts", out_root=str(tmp_path), gpu_ids="[0]"), "gaussian")
    opt = options.parse(yml, is_train=True)
    assert opt["train"]["fs"] is True and opt["train"]["lpf_type"] == "gaussian" and opt["train"]["hpf_type"] == "gaussian"


def _recording_filter(base):
    class Rec(base):
        def __init__(self):
            super().__init__(filter_type="average")
            self.seen, self.made = [], {}

        def forward(self, img):
            self.seen.append(img)
            out = img + 1.0
            self.made[id(img)] = out
            return out
    return Rec()


def test_generator_loss_routes_operands_by_name():
    """calc_losses_fs: tv -> f(sr_f); pix / hfen -> f(sr_f, hr_f); ssim -> 1 - f(sr_f, hr_f); fea-vgg and everything else, grad-4d-l1
    included (the reference's quirk), -> the unfiltered pair.  Each image is filtered once per call, and not at all when no term of the
    list consumes it."""
    from trainner_amd.dataops import filters as EF
    from trainner_amd.models import losses
    gl = losses.GeneratorLoss({"train": {}}, device="cpu")
    calls = {}

    def term(name, value, two=True):
        def f(*a):
            calls[name] = a
            return (torch.tensor(value), None) if "fea" in name else torch.tensor(value)
        return {"name": name, "weight": 2.0, "function": f}

    gl.loss_list = [term("pix-l1", 1.0), term("hfen-l1", 2.0), term("tv-l1", 3.0), term("fea-vgg19-l1", 4.0)]
    gl.precise_loss_list = [term("grad-4d-l1", 5.0), term("grad-2d-cb", 6.0), term("ssim", 0.25)]
    sr, hr = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    flt = _recording_filter(EF.FilterLow)
    res, log = gl(sr, hr, {}, fsfilter=flt)
    assert list(log) == ["pix-l1", "hfen-l1", "tv-l1", "fea-vgg19-l1"] and [r.item() for r in res] == [2.0, 4.0, 6.0, 8.0]
    assert len(flt.seen) == 2 and {id(t) for t in flt.seen} == {id(sr), id(hr)}
    sr_f, hr_f = flt.made[id(sr)], flt.made[id(hr)]
    assert calls["pix-l1"][0] is sr_f and calls["pix-l1"][1] is hr_f
    assert calls["hfen-l1"][0] is sr_f and calls["hfen-l1"][1] is hr_f
    assert len(calls["tv-l1"]) == 1 and calls["tv-l1"][0] is sr_f
    assert calls["fea-vgg19-l1"][0] is sr and calls["fea-vgg19-l1"][1] is hr
    # the precise call: grad-* unfiltered, ssim filtered and entered as 1 - f
    calls.clear()
    flt = _recording_filter(EF.FilterLow)
    res, log = gl(sr, hr, {}, fsfilter=flt, precise=True)
    assert list(log) == ["grad-4d-l1", "grad-2d-cb", "ssim"] and [r.item() for r in res] == [10.0, 12.0, 2.0 * (1 - 0.25)]
    assert calls["grad-4d-l1"][0] is sr and calls["grad-4d-l1"][1] is hr and calls["grad-2d-cb"][0] is sr
    assert calls["ssim"][0] is flt.made[id(sr)] and calls["ssim"][1] is flt.made[id(hr)] and len(flt.seen) == 2
    # nothing consumes the low-passed images: the filter is not applied
    gl.loss_list = [term("fea-vgg19-l1", 4.0)]
    gl.precise_loss_list = [term("grad-4d-l1", 5.0)]
    flt = _recording_filter(EF.FilterLow)
    gl(sr, hr, {}, fsfilter=flt)
    gl(sr, hr, {}, fsfilter=flt, precise=True)
    assert flt.seen == []
    # tv alone: sr only
    gl.loss_list = [term("tv-l1", 3.0)]
    gl(sr, hr, {}, fsfilter=flt)
    assert len(flt.seen) == 1 and flt.seen[0] is sr
    # without a filter nothing changes: the terms see the pair itself
    calls.clear()
    gl.loss_list = [term("fea-vgg19-l1", 4.0)]
    gl(sr, hr, {})
    assert calls["fea-vgg19-l1"][0] is sr
    # only the engine's own filter modules are taken (anything else would be an eager filter); selectors stay refused
    with pytest.raises(NotImplementedError, match="FilterLow"):
        gl(sr, hr, {}, fsfilter=lambda t: t)
    with pytest.raises(NotImplementedError, match="selector"):
        gl(sr, hr, {}, fsfilter=flt, selector=["pix"])


@pytest.mark.parametrize("conditional", [False, True])
def test_adversarial_filters_before_the_conditional_concatenation(conditional):
    """fake and (a tensor) real go through the high-pass in both stages, before the condition is concatenated; the condition is not
    filtered; the discriminator stage filters fake.detach()."""
    from trainner_amd import hip
    from trainner_amd.dataops import filters as EF
    from trainner_amd.models import losses
    adv = losses.Adversarial({"gan_type": "vanilla", "gan_weight": 1, "gan_opt": {"form": "standard"}}, device="cpu", conditional=conditional)
    fake = torch.rand(1, 3, 8, 8, requires_grad=True) * 1.0
    real, cond = torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8)
    seen = []

    def netD(x):
        seen.append(x)
        return x.mean().reshape(1)

    for stage in ("generator", "discriminator"):
        flt = _recording_filter(EF.FilterHigh)
        seen.clear()
        with pytest.raises(hip.HipEngineError):          # the GAN criterion itself needs the device; the routing is done by then
            adv(fake, real, cond if conditional else None, netD=netD, stage=stage, fsfilter=flt)
        assert [t.requires_grad for t in flt.seen] == [stage == "generator", False]
        assert flt.seen[0].data_ptr() == fake.data_ptr() and flt.seen[1] is real
        want = fake.detach() + 1.0
        got = seen[0]
        if conditional:
            assert got.shape[1] == 6 and torch.equal(got[:, :3], cond) and torch.equal(got[:, 3:].detach(), want)
        else:
            assert torch.equal(got.detach(), want)
    with pytest.raises(NotImplementedError, match="FilterHigh"):
        adv(fake, real, cond if conditional else None, netD=netD, stage="generator", fsfilter=lambda t: t)


def test_step_memo_returns_one_result_per_distinct_input(monkeypatch):
    """The per-step memo of the filter modules, with the launch replaced by a counter: a second call with the same tensor returns the
    SAME result (one autograd node), a detached alias of the input gets a detached alias of the result, memo_clear drops it."""
    from trainner_amd.dataops import filters as EF
    launches = []

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, taps, reuse):
            if reuse is None:
                launches.append("fwd")
            return x * 2.0 if reuse is None else reuse.detach()

        @staticmethod
        def backward(ctx, g):
            launches.append("bwd")
            return g * 2.0, None, None

    f = EF.FilterLow(filter_type="average")
    monkeypatch.setattr(EF.FilterLow, "fn", Fn)
    x = torch.rand(1, 3, 8, 8).requires_grad_(True)
    a, b = f(x), f(x)
    assert a is b and launches == ["fwd"]
    c = f(x.detach())
    assert not c.requires_grad and c.data_ptr() == a.data_ptr() and launches == ["fwd"]
    (a.sum() + b.sum()).backward()
    assert launches == ["fwd", "bwd"] and torch.equal(x.grad, torch.full_like(x, 4.0))
    # an entry made without a graph serves a later call that needs one without a second forward launch
    f.memo_clear()
    y = torch.rand(1, 3, 8, 8)
    d = f(y)
    yg = y.requires_grad_(True)
    e = f(yg)
    assert launches == ["fwd", "bwd", "fwd"] and e.requires_grad and e.data_ptr() == d.data_ptr()
    f.memo_clear()
    f(y.detach())
    assert launches == ["fwd", "bwd", "fwd", "fwd"]
    # FilterHigh clears its own memo and its low-pass's
    h = EF.FilterHigh(filter_type="average")
    h._memo[1] = h.filter_low._memo[1] = None
    h.memo_clear()
    assert h._memo == {} and h.filter_low._memo == {}


def test_header_and_exports_declare_the_new_entry_points():
    from trainner_amd import hip
    with open(os.path.join(ROOT, "include", "trainner_hip.h")) as fh:
        declared = set(re.findall(r"\b(tnr_\w+)\s*\(", fh.read()))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(hip.EXPORTS)
    lib = hip.load()          # types every export: a symbol the library lacks raises here
    assert lib.tnr_version() == hip.ABI_VERSION == 3          # additions only: no descriptor changed
    from trainner_amd import build, ops
    assert "freqsep.hip" in build.SOURCES
    assert all(hasattr(ops, n) for n in ("freqsep_low", "freqsep_high_fwd", "freqsep_high_bwd"))


def test_no_device_no_fallback():
    """Without a HIP device the modules raise; they never compute in eager PyTorch."""
    from trainner_amd import hip
    from trainner_amd.dataops import filters as EF
    x = torch.rand(2, 3, 40, 40)
    for f in (EF.FilterLow(filter_type="average"), EF.FilterLow(filter_type="gaussian"), EF.FilterHigh(filter_type="average")):
        with pytest.raises(hip.HipEngineError):
            f(x)
