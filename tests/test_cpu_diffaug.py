"""DiffAugment (diffaug / dapolicy), the parts that need no device: the fp64 restatement of tools/make_golden_diffaug.py against
tests/golden/diffaug.pt (the REAL reference's fp64 runs), hand-worked cases of every stage, `draw` against the reference's recorded
draws and ranges, the option surface, the routing of Adversarial.forward (with recording stand-ins), and header <-> library <-> binding
agreement."""
import os
import re

import pytest
import torch

from tools import make_golden_diffaug as T
from trainner_amd.dataops import diffaug as ED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "diffaug.pt")
NEW_EXPORTS = {"tnr_diffaug_workspace_bytes", "tnr_diffaug_mean", "tnr_diffaug_fwd", "tnr_diffaug_bwd"}


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


def test_fixture_is_small_and_complete(fx):
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert set(fx["cases"]) == set(T.CASES) and fx["recipe"] == T.RECIPE
    for case in T.CASES:
        sets = T.sets_for(case)
        assert set(fx["cases"][case]["sets"]) == set(sets)
        for name, (policy, force, seed) in sets.items():
            t = fx["cases"][case]["sets"][name]
            assert t["policy"] == policy and t["seed"] == seed and t["forced"] == bool(force)
    # the hand-set extremes are what they claim to be
    for case, (N, C, H, W) in T.CASES.items():
        s = fx["cases"][case]["sets"]
        assert [s["recipe-" + k]["kind"] for k in ED.KINDS[1:]] == list(ED.KINDS[1:])
        assert s["flip-on"]["flip"] and not s["flip-off"]["flip"]
        if H == W:
            assert (s["rotate-plus"]["rot"], s["rotate-minus"]["rot"], s["rotate-none"]["rot"]) == (1, -1, 0)
            assert s["recipe-translation"]["rot"] == 1 and s["recipe-zoom_in"]["rot"] == -1 and s["recipe-translation"]["flip"]
        else:
            assert "rotate" not in s["seeded-recipe"]["policy"] and "rotate-plus" not in s
        assert s["zoomin-hi-first"]["zoom"] == (0, 0, int(H / 1.999), int(W / 1.999))
        h_delta, w_delta, new_h, new_w = s["zoomin-lo-last"]["zoom"]
        assert (new_h, new_w) == (int(H / 1.001), int(W / 1.001)) and h_delta + new_h <= H and w_delta + new_w <= W
        assert s["zoomout-hi-neg"]["zoom"] == (2 * (W // 2), 0, 2 * (H // 2), 0) and s["zoomout-hi-pos"]["zoom"] == (0, 2 * (W // 2), 0, 2 * (H // 2))
        my, mx = int(H * 0.125 + 0.5), int(W * 0.125 + 0.5)
        prm = T.params_from_tape("translation", s["transl-max"]["tape"], T.CASES[case])
        assert prm.translation[0].abs().tolist() == [my] * N and prm.translation[1].abs().tolist() == [mx] * N
    assert set(fx["steps"]) == {"sr", "pix2pix"}
    assert len(fx["steps"]["sr"]["calls"]) == 8 and all(c["policy"] == T.RECIPE for c in fx["steps"]["sr"]["calls"])
    # the standard GAN form of Pix2Pix feeds no real image in the generator stage: three calls per step
    assert len(fx["steps"]["pix2pix"]["calls"]) == 6
    assert all(c["shape"][1] == 3 for c in fx["steps"]["pix2pix"]["calls"])          # augmented BEFORE the concatenation


@pytest.mark.parametrize("case", list(T.CASES))
def test_restatement_matches_the_reference_record(fx, case):
    rec = fx["cases"][case]
    x = T.make_input(case)
    m = T.seeded_map(tuple(x.shape))
    assert T.probe_error(x, rec["x"])[0] == 0.0 and T.probe_error(m, rec["m"])[0] == 0.0
    for name, t in rec["sets"].items():
        prm = T.params_from_tape(t["policy"], t["tape"], tuple(x.shape))
        assert (prm.kind, prm.flip, prm.rot, prm.zoom) == (t["kind"], t["flip"], t["rot"], t["zoom"])
        out, grad = T.restate_with_grad(x, prm, m)
        assert T.probe_error(out, t["out"])[0] <= 1e-12 and T.probe_error(out, t["out"])[1] <= 1e-9, name
        assert T.probe_error(grad, t["grad"])[0] <= 1e-12 and T.probe_error(grad, t["grad"])[1] <= 1e-9, name
        assert abs(out.abs().max().item() - t["out_absmax"]) <= 1e-12 and abs(grad.abs().max().item() - t["grad_absmax"]) <= 1e-12


def test_hand_cases():
    ones = torch.ones(1, 3, 8, 8, dtype=torch.float64)
    # translation by (+1, -2): out(y, x) = in(y + 1, x - 2): the last row and the first two columns are vacated
    out = T.restate(ones, ED.Params(1, 8, 8, kind="translation", translation=([1], [-2])))
    want = torch.ones(8, 8, dtype=torch.float64)
    want[7, :] = 0
    want[:, :2] = 0
    assert torch.equal(out[0, 0], want) and torch.equal(out[0, 2], want)
    # a cutout at offset 0: the 4 x 4 box starts at -2 and is clipped to the 2 x 2 quarter box
    out = T.restate(ones, ED.Params(1, 8, 8, cutout=([0], [0])))
    want = torch.ones(8, 8, dtype=torch.float64)
    want[:2, :2] = 0
    assert torch.equal(out[0, 1], want)
    # ... and at the far corner (offset 8 is drawn when the box size is even): rows / columns 6, 7
    out = T.restate(ones, ED.Params(1, 8, 8, cutout=([8], [8])))
    want = torch.ones(8, 8, dtype=torch.float64)
    want[6:, 6:] = 0
    assert torch.equal(out[0, 1], want)
    # an odd box (9 x 9 image: 5 x 5) far outside still zeroes the border row and column its clamped indices land on
    out = T.restate(torch.ones(1, 1, 9, 9, dtype=torch.float64), ED.Params(1, 9, 9, cutout=([8], [0])))
    want = torch.ones(9, 9, dtype=torch.float64)
    want[6:, :3] = 0
    assert torch.equal(out[0, 0], want)
    x = torch.rand(2, 3, 8, 8, dtype=torch.float64)
    # zoom_in with the whole image as its crop is the identity
    assert torch.equal(T.restate(x, ED.Params(2, 8, 8, kind="zoom_in", zoom=(0, 0, 8, 8))), x)
    # zoom_out without padding likewise
    assert torch.equal(T.restate(x, ED.Params(2, 8, 8, kind="zoom_out", zoom=(0, 0, 0, 0))), x)
    # brightness only shifts the mean
    b = torch.tensor([0.25, -0.5], dtype=torch.float64)
    one = torch.ones(2, dtype=torch.float64)
    out = T.restate(x, ED.Params(2, 8, 8, color=(b, one, one)))
    assert (out - (x + b.reshape(2, 1, 1, 1))).abs().max().item() <= 4e-16
    # contrast 1 and saturation 1 are identities; saturation 0 leaves the channel mean, contrast 0 the image mean
    zero = torch.zeros(2, dtype=torch.float64)
    assert (T.restate(x, ED.Params(2, 8, 8, color=(zero, one, one))) - x).abs().max().item() <= 4e-16
    out = T.restate(x, ED.Params(2, 8, 8, color=(zero, zero, one)))
    assert (out - x.mean(1, keepdim=True).expand_as(x)).abs().max().item() <= 4e-16
    out = T.restate(x, ED.Params(2, 8, 8, color=(zero, one, zero)))
    assert (out - x.mean((1, 2, 3), keepdim=True).expand_as(x)).abs().max().item() <= 4e-16
    # flip and the two rotations
    assert torch.equal(T.restate(x, ED.Params(2, 8, 8, flip=True)), x.flip(3))
    assert torch.equal(T.restate(x, ED.Params(2, 8, 8, rot=1))[..., 0, 0], x[..., 0, 7])
    assert torch.equal(T.restate(x, ED.Params(2, 8, 8, rot=-1))[..., 0, 0], x[..., 7, 0])


@pytest.mark.parametrize("case", list(T.CASES))
def test_seeded_host_draws_are_the_references(fx, case):
    """`draw` with the host generators seeded as the tool seeded them makes the reference's batch-wide draws exactly (the per-image
    draws come from another stream: torch's)."""
    shape = T.CASES[case]
    N, _, H, W = shape
    for name, t in fx["cases"][case]["sets"].items():
        if t["forced"]:
            continue
        T.seed_all(t["seed"])
        got = ED.draw(t["policy"], N, H, W, "cpu")
        assert (got.kind, got.flip, got.rot, got.zoom) == (t["kind"], t["flip"], t["rot"], t["zoom"]), (name, got.kind, got.zoom)
        ref = T.params_from_tape(t["policy"], t["tape"], shape)
        for a, b in ((got.color, ref.color), (got.translation, ref.translation), (got.cutout, ref.cutout)):
            assert (a is None) == (b is None)
            # same torch generator, same call order on the CPU: the per-image draws agree too
            for u, v in zip(a or (), b or ()):
                assert torch.equal(u.double(), v.double().float().double()), name


def test_device_side_draws_lie_in_the_references_ranges():
    torch.manual_seed(5)
    N, H, W = 4096, 33, 40
    p = ED.draw("color,translation,cutout", N, H, W, "cpu")
    b, sat, con = p.color
    assert all(t.dtype == torch.float32 and t.numel() == N for t in p.color)
    assert b.min() >= -0.5 and b.max() < 0.5 and sat.min() >= 0 and sat.max() < 2 and con.min() >= 0.5 and con.max() < 1.5
    assert b.min() < -0.49 and b.max() > 0.49 and sat.max() > 1.98 and con.min() < 0.51
    ty, tx = p.translation
    assert (int(ty.min()), int(ty.max())) == (-4, 4) and (int(tx.min()), int(tx.max())) == (-5, 5)          # round(33 / 8), round(40 / 8)
    oy, ox = p.cutout
    # box 17 x 20: the odd size draws offsets in [0, H), the even one in [0, W]
    assert ED.cutout_size(H, W) == (17, 20)
    assert (int(oy.min()), int(oy.max())) == (0, H - 1) and (int(ox.min()), int(ox.max())) == (0, W)
    blk = p.block("cpu")
    assert blk.shape == (N, 8) and blk.dtype == torch.float32
    assert torch.equal(blk[:, 2], con) and torch.equal(blk.view(torch.int32)[:, 3], ty) and torch.equal(blk.view(torch.int32)[:, 6], ox)


def test_host_draws_are_consumed_as_the_reference_consumes_them():
    """rand_90's if / elif takes one draw when the first is below prob / 2 and two otherwise; flip one; zoom_in three and zoom_out two
    after the choice."""
    def consumed(policy, force, H=16, W=16):
        t = T.Tape(force=force)
        with t.on(ED):
            p = ED.draw(policy, 2, H, W, "cpu")
        return [k for k, _ in t.log], p

    assert consumed("rotate", {"random": [0.1]})[0] == ["random"] and consumed("rotate", {"random": [0.1]})[1].rot == 1
    kinds, p = consumed("rotate", {"random": [0.9, 0.1]})
    assert kinds == ["random", "random"] and p.rot == -1
    kinds, p = consumed("rotate", {"random": [0.3, 0.6]})
    assert kinds == ["random", "random"] and p.rot == 0
    kinds, p = consumed("flip", {"random": [0.6]})
    assert kinds == ["random"] and p.flip
    kinds, p = consumed("transl_zoom", {"choice": [1], "uniform": [1.6], "random": [0.5, 0.25]})
    assert kinds == ["choice", "uniform", "random", "random"] and p.kind == "zoom_in" and p.zoom == (3, 1, 10, 10)
    kinds, p = consumed("transl_zoom", {"choice": [2], "uniform": [0.5, -0.5]})
    assert kinds == ["choice", "uniform", "uniform"] and p.kind == "zoom_out" and p.zoom == (4 + 2, 4 - 2, 4 + 2, 4 - 2)
    kinds, p = consumed("transl_zoom", {"choice": [0]})
    assert kinds == ["choice", "randint", "randint"] and p.kind == "translation"
    kinds, p = consumed("zoom", {"choice": [0], "uniform": [1.0]})          # scale exactly 1: the reference returns the image
    assert kinds == ["choice", "uniform"] and p.kind == "identity"
    kinds, p = consumed("translation", {})
    assert kinds == ["randint", "randint"]          # no choice for a single-entry policy
    kinds, p = consumed(T.RECIPE, {"choice": [0], "random": [0.9, 0.9, 0.9]})
    assert kinds == ["rand"] * 3 + ["choice", "randint", "randint", "random", "random", "random", "randint", "randint"]


def test_option_surface(caplog):
    """Fails before this feature: `diffaug: true` used to raise NotImplementedError in Adversarial.__init__."""
    import logging
    from trainner_amd.models import losses
    from trainner_amd.models.base_model import BaseModel

    class Dp:
        active = False

    def model_with(train):
        m = BaseModel.__new__(BaseModel)
        m.opt, m.device, m.dp = {"train": dict({"gan_type": "vanilla", "gan_weight": 5e-3}, **train)}, "cpu", Dp()
        m.setup_gan()
        return m

    m = model_with({})
    assert not m.adversarial.diffaug
    m = model_with({"diffaug": True})
    assert m.adversarial.diffaug and m.adversarial.dapolicy == "color,translation,cutout"
    m = model_with({"diffaug": True, "dapolicy": T.RECIPE})
    assert m.adversarial.dapolicy == T.RECIPE
    with caplog.at_level(logging.INFO, logger="base"):
        model_with({"diffaug": True})
    assert any("Differential augmentations enabled" in r.getMessage() for r in caplog.records)
    for bad in ("offset", "offset_h", "offset_v"):
        with pytest.raises(NotImplementedError, match="'%s'" % bad):
            model_with({"diffaug": True, "dapolicy": "color," + bad})
    for order in ("cutout,color", "rotate,flip", "translation,zoom", "color,color", "flip,transl_zoom"):
        with pytest.raises(NotImplementedError, match=order):
            model_with({"diffaug": True, "dapolicy": order})
    with pytest.raises(KeyError, match="sharpen"):
        ED.parse_policy("color,sharpen")
    with pytest.raises(NotImplementedError, match="gan_featmaps"):
        losses.Adversarial({"gan_type": "vanilla", "gan_weight": 1, "gan_featmaps": True}, device="cpu")
    with pytest.raises(NotImplementedError, match="gan_featmaps"):
        losses.Adversarial({"gan_type": "vanilla", "gan_weight": 1, "gan_featmaps": True}, device="cpu", diffaug=True, dapolicy="color")
    x = torch.rand(2, 3, 8, 12)
    with pytest.raises(NotImplementedError, match="channels_first=False"):
        ED.DiffAugment(x, "color", channels_first=False)
    with pytest.raises(NotImplementedError, match="rotate"):
        ED.DiffAugment(x, "color,rotate")
    with pytest.raises(NotImplementedError, match="rotate"):
        ED.draw("rotate", 2, 8, 12, "cpu")
    with pytest.raises(NotImplementedError, match="offset_h"):
        ED.DiffAugment(x, "offset_h")
    with pytest.raises(NotImplementedError, match="channels"):
        ED.DiffAugment(torch.rand(1, 5, 8, 8), "color")
    assert ED.DiffAugment(x, "") is x          # an empty policy is the identity, as in the reference


def test_no_device_no_fallback():
    from trainner_amd import hip
    with pytest.raises(hip.HipEngineError):
        ED.DiffAugment(torch.rand(2, 3, 8, 8), "color,translation,cutout")


@pytest.mark.parametrize("conditional", [False, True])
@pytest.mark.parametrize("diffaug", [True, False])
def test_adversarial_augments_after_the_filter_and_before_the_concatenation(conditional, diffaug, monkeypatch):
    """fsfilter -> diffaug -> concat; fake and (a tensor) real are two calls per stage, each with the policy; the discriminator stage
    augments fake.detach(); the condition is not augmented; without `diffaug` nothing is called."""
    from trainner_amd import hip
    from trainner_amd.dataops import filters as EF
    from trainner_amd.models import losses

    class Rec(EF.FilterHigh):
        def __init__(self):
            super().__init__(filter_type="average")
            self.seen = []

        def forward(self, img):
            self.seen.append(img)
            return img + 1.0

    aug = []

    def fake_aug(x, policy="", channels_first=True, params=None):
        aug.append((x, policy))
        return x * 2.0

    monkeypatch.setattr(losses.diffaug_ops, "DiffAugment", fake_aug)
    adv = losses.Adversarial({"gan_type": "vanilla", "gan_weight": 1, "gan_opt": {"form": "standard"}}, device="cpu", diffaug=diffaug,
                             dapolicy=T.RECIPE if diffaug else None, conditional=conditional)
    fake = torch.rand(1, 3, 8, 8, requires_grad=True) * 1.0
    real, cond = torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8)
    seen = []

    def netD(x):
        seen.append(x)
        return x.mean().reshape(1)

    for stage in ("generator", "discriminator"):
        for flt in (Rec(), None):
            del aug[:], seen[:]
            with pytest.raises(hip.HipEngineError):          # the GAN criterion itself needs the device; the routing is done by then
                adv(fake, real, cond if conditional else None, netD=netD, stage=stage, fsfilter=flt)
            pre = 1.0 if flt is not None else 0.0
            if not diffaug:
                assert aug == []
                want = fake.detach() + pre
            else:
                assert [p for _, p in aug] == [T.RECIPE, T.RECIPE]
                assert [t.requires_grad for t, _ in aug] == [stage == "generator", False]
                assert torch.equal(aug[0][0].detach(), fake.detach() + pre) and torch.equal(aug[1][0], real + pre)
                assert all(t.shape[1] == 3 for t, _ in aug)
                want = (fake.detach() + pre) * 2.0
            got = seen[0]
            if conditional:
                assert got.shape[1] == 6 and torch.equal(got[:, :3], cond) and torch.equal(got[:, 3:].detach(), want)
            else:
                assert torch.equal(got.detach(), want)
    # real that is no tensor (None in the standard form's generator stage) is not augmented
    del aug[:]
    with pytest.raises(hip.HipEngineError):
        adv(fake, None, cond if conditional else None, netD=netD, stage="generator")
    assert len(aug) == (1 if diffaug else 0)


def test_header_and_exports_declare_the_new_entry_points():
    from trainner_amd import hip
    with open(os.path.join(ROOT, "include", "trainner_hip.h")) as fh:
        declared = set(re.findall(r"\b(tnr_\w+)\s*\(", fh.read()))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(hip.EXPORTS)
    lib = hip.load()          # types every export: a symbol the library lacks raises here
    assert lib.tnr_version() == hip.ABI_VERSION == 3          # additions only: no descriptor changed
    assert lib.tnr_diffaug_workspace_bytes(16) == 16 * 64 * 8
    from trainner_amd import build, ops
    assert "diffaug.hip" in build.SOURCES
    assert all(hasattr(ops, n) for n in ("diffaug_mean", "diffaug_fwd", "diffaug_bwd"))
    # the argument checks run before anything touches the device: rotation on a rectangle, > 4 channels, a crop outside the image
    geo = lambda *g: (hip.C.c_int32 * 9)(*g)
    for args, word in (((1, 3, 8, 12, 0, geo(0, 0, 1, 0, 0, 0, 0, 0, 0)), "rotate"), ((1, 5, 8, 8, 0, geo(0, 0, 0, 0, 0, 0, 0, 0, 0)), "4 channels"),
                       ((1, 3, 8, 8, 0, geo(2, 0, 0, 4, 4, 8, 8, 0, 0)), "zoom_in"), ((1, 3, 8, 8, 0, geo(3, 0, 0, 1, 0, 8, 8, 0, 0)), "zoom_out"),
                       ((1, 3, 8, 8, 2, geo(0, 0, 0, 0, 0, 0, 0, 0, 0)), "layout")):
        assert lib.tnr_diffaug_fwd(1 << 12, *args[:5], 1 << 12, args[5], None, 1 << 13, None) != 0
        assert word in lib.tnr_last_error().decode(), (word, lib.tnr_last_error())
