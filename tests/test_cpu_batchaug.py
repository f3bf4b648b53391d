"""Batch augmentations (mixup / mixopts / ...), the parts that need no device: the fp32 restatement of tools/make_golden_batchaug.py
against tests/golden/batchaug.pt (the REAL reference's runs, bit for bit), hand-worked 4 x 4 cases of every op, `draw` against the
reference's recorded draws (call order included), the refusals, the option surface, the routing of the three models'
`optimize_parameters` (with recording stand-ins), and header <-> library <-> binding agreement."""
import logging
import os
import re

import numpy as np
import pytest
import torch

from oracle import fixtures as FX
from tools import make_golden_batchaug as T
from trainner_amd.dataops import batchaug as EB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "batchaug.pt")
NEW_EXPORTS = {"tnr_batchaug_mix", "tnr_batchaug_mask"}
RECIPES = ("sr/train_sr.yml", "i2i/train_pix2pix.yml", "i2i/train_cyclegan.yml")
# the commented block of the three shipped recipes, uncommented
MIXUP_BLOCK = {"mixup": True, "mixopts": ["blend", "rgb", "mixup", "cutmix", "cutmixup"], "mixprob": [1.0, 1.0, 1.0, 1.0, 1.0],
               "mixalpha": [0.6, 1.0, 1.2, 0.7, 0.7], "aux_mixprob": 1.0, "aux_mixalpha": 1.2}


def mixup_recipe_edit(tree):
    tree["train"].update(MIXUP_BLOCK)


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


def test_fixture_is_small_and_complete(fx):
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert set(fx["cases"]) == set(T.CASES)
    assert fx["recipe"] == {"options": T.RECIPE_OPTS, "probs": T.RECIPE_PROB, "alphas": T.RECIPE_ALPHA}
    assert T.RECIPE_OPTS == MIXUP_BLOCK["mixopts"] and T.RECIPE_ALPHA == MIXUP_BLOCK["mixalpha"]
    for case, (s1, s2) in T.CASES.items():
        sets = T.sets_for(case)
        rec = fx["cases"][case]
        assert rec["shapes"] == (s1, s2) and set(rec["sets"]) == set(sets)
        for name, (call, force, seed) in sets.items():
            t = rec["sets"][name]
            assert t["call"] == call and t["seed"] == seed and t["forced"] == bool(force)
        s = rec["sets"]
        h, w = s2[2:]
        # the hand-set extremes are what they claim to be
        key = lambda n: dict(zip(("aug", "hit", "N", "h", "w", "scale", "v", "col", "perm", "r", "box", "coin", "aux", "mask"), s[n]["key"]))  # noqa: E731
        ch, cw = int(h * 0.7), int(w * 0.7)
        assert key("box-first")["box"] == (0, 0, ch, cw) and key("box-last")["box"] == (h - ch, w - cw, ch, cw)
        assert key("box-empty")["box"][2:] == (0, 0) and key("box-empty")["hit"]
        assert key("box-short")["box"] == (1, 0, h - 1, w - 1)
        for x0 in (1, 2, 3):
            b = key("box-x%d" % x0)["box"]
            assert b[1] == x0 and b[3] % 2 == 1
        assert [key("mixup-" + k)["v"] for k in ("lo", "half", "hi")] == [1e-6, 0.5, 1 - 1e-6]
        N = s1[0]
        assert key("perm-identity")["r"] == list(range(N)) and all(i != j for i, j in enumerate(key("perm-derangement")["r"]))
        assert [(key("cutmixup-%s-%s" % (c, a))["coin"], key("cutmixup-%s-%s" % (c, a))["aux"]) for c in ("in", "out") for a in ("hit", "miss")] == \
            [(True, True), (True, False), (False, True), (False, False)]
        if s1 == s2:
            assert key("cutblur-in")["coin"] and not key("cutblur-out")["coin"]
        assert key("cutout-miss")["aug"] == "cutout" and not key("cutout-miss")["hit"]
        for n in s:
            if n.startswith("miss-"):
                assert not key(n)["hit"]
            if n.startswith("op-") and n != "op-none":
                assert key(n)["hit"], n
    assert set(fx["steps"]) == {"sr", "pix2pix"}
    assert [c["aug"] for c in fx["steps"]["sr"]["calls"]] == T.SR_FORCED == ["cutmixup", "cutout"]
    assert [c["aug"] for c in fx["steps"]["pix2pix"]["calls"]] == T.I2I_FORCED == ["cutblur", "blend"]


@pytest.mark.parametrize("case", list(T.CASES))
def test_restatement_matches_the_reference_record(fx, case):
    """SHA-256 of the restatement's bytes = SHA-256 of the reference's output, for both images and both masked images of every set."""
    rec = fx["cases"][case]
    s1, s2 = T.CASES[case]
    img1, img2 = T.make_pair(case)
    gen, tgt = T.make_pair(case, 1)
    assert T.probe(img1) == rec["x1"] and T.probe(img2) == rec["x2"]
    for name, t in rec["sets"].items():
        prm = T.params_from_tape(t["call"], t["tape"], s1, s2)
        o1, o2 = T.restate(prm, img1, img2)
        assert T.sha(o1) == t["sha"]["img1"] and T.sha(o2) == t["sha"]["img2"], name
        assert T.probe(o1) == t["probes"]["img1"] and T.probe(o2) == t["probes"]["img2"], name
        if prm.aug == "cutout":
            gen_m, tgt_m = T.restate_mask(gen, prm.mask, prm.scale), T.restate_mask(tgt, prm.mask, prm.scale)
        else:
            gen_m, tgt_m = gen, tgt
        assert T.sha(gen_m) == t["sha"]["gen"] and T.sha(tgt_m) == t["sha"]["tgt"], name


@pytest.mark.parametrize("case", list(T.CASES))
def test_draw_reproduces_the_recorded_parameters(fx, case):
    """`draw`, fed the reference's tape, makes the recorded record and leaves the tape empty (same draws, same order); with the real
    generators seeded as the tool seeded them it makes the same record again."""
    s1, s2 = T.CASES[case]
    for name, t in fx["cases"][case]["sets"].items():
        prm = T.params_from_tape(t["call"], t["tape"], s1, s2)          # asserts the tape is used up
        assert prm.key() == t["key"], name
        assert (prm.aug, prm.hit) == (t["aug"], t["hit"])
        if not t["forced"]:
            T.seed_all(t["seed"])
            c = t["call"]
            got = EB.draw(c["options"], c["probs"], c["alphas"], c["aux_prob"], c["aux_alpha"], None, s1, s2, "cpu")
            assert got.key() == t["key"], name


def test_draws_are_consumed_as_the_reference_consumes_them():
    def consumed(call, force, s1=(2, 3, 16, 16), s2=(2, 3, 8, 8)):
        t = T.Tape(force=force)
        with t.on(EB):
            p = EB.draw(call["options"], call["probs"], call["alphas"], call["aux_prob"], call["aux_alpha"], None, s1, s2, "cpu")
        return [k for k, _ in t.log], p

    assert consumed(T.one("none"), {})[0] == ["choice"]
    assert consumed(T.one("blend"), {})[0] == ["choice", "pyrandom", "uniform_", "uniform"]
    assert consumed(T.one("blend", alpha=0.0), {})[0] == ["choice"]          # alpha <= 0 short-circuits the coin
    assert consumed(T.one("rgb"), {})[0] == ["choice", "pyrandom", "permutation"]
    assert consumed(T.one("mixup"), {})[0] == ["choice", "pyrandom", "beta", "randperm"]
    assert consumed(T.one("cutmix"), {})[0] == ["choice", "pyrandom", "randn", "randint", "randint", "randperm"]
    # cutmixup draws the Beta variate BEFORE the auxiliary coin and keeps the order when the auxiliary mixup misses
    kinds, p = consumed(T.one("cutmixup", aux_prob=0.5), {"pyrandom": [0.0, 0.9]})
    assert kinds == ["choice", "pyrandom", "randn", "randint", "randint", "randperm", "beta", "pyrandom", "random"] and not p.aux_hit
    assert consumed(T.one("cutout"), {})[0] == ["choice", "pyrandom", "choice_mask"]
    assert consumed(T.one("cutout", prob=0.0), {})[0] == ["choice", "pyrandom"]
    assert consumed(T.one("cutblur"), {}, s2=(2, 3, 16, 16))[0] == ["choice", "pyrandom", "randn", "randint", "randint", "random"]
    kinds, p = consumed(dict(T.one("mixup"), options=["none", "mixup"], probs=[1, 1], alphas=[1, 1.2]), {"choice": [1]})
    assert p.aug == "mixup" and kinds[0] == "choice"
    # np.int(h * ratio) is int(): 8 * 0.7 = 5.6 -> 5
    _, p = consumed(T.one("cutmix"), {"randn": [0.0], "randint": [3, 2]})
    assert p.box == (3, 2, 5, 5) and p.scale == 2


def _t(vals):
    return torch.tensor(vals, dtype=torch.float32)


def test_hand_cases():
    """4 x 4 images, two per batch, one channel unless the op needs three: every op by hand."""
    a = torch.arange(32, dtype=torch.float32).reshape(2, 1, 4, 4)
    kw = dict(N=2, h=4, w=4, scale=1)
    # none / a miss: the inputs themselves
    o1, o2 = T.restate(EB.Params("mixup", False, **kw), a, a + 100)
    assert o1 is a
    # mixup with lam = 0.25 and r = [1, 0]: 0.25 x[n] + 0.75 x[1 - n] (exact in fp32)
    o1, _ = T.restate(EB.Params("mixup", True, v=0.25, r=[1, 0], **kw), a, a)
    assert torch.equal(o1[0], 0.25 * a[0] + 0.75 * a[1]) and torch.equal(o1[1], 0.25 * a[1] + 0.75 * a[0])
    # cutmix: the 2 x 2 box at (1, 2) comes from the partner, the rest stays
    o1, _ = T.restate(EB.Params("cutmix", True, box=(1, 2, 2, 2), r=[1, 0], **kw), a, a)
    want = a[0].clone()
    want[:, 1:3, 2:4] = a[1][:, 1:3, 2:4]
    assert torch.equal(o1[0], want)
    # ... and on a target at scale 2 the box is twice as large at twice the offset
    A = torch.arange(128, dtype=torch.float32).reshape(2, 1, 8, 8)
    O1, o2 = T.restate(EB.Params("cutmix", True, box=(1, 2, 2, 2), r=[1, 0], N=2, h=4, w=4, scale=2), A, a)
    want = A[0].clone()
    want[:, 2:6, 4:8] = A[1][:, 2:6, 4:8]
    assert torch.equal(O1[0], want) and torch.equal(o2[0], o1[0])
    # cutmixup, coin: inside the mixture, outside the image; no coin: the other way round; auxiliary miss: the partner itself
    mix = 0.5 * a[0] + 0.5 * a[1]
    box = torch.zeros(4, 4, dtype=torch.bool)
    box[0:2, 0:3] = True
    o1, _ = T.restate(EB.Params("cutmixup", True, box=(0, 0, 2, 3), r=[1, 0], v=0.5, aux_hit=True, coin=True, **kw), a, a)
    assert torch.equal(o1[0], torch.where(box, mix, a[0]))
    o1, _ = T.restate(EB.Params("cutmixup", True, box=(0, 0, 2, 3), r=[1, 0], v=0.5, aux_hit=True, coin=False, **kw), a, a)
    assert torch.equal(o1[0], torch.where(box, a[0], mix))
    o1, _ = T.restate(EB.Params("cutmixup", True, box=(0, 0, 2, 3), r=[1, 0], v=0.5, aux_hit=False, coin=False, **kw), a, a)
    assert torch.equal(o1[0], torch.where(box, a[0], a[1]))
    # cutblur: the target is untouched; coin: the input gets the target's box; no coin: the target with the input's box
    b = a + 100
    o1, o2 = T.restate(EB.Params("cutblur", True, box=(0, 0, 2, 3), coin=True, **kw), a, b)
    assert o1 is a and torch.equal(o2[1], torch.where(box, a[1], b[1]))
    o1, o2 = T.restate(EB.Params("cutblur", True, box=(0, 0, 2, 3), coin=False, **kw), a, b)
    assert o1 is a and torch.equal(o2[1], torch.where(box, b[1], a[1]))
    # cutout: the input times the mask, the target untouched; the kept mask is nearest x scale for the target-sized images
    m = np.ones((2, 4, 4), dtype=np.uint8)
    m[0, 1, 2] = m[1, 3, 0] = 0
    neg = -torch.ones(2, 1, 4, 4)
    O1, o2 = T.restate(EB.Params("cutout", True, mask=m, N=2, h=4, w=4, scale=2), A, neg)
    assert O1 is A and o2[0, 0, 1, 2].item() == 0 and np.signbit(o2[0, 0, 1, 2].item())          # -1 * 0 = -0.0: a real product
    assert o2.sum().item() == -30.0
    up = T.restate_mask(A, m, 2)
    assert up[0, 0, 2:4, 4:6].abs().sum().item() == 0 and up[1, 0, 6:8, 0:2].abs().sum().item() == 0 and (up != A).sum().item() == 8
    # rgb: out[:, c] = in[:, perm[c]]
    c3 = torch.arange(96, dtype=torch.float32).reshape(2, 3, 4, 4)
    o1, _ = T.restate(EB.Params("rgb", True, perm=(2, 0, 1), **kw), c3, c3)
    assert torch.equal(o1[:, 0], c3[:, 2]) and torch.equal(o1[:, 1], c3[:, 0]) and torch.equal(o1[:, 2], c3[:, 1])
    # blend: v x + (1 - v) colour[n, c]
    col = _t([[0.0, 1.0, 2.0], [4.0, 8.0, 16.0]])
    o1, _ = T.restate(EB.Params("blend", True, v=0.5, colour=col, **kw), c3, c3)
    assert torch.equal(o1[1, 2], 0.5 * c3[1, 2] + 8.0) and torch.equal(o1[0, 0], 0.5 * c3[0, 0])
    # the separate-rounding rule differs from a fused multiply-add somewhere on ordinary data
    x, y = T.make_pair("sr4")[0], T.make_pair("sr4", 1)[0]
    v = 0.3
    two = T._lerp(v, x, 1.0 - v, y)
    exact = (np.float32(v).astype(np.float64) * x.double() + np.float32(1.0 - v).astype(np.float64) * y.double()).float()
    assert (two != exact).any()


def test_refusals_name_their_values():
    ok = dict(MIXUP_BLOCK)
    for bad, word in ((dict(ok, mixopts=["blend", "sharpen"], mixprob=[1, 1], mixalpha=[1, 1]), "sharpen"),
                      (dict(ok, mixprob=[1.0, 1.0]), r"mixprob \[1.0, 1.0\]"), (dict(ok, mixalpha=[0.6]), r"mixalpha \[0.6\]"),
                      (dict(ok, mix_p=[0.5, 0.5]), r"mix_p \[0.5, 0.5\]"), (dict(ok, mix_p=[0.3, 0.3, 0.3, 0.3, 0.3]), "mix_p"),
                      (dict(ok, aux_mixalpha=0.0), "aux_mixalpha 0.0"), (dict(ok, aux_mixalpha=-1), "aux_mixalpha -1")):
        with pytest.raises(ValueError, match=word):
            EB.BatchAugment(bad)
    EB.BatchAugment(dict(ok, mixopts=["mixup"], mixprob=[1.0], mixalpha=[1.2], aux_mixalpha=0.0))          # no cutmixup: aux unused
    EB.BatchAugment(dict(ok, mix_p=[0.2] * 5))
    ba = EB.BatchAugment(ok)
    x = torch.rand(2, 3, 8, 8)
    with pytest.raises(ValueError, match=r"\(2, 3, 9, 8\)"):
        ba(torch.rand(2, 3, 9, 8), torch.rand(2, 3, 4, 4))
    with pytest.raises(ValueError, match="exact multiple"):
        ba(torch.rand(2, 3, 16, 8), x)
    with pytest.raises(NotImplementedError, match="5 channels"):
        ba(torch.rand(2, 5, 8, 8), torch.rand(2, 5, 8, 8))
    blend = EB.BatchAugment(dict(ok, mixopts=["blend"], mixprob=[1.0], mixalpha=[0.6]))
    with pytest.raises(NotImplementedError, match="blend.*3 channels.*1"):
        blend(torch.rand(2, 1, 8, 8), torch.rand(2, 1, 8, 8))
    blur = EB.BatchAugment(dict(ok, mixopts=["cutblur"], mixprob=[1.0], mixalpha=[0.7]))
    with pytest.raises(ValueError, match="cutblur.*same resolution"):
        blur(torch.rand(2, 3, 16, 16), x)
    with pytest.raises(ValueError, match="no permutation"):
        EB.Params("mixup", True, 3, 4, 4, 1, v=0.5, r=[0, 0, 1])
    with pytest.raises(ValueError, match="box"):
        EB.Params("cutmix", True, 2, 4, 4, 1, box=(2, 2, 3, 1), r=[1, 0])
    with pytest.raises(ValueError, match="parameter record"):
        EB.apply(EB.Params("mixup", True, 3, 4, 4, 1, v=0.5, r=[0, 2, 1]), x, x)


def test_attribute_surface_and_defaults():
    ba = EB.BatchAugment({})
    assert ba.mixopts == ["blend", "rgb", "mixup", "cutmix", "cutmixup", "cutout"]
    assert ba.mixprob == [1.0] * 6 and ba.mixalpha == [0.6, 1.0, 1.2, 0.7, 0.7, 0.001]
    assert (ba.aux_mixprob, ba.aux_mixalpha, ba.mix_p, ba.aug, ba.mask) == (1.0, 1.2, None, None, None)
    ba = EB.BatchAugment(MIXUP_BLOCK)
    assert ba.mixopts == MIXUP_BLOCK["mixopts"] and ba.mixalpha == MIXUP_BLOCK["mixalpha"]
    # a miss and `none` return the very tensors that came in, launch nothing (there is no device here) and keep `aug`
    x1, x2 = torch.rand(2, 3, 16, 16), torch.rand(2, 3, 8, 8)
    for opt in (dict(mixopts=["none"], mixprob=[1.0], mixalpha=[1.0]), dict(mixopts=["mixup"], mixprob=[0.0], mixalpha=[1.2]),
                dict(mixopts=["cutmix"], mixprob=[1.0], mixalpha=[0.0])):
        ba = EB.BatchAugment(opt)
        o1, o2 = ba(x1, x2)
        assert o1 is x1 and o2 is x2 and ba.aug == opt["mixopts"][0] and ba.mask is None
        g1, g2 = ba.apply_mask(x1, x1)
        assert g1 is x1 and g2 is x1
    out = EB.BatchAug(x1, x2, ["none"], [1.0], [1.0])
    assert len(out) == 4 and out[0] is x1 and out[1] is x2 and out[2] is None and out[3] == "none"


def test_no_device_no_fallback():
    from trainner_amd import hip
    ba = EB.BatchAugment(dict(mixopts=["mixup"], mixprob=[1.0], mixalpha=[1.2]))
    with pytest.raises(hip.HipEngineError):
        ba(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 8, 8))
    with pytest.raises(hip.HipEngineError):
        EB.mask_mul(torch.rand(2, 3, 8, 8), torch.ones(2, 1, 8, 8, dtype=torch.uint8), 1)


# ------------------------------------------------------------------------------------------------ the models
class Rec:
    """A recording stand-in for BatchAugment."""

    def __init__(self, events):
        self.events = events

    def __call__(self, img1, img2):
        self.events.append(("aug", img1, img2))
        return img1 + 10.0, img2 + 10.0

    def apply_mask(self, img1, img2):
        self.events.append(("mask", img1, img2))
        return img1 * 2.0, img2 * 2.0


def _bare(cls, events, mixup):
    m = cls.__new__(cls)
    m.model_names, m.accumulations, m.cri_gan, m.D_update_ratio, m.D_init_iters, m.amp = [], 1, False, 1, 0, False
    m.mixup, m.optimizer_G, m.optimizer_D = mixup, None, None
    m.batchaugment = Rec(events) if mixup else None
    m.backward_G = lambda: events.append(("backward_G",))
    m.optimizer_step = lambda *a: None
    return m


@pytest.mark.parametrize("mixup", [True, None])
def test_sr_model_routing(mixup):
    from trainner_amd.models.sr_model import SRModel
    ev = []
    m = _bare(SRModel, ev, mixup)
    HR, LR, REF, GEN = torch.rand(2, 3, 8, 8), torch.rand(2, 3, 2, 2), torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8)
    m.real_H, m.var_L, m.var_ref = HR, LR, REF

    def forward():
        ev.append(("forward", m.real_H, m.var_L))
        m.fake_H = GEN
    m.forward = forward
    m.optimize_parameters(1)
    if not mixup:
        assert [e[0] for e in ev] == ["forward", "backward_G"] and m.real_H is HR and m.var_L is LR and m.fake_H is GEN
        return
    assert [e[0] for e in ev] == ["aug", "forward", "mask", "backward_G"]
    assert ev[0][1] is HR and ev[0][2] is LR                                   # (target, input)
    assert torch.equal(ev[1][1], HR + 10) and torch.equal(ev[1][2], LR + 10)   # the forward sees the augmented pair
    assert ev[2][1] is GEN and torch.equal(ev[2][2], HR + 10)                  # (generated, target)
    assert torch.equal(m.fake_H, GEN * 2) and torch.equal(m.real_H, (HR + 10) * 2) and torch.equal(m.var_L, LR + 10)
    assert m.var_ref is REF                                                    # the discriminator's real input is not touched


@pytest.mark.parametrize("mixup", [True, None])
def test_pix2pix_model_routing(mixup):
    from trainner_amd.models.pix2pix_model import Pix2PixModel
    ev = []
    m = _bare(Pix2PixModel, ev, mixup)
    A, B, GEN = torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8)
    m.real_A, m.real_B = A, B

    def forward():
        ev.append(("forward", m.real_A))
        m.fake_B = GEN
    m.forward = forward
    m.optimize_parameters(1)
    if not mixup:
        assert [e[0] for e in ev] == ["forward", "backward_G"] and m.real_A is A and m.real_B is B and m.fake_B is GEN
        return
    assert [e[0] for e in ev] == ["aug", "forward", "mask", "backward_G"]
    assert ev[0][1] is B and ev[0][2] is A                                     # (real_B, real_A)
    assert torch.equal(ev[1][1], A + 10)
    assert ev[2][1] is GEN and torch.equal(ev[2][2], B + 10)                   # (fake_B, real_B)
    assert torch.equal(m.fake_B, GEN * 2) and torch.equal(m.real_B, (B + 10) * 2) and torch.equal(m.real_A, A + 10)


@pytest.mark.parametrize("mixup", [True, None])
def test_cyclegan_model_routing(mixup):
    from trainner_amd.models.cyclegan_model import CycleGANModel
    ev = []
    m = _bare(CycleGANModel, ev, mixup)
    A, B = torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8)
    FB, FA, RA, RB = (torch.rand(2, 3, 8, 8) for _ in range(4))
    m.real_A, m.real_B = A, B

    def forward():
        ev.append(("forward", m.real_A, m.real_B))
        m.fake_B, m.fake_A, m.rec_A, m.rec_B = FB, FA, RA, RB
    m.forward = forward
    m.optimize_parameters(1)
    if not mixup:
        assert [e[0] for e in ev] == ["forward", "backward_G"] and m.real_A is A and m.fake_B is FB and m.fake_A is FA
        return
    assert [e[0] for e in ev] == ["aug", "forward", "mask", "mask", "backward_G"]
    assert ev[0][1] is B and ev[0][2] is A
    assert torch.equal(ev[1][1], A + 10) and torch.equal(ev[1][2], B + 10)
    assert ev[2][1] is FB and torch.equal(ev[2][2], B + 10) and ev[3][1] is FA and torch.equal(ev[3][2], A + 10)
    assert torch.equal(m.fake_B, FB * 2) and torch.equal(m.fake_A, FA * 2)
    assert torch.equal(m.real_B, (B + 10) * 2) and torch.equal(m.real_A, (A + 10) * 2)
    assert m.rec_A is RA and m.rec_B is RB                                     # computed from the unmasked fakes


def _setup(opt):
    from trainner_amd.models.base_model import BaseModel
    m = BaseModel.__new__(BaseModel)
    m.opt, m.batchaugment = opt, None
    m.setup_batchaug()
    return m


def test_setup_batchaug(caplog):
    """Fails before this feature: `mixup: true` used to raise NotImplementedError."""
    m = _setup({"scale": 4, "train": {}})
    assert not m.mixup and m.batchaugment is None
    with caplog.at_level(logging.INFO, logger="base"):
        m = _setup({"scale": 4, "train": dict(MIXUP_BLOCK)})
    assert m.mixup and isinstance(m.batchaugment, EB.BatchAugment) and m.batchaugment.mixopts == MIXUP_BLOCK["mixopts"]
    assert any("Batch augmentations enabled" in r.getMessage() for r in caplog.records)
    blur = dict(MIXUP_BLOCK, mixopts=["cutblur"], mixprob=[1.0], mixalpha=[0.7])
    with pytest.raises(NotImplementedError, match="cutblur.*scale 4"):
        _setup({"scale": 4, "train": blur})
    assert _setup({"scale": 1, "train": blur}).batchaugment.mixopts == ["cutblur"]
    with pytest.raises(ValueError, match="sharpen"):
        _setup({"scale": 4, "train": dict(MIXUP_BLOCK, mixopts=["sharpen"])})
    with pytest.raises(NotImplementedError, match="AdaTarget"):          # stays refused
        m.opt = {"use_atg": True}
        m.setup_atg()


@pytest.mark.parametrize("recipe", RECIPES)
def test_shipped_recipes_parse_and_construct_with_the_mixup_block(recipe, tmp_path):
    from trainner_amd.options import options
    opt = options.parse(FX.write_recipe(recipe, str(tmp_path), mixup_recipe_edit), is_train=True)
    assert opt["train"]["mixup"] is True and list(opt["train"]["mixopts"]) == MIXUP_BLOCK["mixopts"]
    m = _setup(opt)
    ba = m.batchaugment
    assert m.mixup and list(ba.mixopts) == MIXUP_BLOCK["mixopts"] and list(ba.mixalpha) == MIXUP_BLOCK["mixalpha"]
    assert (ba.aux_mixprob, ba.aux_mixalpha, ba.mix_p) == (1.0, 1.2, None)


def test_header_and_exports_declare_the_new_entry_points():
    from trainner_amd import build, hip, ops
    with open(os.path.join(ROOT, "include", "trainner_hip.h")) as fh:
        declared = set(re.findall(r"\b(tnr_\w+)\s*\(", fh.read()))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(hip.EXPORTS)
    lib = hip.load()          # types every export: a symbol the library lacks raises here
    assert lib.tnr_version() == hip.ABI_VERSION == 3          # additions only: no descriptor changed
    assert "batchaug.hip" in build.SOURCES and hasattr(ops, "batchaug_mix") and hasattr(ops, "batchaug_mask")
    assert (EB.SELF, EB.PARTNER, EB.LERP_PARTNER, EB.LERP_COLOUR) == (0, 1, 2, 3)
    # the argument checks run before anything touches the device
    prm = lambda *p: (hip.C.c_int32 * 10)(*p)          # noqa: E731
    P = 1 << 12
    for shape, p, word in (((1, 5, 8, 8, 0), prm(0, 0, 0, 0, 0, 0, 0, 1, 2, 3), "4 channels"),
                           ((1, 1, 8, 8, 0), prm(3, 3, 0, 0, 0, 0, 0, 0, 0, 0), "3 channels"),
                           ((1, 3, 8, 8, 0), prm(0, 4, 0, 0, 0, 0, 0, 1, 2, 0), "region code"),
                           ((1, 3, 8, 8, 0), prm(1, 0, 4, 4, 5, 2, 0, 1, 2, 0), "leaves"),
                           ((1, 3, 8, 8, 0), prm(0, 0, 0, 0, 0, 0, 0, 1, 3, 0), "permutation"),
                           ((1, 3, 8, 8, 0), prm(2, 0, 0, 0, 4, 4, 2, 0, 1, 0), "SELF regions only"),
                           ((1, 3, 8, 8, 2), prm(0, 0, 0, 0, 0, 0, 0, 1, 2, 0), "layout")):
        assert lib.tnr_batchaug_mix(P, P, None, P, *shape, p, 1.0, 0.0, 2 * P, None) != 0
        assert word in lib.tnr_last_error().decode(), (word, lib.tnr_last_error())
    assert lib.tnr_batchaug_mix(P, None, None, None, 1, 3, 8, 8, 0, prm(1, 0, 0, 0, 2, 2, 0, 1, 2, 0), 1.0, 0.0, 2 * P, None) != 0
    assert "null or aliased" in lib.tnr_last_error().decode()          # a PARTNER region without a second source
    assert lib.tnr_batchaug_mask(P, P, 1, 3, 8, 8, 0, 3, 2 * P, None) != 0
    assert "scale 3" in lib.tnr_last_error().decode()
    assert lib.tnr_batchaug_mask(P, None, 1, 3, 8, 8, 0, 2, 2 * P, None) != 0
    assert "null" in lib.tnr_last_error().decode()
