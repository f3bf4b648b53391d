"""Batch augmentations on the device (-m gpu): csrc/batchaug.hip through the C ABI (ops.batchaug_mix / batchaug_mask),
dataops/batchaug.py and the models' wiring, against tests/golden/batchaug.pt (the REAL reference's runs,
tools/make_golden_batchaug.py) and the tool's fp32 restatement, which the tool pinned to the reference bit for bit and
tests/test_cpu_batchaug.py pins to the fixture's SHA-256 sums again.

The criterion is bit-identity: no op moves a pixel, and every output element is a copy or fl(a x) + fl(b y).  There is no tolerance
anywhere in the kernel tests; NaNs (the `special` case) are held to their positions, every other element to its bits.  The step
records use the bounds of the other step-record tests, imported from them.
"""
import os

import pytest
import torch

from oracle import detrand, fixtures as FX, ref_harness
from tools import make_golden_batchaug as T
from trainner_amd.dataops import batchaug as EB

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batchaug.pt")
LAYOUTS = ("nchw", "cl")
MIXUP_BLOCK = {"mixup": True, "mixopts": ["blend", "rgb", "mixup", "cutmix", "cutmixup"], "mixprob": [1.0, 1.0, 1.0, 1.0, 1.0],
               "mixalpha": [0.6, 1.0, 1.2, 0.7, 0.7], "aux_mixprob": 1.0, "aux_mixalpha": 1.2}


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=False)


def to_dev(t, layout):
    return t.to(DEV).contiguous(memory_format=torch.channels_last if layout == "cl" else torch.contiguous_format)


def host(t):
    return t.detach().cpu().contiguous()


_PAIRS = {}


def pairs(case):
    """The seeded host tensors of a case, made once: (img1, img2, gen, tgt)."""
    if case not in _PAIRS:
        _PAIRS[case] = T.make_pair(case) + T.make_pair(case, 1)
    return _PAIRS[case]


def same(got, want, case):
    """Bit-identity; torch.equal too wherever no NaN was placed."""
    ok = T.bits_equal(host(got), want)
    return ok and (case == "special" or torch.equal(host(got), want))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", list(T.CASES))
def test_every_set_is_bit_identical_to_the_restatement(fx, case, layout):
    """Both images, the kept mask and both masked images of every set of the case."""
    img1, img2, gen, tgt = pairs(case)
    s1, s2 = T.CASES[case]
    d1, d2, dg, dt = (to_dev(t, layout) for t in (img1, img2, gen, tgt))
    for name, t in fx["cases"][case]["sets"].items():
        prm = T.params_from_tape(t["call"], t["tape"], s1, s2)
        w1, w2 = T.restate(prm, img1, img2)
        ba = EB.BatchAugment(dict(mixopts=t["call"]["options"], mixprob=t["call"]["probs"], mixalpha=t["call"]["alphas"],
                                  aux_mixprob=t["call"]["aux_prob"], aux_mixalpha=t["call"]["aux_alpha"]))
        o1, o2 = ba(d1, d2, params=prm)
        assert same(o1, w1, case) and same(o2, w2, case), (name, prm.aug)
        assert o1.stride() == d1.stride() and o2.stride() == d2.stride() and o1.dtype == o2.dtype == torch.float32
        assert ba.aug == t["aug"]
        if not prm.hit:
            assert o1 is d1 and o2 is d2, name          # no launch: the inputs themselves
        m1, m2 = ba.apply_mask(dg, dt)
        if prm.aug == "cutout":
            assert ba.mask.dtype == torch.uint8 and torch.equal(host(ba.mask).reshape(prm.mask.shape), torch.from_numpy(prm.mask)), name
            assert same(m1, T.restate_mask(gen, prm.mask, prm.scale), case) and same(m2, T.restate_mask(tgt, prm.mask, prm.scale), case), name
            assert m1.stride() == dg.stride()
        else:
            assert ba.mask is None and m1 is dg and m2 is dt


def test_special_values_keep_their_bits_and_their_places(fx):
    """-0.0, +-Inf and NaN: a copied element keeps its bits (SELF and PARTNER are no 1 * x + 0 * y), and a NaN of the partner reaches
    exactly the outputs that read it."""
    img1, img2, _, _ = pairs("special")
    s1, s2 = T.CASES["special"]
    d1, d2 = to_dev(img1, "nchw"), to_dev(img2, "nchw")
    bits = lambda t: host(t).view(torch.int32)          # noqa: E731
    N = s1[0]
    derange = [(i + 1) % N for i in range(N)]
    # cutmix with a box that holds no special pixel of the PARTNER: every special value stays where it was, and only there
    prm = EB.Params("cutmix", True, N, s2[2], s2[3], 2, box=(7, 8, 3, 5), r=derange)
    o1, o2, _ = EB.apply(prm, d1, d2)
    w1, w2 = T.restate(prm, img1, img2)
    assert torch.equal(bits(o1), w1.view(torch.int32)) and torch.equal(bits(o2), w2.view(torch.int32))
    assert torch.isnan(host(o2)).sum().item() == 1 and torch.equal(torch.isnan(host(o2)), torch.isnan(img2))
    assert torch.equal(bits(o2)[0, 0, 0, 0], img2.view(torch.int32)[0, 0, 0, 0]) and host(o2)[0, 0, 0, 0].item() == 0          # -0.0 kept
    # a box over the partner's NaN (image 2, channel 2, row 5, column 7): it moves to the image that reads image 2, once
    prm = EB.Params("cutmix", True, N, s2[2], s2[3], 2, box=(4, 6, 3, 3), r=derange)
    o1, o2, _ = EB.apply(prm, d1, d2)
    want = torch.zeros_like(img2, dtype=torch.bool)
    want[derange.index(2), 2, 5, 7] = True          # the reader; image 2's own pixel lies in the box and is replaced by ITS partner's
    assert torch.equal(torch.isnan(host(o2)), want)
    w1, w2 = T.restate(prm, img1, img2)
    assert T.bits_equal(host(o1), w1) and T.bits_equal(host(o2), w2)
    # mixup reads both sources everywhere: a NaN shows in its own image and in its reader, nowhere else
    prm = EB.Params("mixup", True, N, s2[2], s2[3], 2, v=0.5, r=derange)
    o1, o2, _ = EB.apply(prm, d1, d2)
    got = torch.isnan(host(o2))
    w1, w2 = T.restate(prm, img1, img2)
    assert torch.equal(got, torch.isnan(w2)) and T.bits_equal(host(o2), w2) and T.bits_equal(host(o1), w1)
    # the mask is a real product: -x * 0 = -0.0, NaN * 0 = NaN, Inf * 0 = NaN
    zero = torch.zeros(N, 1, s2[2], s2[3], dtype=torch.uint8, device=DEV)
    out = host(EB.mask_mul(d2, zero, 1))
    assert torch.equal(out.view(torch.int32)[~torch.isnan(out)], (img2 * 0.0).view(torch.int32)[~torch.isnan(out)])
    assert torch.equal(torch.isnan(out), torch.isnan(img2) | torch.isinf(img2)) and (out.view(torch.int32) < 0).any()


@pytest.mark.parametrize("case", ["sr4", "i2i"])
def test_unaligned_view_agrees_with_the_aligned_run(fx, case):
    """An NCHW view whose storage starts one element into an allocation takes the scalar path: same bits."""
    img1, img2, gen, _ = pairs(case)
    s1, s2 = T.CASES[case]

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    for name in ("op-cutmixup", "op-mixup", "op-blend", "op-rgb", "box-x1", "cutout-half") + (("cutblur-in",) if case == "i2i" else ()):
        t = fx["cases"][case]["sets"][name]
        prm = T.params_from_tape(t["call"], t["tape"], s1, s2)
        a1, a2, mask = EB.apply(prm, to_dev(img1, "nchw"), to_dev(img2, "nchw"))
        u1, u2, _ = EB.apply(prm, shifted(img1), shifted(img2))
        assert torch.equal(a1, u1) and torch.equal(a2, u2), name
        if mask is not None:
            assert torch.equal(EB.mask_mul(to_dev(gen, "nchw"), mask, prm.scale), EB.mask_mul(shifted(gen), mask, prm.scale))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case, s", [("i2i", 1), ("sr2", 2), ("sr4", 4), ("sr4odd", 4)])
def test_apply_mask_forward_and_backward(fx, case, s, layout):
    """apply_mask on a tensor that requires grad: forward bitwise, backward gx == g * mask bitwise (its own adjoint), one launch each."""
    _, _, gen, tgt = pairs(case)
    s1, s2 = T.CASES[case]
    t = fx["cases"][case]["sets"]["cutout-half"]
    prm = T.params_from_tape(t["call"], t["tape"], s1, s2)
    assert prm.scale == s and 0 < prm.mask.mean() < 1
    ba = EB.BatchAugment(dict(mixopts=["cutout"], mixprob=[1.0], mixalpha=[0.5]))
    ba.aug, ba.mask = "cutout", prm.on_device("mask", DEV)
    dg = to_dev(gen, layout).requires_grad_(True)
    o1, o2 = ba.apply_mask(dg, to_dev(tgt, layout))
    assert o1.requires_grad and not o2.requires_grad
    assert torch.equal(host(o1), T.restate_mask(gen, prm.mask, s)) and torch.equal(host(o2), T.restate_mask(tgt, prm.mask, s))
    g = detrand.uniform(s1, 77, -1.0, 1.0).float()
    o1.backward(to_dev(g, layout))
    assert torch.equal(host(dg.grad), T.restate_mask(g, prm.mask, s)) and dg.grad.stride() == dg.stride()


def test_two_runs_are_bit_identical(fx):
    img1, img2, gen, _ = pairs("tiles")
    s1, s2 = T.CASES["tiles"]
    for layout in LAYOUTS:
        d1, d2 = to_dev(img1, layout), to_dev(img2, layout)
        for name in ("op-cutmixup", "op-blend", "cutout-half"):
            t = fx["cases"]["tiles"]["sets"][name]
            prm = T.params_from_tape(t["call"], t["tape"], s1, s2)
            a, b = EB.apply(prm, d1, d2), EB.apply(prm, d1, d2)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_half_inputs_are_promoted_and_channels_last_is_kept(fx):
    img1, img2, gen, tgt = pairs("sr2")
    s1, s2 = T.CASES["sr2"]
    t = fx["cases"]["sr2"]["sets"]["op-cutmixup"]
    prm = T.params_from_tape(t["call"], t["tape"], s1, s2)
    for dt in (torch.float16, torch.bfloat16):
        h1, h2 = to_dev(img1.to(dt), "cl"), to_dev(img2.to(dt), "cl")
        o1, o2, _ = EB.apply(prm, h1, h2)
        assert o1.dtype == o2.dtype == torch.float32
        assert o1.is_contiguous(memory_format=torch.channels_last) and o2.is_contiguous(memory_format=torch.channels_last)
        w1, w2 = T.restate(prm, img1.to(dt).float(), img2.to(dt).float())
        assert torch.equal(host(o1), w1) and torch.equal(host(o2), w2)
    t = fx["cases"]["sr2"]["sets"]["cutout-half"]
    prm = T.params_from_tape(t["call"], t["tape"], s1, s2)
    ba = EB.BatchAugment(dict(mixopts=["cutout"], mixprob=[1.0], mixalpha=[0.5]))
    o1, o2 = ba(to_dev(img1.half(), "cl"), to_dev(img2.half(), "cl"), params=prm)
    assert o1.dtype == torch.float16 and o2.dtype == torch.float32          # cutout leaves the target alone
    m1, _ = ba.apply_mask(to_dev(gen.half(), "cl"), to_dev(tgt, "cl"))
    assert m1.dtype == torch.float32 and torch.equal(host(m1), T.restate_mask(gen.half().float(), prm.mask, 2))


# ------------------------------------------------------------------------------------------------ the models
def _engine_sr_model(fxs, tmp_path, mix=None, name="engine_batchaug_sr"):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = ref_harness.esrgan_yaml(name=name, out_root=str(tmp_path), gpu_ids="[0]", **fxs["spec"]["yaml"])
    if mix:
        T.mixup_yaml(yml, mix)
    opt = options.parse(yml, is_train=True)
    model = create_model(opt, verbose=False)
    g, d, f = FX.initial_states(fxs)
    model.netG.load_state_dict(g)
    model.netD.load_state_dict(d)
    netF = [l["function"].network for l in model.generatorlosses.loss_list if "fea" in l["name"]][0]
    sd = netF.state_dict()
    sd.update(f)
    netF.load_state_dict(sd)
    return model


def _replay(calls):
    """A tape that hands the engine's `draw` the reference's recorded draws of all calls, in order."""
    return T.Tape(replay=[d for c in calls for d in c["tape"]])


def test_sr_step_matches_reference_record(fx, tmp_path):
    """optimize_parameters with mixup: true against the real reference's SRModel, two steps (cutmixup, then cutout with alpha 0.3: the
    mask's backward reaches the generator's gradient), replaying the reference's draws, with the bounds tests/test_gpu_step.py uses."""
    import test_gpu_step as TS
    fxs = fx["steps"]["sr"]
    tol = TS.DEFAULT_TOL
    model = _engine_sr_model(fxs, tmp_path, fxs["mix"])
    assert model.mixup and model.batchaugment.mixopts == fxs["mix"]["mixopts"]
    assert [l["name"] for l in model.generatorlosses.loss_list] == fxs["loss_names"]
    tape = _replay(fxs["calls"])
    augs = []
    with tape.on(EB):
        for (s, (LR, HR)), ref_log in zip(FX.batches(fxs), fxs["logs"]):
            model.feed_data({"LR": LR, "HR": HR})
            model.optimize_parameters(s)
            augs.append(model.batchaugment.aug)
            log = model.get_current_log()
            print("\nstep", s, {k: (round(log[k], 7), round(v, 7)) for k, v in ref_log.items()})
            TS.check_logs(log, ref_log, tol=tol["log"])
    assert tape.replay == [] and augs == [c["aug"] for c in fxs["calls"]]
    ref, got = fxs["fake_H"], model.fake_H.detach().cpu()
    scale = max(1.0, ref.abs().max().item())
    diff = (got - ref).abs()
    assert diff.mean().item() <= tol["fake_mean"] * scale and diff.max().item() <= tol["fake_max"] * scale, (diff.mean().item(), diff.max().item())
    lr_steps = 1e-4 * fxs["spec"]["steps"]
    worst, mean, k = FX.state_error({k: v.detach().cpu() for k, v in model.netG.state_dict().items()}, fxs["g_state"], lr_steps=lr_steps)
    assert mean < tol["st_mean"] and worst < tol["st_worst"], ("G state", k, worst, mean)
    ds = {k: v.detach().cpu() for k, v in model.netD.state_dict().items()}
    worst, mean, k = FX.state_error(ds, fxs["d_state"], FX.bn_shadowed_biases(fxs["d_keys"]), lr_steps=lr_steps)
    assert mean < tol["st_mean"] and worst < tol["st_worst"], ("D state", k, worst, mean)


def test_pix2pix_step_matches_reference_record(fx, tmp_path):
    """Pix2Pix with mixup: true, two steps (cutblur, then blend with its colour drawn on the device in the reference's place), with the
    bounds of tests/test_gpu_i2i.py's step-record test."""
    import test_gpu_i2i as TI
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    fxs = fx["steps"]["pix2pix"]
    yml = T.mixup_yaml(ref_harness.i2i_yaml(name="engine_batchaug_i2i", out_root=str(tmp_path), gpu_ids="[0]", **fxs["spec"]["yaml"]),
                       fxs["mix"])
    opt = options.parse(yml, is_train=True)
    model = create_model(opt, verbose=False)
    for n, sd in FX.i2i_initial_states(fxs).items():
        getattr(model, "net" + n).load_state_dict(sd)
    assert dict(opt["network_G"]) == fxs["network_G"] and dict(opt["network_D"]) == fxs["network_D"]
    assert list(model.model_names) == fxs["model_names"] and model.mixup
    tape = _replay(fxs["calls"])
    augs = []
    with tape.on(EB):
        for (s, (A, B)), ref_log in zip(FX.i2i_batches(fxs), fxs["logs"]):
            model.feed_data({"A": A, "B": B, "A_path": ["a"] * A.shape[0]})
            model.optimize_parameters(s)
            augs.append(model.batchaugment.aug)
            log = model.get_current_log()
            print("\nstep", s, {k: (round(log[k], 7), round(v, 7)) for k, v in ref_log.items()})
            TI.check_logs(log, ref_log, 2e-4 if s < 2 else 3e-3)
            if s == 1:
                diff = (model.fake_B.detach().cpu() - fxs["images_step1"]["fake_B"]).abs()
                assert diff.mean().item() <= 2e-5 and diff.max().item() <= 5e-4, (diff.mean().item(), diff.max().item())
    assert tape.replay == [] and augs == [c["aug"] for c in fxs["calls"]]
    diff = (model.fake_B.detach().cpu() - fxs["images"]["fake_B"]).abs()
    assert diff.mean().item() <= 1e-2 and diff.max().item() <= 1e-1, (diff.mean().item(), diff.max().item())
    lr_steps = 2e-4 * fxs["spec"]["steps"]
    for n in fxs["model_names"]:
        sd = {k: v.detach().cpu() for k, v in getattr(model, "net" + n).state_dict().items()}
        skip = FX.norm_shadowed_biases(fxs["keys"][n], fxs["network_G"]["norm_type"]) if n.startswith("G") else ()
        worst, mean, k = FX.state_error(sd, fxs["states"][n], skip, lr_steps=lr_steps)
        assert mean < 0.15 and worst < 2.05, (n, k, worst, mean)


def _count_ops(monkeypatch, model=None):
    """Records every new op as "mix" / "mask@fwd" / "mask@bwd", and the generator forward of `model` as "forward"."""
    from trainner_amd import ops
    calls, phase = [], ["fwd"]
    real_mix, real_mask = ops.batchaug_mix, ops.batchaug_mask
    monkeypatch.setattr(ops, "batchaug_mix", lambda *a, **k: (calls.append("mix"), real_mix(*a, **k))[1])
    monkeypatch.setattr(ops, "batchaug_mask", lambda *a, **k: (calls.append("mask@" + phase[0]), real_mask(*a, **k))[1])

    def backward(ctx, g, _real=EB._MaskFn.backward):
        phase[0] = "bwd"
        try:
            return _real(ctx, g)
        finally:
            phase[0] = "fwd"
    monkeypatch.setattr(EB._MaskFn, "backward", staticmethod(backward))
    return calls


def _mark_forward(model, calls):
    real = model.forward
    model.forward = lambda *a, **k: (calls.append("forward"), real(*a, **k))[1]


def test_launch_counts_of_a_full_step(fx, tmp_path, monkeypatch):
    """Without mixup none of the new ops runs.  A two-image op is two mix launches before the forward; a miss and `none` launch
    nothing; cutout is one mask launch before the forward, two after it (generated and target) and one in the backward."""
    calls = _count_ops(monkeypatch)
    fxs = fx["steps"]["sr"]
    batches = list(FX.batches(fxs))
    plain = _engine_sr_model(fxs, tmp_path / "plain", name="engine_batchaug_plain")
    assert not plain.mixup and plain.batchaugment is None
    for s, (LR, HR) in batches:
        plain.feed_data({"LR": LR, "HR": HR})
        plain.optimize_parameters(s)
    plain.get_current_log()
    assert calls == []
    model = _engine_sr_model(fxs, tmp_path / "mix", fxs["mix"])
    _mark_forward(model, calls)
    want = {"cutmixup": ["mix", "mix", "forward"], "cutout": ["mask@fwd", "forward", "mask@fwd", "mask@fwd", "mask@bwd"]}
    with _replay(fxs["calls"]).on(EB):
        for (s, (LR, HR)), c in zip(batches, fxs["calls"]):
            del calls[:]
            model.feed_data({"LR": LR, "HR": HR})
            model.optimize_parameters(s)
            assert calls == want[c["aug"]], (c["aug"], calls)
    for opt in (dict(mixopts=["none"], mixprob=[1.0], mixalpha=[1.0]), dict(mixopts=["cutmix"], mixprob=[0.0], mixalpha=[0.7])):
        model.batchaugment = EB.BatchAugment(opt)
        del calls[:]
        LR, HR = batches[0][1]
        model.feed_data({"LR": LR, "HR": HR})
        model.optimize_parameters(3)
        assert calls == ["forward"], (opt, calls)
    log = model.get_current_log()
    assert all(v == v and abs(v) != float("inf") for v in log.values()), log


def mixup_recipe_edit(tree):
    """The shipped recipe with its commented batch-augmentation block switched on, nothing else changed."""
    tree["train"].update(MIXUP_BLOCK)


def test_shipped_recipe_with_mixup_steps_under_amp(tmp_path, monkeypatch):
    """The shipped SR recipe (RRDBNet-23, batch 8, crop 128, use_amp: true) with the mixup block uncommented parses, constructs and
    steps; every log entry is finite."""
    import test_gpu_step as TS
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml, _ = TS.shipped_recipe(tmp_path, monkeypatch)
    assert FX.write_recipe("sr/train_sr.yml", str(tmp_path), mixup_recipe_edit) == yml
    opt = options.parse(yml, is_train=True)
    assert opt["use_amp"] is True and opt["train"]["mixup"] is True
    torch.manual_seed(opt["train"]["manual_seed"])
    model = create_model(opt, verbose=False)
    assert model.mixup and list(model.batchaugment.mixopts) == MIXUP_BLOCK["mixopts"]
    calls = _count_ops(monkeypatch)
    ds = opt["datasets"]["train"]
    T.seed_all(11)
    LR, HR = detrand.synthetic_pair(ds["batch_size"], ds["crop_size"], 501)
    model.feed_data({"LR": LR, "HR": HR})
    model.optimize_parameters(1)
    log = model.get_current_log()
    assert set(log) >= {"pix-l1", "fea-vgg19-l1", "l_g_gan", "l_d_real", "l_d_fake"}
    assert all(v == v and abs(v) != float("inf") for v in log.values()), log
    assert model.batchaugment.aug in MIXUP_BLOCK["mixopts"] and calls == ["mix"] * 2          # every recipe op hits: two launches


@pytest.mark.parametrize("recipe", ["i2i/train_pix2pix.yml", "i2i/train_cyclegan.yml"])
def test_shipped_i2i_recipes_construct_with_mixup(recipe, tmp_path):
    """options/i2i/train_pix2pix.yml and train_cyclegan.yml with the block uncommented parse and construct."""
    import test_gpu_i2i as TI
    opt, model, _ = TI._shipped_i2i_recipe(tmp_path, recipe, mixup_recipe_edit)
    assert opt["train"]["mixup"] is True
    assert model.mixup and list(model.batchaugment.mixopts) == MIXUP_BLOCK["mixopts"]
