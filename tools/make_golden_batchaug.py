"""tests/golden/batchaug.pt from the REFERENCE's own batch augmentations (codes/dataops/batchaug.py), run on the CPU where the reference
tree exists (never on a GPU machine):

    python tools/make_golden_batchaug.py

Per case (CASES) and parameter set (sets_for) the real `BatchAug` runs in fp32 on a seeded (target, input) pair, followed by the
reference's `apply_mask` on a second seeded pair.  A `Tape` stands between the module and its generators (`np.random.choice / uniform /
beta / randn / randint / random / permutation`, `random.random`, `torch.randperm`, the tensor `uniform_`): it records every draw in
call order and can force single draws.  The reference's `np.int` no longer exists in numpy 2; this tool installs `np.int = int`
before it imports the reference.

`restate` is our own fp32 restatement in plain torch on the CPU, from an explicit parameter record
(trainner_amd.dataops.batchaug.Params): every output element is a copy, or fl(fl(v) * x) + fl(fl(1 - v) * y) with both products rounded
to fp32 before the sum.  The tool asserts torch.equal(restatement, reference) -- bit-identity, NaN positions included -- for every set
before it writes the file.  Stored per set: the tape, the parameter record's key, a SHA-256 of each output's bytes and a few probed
values; the tests rebuild the full tensors with `restate` where the reference does not exist.
"""
import contextlib
import hashlib
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import detrand  # noqa: E402
from oracle import ref_harness as R  # noqa: E402
from trainner_amd.dataops import batchaug as EB  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "batchaug.pt")
# (target shape, input shape).  tiles: the kernels' workgroup spans 64 threads x 4 floats = 256 floats of a row and 4 x 4 = 16 rows;
# the input has 264 columns and 20 rows (more than one workgroup in both directions, in either layout), the target twice that
CASES = {"sr4": ((5, 3, 48, 48), (5, 3, 12, 12)), "sr4odd": ((3, 3, 52, 44), (3, 3, 13, 11)), "sr2": ((3, 3, 36, 36), (3, 3, 18, 18)),
         "i2i": ((4, 3, 40, 56), (4, 3, 40, 56)), "gray": ((2, 1, 36, 36), (2, 1, 18, 18)),
         "tiles": ((2, 3, 40, 528), (2, 3, 20, 264)), "special": ((3, 3, 24, 32), (3, 3, 12, 16))}
RECIPE_OPTS = ["blend", "rgb", "mixup", "cutmix", "cutmixup"]
RECIPE_PROB = [1.0, 1.0, 1.0, 1.0, 1.0]
RECIPE_ALPHA = [0.6, 1.0, 1.2, 0.7, 0.7]
ALPHA = dict(zip(RECIPE_OPTS, RECIPE_ALPHA), cutout=0.001, cutblur=0.7, none=1.0)          # the recipe's mixalpha per op
AUX_PROB, AUX_ALPHA = 1.0, 1.2
X_SEED = 5200
PROBES = 24


def make_pair(case, which=0):
    """The seeded (target, input) pair of a case; which = 1: the (generated, target) pair `apply_mask` gets."""
    s1, s2 = CASES[case]
    k = X_SEED + 10 * sorted(CASES).index(case) + 4 * which
    a = detrand.uniform(s1, k, -0.1, 1.1).float().contiguous()
    b = detrand.uniform(s2 if which == 0 else s1, k + 1, -0.1, 1.1).float().contiguous()
    if case == "special" and which == 0:
        for t, sc in ((a, 2), (b, 1)):          # hand-placed special values, at the same places of both resolutions
            t[0, 0, 0, 0] = -0.0
            t[1, 1, 2 * sc, 3 * sc] = float("inf")
            t[2, 2, 5 * sc, 7 * sc] = float("nan")
            t[0, 1, 6 * sc, 1 * sc] = float("-inf")
            t[1, 0, 11 * sc, 15 * sc] = -0.0
    return a, b


def ops_of(case):
    (_, C, H, _), (_, _, h, _) = CASES[case]
    names = ["none", "rgb", "mixup", "cutmix", "cutmixup", "cutout"]
    if C == 3:
        names.insert(1, "blend")
    if H == h:
        names.append("cutblur")
    return names


def one(op, alpha=None, prob=1.0, aux_prob=AUX_PROB, aux_alpha=AUX_ALPHA):
    return dict(options=[op], probs=[prob], alphas=[ALPHA[op] if alpha is None else alpha], aux_prob=aux_prob, aux_alpha=aux_alpha)


def sets_for(case):
    """-> {set name: (call options, forced draws per kind, seed)}.  Forced draws are consumed in call order per kind; every other draw
    comes from the generators seeded with `seed`."""
    (N, C, H, W), (_, _, h, w) = CASES[case]
    base = 1000 * (1 + sorted(CASES).index(case))
    sets = {}
    for i, op in enumerate(ops_of(case)):
        sets["op-" + op] = (one(op), {}, base + i)
        sets["miss-" + op] = (one(op, prob=0.0), {}, base + 20 + i)
    if C == 3:
        for i in range(3):
            sets["recipe-%d" % i] = (dict(options=RECIPE_OPTS, probs=RECIPE_PROB, alphas=RECIPE_ALPHA, aux_prob=AUX_PROB,
                                          aux_alpha=AUX_ALPHA), {}, base + 40 + i)
    # boxes (cutmix; `randn` forced to 0 makes the ratio alpha itself)
    ch, cw = int(h * 0.7), int(w * 0.7)
    sets["box-first"] = (one("cutmix"), {"randn": [0.0], "randint": [0, 0]}, base + 50)
    sets["box-last"] = (one("cutmix"), {"randn": [0.0], "randint": [h - ch, w - cw]}, base + 51)
    sets["box-empty"] = (one("cutmix", alpha=0.5 / max(h, w)), {"randn": [0.0]}, base + 52)
    short = (max(h, w) - 0.5) / max(h, w)
    assert int(h * short) == h - 1 and int(w * short) == w - 1 and short < 1
    sets["box-short"] = (one("cutmix", alpha=short), {"randn": [0.0], "randint": [1, 0]}, base + 53)
    odd = (w // 2) | 1          # an odd box width with room for x0 = 1, 2, 3
    a_odd = (odd + 0.5) / w
    assert int(w * a_odd) == odd and odd + 3 <= w
    for x0 in (1, 2, 3):
        sets["box-x%d" % x0] = (one("cutmix", alpha=a_odd), {"randn": [0.0], "randint": [1, x0]}, base + 54 + x0)
    # blend factors at both ends and the middle
    ident, derange = list(range(N)), [(i + 1) % N for i in range(N)]
    for tag, v in (("lo", 1e-6), ("half", 0.5), ("hi", 1 - 1e-6)):
        sets["mixup-" + tag] = (one("mixup"), {"beta": [v]}, base + 60)
        sets["cutmixup-v-" + tag] = (one("cutmixup"), {"beta": [v], "random": [0.9]}, base + 61)
        if C == 3:
            sets["blend-" + tag] = (one("blend"), {"uniform": [v]}, base + 62)
    sets["perm-identity"] = (one("mixup"), {"randperm": [ident]}, base + 63)
    sets["perm-derangement"] = (one("mixup"), {"randperm": [derange]}, base + 64)
    sets["cutmix-derangement"] = (one("cutmix"), {"randperm": [derange]}, base + 65)
    # cutmixup: both coins x the auxiliary mixup's hit and miss (aux_prob 0.5: random.random() 0.1 hits, 0.9 misses)
    for coin, cv in (("in", 0.9), ("out", 0.1)):
        for aux, av in (("hit", 0.1), ("miss", 0.9)):
            sets["cutmixup-%s-%s" % (coin, aux)] = (one("cutmixup", aux_prob=0.5), {"random": [cv], "pyrandom": [0.0, av],
                                                                                      "randperm": [derange]}, base + 66)
    if H == h:
        sets["cutblur-in"] = (one("cutblur"), {"random": [0.9]}, base + 70)
        sets["cutblur-out"] = (one("cutblur"), {"random": [0.1]}, base + 71)
    sets["cutout-half"] = (one("cutout", alpha=0.5), {}, base + 72)
    sets["cutout-recipe"] = (one("cutout"), {}, base + 73)
    sets["cutout-miss"] = (one("cutout", prob=0.0), {}, base + 74)
    return sets


# ------------------------------------------------------------------------------------------------ the draws
class _Proxy:
    def __init__(self, base, **over):
        self._base, self._over = base, over

    def __getattr__(self, k):
        over = object.__getattribute__(self, "_over")
        return over[k] if k in over else getattr(object.__getattribute__(self, "_base"), k)


class _Empty:
    """What the taped `torch.empty` returns: only `uniform_` is ever called on it."""

    def __init__(self, tape, size, device):
        self.tape, self.size, self.device = tape, tuple(size), device

    def uniform_(self, a, b):
        v = self.tape._next("uniform_", lambda: torch.empty(self.size).uniform_(a, b).flatten(),
                            lambda f: torch.tensor(f, dtype=torch.float32).flatten())
        return v.clone().reshape(self.size).to(self.device)


class Tape:
    """Stands between a batchaug module (the reference's or the engine's: both name their generators torch / np / random) and the
    generators.  `force`: per kind, the values handed out first, in call order; `replay`: a full log to hand out, checked kind by
    kind.  `log` collects every draw as (kind, value)."""

    def __init__(self, force=None, replay=None):
        self.log = []
        self.force = {k: list(v) for k, v in (force or {}).items()}
        self.replay = None if replay is None else list(replay)

    def _next(self, kind, real, convert=lambda v: v):
        if self.replay is not None:
            assert self.replay, "the module asks for a '%s' draw, the replayed tape is empty" % kind
            k, v = self.replay.pop(0)
            assert k == kind, "the replayed tape has a '%s' draw where the module asks for '%s'" % (k, kind)
        elif self.force.get(kind):
            v = convert(self.force[kind].pop(0))
        else:
            v = real()
        self.log.append((kind, v))
        return v

    def _choice(self, a, size=None, p=None):
        if size is None:
            return self._next("choice", lambda: int(np.random.choice(a, p=p)), int)
        v = self._next("choice_mask", lambda: np.random.choice(a, size=size, p=p).astype(np.uint8))          # kept as uint8
        return v.astype(np.float64).reshape(size)

    def _randint(self, low, high=None):
        v = self._next("randint", lambda: int(np.random.randint(low, high)), int)
        assert low <= v < high, (low, v, high)
        return v

    def _randperm(self, n):
        v = self._next("randperm", lambda: [int(i) for i in torch.randperm(n)], list)
        assert sorted(v) == list(range(n))
        return torch.tensor(v, dtype=torch.int64)

    @contextlib.contextmanager
    def on(self, mod):
        old = mod.torch, mod.np, mod.random
        nr = _Proxy(np.random, choice=self._choice, randint=self._randint,
                    uniform=lambda a, b: self._next("uniform", lambda: float(np.random.uniform(a, b)), float),
                    beta=lambda a, b: self._next("beta", lambda: float(np.random.beta(a, b)), float),
                    randn=lambda: self._next("randn", lambda: float(np.random.randn()), float),
                    random=lambda: self._next("random", lambda: float(np.random.random()), float),
                    permutation=lambda n: np.asarray(self._next("permutation", lambda: [int(i) for i in np.random.permutation(n)], list)))
        mod.torch = _Proxy(torch, randperm=self._randperm, empty=lambda size, device=None: _Empty(self, size, device))
        mod.np = _Proxy(np, random=nr)
        mod.random = _Proxy(random, random=lambda: self._next("pyrandom", random.random, float))
        try:
            yield self
        finally:
            mod.torch, mod.np, mod.random = old


def seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def params_from_tape(call, tape, shape1, shape2, device="cpu"):
    """The engine's own `draw`, fed the recorded draws in its call order (which must be the reference's: the tape ends up empty)."""
    t = Tape(replay=tape)
    with t.on(EB):
        prm = EB.draw(call["options"], call["probs"], call["alphas"], call["aux_prob"], call["aux_alpha"], call.get("mix_p"),
                      tuple(shape1), tuple(shape2), device)
    assert not t.replay, "the engine's draw consumed fewer draws than the reference: %r left" % (t.replay,)
    return prm


# ------------------------------------------------------------------------------------------------ restatement
def _lerp(a, x, b, y):
    """fl(fl(a) x) + fl(fl(b) y): two fp32 products, each rounded, then one fp32 sum."""
    return torch.tensor(a, dtype=torch.float32) * x + torch.tensor(b, dtype=torch.float32) * y


def _inside(box, s, H, W, device="cpu"):
    y0, x0, bh, bw = (v * s for v in box)
    m = torch.zeros(H, W, dtype=torch.bool, device=device)
    m[y0:y0 + bh, x0:x0 + bw] = True
    return m


def up_mask(mask, s):
    """uint8 N x h x w -> N x 1 x (s h) x (s w), nearest."""
    m = torch.as_tensor(mask).reshape(mask.shape[0], 1, mask.shape[-2], mask.shape[-1])
    return m.repeat_interleave(s, 2).repeat_interleave(s, 3)


def restate_mask(x, mask, s):
    return x * up_mask(mask, s).to(x.device).to(torch.float32)


def restate(prm, img1, img2):
    """(img1_aug, img2_aug) of a parameter record on fp32 tensors (on the CPU, or wherever they live: tools/bench_batchaug.py times
    this on the device as "plain torch"), by the rule of the module's docstring."""
    if not prm.hit:
        return img1, img2
    aug, s = prm.aug, prm.scale
    if aug == "cutout":
        return img1, restate_mask(img2, prm.mask, 1)
    if aug == "rgb":
        p = list(prm.perm)
        return img1[:, p].contiguous(), img2[:, p].contiguous()
    if aug == "blend":
        c = torch.as_tensor(prm.colour).reshape(prm.N, 3, 1, 1).float().to(img1.device)
        return tuple(_lerp(prm.v, t, 1.0 - prm.v, c.expand_as(t)) for t in (img1, img2))
    if aug == "cutblur":
        m = _inside(prm.box, 1, prm.h, prm.w, img1.device)
        return img1, (torch.where(m, img1, img2) if prm.coin else torch.where(m, img2, img1))
    out = []
    for t, sc in ((img1, s), (img2, 1)):
        partner = t[prm.r]
        if aug == "mixup":
            out.append(_lerp(prm.v, t, 1.0 - prm.v, partner))
            continue
        m = _inside(prm.box, sc, prm.h * sc, prm.w * sc, t.device)
        if aug == "cutmix":
            out.append(torch.where(m, partner, t))
        else:
            mixed = _lerp(prm.v, t, 1.0 - prm.v, partner) if prm.aux_hit else partner
            out.append(torch.where(m, mixed, t) if prm.coin else torch.where(m, t, mixed))
    return out[0], out[1]


def bits_equal(a, b):
    """Bit-identity that also holds NaNs to their positions: equal bits where neither is NaN, NaN in both or in neither."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != torch.float32:
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    ai, bi = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(na, nb) and torch.equal(ai[~na], bi[~nb]))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def probe(t, k=PROBES):
    flat = t.detach().cpu().contiguous().view(torch.int32).flatten()          # bits, so NaNs compare
    idx = torch.linspace(0, flat.numel() - 1, k).long()
    return idx.tolist(), flat[idx].tolist()          # (plain lists: a pickled tensor costs more than its 24 values)


# ------------------------------------------------------------------------------------------------ the reference
def _reference_module():
    np.int = int          # numpy 2 dropped the alias the reference still writes
    with R.reference_env():
        for k in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data", "cv2", "torchvision")]:
            del sys.modules[k]
        import dataops.batchaug as BA
    return BA


def reference_run(BA, call, img1, img2, gen, tgt, tape):
    """BatchAug on (img1, img2), then the reference's apply_mask on (gen, tgt) -> (o1, o2, mask or None, aug, m1, m2)."""
    with tape.on(BA):
        o1, o2, mask, aug = BA.BatchAug(img1, img2, call["options"], call["probs"], call["alphas"], call["aux_prob"], call["aux_alpha"],
                                        call.get("mix_p"))
    ba = BA.BatchAugment({})
    ba.mask, ba.aug = mask, aug
    m1, m2 = ba.apply_mask(gen, tgt)
    return o1, o2, mask, aug, m1, m2


def run_cases(BA):
    cases = {}
    for case, (s1, s2) in CASES.items():
        img1, img2 = make_pair(case)
        gen, tgt = make_pair(case, 1)
        rec = {"shapes": (s1, s2), "x1": probe(img1), "x2": probe(img2), "sets": {}}
        for name, (call, force, seed) in sets_for(case).items():
            seed_all(seed)
            tape = Tape(force=force)
            o1, o2, mask, aug, m1, m2 = reference_run(BA, call, img1, img2, gen, tgt, tape)
            prm = params_from_tape(call, tape.log, s1, s2)
            assert prm.aug == aug
            r1, r2 = restate(prm, img1, img2)
            assert bits_equal(r1, o1) and bits_equal(r2, o2), ("the restatement is not bit-equal to the reference", case, name)
            if aug == "cutout":
                assert torch.equal(up_mask(prm.mask, prm.scale).float(), mask), (case, name)
                q1, q2 = restate_mask(gen, prm.mask, prm.scale), restate_mask(tgt, prm.mask, prm.scale)
            else:
                assert mask is None
                q1, q2 = gen, tgt
            assert bits_equal(q1, m1) and bits_equal(q2, m2), ("apply_mask", case, name)
            rec["sets"][name] = {"call": call, "seed": seed, "forced": bool(force), "tape": tape.log, "key": prm.key(), "aug": aug,
                                 "hit": prm.hit, "sha": {"img1": sha(o1), "img2": sha(o2), "gen": sha(m1), "tgt": sha(m2)},
                                 "probes": {"img1": probe(o1), "img2": probe(o2)}}
            print("%-8s %-22s %-9s hit %d box %s v %s" % (case, name, aug, prm.hit, prm.box, prm.v))
        cases[case] = rec
    return cases


# ------------------------------------------------------------------------------------------------ step records
STEP_YAML = dict(nb=1, batch=2, crop=64, d_nf=16)          # the small configuration of the other step records
STEP_SEED, STEP_K, DRAW_SEED = 381, 2, 983
SR_MIX = dict(mixopts=RECIPE_OPTS + ["cutout"], mixprob=RECIPE_PROB + [1.0], mixalpha=RECIPE_ALPHA + [0.3], aux_mixprob=1.0,
              aux_mixalpha=1.2)
SR_FORCED = ["cutmixup", "cutout"]          # step 1, step 2: the mask's backward reaches the generator's gradient in step 2
I2I_SPEC = dict(yaml=dict(model="pix2pix", batch=2, crop=64, n_blocks=2, ngf=16, ndf=16, pixel_weight=100.0, gan_form="standard"),
                steps=2, seed=93)
I2I_MIX = dict(mixopts=RECIPE_OPTS + ["cutblur"], mixprob=RECIPE_PROB + [1.0], mixalpha=RECIPE_ALPHA + [0.7], aux_mixprob=1.0,
               aux_mixalpha=1.2)
I2I_FORCED = ["cutblur", "blend"]


def mixup_yaml(path, mix):
    """Add `mixup: true` and the block's other keys to the train block of a yaml written by oracle.ref_harness.esrgan_yaml / i2i_yaml."""
    with open(path) as fh:
        txt = fh.read()
    assert txt.count("\nlogger:") == 1
    lines = "\n  mixup: true" + "".join("\n  %s: %s" % (k, v) for k, v in mix.items())
    with open(path, "w") as fh:
        fh.write(txt.replace("\nlogger:", lines + "\nlogger:"))
    return path


def call_of(mix):
    return dict(options=mix["mixopts"], probs=mix["mixprob"], alphas=mix["mixalpha"], aux_prob=mix["aux_mixprob"],
                aux_alpha=mix["aux_mixalpha"])


@contextlib.contextmanager
def recorded_calls(mix, forced):
    """Every BatchAug call of the reference model, in order, with the op draw forced: {"shapes", "tape"}."""
    BA = sys.modules["dataops.batchaug"]
    tape = Tape(force={"choice": [mix["mixopts"].index(f) for f in forced]})
    real, calls = BA.BatchAug, []

    def wrapped(img1, img2, *a, **k):
        start = len(tape.log)
        out = real(img1, img2, *a, **k)
        calls.append({"shapes": (tuple(img1.shape), tuple(img2.shape)), "tape": tape.log[start:], "aug": out[3]})
        return out

    BA.BatchAug = wrapped
    try:
        with tape.on(BA):
            yield calls
    finally:
        BA.BatchAug = real


def sr_step_record():
    from oracle.make_golden import D_SEED, F_SEED, G_SEED, probe_state
    yml = mixup_yaml(R.esrgan_yaml(name="golden_batchaug_sr", **STEP_YAML), SR_MIX)
    opt, model = R.build_reference_model(yml, seed=0)
    assert model.mixup and model.batchaugment.mixopts == SR_MIX["mixopts"]
    names = [l["name"] for l in model.generatorlosses.loss_list]
    detrand.fill_state_dict_(model.netG.state_dict(), G_SEED)
    detrand.fill_state_dict_(model.netD.state_dict(), D_SEED)
    netF = R.reference_netF(model)
    detrand.fill_state_dict_({k: v for k, v in netF.state_dict().items() if k.startswith("feature_net")}, F_SEED, gain=1.0, bias_amp=0.05)
    logs = []
    seed_all(DRAW_SEED)
    with recorded_calls(SR_MIX, SR_FORCED) as calls:
        for s in range(1, STEP_K + 1):
            LR, HR = detrand.synthetic_pair(STEP_YAML["batch"], STEP_YAML["crop"], STEP_SEED + s)
            logs.append(R.reference_step(model, LR, HR, s))
    assert [c["aug"] for c in calls] == SR_FORCED, calls
    print("step sr", [{k: round(v, 6) for k, v in l.items()} for l in logs])
    return {"name": "batchaug_step_sr", "spec": {"yaml": dict(STEP_YAML), "steps": STEP_K, "seed": STEP_SEED}, "mix": SR_MIX,
            "loss_names": names, "calls": calls, "network_G": dict(opt["network_G"]), "network_D": dict(opt["network_D"]),
            "seeds": {"G": G_SEED, "D": D_SEED, "F": F_SEED, "data": STEP_SEED, "draws": DRAW_SEED},
            "logs": logs, "fake_H": model.fake_H.detach().clone(),
            "g_state": probe_state(model.netG.state_dict()), "d_state": probe_state(model.netD.state_dict()),
            "g_keys": [(k, tuple(v.shape)) for k, v in model.netG.state_dict().items()],
            "d_keys": [(k, tuple(v.shape)) for k, v in model.netD.state_dict().items()], "torch": torch.__version__}


def i2i_step_record():
    from oracle.make_golden import probe_state
    from oracle.make_golden_i2i import POOL_SEED, SEEDS, ab_pair
    spec = I2I_SPEC
    yml = mixup_yaml(R.i2i_yaml(name="golden_batchaug_pix2pix", **spec["yaml"]), I2I_MIX)
    opt, model = R.build_reference_model(yml, seed=0)
    assert model.mixup and model.batchaugment.mixopts == I2I_MIX["mixopts"]
    names = list(model.model_names)
    for n in names:
        detrand.fill_state_dict_(getattr(model, "net" + n).state_dict(), SEEDS[n])
    batch, crop = spec["yaml"]["batch"], spec["yaml"]["crop"]
    logs = []
    seed_all(DRAW_SEED)
    random.seed(POOL_SEED)
    with R.reference_env(), recorded_calls(I2I_MIX, I2I_FORCED) as calls:
        for s in range(1, spec["steps"] + 1):
            A, B = ab_pair(batch, crop, spec["seed"] + s)
            model.feed_data({"A": A, "B": B, "A_path": ["a"] * batch})
            model.optimize_parameters(s)
            logs.append(dict(model.get_current_log()))
            if s == 1:
                imgs1 = {"fake_B": model.fake_B.detach().clone()}
    assert [c["aug"] for c in calls] == I2I_FORCED, calls
    print("step pix2pix", [{k: round(v, 6) for k, v in l.items()} for l in logs])
    return {"name": "batchaug_step_pix2pix", "spec": spec, "mix": I2I_MIX, "calls": calls, "network_G": dict(opt["network_G"]),
            "network_D": dict(opt["network_D"]), "seeds": dict(SEEDS, data=spec["seed"], pool=POOL_SEED, draws=DRAW_SEED),
            "model_names": names, "logs": logs, "images": {"fake_B": model.fake_B.detach().clone()}, "images_step1": imgs1,
            "states": {n: probe_state(getattr(model, "net" + n).state_dict()) for n in names},
            "keys": {n: [(k, tuple(v.shape)) for k, v in getattr(model, "net" + n).state_dict().items()] for n in names},
            "torch": torch.__version__}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    BA = _reference_module()
    fx = {"cases": run_cases(BA), "recipe": {"options": RECIPE_OPTS, "probs": RECIPE_PROB, "alphas": RECIPE_ALPHA}, "torch": torch.__version__,
          "steps": {"sr": sr_step_record(), "pix2pix": i2i_step_record()}}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(fx, OUT)
    size = os.path.getsize(OUT)
    assert size < 1 << 20, size
    print("->", OUT, "%.1f KB" % (size / 1024))


if __name__ == "__main__":
    main()
