"""tests/golden/diffaug.pt from the REFERENCE's own DiffAugment (codes/dataops/diffaug.py), run on the CPU where the reference tree
exists (never on a GPU machine):

    python tools/make_golden_diffaug.py

Per case (CASES) and parameter set (sets_for) the real reference functions run in fp32 and in fp64 with the SAME draws: a `Tape`
stands between the module and its generators (`torch.rand`, `torch.randint`, `np.random.uniform`, `np.random.random`,
`random.choice`), records every draw of the fp32 run and feeds it to the fp64 run.  Seeded sets draw from the seeded generators;
hand-set extremes force single draws (translation at +-max, cutout boxes clipped at the corners, zoom scales at both ends with the crop /
displacement at both ends, flip, both rotations, each `transl_zoom` choice).  The fixture holds per set

    tape                  every draw in call order: what the tests replay through the ENGINE's `draw` (same Tape, same call order)
    out, grad             probes of the fp64 output and of the fp64 gradient of sum(out * m), m a seeded map in [-1, 1)
    e32_out, e32_grad     max |fp32 run - fp64 run| of the reference itself: the yardsticks of the GPU tests
    out_absmax, grad_absmax

`restate` is our own fp64 restatement of the composite  out = cutout_mask . Geo(Colour(x))  from an explicit parameter record
(trainner_amd.dataops.diffaug.Params); the tool asserts restate == reference to 1e-12 (output and gradient) before it writes the
file, so the tests can compare the engine with `restate`'s full tensors where the reference does not exist.
"""
import contextlib
import os
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import detrand  # noqa: E402
from oracle import ref_harness as R  # noqa: E402
from tools.make_golden_ssim import probe, probe_error  # noqa: E402,F401
from trainner_amd.dataops import diffaug as ED  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "diffaug.pt")
CASES = {"sq32": (3, 3, 32, 32), "odd33": (2, 3, 33, 33), "rect40x56": (2, 3, 40, 56), "gray36": (2, 1, 36, 36),
         "tiles": (2, 3, 70, 70)}          # tiles: larger than the kernels' 64 x 4 and 16 x 16 thread grids in both directions
RECIPE = "color,transl_zoom,flip,rotate,cutout"
SINGLE = ("color", "translation", "zoom", "transl_zoom", "flip", "rotate", "cutout")
MAP_SEED, X_SEED = 6161, 4100


def make_input(case):
    shape = CASES[case]
    return detrand.uniform(shape, X_SEED + sorted(CASES).index(case), -0.1, 1.1).float().contiguous()


def seeded_map(shape, seed=MAP_SEED):
    return detrand.uniform(shape, seed, -1.0, 1.0).float()


def policy_for(case, policy):
    """rect40x56 takes the policies without `rotate` (H != W)."""
    _, _, H, W = CASES[case]
    if H == W:
        return policy
    return ",".join(p for p in policy.split(",") if p != "rotate")


def sets_for(case):
    """-> {set name: (policy, forced draws per kind, seed or None)}.  Forced draws are consumed in call order per kind; every other
    draw comes from the generators seeded with `seed`."""
    N, _, H, W = CASES[case]
    square = H == W
    sets = {}
    base = 100 * (1 + sorted(CASES).index(case))
    for i, p in enumerate(SINGLE):
        if p == "rotate" and not square:
            continue
        sets["seeded-" + p] = (p, {}, base + i)
    sets["seeded-recipe"] = (policy_for(case, RECIPE), {}, base + 20)
    sets["seeded-default"] = ("color,translation,cutout", {}, base + 21)
    # translation at +-max on both axes
    my, mx = int(H * 0.125 + 0.5), int(W * 0.125 + 0.5)
    sy, sx = [1, -1, 1][:N], [1, -1, -1][:N]
    sets["transl-max"] = ("translation", {"randint": [[my * s for s in sy], [mx * s for s in sx]]}, base + 30)
    sets["transl-max-b"] = ("translation", {"randint": [[-my * s for s in sy], [mx * s for s in sy]]}, base + 31)
    # cutout boxes clipped at each corner
    ch, cw = ED.cutout_size(H, W)
    hy, hx = H + (1 - ch % 2) - 1, W + (1 - cw % 2) - 1
    sets["cutout-corners-a"] = ("cutout", {"randint": [[0, hy, 0][:N], [0, hx, hx][:N]]}, base + 32)
    sets["cutout-corners-b"] = ("cutout", {"randint": [[hy, 0, hy][:N], [0, hx, hx][:N]]}, base + 33)
    # zoom_in: scale just under 2 and just over 1, the crop at both ends
    for tag, scale in (("hi", 1.999), ("lo", 1.001)):
        for end, r in (("first", 0.0), ("last", 0.999999)):
            sets["zoomin-%s-%s" % (tag, end)] = ("zoom", {"choice": [0], "uniform": [scale], "random": [r, r]}, base + 34)
    # zoom_out: scale 0.1 and 1.0, the displacement at +-max
    for tag, scale in (("lo", 0.1), ("hi", 1.0)):
        for end, r in (("neg", -1.0), ("pos", 1.0)):
            sets["zoomout-%s-%s" % (tag, end)] = ("zoom", {"choice": [1], "uniform": [scale, r]}, base + 35)
    sets["flip-on"] = ("flip", {"random": [0.9]}, base + 36)
    sets["flip-off"] = ("flip", {"random": [0.1]}, base + 37)
    if square:
        sets["rotate-plus"] = ("rotate", {"random": [0.1]}, base + 38)
        sets["rotate-minus"] = ("rotate", {"random": [0.9, 0.1]}, base + 39)
        sets["rotate-none"] = ("rotate", {"random": [0.9, 0.9]}, base + 40)
    # each transl_zoom choice inside the recipe, with the flip and both rotations
    rot = (lambda *r: list(r)) if square else (lambda *r: [])
    sets["recipe-translation"] = (policy_for(case, RECIPE), {"choice": [0], "random": [0.9] + rot(0.1)}, base + 41)
    sets["recipe-zoom_in"] = (policy_for(case, RECIPE), {"choice": [1], "random": [0.3, 0.7, 0.9] + rot(0.9, 0.1)}, base + 42)
    sets["recipe-zoom_out"] = (policy_for(case, RECIPE), {"choice": [2], "random": [0.1] + rot(0.1)}, base + 43)
    return sets


# ------------------------------------------------------------------------------------------------ the draws
class _Proxy:
    def __init__(self, base, **over):
        self._base, self._over = base, over

    def __getattr__(self, k):
        over = object.__getattribute__(self, "_over")
        return over[k] if k in over else getattr(object.__getattribute__(self, "_base"), k)


class Tape:
    """Stands between a DiffAugment module (the reference's or the engine's: both name their generators torch / np / random) and the
    generators.  `force`: per kind, the values handed out first, in call order; `replay`: a full log to hand out, checked kind by kind.
    `log` collects every draw as (kind, value)."""

    def __init__(self, force=None, replay=None):
        self.log = []
        self.force = {k: list(v) for k, v in (force or {}).items()}
        self.replay = None if replay is None else list(replay)

    def _next(self, kind, real, convert):
        if self.replay is not None:
            k, v = self.replay.pop(0)
            assert k == kind, "the replayed tape has a '%s' draw where the module asks for '%s'" % (k, kind)
        elif self.force.get(kind):
            v = convert(self.force[kind].pop(0))
        else:
            v = real()
        self.log.append((kind, v))
        return v

    def _rand(self, *size, dtype=None, device=None):
        v = self._next("rand", lambda: torch.rand(*size, dtype=torch.float32).double().flatten(),
                       lambda f: torch.tensor(f, dtype=torch.float64).flatten())
        # fp64 values are handed out as they are (an fp32 consumer rounds them itself)
        return v.reshape(*size).to(dtype if dtype == torch.float32 and self.replay is None else torch.float64).to(device)

    def _randint(self, low, high, size=None, device=None):
        v = self._next("randint", lambda: torch.randint(low, high, size=size).flatten(),
                       lambda f: torch.tensor(f, dtype=torch.int64).flatten())
        assert int(v.min()) >= low and int(v.max()) < high
        return v.reshape(size).to(device)

    def _uniform(self, a, b):
        return self._next("uniform", lambda: np.random.uniform(a, b), float)

    def _random(self):
        return self._next("random", lambda: np.random.random(), float)

    def _choice(self, seq):
        return seq[self._next("choice", lambda: random.choice(range(len(seq))), int)]

    @contextlib.contextmanager
    def on(self, mod):
        old = mod.torch, mod.np, mod.random
        mod.torch = _Proxy(torch, rand=self._rand, randint=self._randint)
        mod.np = _Proxy(np, random=_Proxy(np.random, uniform=self._uniform, random=self._random))
        mod.random = _Proxy(random, choice=self._choice)
        try:
            yield self
        finally:
            mod.torch, mod.np, mod.random = old


def seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def params_from_tape(policy, tape, shape):
    """The engine's own `draw`, fed the recorded draws in its call order (which is the reference's): colour factors stay fp64."""
    N, _, H, W = shape
    t = Tape(replay=tape)
    with t.on(ED):
        prm = ED.draw(policy, N, H, W, "cpu")
    assert not t.replay, "the engine's draw consumed fewer draws than the reference: %r left" % (t.replay,)
    return prm


# ------------------------------------------------------------------------------------------------ restatement
def _axis_taps(kind, out, zoom_in, zoom_out, shift, N, dtype, dev="cpu"):
    """Per output coordinate of one axis: (i0, i1, w0, w1), indices [N, out] in image coordinates (outside [0, out) = reads 0) and
    weights [out]; w is None for the copy kinds (one tap, no product)."""
    d = torch.arange(out, device=dev)
    if kind == "identity":
        return d.expand(N, out), None, None, None
    if kind == "translation":
        return d[None, :] + shift.to(dev).reshape(N, 1).long(), None, None, None
    if kind == "zoom_in":
        off, size = zoom_in
    else:
        off, size = zoom_out
    scale = torch.tensor(size, dtype=dtype, device=dev) / torch.tensor(out, dtype=dtype, device=dev)
    src = (scale * (d.to(dtype) + 0.5) - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=size - 1)
    l1 = (src - i0.to(dtype)).clamp(0, 1)
    i1 = (i0 + 1).clamp(max=size - 1)
    return (i0 + off).expand(N, out), (i1 + off).expand(N, out), 1 - l1, l1


def _take(sp, iy, ix):
    """sp: the image with a one-pixel zero frame; iy [N, H'], ix [N, W'] image coordinates (anything outside reads the frame)."""
    N, C, Hp, Wp = sp.shape
    iy = (iy + 1).clamp(0, Hp - 1)
    ix = (ix + 1).clamp(0, Wp - 1)
    n = torch.arange(N, device=sp.device)[:, None, None, None]
    c = torch.arange(C, device=sp.device)[None, :, None, None]
    return sp[n, c, iy[:, None, :, None], ix[:, None, None, :]]


def cutout_mask(prm, dtype=torch.float64, dev="cpu"):
    """[N, H, W]: 0 inside the box of (round(H/2), round(W/2)) whose first row / column is offset - size // 2, both ends clamped into
    the image (a box that leaves the image still zeroes the border row / column its clamped indices land on)."""
    H, W = prm.H, prm.W
    ch, cw = ED.cutout_size(H, W)
    oy, ox = (t.to(dev).long().reshape(-1, 1) for t in prm.cutout)
    ys, xs = torch.arange(H, device=dev)[None, :], torch.arange(W, device=dev)[None, :]
    iny = (ys >= (oy - ch // 2).clamp(0, H - 1)) & (ys <= (oy + ch - 1 - ch // 2).clamp(0, H - 1))
    inx = (xs >= (ox - cw // 2).clamp(0, W - 1)) & (xs <= (ox + cw - 1 - cw // 2).clamp(0, W - 1))
    return 1 - (iny[:, :, None] & inx[:, None, :]).to(dtype)


def restate(x, prm):
    """out = cutout_mask . Geo(Colour(x)) in x's dtype with plain differentiable torch operations, on x's device."""
    N, C, H, W = x.shape
    dt, dev = x.dtype, x.device
    s = x
    if prm.color is not None:
        b, sat, con = (t.to(dev).to(dt).reshape(N, 1, 1, 1) for t in prm.color)
        s = x + b
        mc = s.mean(dim=1, keepdim=True)
        s = (s - mc) * sat + mc
        m = x.mean(dim=(1, 2, 3), keepdim=True) + b
        s = (s - m) * con + m
    if prm.kind != "identity":
        zi_y = zi_x = zo_y = zo_x = ty = tx = None
        if prm.kind == "translation":
            ty, tx = prm.translation
        elif prm.kind == "zoom_in":
            h_delta, w_delta, new_h, new_w = prm.zoom
            zi_y, zi_x = (h_delta, new_h), (w_delta, new_w)
        else:
            left, right, top, bottom = prm.zoom
            zo_y, zo_x = (-top, H + top + bottom), (-left, W + left + right)
        y0, y1, wy0, wy1 = _axis_taps(prm.kind, H, zi_y, zo_y, ty, N, dt, dev)
        x0, x1, wx0, wx1 = _axis_taps(prm.kind, W, zi_x, zo_x, tx, N, dt, dev)
        sp = F.pad(s, (1, 1, 1, 1))
        if wy0 is None:
            s = _take(sp, y0, x0)
        else:
            wy0, wy1 = wy0.reshape(1, 1, H, 1), wy1.reshape(1, 1, H, 1)
            wx0, wx1 = wx0.reshape(1, 1, 1, W), wx1.reshape(1, 1, 1, W)
            s = wy0 * (wx0 * _take(sp, y0, x0) + wx1 * _take(sp, y0, x1)) + wy1 * (wx0 * _take(sp, y1, x0) + wx1 * _take(sp, y1, x1))
    if prm.flip:
        s = s.flip(-1)
    if prm.rot:
        s = torch.rot90(s, prm.rot, dims=(2, 3))
    if prm.cutout is not None:
        s = s * cutout_mask(prm, dt, dev).unsqueeze(1)
    return s


def restate_with_grad(x, prm, m, dtype=torch.float64):
    x = x.detach().to(dtype).contiguous().requires_grad_(True)
    out = restate(x, prm)
    (out * m.to(dtype)).sum().backward()
    return out.detach(), x.grad.detach()


# ------------------------------------------------------------------------------------------------ the reference
def _reference_module():
    with R.reference_env():
        for k in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data", "cv2", "torchvision")]:
            del sys.modules[k]
        import dataops.diffaug as DA
    return DA


def reference_run(DA, policy, x, m, dtype, tape):
    x = x.detach().to(dtype).contiguous().requires_grad_(True)
    with tape.on(DA):
        out = DA.DiffAugment(x, policy=policy)
    (out * m.to(dtype)).sum().backward()
    return out.detach(), x.grad.detach()


def run_cases(DA):
    cases = {}
    for case, shape in CASES.items():
        x = make_input(case)
        m = seeded_map(shape)
        rec = {"shape": shape, "x": probe(x), "m": probe(m), "sets": {}}
        for name, (policy, force, seed) in sets_for(case).items():
            seed_all(seed)
            t32 = Tape(force=force)
            o32, g32 = reference_run(DA, policy, x, m, torch.float32, t32)
            t64 = Tape(replay=t32.log)
            o64, g64 = reference_run(DA, policy, x, m, torch.float64, t64)
            assert not t64.replay
            prm = params_from_tape(policy, t32.log, shape)
            ro, rg = restate_with_grad(x, prm, m)
            assert (ro - o64).abs().max().item() <= 1e-12, (case, name, (ro - o64).abs().max().item())
            assert (rg - g64).abs().max().item() <= 1e-12, (case, name, (rg - g64).abs().max().item())
            t = {"policy": policy, "seed": seed, "forced": bool(force), "tape": t32.log, "kind": prm.kind, "flip": prm.flip,
                 "rot": prm.rot, "zoom": prm.zoom, "out": probe(o64), "grad": probe(g64),
                 "out_absmax": o64.abs().max().item(), "grad_absmax": g64.abs().max().item(),
                 "e32_out": (o32.double() - o64).abs().max().item(), "e32_grad": (g32.double() - g64).abs().max().item()}
            rec["sets"][name] = t
            print("%-10s %-20s %-38s %-11s flip %d rot %2d e32_out %.2e e32_grad %.2e max|o| %.3f max|g| %.3f" % (
                case, name, policy, prm.kind, prm.flip, prm.rot, t["e32_out"], t["e32_grad"], t["out_absmax"], t["grad_absmax"]))
        cases[case] = rec
    return cases


# ------------------------------------------------------------------------------------------------ step records
STEP_YAML = dict(nb=1, batch=2, crop=64, d_nf=16)          # the small configuration of the frequency-separation step records
STEP_SEED, STEP_K, DRAW_SEED = 371, 2, 977
I2I_SPEC = dict(yaml=dict(model="pix2pix", batch=2, crop=64, n_blocks=2, ngf=16, ndf=16, pixel_weight=100.0, gan_form="standard"),
                steps=2, seed=91)


def diffaug_yaml(path, policy=RECIPE):
    """Add `diffaug: true` and `dapolicy` to the train block of a yaml written by oracle.ref_harness.esrgan_yaml / i2i_yaml."""
    with open(path) as fh:
        txt = fh.read()
    assert txt.count("\nlogger:") == 1
    lines = "\n  diffaug: true\n  dapolicy: '%s'" % policy
    with open(path, "w") as fh:
        fh.write(txt.replace("\nlogger:", lines + "\nlogger:"))
    return path


@contextlib.contextmanager
def recorded_calls():
    """Every DiffAugment call of the reference's Adversarial, in order: {"shape", "policy", "tape"} (the reference's models must be
    imported already)."""
    losses_mod, DA = sys.modules["models.losses"], sys.modules["dataops.diffaug"]
    real, tape, calls = losses_mod.DiffAugment, Tape(), []

    def wrapped(x, policy="", channels_first=True):
        start = len(tape.log)
        out = real(x, policy=policy, channels_first=channels_first)
        calls.append({"shape": tuple(x.shape), "policy": policy, "requires_grad": bool(x.requires_grad), "tape": tape.log[start:]})
        return out

    losses_mod.DiffAugment = wrapped
    try:
        with tape.on(DA):
            yield calls
    finally:
        losses_mod.DiffAugment = real


def sr_step_record():
    from oracle.make_golden import D_SEED, F_SEED, G_SEED, probe_state
    yml = diffaug_yaml(R.esrgan_yaml(name="golden_diffaug_sr", **STEP_YAML))
    opt, model = R.build_reference_model(yml, seed=0)
    assert model.adversarial.diffaug and model.adversarial.dapolicy == RECIPE
    names = [l["name"] for l in model.generatorlosses.loss_list]
    detrand.fill_state_dict_(model.netG.state_dict(), G_SEED)
    detrand.fill_state_dict_(model.netD.state_dict(), D_SEED)
    netF = R.reference_netF(model)
    detrand.fill_state_dict_({k: v for k, v in netF.state_dict().items() if k.startswith("feature_net")}, F_SEED, gain=1.0, bias_amp=0.05)
    logs = []
    seed_all(DRAW_SEED)
    with recorded_calls() as calls:
        for s in range(1, STEP_K + 1):
            LR, HR = detrand.synthetic_pair(STEP_YAML["batch"], STEP_YAML["crop"], STEP_SEED + s)
            logs.append(R.reference_step(model, LR, HR, s))
    assert len(calls) == 4 * STEP_K, len(calls)
    print("step sr", [{k: round(v, 6) for k, v in l.items()} for l in logs], [params_from_tape(c["policy"], c["tape"], c["shape"]).kind for c in calls])
    return {"name": "diffaug_step_sr", "spec": {"yaml": dict(STEP_YAML), "steps": STEP_K, "seed": STEP_SEED}, "policy": RECIPE,
            "loss_names": names, "calls": calls, "network_G": dict(opt["network_G"]), "network_D": dict(opt["network_D"]),
            "seeds": {"G": G_SEED, "D": D_SEED, "F": F_SEED, "data": STEP_SEED, "draws": DRAW_SEED},
            "logs": logs, "fake_H": model.fake_H.detach().clone(),
            "g_state": probe_state(model.netG.state_dict()), "d_state": probe_state(model.netD.state_dict()),
            "g_keys": [(k, tuple(v.shape)) for k, v in model.netG.state_dict().items()],
            "d_keys": [(k, tuple(v.shape)) for k, v in model.netD.state_dict().items()], "torch": torch.__version__}


def i2i_step_record():
    """The layout of oracle/make_golden_i2i.run_case's records, with diffaug: true (the conditional case: the augmentation comes
    before the concatenation, the condition is not augmented)."""
    from oracle.make_golden import probe_state
    from oracle.make_golden_i2i import POOL_SEED, SEEDS, ab_pair
    spec = I2I_SPEC
    yml = diffaug_yaml(R.i2i_yaml(name="golden_diffaug_pix2pix", **spec["yaml"]))
    opt, model = R.build_reference_model(yml, seed=0)
    assert model.adversarial.diffaug and model.adversarial.dapolicy == RECIPE
    names = list(model.model_names)
    for n in names:
        detrand.fill_state_dict_(getattr(model, "net" + n).state_dict(), SEEDS[n])
    batch, crop = spec["yaml"]["batch"], spec["yaml"]["crop"]
    logs = []
    seed_all(DRAW_SEED)
    random.seed(POOL_SEED)
    with R.reference_env(), recorded_calls() as calls:
        for s in range(1, spec["steps"] + 1):
            A, B = ab_pair(batch, crop, spec["seed"] + s)
            model.feed_data({"A": A, "B": B, "A_path": ["a"] * batch})
            model.optimize_parameters(s)
            logs.append(dict(model.get_current_log()))
            if s == 1:
                imgs1 = {"fake_B": model.fake_B.detach().clone()}
    print("step pix2pix", [{k: round(v, 6) for k, v in l.items()} for l in logs], len(calls), "calls",
          [params_from_tape(c["policy"], c["tape"], c["shape"]).kind for c in calls])
    return {"name": "diffaug_step_pix2pix", "spec": spec, "policy": RECIPE, "calls": calls, "network_G": dict(opt["network_G"]),
            "network_D": dict(opt["network_D"]), "seeds": dict(SEEDS, data=spec["seed"], pool=POOL_SEED, draws=DRAW_SEED),
            "model_names": names, "logs": logs, "images": {"fake_B": model.fake_B.detach().clone()}, "images_step1": imgs1,
            "states": {n: probe_state(getattr(model, "net" + n).state_dict()) for n in names},
            "keys": {n: [(k, tuple(v.shape)) for k, v in getattr(model, "net" + n).state_dict().items()] for n in names},
            "torch": torch.__version__}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    DA = _reference_module()
    fx = {"cases": run_cases(DA), "recipe": RECIPE, "torch": torch.__version__,
          "steps": {"sr": sr_step_record(), "pix2pix": i2i_step_record()}}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(fx, OUT)
    size = os.path.getsize(OUT)
    assert size < 1 << 20, size
    print("->", OUT, "%.1f KB" % (size / 1024))


if __name__ == "__main__":
    main()
