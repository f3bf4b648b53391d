"""tests/golden/optimizers.pt from the REFERENCE's own optimiser factory (codes/models/optimizers.py config_optimizer: torch.optim.SGD /
RMSprop and its SGDP, AdamP, Ranger, MADGRAD classes) -- run on the CPU where the reference tree exists (never on a GPU machine):

    python tools/make_golden_optimizers.py

Every case of tests/optim_restate.py CONFIGS takes STEPS planted steps over its tensor set (SHAPES; inputs and gradients are pure
functions of seeds: make_params, planted_grads).  Recorded at steps CHECK, per case: probes of the reference's fp64 parameters and state
(per tensor: 16 evenly spaced elements, the sum and max |.|), the reference's OWN fp32 deviation from its fp64 run per tensor (e32, the
yardstick of the GPU tests) with the fp64 scale (max |.|), the projection decisions and margins of every tensor and step, and the key
lists of state_dict().  Ranger computes in fp32 whatever it is given (`p.data.float()`), so for it the recorded values are the fp64
restatement's and the yardstick is the restatement's fp32 run against its fp64 run.

Asserted before the file is written:
  * restatement == reference: to 1e-12 of the tensor's scale in fp64; bit-equal in fp32 for Ranger
  * every planted decision of adamp / sgdp has its margin r outside [1/3, 3] at every step of the fp64 run, and is the planted one
  * Ranger passes through the unrectified and the rectified branch (the switch falls between steps 5 and 6) and through a lookahead
    step with k 3 and with the default 6
  * every yardstick is non-zero
  * restatement == reference in the same way for every option case of optim_restate.OPTION_CASES (Nesterov and no weight decay for
    AdamP / SGDP, MADGRAD without momentum and with the 'Adam' decay, Ranger without gradient centralisation and with gc_conv_only,
    SGD without momentum); nothing of these is stored
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

from oracle import ref_harness as R  # noqa: E402
import optim_restate as X  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "optimizers.pt")
NPROBE = 16


def probe(t):
    """[NPROBE + 2] fp64: evenly spaced elements (repeating when the tensor is smaller), the sum, max |.|."""
    f = t.detach().double().reshape(-1)
    idx = torch.linspace(0, f.numel() - 1, NPROBE).round().long()
    return torch.cat([f[idx], f.sum().reshape(1), f.abs().max().reshape(1)])


def probes(ts):
    return torch.stack([probe(t) for t in ts])


def _reference_module():
    with R.reference_env():
        for m in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data", "cv2", "torchvision")]:
            del sys.modules[m]
        import models.optimizers as RO
    return RO


def reference_optimizer(RO, case, params, hp=None):
    hp = X.CONFIGS[case] if hp is None else hp
    opt = X.train_opt(hp)
    opt["optim_G"] = X.rule_of(case)
    if opt["optim_G"] == "rmsprop":
        assert opt.pop("alpha_G") == 0.99          # torch.optim.RMSprop's default; the reference passes none (alpha_G is Ranger's)
    with R.reference_env():
        return RO.config_optimizer(opt, "G", optim_params=params)


def reference_run(RO, case, dtype, grads, hp=None, keys=None):
    """-> ({step: (params, [state])}, optimizer) with the reference's own class stepping `grads` ([step][tensor], fp32)."""
    ps = [torch.nn.Parameter(p.to(dtype)) for p in X.make_params()]
    o = reference_optimizer(RO, case, ps, hp)
    keys = X.STATE_KEYS[X.rule_of(case)] if keys is None else keys
    rec = {}
    for s in range(1, X.STEPS + 1):
        for p, g in zip(ps, grads[s - 1]):
            p.grad = g.to(dtype).clone()           # (the reference centralises / decays some gradients in place)
        o.step()
        if s in X.CHECK:
            rec[s] = ([p.detach().clone() for p in ps], [{k: o.state[p][k].detach().clone() for k in keys} for p in ps])
    return rec, o


def check_decisions(case, decisions):
    for s, dec in enumerate(decisions, 1):
        for ti, (mode, margins) in enumerate(dec):
            if len(X.SHAPES[ti]) < 2:
                assert mode == 0 and margins == [], (case, s, ti)
                continue
            kind = X.plant_kind(ti, s)
            assert mode == {0: 1, 1: 2, 2: 0}[kind], (case, s, ti, kind, mode, margins)
            assert all(r < 1 / 3 or r > 3 for r in margins), (case, s, ti, margins)


def check_option_cases(RO):
    """restatement == reference for the options the recorded runs do not take (X.OPTION_CASES): asserted, nothing stored."""
    for case in X.OPTION_CASES:
        rule, hp = X.rule_of(case), X.hp_of(case)
        dtype = torch.float32 if rule == "ranger" else torch.float64
        _, grads, decisions = X.trajectory(case, dtype=torch.float64)
        got = X.trajectory(case, dtype=dtype, grads64=grads)[0]
        keys = tuple(got[X.CHECK[0]][1][0].keys())
        ref, _ = reference_run(RO, case, dtype, grads, hp, keys)
        worst = 0.0
        for s in X.CHECK:
            for ti in range(len(X.SHAPES)):
                for a, b in [(ref[s][0][ti], got[s][0][ti])] + [(ref[s][1][ti][k], got[s][1][ti][k]) for k in keys]:
                    if rule == "ranger":
                        assert torch.equal(a, b), (case, s, ti)
                    else:
                        d = float((a - b).abs().max()) / max(float(a.abs().max()), 1e-30)
                        worst = max(worst, d)
                        assert d <= 1e-12, (case, s, ti, d)
        if rule in ("adamp", "sgdp"):
            check_decisions(case, decisions)
        print("%-30s restatement == reference (%s)" % (case, "bit-equal fp32" if rule == "ranger" else "fp64, worst %.1e of scale" % worst))


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    RO = _reference_module()
    check_option_cases(RO)
    fx = {"cases": {}, "torch": torch.__version__, "shapes": X.SHAPES, "check": X.CHECK, "nprobe": NPROBE}
    for case, hp in X.CONFIGS.items():
        rule = X.rule_of(case)
        keys = X.STATE_KEYS[rule]
        r64, grads, decisions = X.trajectory(case, dtype=torch.float64)
        r32, _, dec32 = X.trajectory(case, dtype=torch.float32, grads64=grads)
        if rule == "ranger":
            ref32, o = reference_run(RO, case, torch.float32, grads)
            for s in X.CHECK:
                for ti in range(len(X.SHAPES)):
                    assert torch.equal(ref32[s][0][ti], r32[s][0][ti]), (case, s, ti)
                    for k in keys:
                        assert torch.equal(ref32[s][1][ti][k], r32[s][1][ti][k]), (case, s, ti, k)
            want, yard = r64, r32
            flags = [X.ranger_scalars(t, *hp["betas"], hp["N_sma_threshhold"])[0] for t in range(1, X.STEPS + 1)]
            assert flags == [False] * 5 + [True] * 3, flags
            assert any(t % hp["k"] == 0 for t in range(1, X.STEPS + 1))
        else:
            ref64, o = reference_run(RO, case, torch.float64, grads)
            ref32, _ = reference_run(RO, case, torch.float32, grads)
            for s in X.CHECK:
                for ti in range(len(X.SHAPES)):
                    pairs = [(ref64[s][0][ti], r64[s][0][ti])] + [(ref64[s][1][ti][k], r64[s][1][ti][k]) for k in keys]
                    for a, b in pairs:
                        assert float((a - b).abs().max()) <= 1e-12 * max(float(a.abs().max()), 1e-30), (case, s, ti, float((a - b).abs().max()))
            want, yard = ref64, ref32
        if rule in ("adamp", "sgdp"):
            check_decisions(case, decisions)
            assert [[m for m, _ in d] for d in dec32] == [[m for m, _ in d] for d in decisions], case
        sd = o.state_dict()
        rec = {"hp": dict(hp), "state_keys": sorted(sd["state"][0].keys()), "group_keys": sorted(k for k in sd["param_groups"][0] if k != "params"),
               "top_keys": sorted(k for k in sd["state"] if not isinstance(k, int)),
               "decisions": [[(m, [float(r) for r in mg]) for m, mg in d] for d in decisions], "steps": {}}
        for s in X.CHECK:
            st = {"p": probes(want[s][0]),
                  "e32_p": torch.tensor([float((a.double() - b.double()).abs().max()) for a, b in zip(yard[s][0], want[s][0])]),
                  "scale_p": torch.tensor([float(b.double().abs().max()) for b in want[s][0]])}
            for k in keys:
                st[k] = probes([d[k] for d in want[s][1]])
                st["e32_" + k] = torch.tensor([float((a[k].double() - b[k].double()).abs().max()) for a, b in zip(yard[s][1], want[s][1])])
                st["scale_" + k] = torch.tensor([float(b[k].double().abs().max()) for b in want[s][1]])
            assert float(st["e32_p"].max()) > 0 and all(float(st["e32_" + k].max()) > 0 for k in keys if k not in X.PARAM_COPIES), (case, s)
            rec["steps"][s] = st
            print("%-10s step %d  e32_p max %.2e of scale %.2e" % (case, s, float(st["e32_p"].max()), float(st["scale_p"].max())),
                  " ".join("%s %.2e" % (k, float(st["e32_" + k].max())) for k in keys))
        fx["cases"][case] = rec
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(fx, OUT)
    print("->", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
