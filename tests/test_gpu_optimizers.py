"""The optimisers beside Adam on the device (csrc/optimizers.hip): sgd, rmsprop, madgrad, adamp, sgdp, ranger.

Kernel level.  The tensor set of optim_restate.SHAPES lives in ONE flat buffer (every tensor 256-byte aligned) with its segment table
and takes the 8 planted steps of tests/golden/optimizers.pt.  After steps 1, 5, 6 and 8 the parameters and every state buffer are
compared, per tensor and with no element skipped (the planted margins make every projection decision the same on both sides), with the
fp64 restatement (checked against the reference's own classes by the golden tool and tests/test_cpu_optimizers.py) under the project's
rule for kernels without a derived bound (test_gpu_membound_kernels.yardstick): device error <= 2 x the fp32 reference's own error +
2e-7 x scale.  The fp32 figure is the golden's (the reference's own fp32 run) for the recorded configurations, the fp32 restatement's
for the option cases, which the golden does not hold.  State that is a pure copy compares with torch.equal (x0; slow_buffer between
lookahead steps).  The alignment gaps of every buffer are pre-filled with a sentinel and must keep its bits.

Step level.  Three small SR configurations ((adamp, sgdp), (ranger, madgrad), (sgd, rmsprop)), three steps each: a step pre-hook clones
each network's flat parameters, gradients and state, and the engine's parameters after the step are compared with the fp64 restatement
applied to those inputs under the same yardstick -- the wiring of the real networks' segment tables (BN vectors, Linear layers,
3-channel rows), independent of a reference trajectory.  The real gradients are not planted: a tensor whose fp64 margin lies in
[1/2, 2] may match the restatement under either decision; every tensor is compared."""
import os

import pytest
import torch

import optim_restate as X
import test_gpu_step as TS
from oracle import detrand, fixtures as FX, ref_harness

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -123.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPTION_CASES = X.OPTION_CASES


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


# What one yardstick comparison covers: every tensor of at least 256 elements on its own; the five smaller ones ([1], [64], [5,1],
# [1,100], [8,3,3,3]; all of the same +-0.1 start scale) together.  The yardstick is a MAXIMUM of rounding errors accumulated over up to
# 8 steps: over one or five elements that maximum is one draw, and two correct fp32 evaluations differ by more than a factor of two in
# it as often as not ([1] alone: MADGRAD's `s` after 8 steps, device 1.9e-10 against the reference's 4.4e-11 at scale 3.8e-4, 0.5 ulp
# against 0.1 ulp).  No element is left out.  A per-tensor comparison of the five with an absolute floor was tried and
# dropped: a floor in units of the RESULT's scale has no footing where the update cancels against the parameter (MADGRAD without momentum,
# step 1, the [1] tensor: p = x0 - s / rms leaves 5.4e-3 of operands near 0.1; device 5.0e-9, the fp32 restatement 1.3e-9, both under one
# ulp of the operands), and a floor in units of the operands is a second rule beside the project's one.
def groups_of(shapes):
    return [("small", [ti for ti, s in enumerate(shapes) if _numel(s) < 256])] + \
           [("x".join(map(str, s)), [ti]) for ti, s in enumerate(shapes) if _numel(s) >= 256]


GROUPS, WRAP_GROUPS = groups_of(X.SHAPES), groups_of(X.WRAP_SHAPES)


hp_of = X.hp_of

_REF = {}


SETS = {"main": (X.SHAPES, X.STEPS, X.CHECK), "wrap": (X.WRAP_SHAPES, X.WRAP_STEPS, X.WRAP_CHECK)}


def reference(case, which="main"):
    """(fp64 records, gradients, e32, state keys) of `case` over the tensor set `which`, computed once and shared, left unchanged.
    e32[step][key][tensor]: the fp32 figure -- the golden's for the recorded runs over the main set, else the fp32 restatement's."""
    if (case, which) not in _REF:
        hp = hp_of(case)
        shapes, steps, check = SETS[which]
        kw = dict(shapes=shapes, steps=steps, check=check)
        rec, grads, _ = X.trajectory(case, hp=hp, dtype=torch.float64, **kw)
        keys = tuple(rec[check[0]][1][0].keys())
        if case in OPTION_CASES or which != "main":
            r32, _, _ = X.trajectory(case, hp=hp, dtype=torch.float32, grads64=grads, **kw)
            e32 = {s: dict([("p", [float((a.double() - b).abs().max()) for a, b in zip(r32[s][0], rec[s][0])])] +
                           [(k, [float((a[k].double() - b[k]).abs().max()) for a, b in zip(r32[s][1], rec[s][1])]) for k in keys])
                   for s in check}
        else:
            g = torch.load(os.path.join(ROOT, "tests", "golden", "optimizers.pt"), weights_only=False)["cases"][case]["steps"]
            e32 = {s: {k: g[s]["e32_" + k].tolist() for k in ("p",) + keys} for s in check}
        _REF[(case, which)] = (rec, grads, e32, keys)
    return _REF[(case, which)]


def _ops():
    from trainner_amd import ops
    return ops


def flat_of(tensors, entries, total):
    buf = torch.full((total,), SENT, dtype=torch.float32)
    for v, t in zip(X.views(buf, entries), tensors):
        v.copy_(t)
    return buf.to(DEV)


def gaps_intact(buf, entries):
    mask = torch.ones(buf.numel(), dtype=torch.bool)
    for v in X.views(mask, entries):
        v.fill_(False)
    got = buf.cpu()[mask]
    return torch.equal(got, torch.full_like(got, SENT))


def device_step(rule, hp, table, p, g, st, t):
    ops = _ops()
    if rule == "sgd":
        ops.sgd_step(p, g, st.get("momentum_buffer"), table, hp["lr"], hp["momentum"], hp["weight_decay"])
    elif rule == "rmsprop":
        ops.rmsprop_step(p, g, st["square_avg"], table, hp["lr"], hp["alpha"], hp["eps"], hp["weight_decay"])
    elif rule == "madgrad":
        ops.madgrad_step(p, g, st["grad_sum_sq"], st["s"], st.get("x0"), table, hp["lr"], hp["eps"], t - 1, hp["momentum"], hp["weight_decay"],
                         hp["decay_type"])
    elif rule == "adamp":
        ops.adamp_step(p, g, st["exp_avg"], st["exp_avg_sq"], table, hp["lr"], *hp["betas"], hp["eps"], t, hp["nesterov"], hp["delta"],
                       hp["wd_ratio"], hp["weight_decay"])
    elif rule == "sgdp":
        ops.sgdp_step(p, g, st["momentum"], table, hp["lr"], hp["momentum"], hp["dampening"], hp["eps"], hp["nesterov"], hp["delta"],
                      hp["wd_ratio"], hp["weight_decay"])
    elif rule == "ranger":
        ops.ranger_step(p, g, st["exp_avg"], st["exp_avg_sq"], st["slow_buffer"], table, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"],
                        t, hp["k"], hp["alpha"], hp["N_sma_threshhold"], hp["use_gc"], hp["gc_conv_only"])
    else:
        raise KeyError(rule)


def device_run(case, check=None, steps=None, which="main"):
    """-> ({step: {'p': flat, key: flat}} (device clones), entries, final buffers, table)"""
    from trainner_amd.flat import SegTable
    rule, hp = X.rule_of(case), hp_of(case)
    shapes, steps_, check_ = SETS[which]
    steps, check = steps or steps_, check or check_
    rec, grads, _, keys = reference(case, which)
    entries, total = X.layout(shapes)
    table = SegTable(entries, DEV)
    params = X.make_params(shapes)
    p = flat_of(params, entries, total)
    st = {k: flat_of(params if k in X.PARAM_COPIES else [torch.zeros_like(q) for q in params], entries, total) for k in keys}
    out = {}
    for s in range(1, steps + 1):
        g = flat_of(grads[s - 1], entries, total)
        device_step(rule, hp, table, p, g, st, s)
        if s in check:
            out[s] = dict([("p", p.clone())] + [(k, v.clone()) for k, v in st.items()])
    torch.cuda.synchronize()
    return out, entries, dict([("p", p)] + list(st.items())), table


def yardstick(what, got, ref64, e32):
    """err(device) <= 2 x err(fp32 reference) + 2e-7 x scale, both against fp64; prints the figures.  -> device / bound"""
    scale = float(ref64.abs().max())
    e_dev = float((got.double().cpu() - ref64).abs().max())
    bound = 2.0 * e32 + 2e-7 * scale
    ratio = e_dev / bound if bound else (0.0 if e_dev == 0 else float("inf"))
    print("YARDSTICK %-44s dev %.3e  fp32 %.3e  scale %.3e  dev/bound %.3f" % (what, e_dev, e32, scale, ratio))
    assert e_dev <= bound, (what, e_dev, e32, scale)
    return ratio


@pytest.mark.parametrize("case", list(X.CONFIGS) + list(OPTION_CASES))
def test_kernels_follow_the_fp64_restatement(case):
    rec, _, e32, keys = reference(case)
    out, entries, final, _ = device_run(case)
    hp = hp_of(case)
    init = X.make_params()
    worst = 0.0
    for s in X.CHECK:
        for key in ("p",) + keys:
            got = X.views(out[s][key], entries)
            for name, tis in GROUPS:
                want = [rec[s][0][ti] if key == "p" else rec[s][1][ti][key] for ti in tis]
                worst = max(worst, yardstick("%s step %d %s %s" % (case, s, key, name), torch.cat([got[ti].reshape(-1) for ti in tis]),
                                             torch.cat([w.reshape(-1) for w in want]), max(e32[s][key][ti] for ti in tis)))
        if "x0" in keys:
            for ti, v in enumerate(X.views(out[s]["x0"], entries)):
                assert torch.equal(v.cpu(), init[ti]), (s, ti)
        if "slow_buffer" in keys:
            last = max([t for t in X.CHECK if t <= s and t % hp["k"] == 0], default=None)       # slow moves on lookahead steps only
            moved = any(t % hp["k"] == 0 for t in range(1, s + 1))
            for ti, v in enumerate(X.views(out[s]["slow_buffer"], entries)):
                if not moved:
                    assert torch.equal(v.cpu(), init[ti]), (s, ti)
                elif last is not None and not any(t % hp["k"] == 0 for t in range(last + 1, s + 1)):
                    assert torch.equal(v, X.views(out[last]["slow_buffer"], entries)[ti]), (s, last, ti)
    for key, buf in final.items():
        assert gaps_intact(buf, entries), key
    print("WORST dev/bound %-30s %.3f" % (case, worst))


@pytest.mark.parametrize("rule", X.NAMES)
def test_second_grid_stride_pass(rule):
    """The tensor set of optim_restate.WRAP_SHAPES: more chunks than the chunk launches' block cap and more rows than four times the row
    launches' (asserted on the table), so every kernel's blocks loop a second time, into other tensors than their first pass saw.
    Three steps (the third is Ranger's lookahead step), the same yardstick and grouping, the same gap check."""
    rec, _, e32, keys = reference(rule, "wrap")
    out, entries, final, table = device_run(rule, which="wrap")
    assert table.nchunks > 2048 and table.nrows > 4 * 2048, (table.nchunks, table.nrows)
    assert int(table.chunks[2048, 2]) == 1 and int(table.rowseg[8192]) == 0 and int(table.rowseg[-1]) == 3
    worst = 0.0
    for s in X.WRAP_CHECK:
        for key in ("p",) + keys:
            got = X.views(out[s][key], entries)
            for name, tis in WRAP_GROUPS:
                want = [rec[s][0][ti] if key == "p" else rec[s][1][ti][key] for ti in tis]
                worst = max(worst, yardstick("wrap %s step %d %s %s" % (rule, s, key, name), torch.cat([got[ti].reshape(-1) for ti in tis]),
                                             torch.cat([w.reshape(-1) for w in want]), max(e32[s][key][ti] for ti in tis)))
    for key, buf in final.items():
        assert gaps_intact(buf, entries), key
    print("WORST dev/bound wrap %-25s %.3f" % (rule, worst))


@pytest.mark.parametrize("rule", X.NAMES)
def test_fault_latch_blocks_every_optimizer(rule):
    """With the latch word set, parameters and state keep their bits; cleared again, the same launch moves them."""
    from trainner_amd.flat import SegTable
    ops = _ops()
    hp = hp_of(rule)
    _, grads, _, keys = reference(rule)
    entries, total = X.layout()
    table = SegTable(entries, DEV)
    params = X.make_params()
    p = flat_of(params, entries, total)
    g = flat_of(grads[0], entries, total)
    st = {k: flat_of([torch.full_like(q, 0.25) for q in params], entries, total) for k in keys}
    before = dict([("p", p.clone())] + [(k, v.clone()) for k, v in st.items()])
    word = ops.fault_word(p.device)
    try:
        word.fill_(1)
        device_step(rule, hp, table, p, g, st, 3)           # step 3: a lookahead step of the recorded Ranger configuration
        torch.cuda.synchronize()
        for k, v in dict([("p", p)] + list(st.items())).items():
            assert torch.equal(v, before[k]), k
    finally:
        word.zero_()
    device_step(rule, hp, table, p, g, st, 3)
    assert not torch.equal(p, before["p"])
    for k in keys:
        if k != "x0":
            assert not torch.equal(st[k], before[k]), k


def test_steps_are_bit_reproducible():
    for case in ("adamp", "sgdp", "ranger"):
        a = device_run(case, check=(X.STEPS,))[0]
        b = device_run(case, check=(X.STEPS,))[0]
        for k in a[X.STEPS]:
            assert torch.equal(a[X.STEPS][k], b[X.STEPS][k]), (case, k)


# ------------------------------------------------------------------------------------------------ step level
KW = dict(nb=1, batch=2, crop=64, d_nf=16)
RULE_OF_CLASS = {"FusedSGD": "sgd", "FusedRMSprop": "rmsprop", "FusedMADGRAD": "madgrad", "FusedAdamP": "adamp", "FusedSGDP": "sgdp",
                 "FusedRanger": "ranger"}


def optim_yaml(tmp_path, optim_g, optim_d, resume=None):
    yml = ref_harness.esrgan_yaml(name="engine_case", out_root=str(tmp_path), gpu_ids="[0]", **KW)
    txt = open(yml).read()
    assert txt.count("  optim_G: adam") == 1 and txt.count("  optim_D: adam") == 1
    txt = txt.replace("  optim_G: adam", "  optim_G: " + optim_g).replace("  optim_D: adam", "  optim_D: " + optim_d)
    if resume:
        txt = txt.replace("path:\n", "path:\n  resume_state: %s\n" % resume, 1)
    with open(yml, "w") as fh:
        fh.write(txt)
    return yml


def build_model(tmp_path, optim_g, optim_d):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    opt = options.parse(optim_yaml(tmp_path, optim_g, optim_d), is_train=True)
    m = create_model(opt, verbose=False)
    g = detrand.fill_state_dict_({k: v.detach().cpu().clone() for k, v in m.netG.state_dict().items()}, 101)
    d = detrand.fill_state_dict_({k: v.detach().cpu().clone() for k, v in m.netD.state_dict().items()}, 202)
    TS.load_initial(m, g, d, FX.vgg_state(77))
    return opt, m


def hp_of_optimizer(o):
    hp = {k: v for k, v in o.param_groups[0].items() if k != "params"}
    for k in ("use_gc", "gc_conv_only", "decay_type"):
        if hasattr(o, k):
            hp[k] = getattr(o, k)
    if hasattr(o, "N_sma_threshhold"):
        hp["N_sma_threshhold"], hp["alpha"] = o.N_sma_threshhold, o.alpha
    return hp


def capture(o, store):
    """Step pre-hook: the flat parameters, gradients and state of each network the optimiser is about to step."""
    def hook(optim, args, kwargs):
        group = optim.param_groups[0]
        optim._ensure_state(group)
        snap = []
        for holder in optim._holders(group):
            snap.append(dict(holder=holder, entries=holder.seg_table().entries, p=holder.flat.cpu().clone(), g=holder.grad.cpu().clone(),
                             state=[b.cpu().clone() for b in optim._moments[id(holder)]], keys=optim._state_keys(group),
                             t=optim._t.get(0, 0) + 1))
        store[:] = snap
    o.register_step_pre_hook(hook)


def restated_step(rule, hp, snap, dtype, flip=False):
    """-> ([parameters after the step], [(mode, margins)]) of the restatement applied to the captured inputs."""
    out, decisions = [], []
    ps, gs = X.views(snap["p"], snap["entries"]), X.views(snap["g"], snap["entries"])
    sts = [X.views(b, snap["entries"]) for b in snap["state"]]
    for ti, (p, g) in enumerate(zip(ps, gs)):
        q = p.to(dtype).clone()
        st = {k: sts[i][ti].to(dtype).clone() for i, k in enumerate(snap["keys"])}
        decisions.append(X.rule_step(rule, q, g.clone(), st, dict(hp, flip=flip), snap["t"]))
        out.append(q)
    return out, decisions


def check_step(o, snaps, tag, fired):
    rule, hp = RULE_OF_CLASS[type(o).__name__], hp_of_optimizer(o)
    worst = 0.0
    for snap in snaps:
        want, decisions = restated_step(rule, hp, snap, torch.float64)
        f32, _ = restated_step(rule, hp, snap, torch.float32)
        got = X.views(snap["holder"].flat.cpu(), snap["entries"])
        alt = None
        for ti, (w, (mode, margins)) in enumerate(zip(want, decisions)):
            scale = float(w.abs().max())
            e32 = float((f32[ti].double() - w).abs().max())
            bound = 2.0 * e32 + 2e-7 * scale
            e_dev = float((got[ti].double() - w).abs().max())
            close = any(0.5 <= r <= 2 for r in margins)
            if close and e_dev > bound:             # a close call may be decided the other way: compare under the flipped decision
                if alt is None:
                    alt = (restated_step(rule, hp, snap, torch.float64, flip=True)[0], restated_step(rule, hp, snap, torch.float32, flip=True)[0])
                w2 = alt[0][ti]
                e_dev, bound = float((got[ti].double() - w2).abs().max()), 2.0 * float((alt[1][ti].double() - w2).abs().max()) + 2e-7 * scale
            assert e_dev <= bound, (tag, ti, tuple(w.shape), e_dev, bound, mode, margins)
            worst = max(worst, e_dev / bound if bound else 0.0)
            if margins:
                fired.append((tag, mode, margins))
    print("WORST dev/bound %-30s %.3f" % (tag, worst))


@pytest.mark.parametrize("pair", [("adamp", "sgdp"), ("ranger", "madgrad"), ("sgd", "rmsprop")], ids="-".join)
def test_sr_step_follows_the_restatement(pair, tmp_path):
    _, m = build_model(tmp_path, *pair)
    sg, sd, fired = [], [], []
    capture(m.optimizer_G, sg)
    capture(m.optimizer_D, sd)
    for s in range(1, 4):
        LR, HR = detrand.synthetic_pair(KW["batch"], KW["crop"], 940 + s)
        m.feed_data({"LR": LR, "HR": HR})
        m.optimize_parameters(s)
        torch.cuda.synchronize()
        check_step(m.optimizer_G, sg, "G %s step %d" % (pair[0], s), fired)
        check_step(m.optimizer_D, sd, "D %s step %d" % (pair[1], s), fired)
        m.get_current_log()
    if pair == ("adamp", "sgdp"):
        assert any(mode != 0 and min(mg) < 0.5 for _, mode, mg in fired), "no tensor fired with r < 1/2"
        assert any(mode == 0 and min(mg) > 2 for _, mode, mg in fired), "no tensor stayed unprojected with r > 2"
        print("fired", sorted({tag.split()[0] for tag, mode, mg in fired if mode}), "not fired", sorted({tag.split()[0] for tag, mode, mg in fired if not mode}))


def test_ranger_adamp_state_resumes_bit_for_bit(tmp_path):
    """optim_G: ranger / optim_D: adamp constructs, steps, saves a .state and a fresh model resumed from it (the train.py resume flow)
    continues bit for bit: weights, every state buffer and the step counts travel through the file."""
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    opt, a = build_model(tmp_path, "ranger", "adamp")

    def steps(m, first, last):
        logs = []
        for s in range(first, last + 1):
            LR, HR = detrand.synthetic_pair(KW["batch"], KW["crop"], 900 + s)
            m.feed_data({"LR": LR, "HR": HR})
            m.optimize_parameters(s)
            logs.append(dict(m.get_current_log()))
        return logs

    steps(a, 1, 3)
    a.save(3)
    a.save_training_state(0, 3)
    state_path = os.path.join(opt["path"]["training_state"], "3.state")
    logs_a = steps(a, 4, 6)                   # step 6: Ranger's lookahead and its first rectified step
    ropt = options.parse(optim_yaml(tmp_path, "ranger", "adamp", resume=state_path), is_train=True)
    resume_state = torch.load(ropt["path"]["resume_state"], weights_only=False)
    options.check_resume(ropt)
    b = create_model(ropt, verbose=False)
    netF = [l["function"].network for l in b.generatorlosses.loss_list if "fea" in l["name"]][0]
    sd = netF.state_dict()
    sd.update(FX.vgg_state(77))
    netF.load_state_dict(sd)
    b.resume_training(resume_state)
    b.update_schedulers(ropt["train"])
    assert steps(b, 4, 6) == logs_a
    for net in ("netG", "netD"):
        sa, sb = getattr(a, net).state_dict(), getattr(b, net).state_dict()
        for k, v in sa.items():
            assert torch.equal(v, sb[k]), (net, k)
    for oa, ob in zip(a.optimizers, b.optimizers):
        for (ka, va), (kb, vb) in zip(oa.state_dict()["state"].items(), ob.state_dict()["state"].items()):
            assert ka == kb and va["step"] == vb["step"] == 6 and va.keys() == vb.keys()
            for k in va:
                if k != "step":
                    assert torch.equal(va[k], vb[k]), (ka, k)
