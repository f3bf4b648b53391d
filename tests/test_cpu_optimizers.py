"""The optimisers beside Adam, host side (-m "not gpu"): the plain-torch restatement against tests/golden/optimizers.pt (the
reference's own classes, tools/make_golden_optimizers.py), the planted projection margins, config_optimizer's option reading and
refusals, and the Fused* classes' state layout and resume -- stepped with the ops entry points replaced by the restatement
(optim_restate.install, as tests/emul_backend.py does for Adam; the product has no CPU path).  Where the reference checkout is present
the state also crosses between the two engines, both ways."""
import io
import os

import pytest
import torch

import optim_restate as X
from oracle import detrand, ref_harness as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "optimizers.pt")
CASES = list(X.CONFIGS)
RULES = list(X.NAMES)
CLASSES = {"sgd": "FusedSGD", "rmsprop": "FusedRMSprop", "madgrad": "FusedMADGRAD", "adamp": "FusedAdamP", "sgdp": "FusedSGDP",
           "ranger": "FusedRanger"}


def golden():
    if not hasattr(golden, "fx"):
        golden.fx = torch.load(GOLDEN, weights_only=False)
    return golden.fx


def probe(t, n):
    f = t.detach().double().reshape(-1)
    idx = torch.linspace(0, f.numel() - 1, n).round().long()
    return torch.cat([f[idx], f.sum().reshape(1), f.abs().max().reshape(1)])


_TRAJ = {}


def trajectory64(case):
    """The fp64 restatement's run of `case`, computed once and shared (left unchanged by its users)."""
    if case not in _TRAJ:
        _TRAJ[case] = X.trajectory(case, dtype=torch.float64)
    return _TRAJ[case]


# ------------------------------------------------------------------------------------------------ restatement vs golden
@pytest.mark.parametrize("case", CASES)
def test_restatement_meets_golden(case):
    """Every probe of the parameters and the state at steps 1, 5, 6 and 8, to 1e-10 of the tensor's scale (the tool asserted 1e-12 on
    the machine that wrote the file; another host's libm may differ in the last bits of pow / sqrt over 8 steps)."""
    fx = golden()
    rec, _, _ = trajectory64(case)
    g = fx["cases"][case]
    assert tuple(fx["shapes"]) == X.SHAPES and tuple(fx["check"]) == X.CHECK
    for s in X.CHECK:
        ps, sts = rec[s]
        for key in ("p",) + X.STATE_KEYS[X.rule_of(case)]:
            for ti in range(len(X.SHAPES)):
                t = ps[ti] if key == "p" else sts[ti][key]
                want = g["steps"][s][key][ti]
                scale = max(float(g["steps"][s]["scale_" + key][ti]), 1e-30)
                got = probe(t, fx["nprobe"])
                assert float((got[:-2] - want[:-2]).abs().max()) <= 1e-10 * scale, (case, s, key, ti)
                assert abs(float(got[-2] - want[-2])) <= 1e-10 * scale * t.numel(), (case, s, key, ti)
                assert abs(float(got[-1] - want[-1])) <= 1e-10 * scale, (case, s, key, ti)


@pytest.mark.parametrize("case", ["adamp", "sgdp"])
def test_planted_margins(case):
    """Every planted decision is the planted one, with its margin r outside [1/3, 3], at every step; the three kinds occur within
    each step and every tensor with an even row count sees all three over the steps."""
    _, _, decisions = trajectory64(case)
    recorded = golden()["cases"][case]["decisions"]
    seen = set()
    for s, dec in enumerate(decisions, 1):
        kinds = set()
        for ti, (mode, margins) in enumerate(dec):
            if len(X.SHAPES[ti]) < 2:
                assert mode == 0 and margins == []
                continue
            kind = X.plant_kind(ti, s)
            kinds.add(kind)
            seen.add((ti, kind))
            assert mode == {0: 1, 1: 2, 2: 0}[kind], (s, ti, kind, mode, margins)
            assert all(r < 1 / 3 or r > 3 for r in margins), (s, ti, margins)
            assert mode == recorded[s - 1][ti][0]
        assert kinds == {0, 1, 2}, (s, kinds)
    for ti, shape in enumerate(X.SHAPES):
        if len(shape) > 1 and shape[0] % 2 == 0:
            assert {k for t, k in seen if t == ti} == {0, 1, 2}, ti


def test_ranger_branches():
    """beta2 0.999, threshold 5: steps 1-5 unrectified, 6-8 rectified; k 3 and k 6 both meet a lookahead step."""
    for case in ("ranger", "ranger_k6"):
        hp = X.CONFIGS[case]
        flags = [X.ranger_scalars(t, *hp["betas"], hp["N_sma_threshhold"])[0] for t in range(1, X.STEPS + 1)]
        assert flags == [False] * 5 + [True] * 3
        assert any(t % hp["k"] == 0 for t in range(1, X.STEPS + 1))


# ------------------------------------------------------------------------------------------------ host classes
SMALL = ((8, 3, 3, 3), (8,), (16, 64), (16,), (6, 10), (64,), (1,))


class Net(torch.nn.Module):
    def __init__(self, seed=900):
        super().__init__()
        self.ws = torch.nn.ParameterList([torch.nn.Parameter(detrand.uniform(s, seed + i, -0.1, 0.1)) for i, s in enumerate(SMALL)])

    def flat_params(self):
        from trainner_amd.flat import FlatParams
        if not hasattr(self, "_flat"):
            self._flat = FlatParams(self)
        return self._flat.ensure()


def small_grads(ps, step):
    """Planted like the golden's: rows orthogonal to p (the channel test fires) or noise + 0.5 p (nothing fires)."""
    out = []
    for ti, p in enumerate(ps):
        n = detrand.uniform(p.shape, 7000 + 50 * step + ti, -0.1, 0.1).double()
        q = p.detach().double()
        if p.dim() > 1 and (ti + step) % 2 == 0:
            P, N = q.reshape(p.shape[0], -1), n.reshape(p.shape[0], -1)
            g = (N - P * ((N * P).sum(1, keepdim=True) / (P * P).sum(1, keepdim=True))).reshape(p.shape)
        else:
            g = n + 0.5 * q
        out.append(g.float())
    return out


def build(case, net, name="G", extra=None):
    from trainner_amd.models import optimizers
    opt = X.train_opt(X.CONFIGS[case], name)
    opt["optim_" + name] = X.rule_of(case)
    opt.update(extra or {})
    return optimizers.config_optimizer(opt, name, net)


def take_steps(net, opt, steps):
    for s in steps:
        ps = list(net.parameters())
        for p, g in zip(ps, small_grads(ps, s)):
            p.grad.copy_(g)
        opt.step()


@pytest.fixture
def restated(monkeypatch):
    from trainner_amd import ops
    X.install(monkeypatch, ops)


@pytest.mark.parametrize("rule", RULES)
def test_config_optimizer_builds_each_class(rule):
    """From the reference's option names, with its defaults; the param-group keys are the reference class's."""
    from trainner_amd.models import optimizers
    o = build(rule, Net())
    assert type(o).__name__ == CLASSES[rule]
    g = golden()["cases"][rule]
    assert sorted(k for k in o.param_groups[0] if k != "params") == g["group_keys"]
    hp = X.CONFIGS[rule]
    for k, v in hp.items():
        if k in o.param_groups[0]:
            assert o.param_groups[0][k] == v, k
    d = optimizers.config_optimizer({"optim_D": rule}, "D", Net()).param_groups[0]      # the reference's defaults
    assert d["lr"] == 1e-4 and d["weight_decay"] == 0
    want = {"sgd": dict(momentum=0.9), "rmsprop": dict(eps=1e-8, alpha=0.99), "madgrad": dict(momentum=0.9, eps=1e-8),
            "adamp": dict(betas=(0.9, 0.999), eps=1e-8, delta=0.1, wd_ratio=0.1, nesterov=False),
            "sgdp": dict(momentum=0.9, dampening=0, eps=1e-8, delta=0.1, wd_ratio=0.1, nesterov=False),
            "ranger": dict(betas=(0.9, 0.999), eps=1e-8, alpha=0.5, k=6, N_sma_threshhold=5)}[rule]
    for k, v in want.items():
        assert d[k] == v, (k, d[k])


def test_config_optimizer_keeps_falsy_values():
    from trainner_amd.models import optimizers
    C = optimizers.config_optimizer
    assert C({"optim_G": "sgd", "momentum_G": 0, "lr_G": 0}, "G", Net()).param_groups[0]["momentum"] == 0
    assert C({"optim_G": "sgd", "beta1_G": 0.5}, "G", Net()).param_groups[0]["momentum"] == 0.5       # momentum defaults to beta1
    o = C({"optim_G": "ranger", "use_gc_G": False, "gc_conv_only_G": True, "k_G": 2, "alpha_G": 0.0, "N_sma_threshhold_G": 0}, "G", Net())
    assert (o.use_gc, o.gc_conv_only, o.param_groups[0]["k"], o.alpha, o.N_sma_threshhold) == (False, True, 2, 0.0, 0)
    o = C({"optim_D": "madgrad", "momentum_D": 0, "decay_type_D": "Adam", "eps_D": 0}, "D", Net())
    assert (o.param_groups[0]["momentum"], o.decay_type, o.param_groups[0]["eps"]) == (0, "Adam", 0)
    assert C({"optim_D": "madgrad"}, "D", Net()).decay_type == "AdamW"
    o = C({"optim_G": "sgdp", "dampening_G": 0.0, "nesterov_G": True, "delta_G": 0.0, "wd_ratio_G": 0.0}, "G", Net()).param_groups[0]
    assert (o["dampening"], o["nesterov"], o["delta"], o["wd_ratio"]) == (0.0, True, 0.0, 0.0)


def test_config_optimizer_refusals():
    from trainner_amd.models import optimizers
    C = optimizers.config_optimizer
    with pytest.raises(NotImplementedError, match="gc_loc_G"):
        C({"optim_G": "ranger", "gc_loc_G": False}, "G", Net())
    with pytest.raises(NotImplementedError, match="freeze_loc.*ranger"):
        C({"optim_D": "ranger", "freeze_loc": 2}, "D", Net())
    with pytest.raises(NotImplementedError, match="freeze_loc.*madgrad"):
        C({"optim_D": "madgrad", "freeze_loc": 2}, "D", Net())
    C({"optim_D": "madgrad", "momentum_D": 0, "freeze_loc": 2}, "D", Net())          # exact without momentum: accepted
    C({"optim_G": "ranger", "freeze_loc": 2}, "G", Net())                             # FreezeD freezes the discriminator only
    with pytest.raises(NotImplementedError, match="lion"):
        C({"optim_G": "lion"}, "G", Net())
    with pytest.raises(NotImplementedError):
        optimizers.get_optim_params(Net(), True, param_filter="RRDB")
    with pytest.raises(NotImplementedError, match="closure"):
        build("adamp", Net()).step(closure=lambda: 0.0)


@pytest.mark.parametrize("rule,key,value", [("sgd", "nesterov", True), ("sgd", "dampening", 0.1), ("sgd", "maximize", True),
                                            ("rmsprop", "momentum", 0.5), ("rmsprop", "centered", True), ("rmsprop", "maximize", True)])
def test_torch_group_options_are_refused_by_name(rule, key, value, restated):
    """The param groups of FusedSGD / FusedRMSprop carry torch's keys (a .state written by the reference's torch class loads); a value
    the launch does not implement raises with its name instead of stepping as the plain rule."""
    net = Net()
    o = build(rule, net)
    take_steps(net, o, [1])
    sd = _saved(o.state_dict())
    sd["param_groups"][0][key] = value
    o2 = build(rule, net)
    o2.load_state_dict(sd)
    with pytest.raises(NotImplementedError, match=key):
        take_steps(net, o2, [2])


def test_wrap_set_exceeds_both_grid_caps():
    """optim_restate.WRAP_SHAPES in one flat buffer: more chunks than the 2048 blocks of a chunk launch, more rows than the 4 x 2048 of a
    row launch -- what tests/test_gpu_optimizers.py::test_second_grid_stride_pass relies on; SHAPES stays below both."""
    from trainner_amd.flat import SegTable
    wrap, main = SegTable(X.layout(X.WRAP_SHAPES)[0], "cpu"), SegTable(X.layout()[0], "cpu")
    assert (wrap.nchunks, wrap.nrows) == (2197, 9024) and wrap.nchunks > 2048 and wrap.nrows > 8192
    assert (main.nchunks, main.nrows) == (679, 2714)


def _saved(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


@pytest.mark.parametrize("case", CASES + ["sgd_nomomentum", "madgrad_nomomentum"])
def test_resume_is_bit_exact(case, restated):
    """3 steps, state_dict() -> a fresh instance's load_state_dict() -> 2 more == 5 uninterrupted steps, bit for bit; the state_dict has
    the key lists the reference's class recorded."""
    extra = {"momentum_G": 0} if case.endswith("nomomentum") else {}
    case = case.replace("_nomomentum", "")
    a, b = Net(), Net()
    oa, ob = build(case, a, extra=extra), build(case, b, extra=extra)
    take_steps(a, oa, range(1, 6))
    take_steps(b, ob, range(1, 4))
    sd = _saved(ob.state_dict())
    c = Net()
    c.load_state_dict(_saved(b.state_dict()))
    oc = build(case, c, extra=extra)
    oc.load_state_dict(sd)
    take_steps(c, oc, range(4, 6))
    for pa, pc in zip(a.parameters(), c.parameters()):
        assert torch.equal(pa, pc)
    sa, sc = oa.state_dict(), oc.state_dict()
    assert sa["state"].keys() == sc["state"].keys()
    for k in sa["state"]:
        if isinstance(k, int):
            for kk in sa["state"][k]:
                va, vc = sa["state"][k][kk], sc["state"][k][kk]
                assert torch.equal(torch.as_tensor(va), torch.as_tensor(vc)), (k, kk)
        else:
            assert torch.equal(sa["state"][k], sc["state"][k])
    if not extra:
        g = golden()["cases"][case]
        assert sorted(sa["state"][0].keys()) == g["state_keys"]
        assert sorted(k for k in sa["state"] if not isinstance(k, int)) == g["top_keys"]
        assert sorted(k for k in sa["param_groups"][0] if k != "params") == g["group_keys"]
        assert sorted(sa["state"].keys(), key=str) == sorted(list(range(len(SMALL))) + g["top_keys"], key=str)
    elif case == "sgd":
        assert sa["state"] == {}
    else:
        assert sorted(sa["state"][0].keys()) == ["grad_sum_sq", "s"] and int(sa["state"]["k"]) == 5


def test_alignment_gaps_and_untouched_tables(restated):
    """State views alias the flat state buffers, and touch() does not rebuild the segment table while a re-laid buffer does."""
    net = Net()
    o = build("ranger", net)
    take_steps(net, o, [1])
    holder = net.flat_params()
    table = holder.seg_table()
    holder.touch()
    assert holder.seg_table() is table
    assert [e[1] for e in table.entries] == [tuple(s) for s in SMALL]
    segs = table.segs.tolist()
    assert segs[0] == [0, 216, 8, 27, 4, 0] and segs[1][2:] == [0, 8, 1, -1] and segs[2][2:] == [16, 64, 2, 8]
    assert table.nrows == 8 + 16 + 6 and int(table.chunks[:, 1].sum()) == sum(p.numel() for p in net.parameters())
    for p in net.parameters():
        assert o.state[p]["slow_buffer"].data_ptr() == o._moments[id(holder)][2].data_ptr() + 4 * p._tnr_flat[1]
    holder.flat = None                       # what a moved / replaced parameter leads to: ensure() re-lays the buffer
    assert net.flat_params().seg_table() is not table


# ------------------------------------------------------------------------------------------------ interchange with the reference
@pytest.mark.skipif(not R.reference_available(), reason="needs the reference checkout (build container)")
@pytest.mark.parametrize("case", CASES)
def test_state_interchange_with_reference(case, restated):
    """The engine's state loads into the reference's class and the reference's into the engine's; one further step of each agrees:
    the project's yardstick rule with the reference's fp32 step as the fp32 figure, both against the fp64 restatement of that step
    from the loaded state: err(engine) <= 2 err(reference) + 2e-7 scale, per tensor."""
    from tools import make_golden_optimizers as MG
    RO = MG._reference_module()
    rule = X.rule_of(case)
    for direction in ("engine->reference", "reference->engine"):
        src_net = Net()
        ref_ps = [torch.nn.Parameter(p.detach().clone()) for p in src_net.parameters()]
        ref = MG.reference_optimizer(RO, case, ref_ps)
        eng = build(case, src_net)
        if direction == "engine->reference":
            take_steps(src_net, eng, range(1, 4))
            for q, p in zip(ref_ps, src_net.parameters()):
                q.data.copy_(p.data)
            ref.load_state_dict(_saved(eng.state_dict()))
        else:
            for s in range(1, 4):
                for q, g in zip(ref_ps, small_grads(ref_ps, s)):
                    q.grad = g.clone()
                ref.step()
            with torch.no_grad():
                for q, p in zip(ref_ps, src_net.parameters()):
                    p.copy_(q)
            eng.load_state_dict(_saved(ref.state_dict()))
        # the fp64 restatement continues from the loaded state
        keys = [k for k in X.STATE_KEYS[rule]]
        run = X.Run(rule, [q.detach() for q in ref_ps], X.CONFIGS[case], torch.float64)
        run.state = [{k: ref.state[q][k].detach().double().clone() for k in keys} for q in ref_ps]
        run.t = 3
        gs = small_grads(ref_ps, 4)
        run.step(gs)
        for q, g in zip(ref_ps, gs):
            q.grad = g.clone()
        ref.step()
        for p, g in zip(src_net.parameters(), gs):
            p.grad.copy_(g)
        eng.step()
        for ti, (p, q, w) in enumerate(zip(src_net.parameters(), ref_ps, run.p)):
            scale = float(w.abs().max())
            e_eng, e_ref = float((p.double() - w).abs().max()), float((q.double() - w).abs().max())
            assert e_eng <= 2 * e_ref + 2e-7 * scale, (direction, ti, e_eng, e_ref, scale)
