"""Plain-torch restatement of the six optimisers beside Adam (sgd, rmsprop, madgrad, adamp, sgdp, ranger), per tensor, written from
their update rules; usable in fp64 (the tests' reference) and in fp32 (a yardstick).  A helper, not a test.

Also here, because the golden tool, the CPU tests and the GPU tests share them: the tensor set, the hyper-parameters of the recorded
runs, the planted gradients, and `install()`, which replaces the engine's ops entry points by the restatement (as
tests/emul_backend.py does for Adam) so the host classes can be stepped without a device.

Projection margins: every AdamP / SGDP decision is `max |cos| < delta / sqrt(row length)`; its margin is
r = max |cos| sqrt(row length) / delta (the decision fires when r < 1).  `step()` returns them per tensor.
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import detrand  # noqa: E402

NAMES = ("sgd", "rmsprop", "madgrad", "adamp", "sgdp", "ranger")
ALIGN = 64
# rows of 1 to 8192 elements ([4, 8192] and [64, 64, 3, 3]: longer than a wave), 2500 rows of 5, a 1-D tensor of 586 chunks.  In one
# flat buffer: 679 chunks and 2714 rows = 679 four-row blocks, all below the launches' 2048-block grid cap: ONE grid-stride pass.
SHAPES = ((1,), (64,), (5, 1), (1, 100), (8, 3, 3, 3), (16, 64), (16, 65), (100, 37), (64, 64, 3, 3), (4, 8192), (2500, 5), (600001,))
BIG = len(SHAPES) - 1           # rebuilt from its seed, never stored: the golden keeps probes of it
# The second grid-stride pass of every kernel: 2200 chunks (cap 2048 blocks, one chunk each) and 9024 rows (cap 2048 blocks x 4 rows =
# 8192).  [9000, 5] comes first, so the second pass of the row kernels ends that tensor and goes on into the next 2-D tensors; the 1-D
# tensor next, so the second pass of the chunk kernels ends it and goes on into tensors with other segment entries.
WRAP_SHAPES = ((9000, 5), (2200003,), (16, 65), (8, 3, 3, 3), (64,))
WRAP_STEPS, WRAP_CHECK = 3, (1, 3)          # step 3: the lookahead step of the recorded Ranger configuration (k 3)
STEPS, CHECK = 8, (1, 5, 6, 8)
STATE_KEYS = {"sgd": ("momentum_buffer",), "rmsprop": ("square_avg",), "madgrad": ("grad_sum_sq", "s", "x0"),
              "adamp": ("exp_avg", "exp_avg_sq"), "sgdp": ("momentum",), "ranger": ("exp_avg", "exp_avg_sq", "slow_buffer")}
PARAM_COPIES = ("x0", "slow_buffer")
# the recorded runs (tools/make_golden_optimizers.py); every key is the reference classes' own
CONFIGS = {
    "sgd": dict(lr=0.01, momentum=0.9, weight_decay=1e-3),
    "rmsprop": dict(lr=0.01, alpha=0.99, eps=1e-8, weight_decay=1e-3),
    "madgrad": dict(lr=0.01, momentum=0.9, eps=1e-6, weight_decay=1e-3, decay_type="AdamW"),
    "adamp": dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, delta=0.1, wd_ratio=0.1, nesterov=False),
    "sgdp": dict(lr=0.01, momentum=0.9, dampening=0, weight_decay=1e-2, nesterov=False, eps=1e-8, delta=0.1, wd_ratio=0.1),
    "ranger": dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3, alpha=0.5, k=3, N_sma_threshhold=5, use_gc=True,
                   gc_conv_only=False),
    "ranger_k6": dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, use_gc=True,
                      gc_conv_only=False),
}


# options the recorded runs do not take; tools/make_golden_optimizers.py asserts the restatement against the reference for each
OPTION_CASES = {
    "sgd_nomomentum": dict(momentum=0),
    "adamp_nesterov": dict(nesterov=True), "adamp_nowd": dict(weight_decay=0), "adamp_nesterov_nowd": dict(nesterov=True, weight_decay=0),
    "sgdp_nesterov": dict(nesterov=True), "sgdp_nowd": dict(weight_decay=0), "sgdp_nesterov_nowd": dict(nesterov=True, weight_decay=0),
    "madgrad_nomomentum": dict(momentum=0), "madgrad_adamdecay": dict(decay_type="Adam"),
    "madgrad_nomomentum_adamdecay": dict(momentum=0, decay_type="Adam"),
    "ranger_nogc": dict(use_gc=False), "ranger_convonly": dict(gc_conv_only=True),
}


def hp_of(case):
    return dict(CONFIGS[rule_of(case)], **OPTION_CASES[case]) if case in OPTION_CASES else dict(CONFIGS[case])


def rule_of(case):
    return case.split("_")[0]


def train_opt(hp, name="G"):
    """The reference's option names (codes/models/optimizers.py:89-129) for a CONFIGS entry."""
    names = {"lr": "lr_" + name, "weight_decay": "weight_decay_" + name, "eps": "eps_" + name, "nesterov": "nesterov_" + name, "delta": "delta_" + name,
             "wd_ratio": "wd_ratio_" + name, "momentum": "momentum_" + name, "dampening": "dampening_" + name, "alpha": "alpha_" + name, "k": "k_" + name,
             "N_sma_threshhold": "N_sma_threshhold_" + name, "use_gc": "use_gc_" + name, "gc_conv_only": "gc_conv_only_" + name, "decay_type": "decay_type_" + name}
    opt = {}
    for k, v in hp.items():
        if k == "betas":
            opt["beta1_" + name], opt["beta2_" + name] = v
        else:
            opt[names[k]] = v
    return opt


# ------------------------------------------------------------------------------------------------ inputs
def make_params(shapes=SHAPES):
    """The tensor set, fp32, a pure function of the seeds."""
    return [detrand.uniform(s, 4100 + i, -0.1, 0.1) for i, s in enumerate(shapes)]


def plant_kind(ti, step, shape=None):
    """0: every row orthogonal to p (the per-channel test fires); 1: rows +-p_row / |p_row|^2 with alternating sign (only the
    whole-tensor test fires; needs an even row count, else kind 0); 2: noise + 0.5 p (nothing fires).  Mixed over the tensors within
    a step, alternating over the steps."""
    shape = SHAPES[ti] if shape is None else shape
    kind = (ti + step) % 3
    if kind == 1 and (len(shape) < 2 or shape[0] % 2):
        kind = 0
    return kind


def planted_grads(step, ps):
    """The gradients of step `step` (1-based) for the current parameters `ps` (the fp64 run's): built in fp64, returned in fp32, and
    every run -- fp64, fp32, device -- steps with these fp32 values."""
    out = []
    for ti, p in enumerate(ps):
        noise = detrand.uniform(p.shape, 5200 + 100 * step + ti, -0.1, 0.1).double()
        p64 = p.detach().double().cpu()
        kind = plant_kind(ti, step, tuple(p.shape))
        if p.dim() < 2:
            g = noise + (0.5 * p64 if kind == 2 else 0)
        else:
            P, N = p64.reshape(p.shape[0], -1), noise.reshape(p.shape[0], -1)
            pp = (P * P).sum(1, keepdim=True)
            if kind == 0:
                g = N - P * ((N * P).sum(1, keepdim=True) / pp)
            elif kind == 1:
                sign = torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(p.shape[0] // 2).reshape(-1, 1)
                g = sign * P / pp
            else:
                g = N + 0.5 * P
            g = g.reshape(p.shape)
        out.append(g.float())
    return out


def layout(shapes=SHAPES):
    """-> ([(offset, shape)], total): the tensors in one flat buffer, every one 256-byte aligned (trainner_amd/flat.py)."""
    entries, off = [], 0
    for s in shapes:
        n = 1
        for d in s:
            n *= d
        entries.append((off, tuple(s)))
        off += (n + ALIGN - 1) // ALIGN * ALIGN
    return entries, off


def views(flat, entries):
    out = []
    for o, s in entries:
        n = 1
        for d in s:
            n *= d
        out.append(flat[o:o + n].view(s))
    return out


# ------------------------------------------------------------------------------------------------ the rules
def projection(p, g, perturb, delta, wd_ratio, eps, flip=False):
    """-> (perturb, weight-decay ratio, mode, margins): mode 1 = projected per output channel, 2 = on the whole tensor, 0 = left alone;
    margins = [r of the channel test, r of the whole-tensor test (absent if the channel test fired)].  flip: every test whose margin
    lies in [1/2, 2] is decided the other way (what an equally valid evaluation of a close call may do)."""
    if p.dim() <= 1:
        return perturb, 1.0, 0, []
    margins = []
    for mode, rows in ((1, p.shape[0]), (2, 1)):
        P, G, Q = p.reshape(rows, -1), g.reshape(rows, -1), perturb.reshape(rows, -1)
        cos = ((G * P).sum(1) / (G.norm(dim=1).clamp_min(eps) * P.norm(dim=1).clamp_min(eps))).abs()
        n = P.shape[1]
        margins.append(float(cos.max()) * math.sqrt(n) / max(delta, 1e-300))
        fire = float(cos.max()) < delta / math.sqrt(n)
        if flip and 0.5 <= margins[-1] <= 2:
            fire = not fire
        if fire:
            pn = P / (P.norm(dim=1, keepdim=True) + eps)
            return (Q - pn * (pn * Q).sum(1, keepdim=True)).reshape(p.shape), wd_ratio, mode, margins
    return perturb, 1.0, 0, margins


def ranger_scalars(t, b1, b2, threshold):
    beta2_t = b2 ** t
    n_max = 2 / (1 - b2) - 1
    n_sma = n_max - 2 * t * beta2_t / (1 - beta2_t)
    if n_sma > threshold:
        return True, math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - b1 ** t)
    return False, 1.0 / (1 - b1 ** t)


def init_state(rule, p, hp):
    keys = STATE_KEYS[rule]
    if rule in ("sgd", "madgrad") and not hp.get("momentum", 0):
        keys = tuple(k for k in keys if k not in ("momentum_buffer", "x0"))
    return {k: (p.clone() if k in PARAM_COPIES else torch.zeros_like(p)) for k in keys}


def rule_step(rule, p, g, st, hp, t):
    """One step (number t, 1-based) of one tensor, in place, in the dtype of p.  -> (mode, margins) of the projection rules."""
    g = g.to(p.dtype)
    wd = hp.get("weight_decay", 0)
    if rule == "sgd":
        if wd:
            g = g + wd * p
        if hp["momentum"]:
            st["momentum_buffer"].mul_(hp["momentum"]).add_(g)
            g = st["momentum_buffer"]
        p.add_(g, alpha=-hp["lr"])
    elif rule == "rmsprop":
        if wd:
            g = g + wd * p
        st["square_avg"].mul_(hp["alpha"]).addcmul_(g, g, value=1 - hp["alpha"])
        p.addcdiv_(g, st["square_avg"].sqrt() + hp["eps"], value=-hp["lr"])
    elif rule == "madgrad":
        eps, mom = hp["eps"], hp["momentum"]
        lr = hp["lr"] + eps
        lamb = lr * math.sqrt(t)                       # k + 1 = t
        if wd:
            if hp["decay_type"] == "AdamW":
                p.mul_(1 - lr * wd)
            else:
                g = g + wd * p
        x0 = st["x0"] if mom else p + st["s"] / (st["grad_sum_sq"].pow(1 / 3) + eps)
        st["grad_sum_sq"].addcmul_(g, g, value=lamb)
        rms = st["grad_sum_sq"].pow(1 / 3) + eps
        st["s"].add_(g, alpha=lamb)
        z = x0 - st["s"] / rms
        if mom:
            ck = 1 - mom
            p.mul_(1 - ck).add_(z, alpha=ck)
        else:
            p.copy_(z)
    elif rule == "adamp":
        b1, b2 = hp["betas"]
        st["exp_avg"].mul_(b1).add_(g, alpha=1 - b1)
        st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = st["exp_avg_sq"].sqrt() / math.sqrt(1 - b2 ** t) + hp["eps"]
        perturb = (b1 * st["exp_avg"] + (1 - b1) * g) / denom if hp["nesterov"] else st["exp_avg"] / denom
        perturb, ratio, mode, margins = projection(p, g, perturb, hp["delta"], hp["wd_ratio"], hp["eps"], hp.get("flip", False))
        if wd > 0:
            p.mul_(1 - hp["lr"] * wd * ratio)
        p.add_(perturb, alpha=-hp["lr"] / (1 - b1 ** t))
        return mode, margins
    elif rule == "sgdp":
        mom = hp["momentum"]
        st["momentum"].mul_(mom).add_(g, alpha=1 - hp["dampening"])
        perturb = g + mom * st["momentum"] if hp["nesterov"] else st["momentum"]
        perturb, ratio, mode, margins = projection(p, g, perturb, hp["delta"], hp["wd_ratio"], hp["eps"], hp.get("flip", False))
        if mode and not hp["nesterov"]:
            st["momentum"].copy_(perturb)          # the reference projects `buf` itself in place (d_p = buf, `perturb -= ...`)
        if wd > 0:
            p.mul_(1 - hp["lr"] * wd * ratio / (1 - mom))
        p.add_(perturb, alpha=-hp["lr"])
        return mode, margins
    elif rule == "ranger":
        b1, b2 = hp["betas"]
        if hp["use_gc"] and p.dim() > (3 if hp["gc_conv_only"] else 1):
            g = g + (-g.mean(dim=tuple(range(1, p.dim())), keepdim=True))
        st["exp_avg"].mul_(b1).add_(g, alpha=1 - b1)
        st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
        rect, step_size = ranger_scalars(t, b1, b2, hp["N_sma_threshhold"])
        if rect:
            G = st["exp_avg"] / (st["exp_avg_sq"].sqrt() + hp["eps"])
        else:
            G = st["exp_avg"]                      # the reference aliases: its `G += wd p` below lands in exp_avg as well
        if wd != 0:
            G.add_(p, alpha=wd)
        p.add_(G, alpha=-step_size * hp["lr"])
        if t % hp["k"] == 0:
            st["slow_buffer"].add_(p - st["slow_buffer"], alpha=hp["alpha"])
            p.copy_(st["slow_buffer"])
    else:
        raise KeyError(rule)
    return 0, []


class Run:
    """The restatement stepping a list of tensors."""

    def __init__(self, rule, params, hp, dtype=torch.float64):
        self.rule, self.hp, self.t = rule, dict(hp), 0
        self.p = [q.detach().to(dtype).clone() for q in params]
        self.state = None

    def step(self, grads):
        """-> [(mode, margins)] per tensor"""
        if self.state is None:          # as the reference: state is created at the first step, from the parameters of that moment
            self.state = [init_state(self.rule, q, self.hp) for q in self.p]
        self.t += 1
        return [rule_step(self.rule, q, g, st, self.hp, self.t) for q, g, st in zip(self.p, grads, self.state)]


def trajectory(case, hp=None, dtype=torch.float64, grads64=None, shapes=SHAPES, steps=STEPS, check=CHECK):
    """The STEPS planted steps of `case`.  The gradients are planted against the fp64 run's parameters, so the fp64 run goes first and
    hands its gradients (`grads64`: [step][tensor]) to the others.  -> (records {step: (params, state)} at CHECK, gradients, decisions)"""
    hp = hp_of(case) if hp is None else hp
    run = Run(rule_of(case), make_params(shapes), hp, dtype)
    rec, grads, decisions = {}, [], []
    for s in range(1, steps + 1):
        gs = planted_grads(s, run.p) if grads64 is None else grads64[s - 1]
        grads.append(gs)
        decisions.append(run.step(gs))
        if s in check:
            rec[s] = ([q.clone() for q in run.p], [{k: v.clone() for k, v in st.items()} for st in run.state])
    return rec, grads, decisions


# ------------------------------------------------------------------------------------------------ the ops entry points, restated
def _each(table, *bufs):
    return zip(*[views(b, table.entries) if b is not None else [None] * len(table.entries) for b in bufs])


def sgd_step(p, g, buf, table, lr, momentum=0.0, wd=0.0):
    for pv, gv, bv in _each(table, p, g, buf):
        rule_step("sgd", pv, gv, {"momentum_buffer": bv}, dict(lr=lr, momentum=momentum, weight_decay=wd), 0)


def rmsprop_step(p, g, square_avg, table, lr, alpha, eps, wd=0.0):
    for pv, gv, sv in _each(table, p, g, square_avg):
        rule_step("rmsprop", pv, gv, {"square_avg": sv}, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=wd), 0)


def madgrad_step(p, g, grad_sum_sq, s, x0, table, lr, eps, k, momentum, decay=0.0, decay_type="AdamW"):
    for pv, gv, qv, sv, xv in _each(table, p, g, grad_sum_sq, s, x0):
        rule_step("madgrad", pv, gv, {"grad_sum_sq": qv, "s": sv, "x0": xv},
                  dict(lr=lr, eps=eps, momentum=momentum, weight_decay=decay, decay_type=decay_type), k + 1)


def adamp_step(p, g, m, v, table, lr, b1, b2, eps, t, nesterov=False, delta=0.1, wd_ratio=0.1, wd=0.0):
    for pv, gv, mv, vv in _each(table, p, g, m, v):
        rule_step("adamp", pv, gv, {"exp_avg": mv, "exp_avg_sq": vv},
                  dict(lr=lr, betas=(b1, b2), eps=eps, nesterov=nesterov, delta=delta, wd_ratio=wd_ratio, weight_decay=wd), t)


def sgdp_step(p, g, buf, table, lr, momentum, dampening, eps, nesterov=False, delta=0.1, wd_ratio=0.1, wd=0.0):
    for pv, gv, bv in _each(table, p, g, buf):
        rule_step("sgdp", pv, gv, {"momentum": bv}, dict(lr=lr, momentum=momentum, dampening=dampening, eps=eps, nesterov=nesterov,
                                                         delta=delta, wd_ratio=wd_ratio, weight_decay=wd), 0)


def ranger_step(p, g, m, v, slow, table, lr, b1, b2, eps, wd, t, k=6, alpha=0.5, nsma_threshold=5, use_gc=True, gc_conv_only=False):
    for pv, gv, mv, vv, sv in _each(table, p, g, m, v, slow):
        rule_step("ranger", pv, gv, {"exp_avg": mv, "exp_avg_sq": vv, "slow_buffer": sv},
                  dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, k=k, alpha=alpha, N_sma_threshhold=nsma_threshold, use_gc=use_gc,
                       gc_conv_only=gc_conv_only), t)


def fill(t, value):
    t.fill_(value)


OPS = ("sgd_step", "rmsprop_step", "madgrad_step", "adamp_step", "sgdp_step", "ranger_step", "fill")


def install(monkeypatch, ops):
    """Replace the engine's optimiser entry points by the restatement (CPU tests of the host classes)."""
    for name in OPS:
        monkeypatch.setattr(ops, name, globals()[name])
