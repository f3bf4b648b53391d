"""Optimiser factory of the SR path.

`config_optimizer(train_opt, name, net)` keeps the reference's contract (codes/models/optimizers.py:
74-134: lr_<G|D> default 1e-4, beta1 0.9, beta2 0.999, weight decay 0, Adam default eps 1e-8) but the
'adam' branch (:130-132) returns FusedAdam: torch.optim.Adam's update rule as ONE HIP launch over the
network's flat parameter buffer instead of ~700 per-tensor kernels.  state_dict()/load_state_dict()
use torch.optim.Adam's layout ('step', 'exp_avg', 'exp_avg_sq' per parameter) so `.state` files
written by either engine resume in the other (base_model.py:454-500).

The other branches (:100-129) return FusedSGD, FusedRMSprop, FusedSGDP, FusedAdamP, FusedRanger and
FusedMADGRAD: the reference classes' update rules as 1, 1, 4, 4, 2 and 1 launches over the same flat
buffers (csrc/optimizers.hip), each with the state layout and param-group keys of the class the
reference would have built.
"""
import logging
import math
import os

import torch

from .. import ops

logger = logging.getLogger("base")


def get_optim_params(networks, only_requires_grad=True, param_filter=None):
    if isinstance(networks, torch.nn.Module):
        networks = [networks]
    if param_filter:
        raise NotImplementedError("parameter filters are not implemented by the HIP engine")
    params = []
    for net in networks:
        params += [p for p in net.parameters() if p.requires_grad or not only_requires_grad]
    return params, []


class FusedFlatOptimizer(torch.optim.Optimizer):
    """What the fused optimisers share: the flat buffers their parameters live in, one flat state buffer per state key (the
    per-parameter state entries are views into them), re-homing of loaded state, and ONE host step counter per group."""
    STATE_KEYS = ()          # per-parameter state held in flat buffers, in the order of self._moments[...]
    PARAM_COPIES = ()        # those of them that start as a copy of the parameters (the rest start at zero)
    STEP_IN_STATE = True     # the class's layout carries a per-parameter 'step'

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._moments = {}     # id(FlatParams) -> the flat state buffers (STATE_KEYS order)
        self._t = {}           # group index -> optimiser steps taken (ONE host counter per group; the per-parameter `step` entries of
                               # the reference layouts exist only in state_dict(), where the reference resuming from it needs them)

    def _state_keys(self, group):
        return self.STATE_KEYS

    def _step_entry(self, t):
        return torch.tensor(float(t))

    def _holders(self, group):
        """The distinct flat buffers the group's parameters live in (insertion ordered)."""
        holders = {}
        for p in group["params"]:
            h = getattr(p, "_tnr_flat", None)
            if h is None:
                raise RuntimeError("%s: parameter is not part of a HIP-engine network (no flat storage)" % type(self).__name__)
            holders.setdefault(id(h[0]), h[0])
        return list(holders.values())

    def _ensure_state(self, group):
        keys = self._state_keys(group)
        for holder in self._holders(group):
            holder.ensure()
            key = id(holder)
            mv = self._moments.get(key)
            if mv is None or (mv and (mv[0].numel() != holder.total or mv[0].device != holder.flat.device)):
                mv = tuple(holder.flat.clone() if k in self.PARAM_COPIES else torch.zeros_like(holder.flat) for k in keys)
                self._moments[key] = mv
                for p in (group["params"] if keys else ()):      # (a rule without state leaves self.state empty, as torch's does)
                    if p._tnr_flat[0] is not holder:
                        continue
                    st = self.state[p]
                    o, n = p._tnr_flat[1], p.numel()
                    for k, buf in zip(keys, mv):
                        old = st.get(k)
                        st[k] = buf[o:o + n].view(p.shape)
                        if old is not None:          # state arrived through load_state_dict
                            st[k].copy_(old)

    def _group_step(self, group, holder, state, t):
        """One optimiser step (number t, 1-based) of `group` over `holder`'s buffers; `state` are its flat state buffers."""
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("closures are not supported")
        for gi, group in enumerate(self.param_groups):
            self._ensure_state(group)
            t = self._t.get(gi, 0) + 1
            for holder in self._holders(group):
                self._group_step(group, holder, self._moments[id(holder)], t)
                holder.touch()                       # packed weights of this network are stale now
            self._t[gi] = t

    def group_steps(self):
        """Optimiser steps taken, per parameter group."""
        return [self._t.get(gi, 0) for gi in range(len(self.param_groups))]

    def state_dict(self):
        """The reference class's layout.  `step` is materialised here, one entry PER parameter: torch.optim.Adam (the reference resuming
        from this state, base_model.py:479-491) increments each entry in place and torch.save keeps aliasing -- a shared tensor would be
        bumped once per parameter per step."""
        for gi, group in enumerate(self.param_groups):
            if self._moments or gi in self._t:
                self._ensure_state(group)
            keys = self._state_keys(group)
            for p in group["params"]:
                if self.STEP_IN_STATE and keys and p in self.state and keys[0] in self.state[p]:
                    self.state[p]["step"] = self._step_entry(self._t.get(gi, 0))
        return super().state_dict()

    def zero_grad(self, set_to_none=False):
        """Zero the flat gradient buffers in place (views stay attached to the parameters)."""
        for group in self.param_groups:
            for holder in self._holders(group):
                holder.ensure()
                ops.fill(holder.grad, 0.0)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._moments = {}       # re-home the loaded state into flat buffers on next use
        self._t = {}
        for gi, group in enumerate(self.param_groups):
            steps = {int(float(self.state[p]["step"])) for p in group["params"] if p in self.state and "step" in self.state[p]}
            if len(steps) > 1:
                # a reference checkpoint may legitimately hold this: a parameter whose grad was None for some steps (frozen
                # or unfrozen mid-run) lags the others.  The fused classes keep ONE counter per group (bias corrections are launch
                # arguments): resume from the most advanced one -- what the bulk of the parameters had -- and say so.
                # TNR_STRICT_OPTIM_STATE=1 turns this into an error.
                msg = "%s: the parameters of group %d carry different step counts %s; resuming with step %d for all of them" % (
                    type(self).__name__, gi, sorted(steps), max(steps))
                if os.environ.get("TNR_STRICT_OPTIM_STATE") == "1":
                    raise ValueError(msg)
                logger.warning(msg)
            if steps:
                self._t[gi] = max(steps)
            self._loaded_group(gi, group)
            if any(p in self.state and self.state[p] for p in group["params"]):
                self._ensure_state(group)

    def _loaded_group(self, gi, group):
        pass


class FusedAdam(FusedFlatOptimizer):
    STATE_KEYS = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _group_step(self, group, holder, state, t):
        b1, b2 = group["betas"]
        bc1 = 1.0 - b1 ** t
        bc2 = 1.0 - b2 ** t
        ops.adam_step(holder.flat, holder.grad, state[0], state[1], group["lr"] / bc1, b1, b2, math.sqrt(bc2), group["eps"],
                      group["weight_decay"])

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._ensure_state(group)


def _torch_defaults(cls, **kw):
    """The param-group keys of a torch.optim class as THIS torch spells them (they vary between releases)."""
    return dict(cls([torch.zeros(1)], **kw).defaults)


class FusedSGD(FusedFlatOptimizer):
    """torch.optim.SGD as the reference builds it (optimizers.py:100-102: lr, weight_decay, momentum)."""
    STEP_IN_STATE = False

    def __init__(self, params, lr=1e-4, momentum=0.9, weight_decay=0):
        super().__init__(params, _torch_defaults(torch.optim.SGD, lr=lr, momentum=momentum, weight_decay=weight_decay))

    def _state_keys(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def _group_step(self, group, holder, state, t):
        for key in ("nesterov", "dampening", "maximize"):          # (a loaded .state may carry them in its param groups)
            if group.get(key):
                raise NotImplementedError("SGD with %s = %r is not implemented by the HIP engine" % (key, group[key]))
        ops.sgd_step(holder.flat, holder.grad, state[0] if state else None, holder.seg_table(), group["lr"], group["momentum"],
                     group["weight_decay"])


class FusedRMSprop(FusedFlatOptimizer):
    """torch.optim.RMSprop as the reference builds it (optimizers.py:103-105: lr, weight_decay, eps; alpha 0.99, not centered)."""
    STATE_KEYS = ("square_avg",)

    def __init__(self, params, lr=1e-4, eps=1e-8, weight_decay=0):
        super().__init__(params, _torch_defaults(torch.optim.RMSprop, lr=lr, eps=eps, weight_decay=weight_decay))

    def _group_step(self, group, holder, state, t):
        for key in ("momentum", "centered", "maximize"):
            if group.get(key):
                raise NotImplementedError("RMSprop with %s = %r is not implemented by the HIP engine" % (key, group[key]))
        ops.rmsprop_step(holder.flat, holder.grad, state[0], holder.seg_table(), group["lr"], group["alpha"], group["eps"],
                         group["weight_decay"])


class FusedAdamP(FusedFlatOptimizer):
    """AdamP (modules/optimizers/adamp/adamp.py); `step` is a Python int in its layout."""
    STATE_KEYS = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, delta=0.1, wd_ratio=0.1, nesterov=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, delta=delta, wd_ratio=wd_ratio,
                                      nesterov=nesterov))

    def _step_entry(self, t):
        return int(t)

    def _group_step(self, group, holder, state, t):
        b1, b2 = group["betas"]
        ops.adamp_step(holder.flat, holder.grad, state[0], state[1], holder.seg_table(), group["lr"], b1, b2, group["eps"], t,
                       group["nesterov"], group["delta"], group["wd_ratio"], group["weight_decay"])


class FusedSGDP(FusedFlatOptimizer):
    """SGDP (modules/optimizers/adamp/sgdp.py)."""
    STATE_KEYS = ("momentum",)
    STEP_IN_STATE = False

    def __init__(self, params, lr=1e-4, momentum=0, dampening=0, weight_decay=0, nesterov=False, eps=1e-8, delta=0.1, wd_ratio=0.1):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      eps=eps, delta=delta, wd_ratio=wd_ratio))

    def _group_step(self, group, holder, state, t):
        ops.sgdp_step(holder.flat, holder.grad, state[0], holder.seg_table(), group["lr"], group["momentum"], group["dampening"],
                      group["eps"], group["nesterov"], group["delta"], group["wd_ratio"], group["weight_decay"])


class FusedRanger(FusedFlatOptimizer):
    """Ranger (modules/optimizers/ranger/ranger.py): gradient centralisation, rectified Adam and lookahead.  As there, alpha, the
    N_sma threshold and the gradient-centralisation switches are the constructor's, k is the group's; `step` is a Python int."""
    STATE_KEYS = ("exp_avg", "exp_avg_sq", "slow_buffer")
    PARAM_COPIES = ("slow_buffer",)

    def __init__(self, params, lr=1e-3, betas=(.95, 0.999), eps=1e-5, weight_decay=0, alpha=0.5, k=6, N_sma_threshhold=5, use_gc=True,
                 gc_conv_only=False, gc_loc=True):
        if not gc_loc:
            raise NotImplementedError("ranger: gc_loc false (centralising the update instead of the gradient) is not implemented by the HIP engine")
        if not 0.0 <= alpha <= 1.0:
            raise ValueError("Invalid slow update rate: {}".format(alpha))
        if k < 1:
            raise ValueError("Invalid lookahead steps: {}".format(k))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, alpha=alpha, k=k,
                                      N_sma_threshhold=N_sma_threshhold, step_counter=0))
        self.N_sma_threshhold, self.alpha, self.k = N_sma_threshhold, alpha, k
        self.gc_loc, self.use_gc, self.gc_conv_only = gc_loc, use_gc, gc_conv_only

    def _step_entry(self, t):
        return int(t)

    def _group_step(self, group, holder, state, t):
        b1, b2 = group["betas"]
        ops.ranger_step(holder.flat, holder.grad, state[0], state[1], state[2], holder.seg_table(), group["lr"], b1, b2, group["eps"],
                        group["weight_decay"], t, group["k"], self.alpha, self.N_sma_threshhold, self.use_gc, self.gc_conv_only)


class FusedMADGRAD(FusedFlatOptimizer):
    """MADGRAD (modules/optimizers/madgrad/madgrad.py).  Its step counter is ONE top-level state entry `k` (a long tensor of one
    element), shared by all groups; decay_type is the constructor's, not a group key."""
    STEP_IN_STATE = False
    PARAM_COPIES = ("x0",)

    def __init__(self, params, lr=1e-2, momentum=0.9, eps=1e-6, weight_decay=0, decay_type="Adam"):
        if momentum < 0 or momentum >= 1:
            raise ValueError("Momentum {} must be in the range [0,1]".format(momentum))
        super().__init__(params, dict(lr=lr, eps=eps, momentum=momentum, weight_decay=weight_decay))
        self.decay_type = decay_type

    def _state_keys(self, group):
        return ("grad_sum_sq", "s", "x0") if group["momentum"] != 0 else ("grad_sum_sq", "s")

    def _group_step(self, group, holder, state, t):
        ops.madgrad_step(holder.flat, holder.grad, state[0], state[1], state[2] if len(state) > 2 else None, holder.seg_table(),
                         group["lr"], group["eps"], t - 1, group["momentum"], group["weight_decay"], self.decay_type)

    def state_dict(self):
        if self._t:
            self.state["k"] = torch.tensor([max(self._t.values())], dtype=torch.long)
        return super().state_dict()

    def _loaded_group(self, gi, group):
        if "k" in self.state:
            self._t[gi] = int(self.state["k"].item())


def config_optimizer(train_opt, name, net=None, optim_params=None):
    if name not in ("G", "D"):
        raise NotImplementedError("Invalid optimizer name: {}".format(name))
    for n in ([net] if isinstance(net, torch.nn.Module) else (net or [])):
        if hasattr(n, "flat_params"):
            n.flat_params()              # parameters become views of the network's flat buffer
    if not optim_params:
        optim_params, _ = get_optim_params(net, True)
    def opt_or(key, default):
        # missing keys read as None (NoneDict); legitimate falsy values (beta1_G: 0, lr_D: 0) are kept
        v = train_opt.get(key + name, None)
        return default if v is None else v

    optim = opt_or("optim_", "adam")
    lr = opt_or("lr_", 1e-4)
    wd = opt_or("weight_decay_", 0)
    eps = opt_or("eps_", 1e-8)
    nesterov = opt_or("nesterov_", False)
    delta = opt_or("delta_", 0.1)
    wd_ratio = opt_or("wd_ratio_", 0.1)
    beta1 = opt_or("beta1_", 0.9)
    momentum = opt_or("momentum_", beta1)
    beta2 = opt_or("beta2_", 0.999)
    # FreezeD relies on "zero gradient history => zero update" (base_model._zero_frozen_grads): Ranger's lookahead and MADGRAD's
    # momentum average move a tensor whose gradients are all zero
    frozen = name == "D" and train_opt.get("freeze_loc", None)
    if optim == "adam":
        return FusedAdam(optim_params, lr=lr, weight_decay=wd, betas=(beta1, beta2))
    if optim == "sgd":
        return FusedSGD(optim_params, lr=lr, weight_decay=wd, momentum=momentum)
    if optim == "rmsprop":
        return FusedRMSprop(optim_params, lr=lr, weight_decay=wd, eps=eps)
    if optim == "sgdp":
        return FusedSGDP(optim_params, lr=lr, weight_decay=wd, momentum=momentum, dampening=opt_or("dampening_", 0), nesterov=nesterov,
                         eps=eps, delta=delta, wd_ratio=wd_ratio)
    if optim == "adamp":
        return FusedAdamP(optim_params, lr=lr, weight_decay=wd, betas=(beta1, beta2), nesterov=nesterov, eps=eps, delta=delta,
                          wd_ratio=wd_ratio)
    if optim == "ranger":
        if frozen:
            raise NotImplementedError("freeze_loc with optim_{}: ranger is not implemented by the HIP engine (the lookahead moves a "
                                      "frozen tensor)".format(name))
        if not opt_or("gc_loc_", True):
            raise NotImplementedError("gc_loc_{}: false is not implemented by the HIP engine".format(name))
        return FusedRanger(optim_params, lr=lr, weight_decay=wd, betas=(beta1, beta2), eps=eps, alpha=opt_or("alpha_", 0.5),
                           k=opt_or("k_", 6), N_sma_threshhold=opt_or("N_sma_threshhold_", 5), use_gc=opt_or("use_gc_", True),
                           gc_conv_only=opt_or("gc_conv_only_", False), gc_loc=True)
    if optim == "madgrad":
        if frozen and momentum != 0:
            raise NotImplementedError("freeze_loc with optim_{}: madgrad and momentum is not implemented by the HIP engine (the momentum "
                                      "average moves a frozen tensor)".format(name))
        return FusedMADGRAD(optim_params, lr=lr, eps=eps, momentum=momentum, weight_decay=wd, decay_type=opt_or("decay_type_", "AdamW"))
    raise NotImplementedError("optimizer [{}] is outside the SR hot path of the HIP engine".format(optim))
