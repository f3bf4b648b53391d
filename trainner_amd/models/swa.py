"""Stochastic weight averaging on the MI355X engine -- the drop-in for codes/models/swa.py.

`get_swa` returns the reference's pair: torch's own `SWALR` on the fused optimiser (the param groups gain `swa_lr`, `.state` files
stay interchangeable) and the averaged model.  The reference's averaged model is `AveragedModel(netG)`, a deep copy updated
tensor by tensor; here it is ONE flat fp32 buffer laid out like the generator's `FlatParams.flat` and one launch per update
(ops.swa_update), with `AveragedModel`'s state_dict: `n_averaged` first, then `module.<key>` in the network's own key order.
"""
from collections import OrderedDict

import torch
from torch.optim.swa_utils import SWALR

from .. import ops


class FlatAveragedModel:
    """The running mean of a HIP-engine network's parameters (AveragedModel with `use_buffers=False`: parameters are averaged,
    non-parameter buffers are kept equal to the source network's as of the last update).  Before the first update it holds the
    network's parameters at construction, like the deep copy AveragedModel makes."""

    def __init__(self, net):
        holder = net.flat_params()
        self._layout = self._layout_of(holder)
        self._names = OrderedDict()          # state_dict key of the network -> (offset, numel, shape) of a parameter, None for a buffer
        where = {id(p): (o, n) for p, o, n in holder.offsets}
        params = dict(net.named_parameters())
        for k, v in net.state_dict().items():
            self._names[k] = where[id(params[k])] + (tuple(v.shape),) if k in params else None
        self.flat = holder.flat.detach().clone()
        self.buffers = OrderedDict((k, v.detach().clone()) for k, v in net.state_dict().items() if self._names[k] is None)
        self.n_averaged = torch.zeros((), dtype=torch.int64, device=self.flat.device)
        self._n = 0                          # host copy of n_averaged: the launch's weight is formed without a device read

    @staticmethod
    def _layout_of(holder):
        return holder.total, tuple((o, n) for _, o, n in holder.offsets)

    def _holder(self, net):
        holder = net.flat_params()
        if self._layout_of(holder) != self._layout or holder.flat.device != self.flat.device:
            raise RuntimeError("the generator's flat parameter buffer was re-laid after the SWA model was built")
        return holder

    def resync(self):
        """After n_averaged was written on the device (data-parallel broadcast): refresh the host copy."""
        self._n = int(self.n_averaged.item())

    @torch.no_grad()
    def update_parameters(self, net):
        holder = self._holder(net)
        ops.swa_update(self.flat, holder.flat, self._n)
        for k, b in self.buffers.items():
            b.copy_(net.state_dict()[k])
        self._n += 1
        self.n_averaged += 1

    def state_dict(self):
        out = OrderedDict(n_averaged=self.n_averaged)
        for k, where in self._names.items():
            out["module." + k] = self.buffers[k] if where is None else self.flat[where[0]:where[0] + where[1]].view(where[2])
        return out

    @torch.no_grad()
    def load_state_dict(self, state_dict, strict=True):
        own = self.state_dict()
        missing, unexpected = [k for k in own if k not in state_dict], [k for k in state_dict if k not in own]
        bad = [k for k in own if k in state_dict and tuple(state_dict[k].shape) != tuple(own[k].shape)]
        if bad or (strict and (missing or unexpected)):
            raise RuntimeError("Error(s) in loading state_dict for FlatAveragedModel: missing %s, unexpected %s, size mismatch %s"
                               % (missing, unexpected, bad))
        for k, v in own.items():
            if k in state_dict:
                v.copy_(state_dict[k])
        self.resync()


def get_swa(optimizer, model, swa_lr=0.005, anneal_epochs=10, anneal_strategy="cos"):
    """-> (swa_scheduler, swa_model), swa.py:4-23."""
    swa_model = FlatAveragedModel(model)
    swa_scheduler = SWALR(optimizer, swa_lr=swa_lr, anneal_epochs=anneal_epochs, anneal_strategy=anneal_strategy)
    return swa_scheduler, swa_model
