"""Differentiable Augmentation of the discriminator's inputs, backed by the HIP kernels of csrc/diffaug.hip.

Keeps the reference's surface (codes/dataops/diffaug.py): `DiffAugment(x, policy='', channels_first=True)` over the policies `color`,
`translation`, `zoom`, `transl_zoom`, `flip`, `rotate` and `cutout`.  One call is one composite

    out = cutout_mask . Geo(Colour(x))

evaluated by one fused launch (two with `color`, whose contrast step needs the image mean), with a gather-form adjoint.  `draw` makes
the random parameters with the reference's distributions and generators -- per-image draws with `torch.rand` / `torch.randint` on the
device, batch-wide draws with the host's `random` / `np.random` in the reference's call order -- and `DiffAugment(..., params=...)`
replays a given record.  Everything the fused kernel's fixed order would change (`cutout` before `color`, ...) and everything outside it
(`offset*`, `channels_first=False`) raises NotImplementedError naming the value: there is no eager-PyTorch fallback.
"""
import random

import numpy as np
import torch

from .. import ops
from ..models.modules._dense import as_layout, dense_layout

KINDS = ("identity", "translation", "zoom_in", "zoom_out")
# the fixed order of the fused kernel: colour, one geometric map, flip, rotation, cutout
_RANK = {"color": 0, "translation": 1, "zoom": 1, "transl_zoom": 1, "flip": 2, "rotate": 3, "cutout": 4}
_CHOICES = {"zoom": ("zoom_in", "zoom_out"), "transl_zoom": ("translation", "zoom_in", "zoom_out")}
_REFUSED = ("offset", "offset_h", "offset_v")


def parse_policy(policy):
    """-> the policy's entries, checked: known names in the one order the kernel evaluates."""
    names = tuple(p for p in policy.split(",")) if policy else ()
    for p in names:
        if p in _REFUSED:
            raise NotImplementedError("DiffAugment policy '{}' is not implemented by the HIP engine".format(p))
        if p not in _RANK:
            raise KeyError("unknown DiffAugment policy '{}'".format(p))
    ranks = [_RANK[p] for p in names]
    if any(b <= a for a, b in zip(ranks, ranks[1:])):
        raise NotImplementedError("DiffAugment policy order '{}' is not implemented by the HIP engine: the fused kernel evaluates "
                                  "color, then one of translation / zoom / transl_zoom, then flip, rotate, cutout".format(policy))
    return names


def _half_up(v):
    return int(v + 0.5)


def _floating(t):
    t = torch.as_tensor(t)
    return t if t.dtype in (torch.float32, torch.float64) else t.float()


def cutout_size(H, W, ratio=0.5):
    return _half_up(H * ratio), _half_up(W * ratio)


class Params:
    """The draws of one DiffAugment call on an N x C x H x W batch.  Per-image fields are tensors of N elements (on the device they
    were drawn on) or None when the policy lacks the op; batch-wide fields are Python values."""

    def __init__(self, N, H, W, color=None, kind="identity", translation=None, zoom=None, flip=False, rot=0, cutout=None):
        if kind not in KINDS:
            raise ValueError("unknown geometric kind '{}'".format(kind))
        if rot not in (-1, 0, 1):
            raise ValueError("rotation must be 0, +1 or -1")
        if rot and H != W:
            raise NotImplementedError("DiffAugment policy 'rotate' needs square images (H = W), got {} x {}".format(H, W))
        self.N, self.H, self.W = int(N), int(H), int(W)
        self.color = None if color is None else tuple(_floating(t).reshape(-1) for t in color)   # b, sat, con (fp32 as drawn; fp64 kept)
        self.kind = kind
        self.translation = None if translation is None else tuple(torch.as_tensor(t).reshape(-1).to(torch.int32) for t in translation)   # ty, tx
        self.zoom = None if zoom is None else tuple(int(v) for v in zoom)   # zoom_in: h_delta, w_delta, new_h, new_w; zoom_out: left, right, top, bottom
        self.flip, self.rot = bool(flip), int(rot)
        self.cutout = None if cutout is None else tuple(torch.as_tensor(t).reshape(-1).to(torch.int32) for t in cutout)   # oy, ox
        if (kind == "translation") != (self.translation is not None) or (kind in ("zoom_in", "zoom_out")) != (self.zoom is not None):
            raise ValueError("geometric kind '{}' and its parameters do not match".format(kind))
        for group in (self.color, self.translation, self.cutout):
            for t in group or ():
                if t.numel() != self.N:
                    raise ValueError("per-image parameters must have N = {} elements".format(self.N))
        self._block = None

    def geo(self):
        """The 9 host integers the kernels take."""
        H, W = self.H, self.W
        offy = offx = inh = inw = 0
        if self.kind == "zoom_in":
            offy, offx, inh, inw = self.zoom
        elif self.kind == "zoom_out":
            left, right, top, bottom = self.zoom
            offy, offx, inh, inw = -top, -left, H + top + bottom, W + left + right
        return (KINDS.index(self.kind), int(self.flip), self.rot, offy, offx, inh, inw, int(self.color is not None),
                int(self.cutout is not None))

    def block(self, device):
        """The per-image parameter block on `device`: fp32 [N, 8] = {b, sat, con | int32 ty, tx, oy, ox, 0}.  Built once, without a
        host synchronisation when the draws already live on the device."""
        if self._block is None or self._block.device != torch.device(device):
            blk = torch.zeros(self.N, 8, dtype=torch.float32, device=device)
            ints = blk.view(torch.int32)
            if self.color is not None:
                blk[:, 0], blk[:, 1], blk[:, 2] = (t.to(device) for t in self.color)
            else:
                blk[:, 1:3] = 1.0
            if self.translation is not None:
                ints[:, 3], ints[:, 4] = (t.to(device) for t in self.translation)
            if self.cutout is not None:
                ints[:, 5], ints[:, 6] = (t.to(device) for t in self.cutout)
            self._block = blk
        return self._block


def draw(policy, N, H, W, device):
    """The draws of one call, with the reference's distributions, generators and call order."""
    names = parse_policy(policy)
    if "rotate" in names and H != W:
        raise NotImplementedError("DiffAugment policy 'rotate' needs square images (H = W), got {} x {}".format(H, W))
    kw = dict(kind="identity")
    for p in names:
        if p == "color":
            b = torch.rand(N, 1, 1, 1, dtype=torch.float32, device=device) - 0.5
            sat = torch.rand(N, 1, 1, 1, dtype=torch.float32, device=device) * 2
            con = torch.rand(N, 1, 1, 1, dtype=torch.float32, device=device) + 0.5
            kw["color"] = (b, sat, con)
        elif p in ("translation", "zoom", "transl_zoom"):
            kind = random.choice(_CHOICES[p]) if p in _CHOICES else p
            if kind == "translation":
                sy, sx = _half_up(H * 0.125), _half_up(W * 0.125)
                ty = torch.randint(-sy, sy + 1, size=[N, 1, 1], device=device)
                tx = torch.randint(-sx, sx + 1, size=[N, 1, 1], device=device)
                kw.update(kind=kind, translation=(ty, tx))
            elif kind == "zoom_in":
                scale = np.random.uniform(1.0, 2.0)
                if scale == 1:
                    continue
                new_h, new_w = int(H / scale), int(W / scale)
                h_delta = int(np.random.random() * (H - new_h))
                w_delta = int(np.random.random() * (W - new_w))
                kw.update(kind=kind, zoom=(h_delta, w_delta, new_h, new_w))
            else:
                scale = np.random.uniform(0.1, 1.0)
                rnd_h, rnd_w = int(H * scale / 2), int(W * scale / 2)
                rnd_n = np.random.uniform(-1.0, 1.0)
                disp_h, disp_w = int(rnd_n * rnd_h), int(rnd_n * rnd_w)
                kw.update(kind=kind, zoom=(rnd_w - disp_w, rnd_w + disp_w, rnd_h - disp_h, rnd_h + disp_h))
        elif p == "flip":
            kw["flip"] = bool(np.random.random() > 0.5)
        elif p == "rotate":
            if np.random.random() < 0.25:
                kw["rot"] = 1
            elif np.random.random() < 0.5:
                kw["rot"] = -1
        elif p == "cutout":
            ch, cw = cutout_size(H, W)
            oy = torch.randint(0, H + (1 - ch % 2), size=[N, 1, 1], device=device)
            ox = torch.randint(0, W + (1 - cw % 2), size=[N, 1, 1], device=device)
            kw["cutout"] = (oy, ox)
    return Params(N, H, W, **kw)


class _DiffAugFn(torch.autograd.Function):
    """out = mask . Geo(Colour(x)); backward gx = Colour^T(Geo^T(mask . g)) from the parameters alone (nothing of x is saved)."""

    @staticmethod
    def forward(ctx, x, prm):
        layout = dense_layout("DiffAugment", x)
        geo, blk = prm.geo(), prm.block(x.device)
        ws = ops.diffaug_mean(x, layout, blk, geo) if prm.color is not None else None
        out = torch.empty_like(x)
        ops.diffaug_fwd(x, layout, blk, geo, ws, out)
        ctx.cfg = (layout, geo, blk, prm.color is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        layout, geo, blk, color = ctx.cfg
        g = as_layout(g, layout)
        ws = ops.diffaug_mean(g, layout, blk, geo, backward=True) if color else None
        gx = torch.empty_like(g)
        ops.diffaug_bwd(g, layout, blk, geo, ws, gx)
        return gx, None


def DiffAugment(x, policy='', channels_first=True, params=None):
    """The reference's entry point.  `params=None` draws; a `Params` record (of `draw`, or built by hand) is replayed."""
    if not policy:
        return x
    if not channels_first:
        raise NotImplementedError("DiffAugment channels_first=False is not implemented by the HIP engine")
    names = parse_policy(policy)
    if x.dim() != 4:
        raise ValueError("DiffAugment takes N x C x H x W batches, got {} dimensions".format(x.dim()))
    N, C, H, W = x.shape
    if C > 4:
        raise NotImplementedError("DiffAugment on {} channels is not implemented by the HIP engine (at most 4)".format(C))
    if "rotate" in names and H != W:
        raise NotImplementedError("DiffAugment policy 'rotate' needs square images (H = W), got {} x {}".format(H, W))
    if x.dtype in (torch.float16, torch.bfloat16, torch.int8, torch.int32):          # as GeneratorLoss._fp32
        x = x.float()
    if params is None:
        params = draw(policy, N, H, W, x.device)
    elif (params.N, params.H, params.W) != (N, H, W):
        raise ValueError("DiffAugment: the parameter record is for {} x {} x {}, the batch is {} x {} x {}".format(
            params.N, params.H, params.W, N, H, W))
    return _DiffAugFn.apply(x, params)
