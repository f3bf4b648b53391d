"""Batch augmentations of the (target, input) pair of a training step (`mixup: true`, `mixopts`, `mixprob`, `mixalpha`, `aux_mixprob`,
`aux_mixalpha`, `mix_p`), backed by the HIP kernels of csrc/batchaug.hip.

Keeps the reference's surface (codes/dataops/batchaug.py): `BatchAugment(train_opt)` with `__call__(img1=target, img2=input)` and
`apply_mask(img1=generated, img2=target)`, and `BatchAug(img1, img2, options, probs, alphas, aux_prob, aux_alpha, mix_p)` over the ops
`none`, `blend`, `rgb`, `mixup`, `cutmix`, `cutmixup`, `cutblur` and `cutout`.  One call selects ONE op for the whole batch.  `draw`
makes the parameter record of a call with the reference's distributions, generators and call order (the host's `random` / `np.random`,
`torch.randperm` on the CPU, the device's `uniform_` for the colour of `blend`), including the draws the reference makes and discards;
`BatchAug(..., params=record)` replays a given record.

No op moves a pixel: every op but `cutout` is one `ops.batchaug_mix` launch per changed image (a box, a code for the region inside and
one for the region outside it; see csrc/batchaug.hip), `cutout` and `apply_mask` are `ops.batchaug_mask` launches, and the backward of
`apply_mask` is that launch again (the product with a 0/1 mask is its own adjoint; only the mask is saved).

A miss (`random.random() >= prob`, or `alpha <= 0`), `none`, and the image an op leaves alone (`cutblur`'s and `cutout`'s target) issue NO
launch: the very tensors that came in are returned, where the reference returns clones.  That is safe here because nothing downstream
writes them in place: the models hand them to the networks, the losses and the discriminator, all of which only read their inputs
(the feed's slots are rewritten by the NEXT `feed_data`, as without `mixup`).  Half-precision inputs are promoted to fp32, as
`DiffAugment` does.  There is no eager-PyTorch fallback: without a device a hit raises `HipEngineError`.
"""
import hashlib
import random

import numpy as np
import torch

from .. import ops
from ..models.modules._dense import as_layout, dense_layout

OPS = ("none", "blend", "rgb", "mixup", "cutmix", "cutmixup", "cutblur", "cutout")
SELF, PARTNER, LERP_PARTNER, LERP_COLOUR = 0, 1, 2, 3          # the region codes of tnr_batchaug_mix

DEFAULT_MIXOPTS = ["blend", "rgb", "mixup", "cutmix", "cutmixup", "cutout"]
DEFAULT_MIXPROB = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
DEFAULT_MIXALPHA = [0.6, 1.0, 1.2, 0.7, 0.7, 0.001]


def check_options(options, probs, alphas, aux_alpha=None, mix_p=None):
    """What the reference would only trip over in the middle of a run, refused with the value named."""
    options = list(options)
    if not options:
        raise ValueError("mixopts is empty")
    for name in options:
        if name not in OPS:
            raise ValueError("unknown batch augmentation '{}' in mixopts (known: {})".format(name, ", ".join(OPS)))
    if len(probs) < len(options):
        raise ValueError("mixprob {} has fewer entries than mixopts {}".format(list(probs), options))
    if len(alphas) < len(options):
        raise ValueError("mixalpha {} has fewer entries than mixopts {}".format(list(alphas), options))
    if mix_p is not None:
        if len(mix_p) != len(options):
            raise ValueError("mix_p {} must have one entry per mixopts entry ({})".format(list(mix_p), len(options)))
        if abs(float(np.sum(np.asarray(mix_p, dtype=np.float64))) - 1.0) > 1e-8 or min(mix_p) < 0:
            raise ValueError("mix_p {} must be probabilities that sum to 1".format(list(mix_p)))
    if "cutmixup" in options and (aux_alpha is None or float(aux_alpha) <= 0):
        raise ValueError("aux_mixalpha {} must be positive with 'cutmixup' in mixopts (it is the Beta distribution's parameter)".format(
            aux_alpha))


def pair_scale(shape1, shape2):
    """scale = img1.size(2) // img2.size(2), for a pair whose sizes are exact multiples of each other."""
    if len(shape1) != 4 or len(shape2) != 4:
        raise ValueError("batch augmentations take N x C x H x W batches, got {} and {} dimensions".format(len(shape1), len(shape2)))
    (N1, _, H1, W1), (N2, _, H2, W2) = shape1, shape2
    s = H1 // H2 if H2 else 0
    if N1 != N2 or s < 1 or H2 * s != H1 or W2 * s != W1:
        raise ValueError("batch augmentations need a target whose size is an exact multiple of the input's (one factor for both axes, "
                         "same batch), got {} and {}".format(tuple(shape1), tuple(shape2)))
    return s


class Params:
    """The draws of one BatchAug call on a target N x C x (s h) x (s w) and an input N x C x h x w.  `hit` is False for a miss (and
    for `none`): nothing but `aug` (and, for `cutout`, the all-ones `mask`) is meaningful then.
        v        the blend factor (`blend`), lambda (`mixup`) or the auxiliary mixup's factor (`cutmixup`)
        colour   `blend`: fp32 N x 3 (as drawn: on the device of the call)
        perm     `rgb`: out[:, c] = in[:, perm[c]]
        r        `mixup` / `cutmix` / `cutmixup`: the batch permutation, a list of N
        box      (y0, x0, bh, bw) on the INPUT image (the target's is s times that), already clipped the way the reference's
                 slices clip
        coin     `cutmixup` / `cutblur`: np.random.random() > 0.5
        aux_hit  `cutmixup`: the auxiliary mixup applies (else the partner itself is pasted)
        mask     `cutout`: uint8 numpy N x h x w"""

    def __init__(self, aug, hit, N, h, w, scale, v=None, colour=None, perm=None, r=None, box=None, coin=None, aux_hit=None, mask=None):
        if aug not in OPS:
            raise ValueError("unknown batch augmentation '{}'".format(aug))
        self.aug, self.hit = aug, bool(hit)
        self.N, self.h, self.w, self.scale = int(N), int(h), int(w), int(scale)
        self.v = None if v is None else float(v)
        self.colour = colour
        self.perm = None if perm is None else tuple(int(p) for p in perm)
        self.r = None if r is None else [int(i) for i in r]
        self.box = None if box is None else tuple(int(b) for b in box)
        self.coin = None if coin is None else bool(coin)
        self.aux_hit = None if aux_hit is None else bool(aux_hit)
        self.mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.N, self.h, self.w)
        if self.r is not None and sorted(self.r) != list(range(self.N)):
            raise ValueError("r {} is no permutation of the {} images".format(self.r, self.N))
        if self.box is not None:
            y0, x0, bh, bw = self.box
            if min(self.box) < 0 or y0 + bh > self.h or x0 + bw > self.w:
                raise ValueError("box {} leaves the {} x {} input image".format(self.box, self.h, self.w))
        self._dev = {}

    def key(self):
        """What identifies the record (tests compare these)."""
        col = None if self.colour is None else [float(c) for c in torch.as_tensor(self.colour).reshape(-1).cpu()]
        return (self.aug, self.hit, self.N, self.h, self.w, self.scale, self.v, col, self.perm, self.r, self.box, self.coin, self.aux_hit,
                None if self.mask is None else hashlib.sha256(self.mask.tobytes()).hexdigest())

    def on_device(self, what, device):
        """r (int32), colour (fp32 N x 3) or mask (uint8 N x 1 x h x w) on `device`, uploaded once from pinned memory without a host
        synchronisation."""
        k = (what, str(device))
        if k not in self._dev:
            if what == "colour":
                t = torch.as_tensor(self.colour).reshape(self.N, 3).to(torch.float32)
            elif what == "r":
                t = torch.tensor(self.r, dtype=torch.int32)
            else:
                t = torch.from_numpy(self.mask).reshape(self.N, 1, self.h, self.w)
            if t.device != torch.device(device):
                if not t.is_cuda and torch.device(device).type == "cuda":
                    t = t.pin_memory()
                t = t.to(device, non_blocking=True)
            self._dev[k] = t.contiguous()
        return self._dev[k]


def _box(fcy, fcx, ch, cw, h, w):
    """The pixels the reference's slices [fcy:fcy+ch, fcx:fcx+cw] name in an h x w image (a negative size wraps, as Python slices do)."""
    ya, yb, _ = slice(fcy, fcy + ch).indices(h)
    xa, xb, _ = slice(fcx, fcx + cw).indices(w)
    return ya, xa, max(0, yb - ya), max(0, xb - xa)


def _draw_cutmix(prob, alpha, N, h, w):
    """_cutmix of the reference: None on a miss, else (box, r)."""
    if alpha <= 0 or random.random() >= prob:
        return None
    cut_ratio = np.random.randn() * 0.01 + alpha
    ch, cw = int(h * cut_ratio), int(w * cut_ratio)
    fcy = np.random.randint(0, h - ch + 1)
    fcx = np.random.randint(0, w - cw + 1)
    r = torch.randperm(N)
    return _box(int(fcy), int(fcx), ch, cw, h, w), [int(i) for i in r]


def draw(options, probs, alphas, aux_prob, aux_alpha, mix_p, shape1, shape2, device):
    """The parameter record of one call on images of `shape1` (target) and `shape2` (input): the reference's draws in its call order."""
    scale = pair_scale(shape1, shape2)
    N, C, h, w = shape2
    idx = np.random.choice(len(options), p=mix_p)
    aug = options[idx]
    prob, alpha = float(probs[idx]), float(alphas[idx])
    kw = dict(N=N, h=h, w=w, scale=scale)
    if aug == "none":
        return Params(aug, False, **kw)
    if aug == "blend":
        if alpha <= 0 or random.random() >= prob:
            return Params(aug, False, **kw)
        if C != 3 or shape1[1] != 3:
            raise NotImplementedError("batch augmentation 'blend' needs 3 channels (its colour has three), got {} and {}".format(
                shape1[1], C))
        c = torch.empty((N, 3, 1, 1), device=device).uniform_(0, 1.0)
        v = np.random.uniform(alpha, 1)
        return Params(aug, True, v=v, colour=c.reshape(N, 3), **kw)
    if aug == "rgb":
        if random.random() >= prob:
            return Params(aug, False, **kw)
        return Params(aug, True, perm=np.random.permutation(C), **kw)
    if aug == "mixup":
        if alpha <= 0 or random.random() >= prob:
            return Params(aug, False, **kw)
        lam = np.random.beta(alpha, alpha)
        return Params(aug, True, v=lam, r=torch.randperm(N), **kw)
    if aug == "cutout":
        if alpha <= 0 or random.random() >= prob:
            return Params(aug, False, mask=np.ones((N, h, w), dtype=np.uint8), **kw)
        m = np.random.choice([0.0, 1.0], size=(N, 1, h, w), p=[alpha, 1 - alpha])
        return Params(aug, True, mask=np.asarray(m).astype(np.uint8), **kw)
    if aug == "cutmix":
        c = _draw_cutmix(prob, alpha, N, h, w)
        if c is None:
            return Params(aug, False, **kw)
        return Params(aug, True, box=c[0], r=c[1], **kw)
    if aug == "cutmixup":
        c = _draw_cutmix(prob, alpha, N, h, w)
        if c is None:
            return Params(aug, False, **kw)
        v = np.random.beta(aux_alpha, aux_alpha)          # drawn before the auxiliary coin, used or not
        aux_hit = not (aux_alpha <= 0 or random.random() >= aux_prob)
        coin = np.random.random() > 0.5
        return Params(aug, True, box=c[0], r=c[1], v=v, aux_hit=aux_hit, coin=coin, **kw)
    if aug == "cutblur":
        if tuple(shape1) != tuple(shape2):
            raise ValueError("batch augmentation 'cutblur': img1 and img2 have to be the same resolution, got {} and {}".format(
                tuple(shape1), tuple(shape2)))
        if alpha <= 0 or random.random() >= prob:
            return Params(aug, False, **kw)
        cut_ratio = np.random.randn() * 0.01 + alpha
        ch, cw = int(h * cut_ratio), int(w * cut_ratio)
        cy = np.random.randint(0, h - ch + 1)
        cx = np.random.randint(0, w - cw + 1)
        coin = np.random.random() > 0.5
        return Params(aug, True, box=_box(int(cy), int(cx), ch, cw, h, w), coin=coin, **kw)
    raise ValueError("{} is not invalid.".format(aug))          # (the reference's wording)


def _fp32(t):
    return t.float() if t.dtype in (torch.float16, torch.bfloat16) else t


def _mix(x, inside, outside, box=(0, 0, 0, 0), a=1.0, b=0.0, perm=None, x2=None, r=None, col=None):
    """One tnr_batchaug_mix launch -> a new tensor in x's dense layout."""
    layout = dense_layout("BatchAug", x) if x2 is None else dense_layout("BatchAug", x, x2)
    C = x.shape[1]
    p = list(perm) if perm is not None else list(range(C))
    out = torch.empty_like(x)
    ops.batchaug_mix(x, layout, [inside, outside] + list(box) + (p + [0, 0, 0, 0])[:4], a, b, out, x2=x2, r=r, col=col)
    return out


def mask_mul(x, mask, s):
    """x * mask[n, y // s, x // s] (one launch) -> a new tensor in x's dense layout.  mask: uint8 N x 1 x h x w on x's device."""
    layout = dense_layout("BatchAug mask", x)
    out = torch.empty_like(x)
    ops.batchaug_mask(x, layout, mask, s, out)
    return out


class _MaskFn(torch.autograd.Function):
    """out = mask . x; backward gx = mask . g: the same launch, and only the mask is saved."""

    @staticmethod
    def forward(ctx, x, mask, s):
        ctx.cfg = (dense_layout("BatchAug mask", x), mask, s)
        return mask_mul(x, mask, s)

    @staticmethod
    def backward(ctx, g):
        layout, mask, s = ctx.cfg
        return mask_mul(as_layout(_fp32(g), layout), mask, s), None, None


def _check_images(img1, img2):
    scale = pair_scale(img1.shape, img2.shape)
    for t in (img1, img2):
        if t.shape[1] > 4:
            raise NotImplementedError("batch augmentations on {} channels are not implemented by the HIP engine (at most 4)".format(
                t.shape[1]))
    if img1.shape[1] != img2.shape[1]:
        raise ValueError("batch augmentations need target and input with the same channels, got {} and {}".format(
            img1.shape[1], img2.shape[1]))
    return scale


def apply(prm, img1, img2):
    """The images of a parameter record: (img1_aug, img2_aug, mask) with mask the uint8 N x 1 x h x w device tensor of `cutout`."""
    scale = _check_images(img1, img2)
    N, C, h, w = img2.shape
    if (prm.N, prm.h, prm.w, prm.scale) != (N, h, w, scale):
        raise ValueError("BatchAug: the parameter record is for {} images of {} x {} at scale {}, the pair has {} of {} x {} at scale {}"
                         .format(prm.N, prm.h, prm.w, prm.scale, N, h, w, scale))
    aug, dev = prm.aug, img2.device
    if aug == "cutout":
        mask = prm.on_device("mask", dev)
        if not prm.hit:
            return img1, img2, mask
        return img1, mask_mul(_fp32(img2), mask, 1), mask
    if not prm.hit:
        return img1, img2, None
    img1, img2 = _fp32(img1), _fp32(img2)
    if aug == "blend":
        if C != 3:
            raise NotImplementedError("batch augmentation 'blend' needs 3 channels (its colour has three), got {}".format(C))
        col = prm.on_device("colour", dev)
        a, b = prm.v, 1.0 - prm.v
        return tuple(_mix(t, LERP_COLOUR, LERP_COLOUR, a=a, b=b, col=col) for t in (img1, img2)) + (None,)
    if aug == "rgb":
        if len(prm.perm) != C:
            raise ValueError("rgb: the permutation {} is not over {} channels".format(prm.perm, C))
        return tuple(_mix(t, SELF, SELF, perm=prm.perm) for t in (img1, img2)) + (None,)
    if aug == "cutblur":
        if img1.shape != img2.shape:
            raise ValueError("batch augmentation 'cutblur': img1 and img2 have to be the same resolution, got {} and {}".format(
                tuple(img1.shape), tuple(img2.shape)))
        inside, outside = (PARTNER, SELF) if prm.coin else (SELF, PARTNER)
        return img1, _mix(img2, inside, outside, box=prm.box, x2=img1), None
    r = prm.on_device("r", dev)
    if aug == "mixup":
        inside = outside = LERP_PARTNER
        a, b, box = prm.v, 1.0 - prm.v, (0, 0, 0, 0)
    elif aug == "cutmix":
        inside, outside, a, b, box = PARTNER, SELF, 1.0, 0.0, prm.box
    else:          # cutmixup
        m = LERP_PARTNER if prm.aux_hit else PARTNER
        a, b = (prm.v, 1.0 - prm.v) if prm.aux_hit else (1.0, 0.0)
        inside, outside = (m, SELF) if prm.coin else (SELF, m)
        box = prm.box
    out = []
    for t, s in ((img1, scale), (img2, 1)):
        out.append(_mix(t, inside, outside, box=tuple(v * s for v in box), a=a, b=b, x2=t, r=r))
    return out[0], out[1], None


def BatchAug(img1, img2, options, probs, alphas, aux_prob=None, aux_alpha=None, mix_p=None, params=None):
    """Mixture of Batch Augmentations: one op for the whole batch.  -> (img1_aug, img2_aug, mask, aug) as the reference; `mask` is the
    INPUT-sized uint8 N x 1 x h x w mask of `cutout` (the reference keeps its nearest x scale float copy; here `apply_mask` reads the
    small one at scale).  `params`: a `Params` record to replay instead of drawing."""
    if params is None:
        _check_images(img1, img2)
        params = draw(options, probs, alphas, aux_prob, aux_alpha, mix_p, tuple(img1.shape), tuple(img2.shape), img2.device)
    img1_aug, img2_aug, mask = apply(params, img1, img2)
    return img1_aug, img2_aug, mask, params.aug


class BatchAugment:
    def __init__(self, train_opt):
        self.mixopts = train_opt.get("mixopts", list(DEFAULT_MIXOPTS))
        self.mixprob = train_opt.get("mixprob", list(DEFAULT_MIXPROB))
        self.mixalpha = train_opt.get("mixalpha", list(DEFAULT_MIXALPHA))
        self.aux_mixprob = train_opt.get("aux_mixprob", 1.0)
        self.aux_mixalpha = train_opt.get("aux_mixalpha", 1.2)
        self.mix_p = train_opt.get("mix_p", None)
        check_options(self.mixopts, self.mixprob, self.mixalpha, self.aux_mixalpha, self.mix_p)
        self.aug = None
        self.mask = None
        self.params = None          # the record of the last call

    def __call__(self, img1, img2, params=None):
        """Apply the configured augmentations.  img1: the target image, img2: the input image."""
        if params is None:
            _check_images(img1, img2)
            params = draw(self.mixopts, self.mixprob, self.mixalpha, self.aux_mixprob, self.aux_mixalpha, self.mix_p,
                          tuple(img1.shape), tuple(img2.shape), img2.device)
        img1_aug, img2_aug, self.mask, self.aug = BatchAug(img1, img2, self.mixopts, self.mixprob, self.mixalpha, self.aux_mixprob,
                                                           self.aux_mixalpha, self.mix_p, params=params)
        self.params = params
        return img1_aug, img2_aug

    def apply_mask(self, img1, img2):
        """cutout-ed pixels are discarded when calculating the loss: generated (img1) and target (img2) are multiplied by the kept
        mask at their own scale -- also after a miss, when the mask is all ones, as in the reference.  Any other op returns its
        arguments."""
        if self.aug != "cutout":
            return img1, img2
        out = []
        for t in (img1, img2):
            s = pair_scale(t.shape, self.mask.shape)
            t = _fp32(t)
            out.append(_MaskFn.apply(t, self.mask, s) if t.requires_grad else mask_mul(t, self.mask, s))
        return out[0], out[1]
