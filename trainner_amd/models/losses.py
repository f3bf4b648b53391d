"""Loss builders of the SR training path, backed by HIP kernels.

Keeps the reference's surface (codes/models/losses.py): `get_loss_fn` -> {'name','weight','function'},
`PerceptualLoss` (:220-340), `Adversarial` (:343-604) and `GeneratorLoss` (:607-962) with the same
option keys, loss names (`pix-l1`, `fea-vgg19-l1`) and weighting order, restricted to the branches the
ESRGAN recipe uses (options/sr/train_sr.yml:107-110,145-146): L1 pixel loss, the VGG L1 perceptual
loss over any dictionary of layers (`perceptual_opt.perceptual_layers`) and the Gram-matrix style loss
(`style_weight`, `perceptual_opt.style_layers`; csrc/gram.hip), vanilla relativistic GAN, plus the SSIM / MS-SSIM term of the "precise" list
(`ssim_type` / `ssim_weight`, losses.py:798-802) and the recipe's edge / smoothness terms
(train_sr.yml:114-120): the difference-only pixel criteria l2, cb, elastic and clipl1, HFEN (`hfen_criterion` /
`hfen_weight`), total variation (`tv_type` / `tv_norm` / `tv_weight`) and the image-gradient loss of the precise list
(`grad_type` / `grad_weight`), and the first two experimental terms (train_sr.yml "Experimental losses"): the spatial profile losses
(`spl_type: spl | cpl | gpl` / `spl_weight`), the overflow loss (`of_type: overflow` / `of_weight`) and the colour, averaging-downscale
and multi-scale pixel losses (`color_criterion: color-<crit>` / `color_weight`, `avg_criterion: avg-<crit>` / `avg_weight`,
`ms_criterion: multiscale-<crit>` / `ms_weight`, <crit> one of l1, l2, cb, elastic, clipl1, l1cosinesim).  With frequency separation (`fs`, base_model.setup_fs) `GeneratorLoss` hands the low-passed images to
the colour / content terms and `Adversarial` shows the discriminator the high-pass residual (dataops/filters.py).  Anything else
raises NotImplementedError (no silent fallback to eager PyTorch).
"""
import torch
import torch.nn as nn

from .. import hip, ops
from ..dataops import diffaug as diffaug_ops
from ..dataops import filters
from . import networks
from .modules import image_losses as IL
from .modules import pooled_losses as PL
from .modules import spl as SPL
from .modules._dense import dense_layout, gscale
from .modules.ssim import MS_SSIM, SSIM


# ----------------------------------------------------------------------------------------------
# HIP-backed criteria
# ----------------------------------------------------------------------------------------------
class _L1MeanFn(torch.autograd.Function):
    """mean(|a - b|): nn.L1Loss(reduction='mean') (losses.py:37-39).  b carries no gradient."""

    @staticmethod
    def forward(ctx, a, b):
        dense_layout("L1", a, b, any_rank=True)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ops.l1_mean_fwd(a, b, 1.0, out)
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga = torch.empty_like(a)          # preserves a's (possibly channels-last) strides
        ops.l1_mean_bwd(a, b, 1.0, gscale(g), ga)
        return ga, None


class _GramFn(torch.autograd.Function):
    """GramMatrix(out_norm='ci') (modules/loss.py:479-506): gram[n] = F F^T / (C H W) for F = the feature map as a C x HW matrix.
    `fea` is a logical NCHW tensor over NHWC storage, as the FeatureExtractor hands it out.  The kernels read the fp32 activations and
    run in the TNR_MMA arithmetic with or without `use_amp`: stricter than the reference, whose autocast runs this product in half
    precision."""

    @staticmethod
    def forward(ctx, fea):
        hip.require_device(fea)
        N, C, H, W = fea.shape
        x = fea.detach().permute(0, 2, 3, 1)
        x = ops.View(x if x.is_contiguous() else x.contiguous())
        G = torch.empty((N, C, C), dtype=torch.float32, device=fea.device)
        ctx.scale = 1.0 / (C * H * W)
        ops.gram_fwd(x, ctx.scale, G)
        ctx.save_for_backward(x.buf)
        return G

    @staticmethod
    def backward(ctx, S):
        (xb,) = ctx.saved_tensors
        dx = torch.empty_like(xb)
        ops.gram_bwd(ops.View(xb), S.contiguous(), ctx.scale, ops.View(dx))
        return dx.permute(0, 3, 1, 2)


class L1Loss(nn.Module):
    def __init__(self, reduction="mean"):
        super().__init__()
        if reduction != "mean":
            raise NotImplementedError("only reduction='mean' is implemented by the HIP engine")

    def forward(self, x, y):
        return _L1MeanFn.apply(x, y.detach())


class _RaGANFn(torch.autograd.Function):
    """Relativistic average BCE-with-logits (GANLoss 'vanilla', modules/loss.py:85-86,120-137) in
    the generator (losses.py:428-433) or discriminator (losses.py:503-512) form.  Returns a 5-vector:
    [weight*(l1+l2)/2, l1, l2, mean(pred_real), mean(pred_fake)].  With a DataParallel group the two
    batch means and the two coupling sums are all-reduced between the kernel phases, so every rank
    sees the GLOBAL-batch relativistic means the reference computes on GPU 0."""

    @staticmethod
    def forward(ctx, pred_fake, pred_real, stage, weight, group):
        hip.require_device(pred_fake)
        pf, pr = pred_fake.contiguous().view(-1), pred_real.contiguous().view(-1)
        dev = pf.device
        sums = torch.empty(8, dtype=torch.float32, device=dev)
        out = torch.empty(5, dtype=torch.float32, device=dev)
        gf = torch.empty_like(pf)
        gr = torch.empty_like(pr)
        ops.ragan_phase_a(pf, pr, sums)
        if group is not None:
            group.all_reduce_sum(sums[0:3])
        ops.ragan_phase_b(pf, pr, stage, sums)
        if group is not None:
            group.all_reduce_sum(sums[3:7])
        ops.ragan_phase_c(pf, pr, stage, weight, sums, out, gf, gr)
        ctx.save_for_backward(gf, gr)
        ctx.shapes = (pred_fake.shape, pred_real.shape)
        ctx.world = 1 if group is None else group.world_size
        return out

    @staticmethod
    def backward(ctx, g):
        gf, gr = ctx.saved_tensors
        g0 = g[0:1].contiguous()
        if ctx.world > 1:
            # every rank back-propagates the global-mean loss; gradient averaging over ranks (dp.py)
            # then divides by world, so pre-multiply to keep d(global loss)/d(local sample) exact
            g0 = g0 * float(ctx.world)
        of = torch.empty_like(gf)
        ops.scale_by(of, gf, g0)
        orr = None
        if ctx.needs_input_grad[1]:
            orr = torch.empty_like(gr)
            ops.scale_by(orr, gr, g0)
            orr = orr.view(ctx.shapes[1])
        return of.view(ctx.shapes[0]), orr, None, None, None


class _GanLabelFn(torch.autograd.Function):
    """GANLoss against a constant label (modules/loss.py:85-88,112-137): mean BCE-with-logits ('vanilla', kind 0) or mean
    squared error ('lsgan', kind 1) of the discriminator's logit map against `target` (1.0 real / 0.0 fake).  One launch
    produces the loss and d loss / d pred (tnr_gan_loss)."""

    @staticmethod
    def forward(ctx, pred, kind, target):
        hip.require_device(pred)
        p = pred.contiguous().view(-1)
        out = torch.empty(1, dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        ops.gan_loss(p, kind, target, out, grad)
        ctx.save_for_backward(grad)
        ctx.shape = pred.shape
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        of = torch.empty_like(grad)
        ops.scale_by(of, grad, g.reshape(1).contiguous())
        return of.view(ctx.shape), None, None


class _CatChannelsFn(torch.autograd.Function):
    """torch.cat((a, b), 1) of two NCHW image batches for the conditional discriminator input (losses.py:445-455,
    522-530): two strided device copies into one buffer; backward hands each operand its channel slice."""

    @staticmethod
    def forward(ctx, a, b):
        out = torch.empty((a.shape[0], a.shape[1] + b.shape[1]) + tuple(a.shape[2:]), dtype=a.dtype, device=a.device)
        out[:, :a.shape[1]].copy_(a)
        out[:, a.shape[1]:].copy_(b)
        ctx.ca = a.shape[1]
        return out

    @staticmethod
    def backward(ctx, g):
        ga = g[:, :ctx.ca].contiguous() if ctx.needs_input_grad[0] else None
        gb = g[:, ctx.ca:].contiguous() if ctx.needs_input_grad[1] else None
        return ga, gb


# ----------------------------------------------------------------------------------------------
# builders
# ----------------------------------------------------------------------------------------------
def get_loss_fn(loss_type=None, weight=0, recurrent=False, reduction="mean", network=None, device="cuda", opt=None,
                allow_featnets=True):
    """Same contract as the reference (losses.py:23-171): returns the criterion itself when
    `recurrent`, else {'name', 'weight', 'function'}."""
    if loss_type in ("L1", "l1"):
        loss_function = L1Loss(reduction=reduction)
        loss_type = "pix-{}".format(loss_type)
    elif loss_type in ("MSE", "l2", "cb", "elastic", "clipl1"):
        loss_function = IL.criterion(loss_type, reduction)
        loss_type = "pix-{}".format(loss_type)
    elif loss_type is not None and loss_type.find("multiscale") >= 0:
        # losses.py:59-64: multiscale-<criterion>, named as a pixel loss (so frequency separation hands it the low-passed pair)
        loss_function = PL.MultiscalePixelLoss(loss_f=PL.inner_criterion(_inner_name(loss_type)))
        loss_type = "pix-{}".format(loss_type)
    elif loss_type is not None and loss_type.find("hfen") >= 0:
        # losses.py:86-92: the criterion is asked for with reduction='sum' (cb and clipl1 ignore it and stay means)
        loss_function = IL.HFENLoss(loss_f=IL.criterion(loss_type.split("-")[1], "sum"))
    elif loss_type is not None and loss_type.find("grad") >= 0:
        parts = loss_type.split("-")            # grad-2d-<criterion> | grad-4d-<criterion> (losses.py:93-99)
        if len(parts) != 3:
            raise NotImplementedError("Loss type [{}] is not implemented by the HIP engine".format(loss_type))
        loss_function = IL.GradientLoss(loss_f=IL.criterion(parts[2]), gradientdir=parts[1])
    elif loss_type in ("gpl", "cpl"):
        # losses.py:100-110: both read datasets.train.znorm
        z_norm = (((opt or {}).get("datasets") or {}).get("train") or {}).get("znorm", False)
        loss_function = (SPL.GPLoss(spl_denorm=z_norm) if loss_type == "gpl" else
                         SPL.CPLoss(rgb=True, yuv=True, yuvgrad=True, spl_denorm=z_norm, yuv_denorm=z_norm))
    elif loss_type == "overflow":
        loss_function = SPL.OFLoss()            # losses.py:140-141
    elif loss_type is not None and loss_type.find("tv") >= 0:
        parts = loss_type.split("-")            # tv-l1 | tv-l2 | dtv-l1 | dtv-l2 (losses.py:111-116)
        if len(parts) != 2 or parts[0] not in ("tv", "dtv") or parts[1] not in ("l1", "l2"):
            raise NotImplementedError("Loss type [{}] is not implemented by the HIP engine".format(loss_type))
        loss_function = IL.TVLoss(tv_type=parts[0], p=parts[1])
    elif loss_type is not None and loss_type.find("fea") >= 0:
        parts = loss_type.split("-")
        if parts[1] == "lpips":
            raise NotImplementedError("LPIPS is outside the SR hot path of the HIP engine")
        if parts[2] not in ("L1", "l1"):
            raise NotImplementedError("feature criterion [{}] is not implemented by the HIP engine (l1 only)".format(parts[2]))
        fea_loss_f = get_loss_fn(parts[2], recurrent=True, reduction="mean", device=device)
        network = networks.define_F(opt).to(device)
        loss_function = PerceptualLoss(criterion=fea_loss_f, network=network, opt=opt)
    elif loss_type == "contextual":
        # losses.py:129-135; the feature network's weights resolve as networks.define_F's do
        from .modules.contextual import Contextual_Loss
        layers = opt["train"].get("cx_vgg_layers", {"conv3_2": 1.0, "conv4_2": 1.0})
        z_norm = opt["datasets"]["train"].get("znorm", False)
        loss_function = Contextual_Loss(layers, max_1d_size=64, distance_type="cosine", calc_type="regular", z_norm=z_norm,
                                        load_path=(opt["train"].get("perceptual_opt") or {}).get("pretrained_path", None),
                                        allow_random_init=bool(opt["train"].get("perceptual_allow_random_init")))
    elif loss_type in ("ssim", "SSIM", "ms-ssim", "MSSSIM"):
        # losses.py:70-85; `opt` is the train block here (losses.py:799-801)
        image_channels = ((opt or {}).get("image_channels") or 3) if allow_featnets else 1
        kw = dict(window_size=11, window_sigma=1.5, size_average=True, data_range=1., channels=image_channels)
        loss_function = SSIM(**kw) if loss_type in ("ssim", "SSIM") else MS_SSIM(normalize="relu", **kw)
    elif loss_type is not None and (loss_type.find("color") >= 0 or loss_type.find("avg") >= 0):
        # losses.py:146-155: color-<criterion> | avg-<criterion> on the AvgPool2d(kernel_size=opt['scale']) images
        if not (opt or {}).get("scale"):
            raise ValueError("Loss type [{}] needs the model's `scale` option for its pool".format(loss_type))
        cls = PL.ColorLoss if loss_type.find("color") >= 0 else PL.AverageLoss
        loss_function = cls(loss_f=PL.inner_criterion(_inner_name(loss_type)), ds_f=nn.AvgPool2d(kernel_size=opt["scale"]))
    else:
        raise NotImplementedError("Loss type [{}] is not implemented by the HIP engine".format(loss_type))
    if recurrent:
        return loss_function.to(device)
    return {"name": loss_type, "weight": weight, "function": loss_function.to(device)}


def _inner_name(loss_type):
    """<criterion> of color-<criterion> / avg-<criterion> / multiscale-<criterion>."""
    parts = loss_type.split("-")
    if len(parts) != 2:
        raise NotImplementedError("Loss type [{}] is not implemented by the HIP engine".format(loss_type))
    return parts[1]


def check_loss_names(feature_criterion=None, feature_network=None, hfen_criterion=None, tv_type=None, tv_norm=None, **_unused):
    """losses.py:174-217 for the feature, HFEN and total-variation names."""
    if feature_criterion and feature_network:
        return "fea-{}-{}".format(feature_network.lower(), feature_criterion.lower())
    if hfen_criterion:
        if hfen_criterion in ("rel_l1", "rel_l2"):
            return "hfen-relativel1"
        return "hfen-{}".format(hfen_criterion.lower())
    if tv_type and tv_norm:           # a tv_type without a tv_norm names nothing, as in the reference
        if tv_norm in (1, "L1"):
            tv_norm = "l1"
        elif tv_norm in (2, "L2"):
            tv_norm = "l2"
        if tv_type == "normal":
            tv_type = "tv"
        elif tv_type == "4D":
            tv_type = "dtv"
        return "{}-{}".format(tv_type, tv_norm)
    return None


class PerceptualLoss(nn.Module):
    """VGG feature (perceptual) loss and Gram-matrix style loss over dictionaries of layers (losses.py:220-340).  The random
    rotations / flips of `perceptual_opt` are refused."""

    def __init__(self, criterion=None, network=None, opt=None):
        super().__init__()
        self.criterion, self.network = criterion, network
        w_l_p, w_l_s = {"conv5_4": 1}, {}
        self.perceptual_weight, self.style_weight = 1.0, 0.0
        if opt:
            train_opt = opt["train"]
            self.perceptual_weight = train_opt.get("feature_weight", 0) or 0
            self.style_weight = train_opt.get("style_weight", 0) or 0
            perc_opts = train_opt.get("perceptual_opt")
            if perc_opts:
                w_l_p = perc_opts.get("perceptual_layers", {"conv5_4": 1})
                w_l_s = perc_opts.get("style_layers", {})
                for k in ("rotations", "flips"):
                    if perc_opts.get(k):
                        raise NotImplementedError("perceptual_opt '{}' is not implemented by the HIP engine".format(k))
        # losses.py:281-293: an empty dictionary falls back on the other term's
        if self.style_weight > 0:
            self.w_l_s = w_l_p if (not w_l_s and w_l_p) else w_l_s
        if self.perceptual_weight > 0:
            self.w_l_p = w_l_s if (not w_l_p and w_l_s) else w_l_p

    def forward(self, x, y):
        fea_x = self.network(x)
        with torch.no_grad():
            fea_y = self.network(y.detach())
        percep_loss = None
        if self.perceptual_weight > 0:
            percep_loss = 0
            for k in self.w_l_p.keys():
                percep_loss = percep_loss + self.criterion(fea_x[k], fea_y[k]) * self.w_l_p[k]
            percep_loss = percep_loss * self.perceptual_weight
        style_loss = None
        if self.style_weight > 0:
            # Data parallelism needs no collective here: a Gram matrix belongs to ONE image and the L1 over [N, C, C] is a batch mean
            # over equal shards, so the ranks' averaged gradient is the global-batch gradient (see GeneratorLoss._log)
            style_loss = 0
            for k in self.w_l_s.keys():
                with torch.no_grad():
                    gram_y = _GramFn.apply(fea_y[k])
                style_loss = style_loss + self.criterion(_GramFn.apply(fea_x[k]), gram_y) * self.w_l_s[k]
            style_loss = style_loss * self.style_weight
        return percep_loss, style_loss


class Adversarial(nn.Module):
    """Discriminator-driven losses (losses.py:343-604) for single-scale discriminators without feature maps:
    `gan_opt.form` relativistic (vanilla GAN: the ESRGAN recipe) or standard (vanilla / lsgan: Pix2Pix, CycleGAN), and the
    conditional formulation (Pix2Pix: D sees the (condition, image) channel concatenation, losses.py:445-455,522-530)."""

    _KINDS = {"vanilla": 0, "lsgan": 1}

    def __init__(self, train_opt=None, device="cpu", diffaug=False, dapolicy="", conditional=False):
        super().__init__()
        if train_opt.get("gan_featmaps"):
            raise NotImplementedError("the feature-map GAN option 'gan_featmaps' is not implemented by the HIP engine")
        self.diffaug = bool(diffaug)
        self.dapolicy = dapolicy or ""
        if self.diffaug:
            diffaug_ops.parse_policy(self.dapolicy)          # an unsupported policy is refused here, not at the first step
        self.device = device
        self.conditional = bool(conditional)
        self.gan_type = train_opt["gan_type"]
        if self.gan_type not in self._KINDS:
            raise NotImplementedError("GAN type [{}] is not implemented by the HIP engine".format(self.gan_type))
        self.l_gan_w = train_opt["gan_weight"]
        self.form = (train_opt.get("gan_opt") or {}).get("form", "relativistic")
        if self.form not in ("relativistic", "standard"):
            raise NotImplementedError("GAN form [{}] is not implemented by the HIP engine".format(self.form))
        if self.form == "relativistic" and self.gan_type != "vanilla":
            raise NotImplementedError("the relativistic form is implemented for gan_type vanilla only")
        self.dp_group = None        # set by the model when running data-parallel

    def _label_loss(self, pred, target_is_real):
        return _GanLabelFn.apply(pred, self._KINDS[self.gan_type], 1.0 if target_is_real else 0.0)

    def _logged(self, t):
        """Logged scalars are global-batch means under data parallelism (equal shards), as the reference's gathered batch."""
        t = t.detach()
        return self.dp_group.mean_scalar(t) if self.dp_group is not None else t

    def forward(self, fake, real=None, condition=None, netD=None, stage="discriminator", fsfilter=None):
        if fsfilter is not None:
            # losses.py:572-576: both images through the high-pass, in both stages and BEFORE the conditional concatenation (the
            # condition image is not filtered).  The discriminator stage filters fake.detach(): no graph is needed there, and the
            # filter's per-step memo hands back the generator stage's result, so netD's forward memo still hits
            _engine_filter(fsfilter, filters.FilterHigh)
            fake = fsfilter(fake if stage == "generator" else fake.detach())
            if isinstance(real, torch.Tensor):
                real = fsfilter(real)
        if self.diffaug:
            # losses.py:578-582: after the frequency separation and before the conditional concatenation (the condition is not
            # augmented); fake and real are separate calls with their own draws, in both stages.  The results are new storage on
            # every call, so netD's forward memo simply misses on them
            fake = diffaug_ops.DiffAugment(fake if stage == "generator" else fake.detach(), policy=self.dapolicy)
            if isinstance(real, torch.Tensor):
                real = diffaug_ops.DiffAugment(real, policy=self.dapolicy)
        if self.conditional:
            # like the reference's dispatch (losses.py:590-604) the second positional argument is the condition in the
            # generator stage (pix2pix_model.py:152-154 passes it by keyword)
            if condition is None:
                raise ValueError("conditional GAN: no condition image was given")
            fake = _CatChannelsFn.apply(condition, fake)
            if real is not None:
                real = _CatChannelsFn.apply(condition, real)
        if stage == "generator":
            pred_g_fake = netD(fake)
            if self.form == "standard":                # D(real) is not needed (losses.py:395-403,424-426)
                return self.l_gan_w * self._label_loss(pred_g_fake, True)
            if real is None:
                # the reference reaches netD(None) here (losses.py:401-403: conv2d on None => TypeError) -- e.g. its shipped
                # options/i2i/train_pix2pix.yml, which has no `gan_opt` and calls the generator stage without `real`
                raise TypeError("the relativistic GAN form (the default when `train.gan_opt.form` is not given) needs the real "
                                "image in the generator stage and none was passed (the reference fails at the same place): "
                                "set train.gan_opt.form: standard")
            with torch.no_grad():
                pred_g_real = netD(real)          # detached in the reference (losses.py:430)
            res = _RaGANFn.apply(pred_g_fake, pred_g_real, 0, self.l_gan_w, self.dp_group)
            return res[0]
        pred_d_fake = netD(fake.detach())
        pred_d_real = netD(real)
        if self.form == "standard":                    # losses.py:497-499,514-523
            l_d_fake = self._label_loss(pred_d_fake, False)
            l_d_real = self._label_loss(pred_d_real, True)
            l_d_total = (l_d_fake + l_d_real) * 0.5
            gan_logs = {"l_d_real": self._logged(l_d_real), "l_d_fake": self._logged(l_d_fake),
                        "D_real": self._logged(ops_mean(pred_d_real)), "D_fake": self._logged(ops_mean(pred_d_fake))}
            return l_d_total, gan_logs
        res = _RaGANFn.apply(pred_d_fake, pred_d_real, 1, 1.0, self.dp_group)
        # kept on device: the model's log dict materialises lazily (one sync instead of four .item())
        gan_logs = {"l_d_real": res[1].detach(), "l_d_fake": res[2].detach(),
                    "D_real": res[3].detach(), "D_fake": res[4].detach()}
        return res[0], gan_logs


def _engine_filter(fsfilter, kind):
    """Frequency separation runs through the engine's own filter modules only: any other callable would be an eager-PyTorch filter."""
    if not isinstance(fsfilter, kind):
        raise NotImplementedError("fsfilter must be a trainner_amd.dataops.filters.{} (built by BaseModel.setup_fs); other frequency-"
                                  "separation filters are not implemented by the HIP engine".format(kind.__name__))


def ops_mean(pred):
    """torch.mean(pred.detach()) of a logit map for the D_real / D_fake log entries (losses.py:519-520)."""
    p = pred.detach().contiguous().view(-1)
    out = torch.empty(1, dtype=torch.float32, device=p.device)
    ops.gan_loss(p, 2, 0.0, out, None)
    return out[0]


class GeneratorLoss(nn.Module):
    """Weighted list of generator losses (losses.py:607-962): pixel, hfen, tv, contextual, feature, cpl, gpl, overflow, colour,
    average, multi-scale, then the precise list grad, ssim; same order and names."""

    _UNSUPPORTED = ("lpips_weight", "fft_weight",
                    "fdpl_weight", "range_weight")
    # losses.py:633-640,775-788: weight key, criterion key, the family its criterion must name
    _POOLED = (("color_weight", "color_criterion", "color"), ("avg_weight", "avg_criterion", "avg"),
               ("ms_weight", "ms_criterion", "multiscale"))

    def __init__(self, opt=None, device="cpu", allow_featnets=True):
        super().__init__()
        train_opt = opt["train"]
        for k in self._UNSUPPORTED:
            if train_opt.get(k):
                raise NotImplementedError("loss option '{}' is outside the SR hot path of the HIP engine".format(k))
        pixel_weight = train_opt.get("pixel_weight", 0) or 0
        pixel_criterion = train_opt.get("pixel_criterion", None)
        self.loss_list = []
        if pixel_weight > 0 and pixel_criterion:
            if pixel_criterion.find("multiscale") >= 0:
                raise NotImplementedError("pixel_criterion [{}] is not implemented by the HIP engine: the multi-scale pixel loss is "
                                          "built from ms_criterion / ms_weight".format(pixel_criterion))
            self.loss_list.append(get_loss_fn(pixel_criterion, pixel_weight, device=device))
        hfen_weight = train_opt.get("hfen_weight", 0) or 0
        hfen_criterion = check_loss_names(hfen_criterion=train_opt.get("hfen_criterion"))
        if hfen_weight > 0 and hfen_criterion:
            self.loss_list.append(get_loss_fn(hfen_criterion, hfen_weight, device=device))
        tv_weight = train_opt.get("tv_weight", 0) or 0
        tv_type = check_loss_names(tv_type=train_opt.get("tv_type"), tv_norm=train_opt.get("tv_norm"))
        if tv_weight > 0 and tv_type:
            self.loss_list.append(get_loss_fn(tv_type, tv_weight, device=device))
        cx_weight = (train_opt.get("cx_weight", 0) or 0) if allow_featnets else 0          # losses.py:686-694,730-733
        cx_type = train_opt.get("cx_type", None) if allow_featnets else None
        if cx_weight > 0 and cx_type:
            self.loss_list.append(get_loss_fn(cx_type, cx_weight, device=device, opt=opt))
        feature_weight = (train_opt.get("feature_weight", 0) or 0) if allow_featnets else 0
        style_weight = (train_opt.get("style_weight", 0) or 0) if allow_featnets else 0
        feat_opts = train_opt.get("perceptual_opt")
        feature_network = (feat_opts or {}).get("feature_network", None) or train_opt.get("feature_network", "vgg19") or "vgg19"
        feature_criterion = check_loss_names(feature_criterion=train_opt.get("feature_criterion"),
                                             feature_network=feature_network)
        if (feature_weight > 0 or style_weight > 0) and feature_criterion:          # losses.py:735
            self.loss_list.append(get_loss_fn(feature_criterion, 1, opt=opt, device=device))
            self.cri_fea = True
        else:
            self.cri_fea = None
        # losses.py:642-659,761-769: spl_type spl -> cpl and gpl, each with spl_weight; any other spl_type builds nothing
        spl_weight = train_opt.get("spl_weight", 0) or 0
        spl_type = train_opt.get("spl_type", None)
        for name in ("cpl", "gpl"):
            if spl_weight > 0 and spl_type in ("spl", name):
                self.loss_list.append(get_loss_fn(name, spl_weight, opt=opt, device=device))
        of_weight = train_opt.get("of_weight", 0) or 0
        of_type = train_opt.get("of_type", None)
        if of_weight > 0 and of_type:
            self.loss_list.append(get_loss_fn(of_type, of_weight, device=device))
        # losses.py:775-788: colour, average, multi-scale, in this order.  A criterion without a weight builds nothing, as in the
        # reference; a weight without its criterion is refused (stricter than the reference, which silently builds nothing), like
        # grad_weight below
        for wkey, ckey, family in self._POOLED:
            weight = train_opt.get(wkey, 0) or 0
            crit = train_opt.get(ckey, None)
            if weight > 0 and not crit:
                raise NotImplementedError("loss option '{}' is set but '{}' is not: give {} ({}-<criterion>) or drop the "
                                          "weight".format(wkey, ckey, ckey, family))
            if weight > 0:
                if crit.find(family) < 0:
                    raise NotImplementedError("{} [{}] is not implemented by the HIP engine (expected {}-<criterion>)".format(
                        ckey, crit, family))
                self.loss_list.append(get_loss_fn(crit, weight, opt=opt, device=device))
        # the "precise" terms (losses.py:780-816), evaluated by the models after the GAN term and always in fp32
        self.precise_loss_list = []
        grad_weight = train_opt.get("grad_weight", 0) or 0
        grad_type = train_opt.get("grad_type", None)
        if grad_weight > 0 and not grad_type:
            # the one place where the engine is stricter than the reference, which silently builds nothing here: a grad weight
            # without a type is refused
            raise NotImplementedError("loss option 'grad_weight' is set but 'grad_type' is not: give grad_type "
                                      "(grad-2d-<criterion> | grad-4d-<criterion>) or drop the weight")
        if grad_weight > 0:
            self.precise_loss_list.append(get_loss_fn(grad_type, grad_weight, device=device))
        ssim_weight = train_opt.get("ssim_weight", 0) or 0
        ssim_type = train_opt.get("ssim_type", None)
        if ssim_weight > 0 and ssim_type:
            self.precise_loss_list.append(get_loss_fn(ssim_type, ssim_weight, opt=train_opt, allow_featnets=allow_featnets,
                                                      device=device))
        self.dp_group = None        # set by SRModel when running data-parallel

    def _effective(self, l, value):
        """weight * value; a batch SUM (HFEN with a sum-reduced criterion: hfen-l1, hfen-l2, hfen-elastic) is also multiplied by the
        world size under data parallelism, because the reference sums over the gathered global batch: the ranks' averaged gradient
        is then the global one and the averaged log entry the global sum."""
        effective = l["weight"] * value
        if self.dp_group is not None and getattr(l["function"], "sum_reduced", False):
            effective = effective * float(self.dp_group.world_size)
        return effective

    def _contextual(self, f, sr, hr):
        """The contextual term on the plain (sr, hr) pair.  Under data parallelism the channel mean of the HR taps is all-reduced inside
        (the reference forms it over the gathered batch); the loss is a batch mean over equal shards like every other term."""
        f.dp_group = self.dp_group
        return f(sr, hr)

    @staticmethod
    def _fea_effective(l, percep_loss, style_loss):
        """losses.py:849-856: weight * percep + weight * style under the one log name; a None term (its weight is 0) is skipped."""
        effective = None
        for term in (percep_loss, style_loss):
            if term is not None:
                effective = l["weight"] * term if effective is None else effective + l["weight"] * term
        return effective

    def _log(self, log_dict, name, effective):
        # under data parallelism the logged value is the global-batch mean, as the reference computes it on the gathered batch.
        # The gradient needs no extra collective: every term here but the sum-reduced HFEN ones (see _effective) is a batch mean
        # over equal shards, so averaging the ranks' gradients makes it the global-batch gradient.  cpl, gpl and overflow are such
        # means too (SPLoss divides its per-image line cosines by the batch size): no collective, no world-size factor.  So are the
        # colour, average and multi-scale terms: every pooled cell belongs to one image and each level's mean (the cosine term of
        # l1cosinesim included) divides by a count proportional to the batch size
        log_dict[name] = self.dp_group.mean_scalar(effective) if self.dp_group is not None else effective.detach()

    @staticmethod
    def _fp32(t):
        """The operand every fp32 loss kernel reads: half and integer types are promoted (losses.py:935-938; bfloat16 added)."""
        return t.float() if t.dtype in (torch.float16, torch.bfloat16, torch.int8, torch.int32) else t

    def _forward_fs(self, loss_list, sr, hr, log_dict, fsfilter):
        """calc_losses_fs (losses.py:865-899) for either list: the operands go by the loss NAME.  sr_f / hr_f are formed on first use
        (not at all when no term of the list consumes them) and shared by every term; the filter's per-step memo also shares them
        between the regular and the precise call, so one adjoint launch carries the summed gradient."""
        low = {}

        def lp(tag, t):
            if tag not in low:
                low[tag] = fsfilter(self._fp32(t))
            return low[tag]

        results = []
        for l in loss_list:
            name, f = l["name"], l["function"]
            if "tv" in name or "overflow" in name:
                effective = self._effective(l, f(lp("sr", sr)))                     # fake_H alone
            elif "pix" in name or "hfen" in name or "cpl" in name or "gpl" in name:
                effective = self._effective(l, f(lp("sr", sr), lp("hr", hr)))
            elif "ssim" in name:
                effective = l["weight"] * (1 - f(lp("sr", sr), lp("hr", hr)))
            elif "fea-vgg" in name:
                effective = self._fea_effective(l, *f(sr, hr))                      # unfiltered
            elif name == "contextual":
                effective = l["weight"] * self._contextual(f, sr, hr)               # unfiltered: the last branch of calc_losses_fs
            else:
                # everything else sees the unfiltered pair.  That includes grad-2d-* / grad-4d-*: the reference's low-pass branch asks
                # for 'gradient' in the name (losses.py:879), which these names do not contain -- its quirk, kept
                effective = self._effective(l, f(self._fp32(sr), self._fp32(hr)))
            results.append(effective)
            self._log(log_dict, name, effective)
        return results, log_dict

    def _forward_precise(self, sr, hr, log_dict, fsfilter=None):
        """get_results_precise (losses.py:922-942): fp32 operands, then weight * (1 - f(sr, hr)) for the ssim terms and
        weight * f(sr, hr) for the gradient loss."""
        sr, hr = self._fp32(sr), self._fp32(hr)
        if sr.dtype != hr.dtype:
            raise TypeError("Error: SR and HR have different precision in precise losses: {} and {}".format(sr.dtype, hr.dtype))
        if sr.type() != hr.type():
            raise TypeError("Error: SR and HR are on different devices in precise losses: {} and {}".format(sr.type(), hr.type()))
        if fsfilter is not None:
            return self._forward_fs(self.precise_loss_list, sr, hr, log_dict, fsfilter)
        results = []
        for l in self.precise_loss_list:
            if "ssim" in l["name"]:
                effective = l["weight"] * (1 - l["function"](sr, hr))
            elif "grad" in l["name"]:
                effective = self._effective(l, l["function"](sr, hr))
            else:
                raise NotImplementedError("precise loss [{}] is not implemented by the HIP engine".format(l["name"]))
            results.append(effective)
            self._log(log_dict, l["name"], effective)
        return results, log_dict

    def forward(self, sr, hr, log_dict, fsfilter=None, selector=None, precise=False):
        if selector:
            raise NotImplementedError("loss selectors are not implemented by the HIP engine")
        if fsfilter is not None:
            _engine_filter(fsfilter, filters.FilterLow)
        if precise:
            return self._forward_precise(sr, hr, log_dict, fsfilter)
        if fsfilter is not None:
            return self._forward_fs(self.loss_list, sr, hr, log_dict, fsfilter)
        results = []
        for l in self.loss_list:
            if "fea-vgg" in l["name"]:
                effective = self._fea_effective(l, *l["function"](sr, hr))
            elif "tv" in l["name"] or "overflow" in l["name"]:
                effective = self._effective(l, l["function"](self._fp32(sr)))              # fake_H alone
            elif l["name"] == "contextual":
                effective = l["weight"] * self._contextual(l["function"], sr, hr)
            elif (l["name"] in ("cpl", "gpl") or l["name"].split("-")[0] in ("color", "avg") or "pix-multiscale" in l["name"]
                  or isinstance(l["function"], (IL.HFENLoss, IL._Criterion))):
                effective = self._effective(l, l["function"](self._fp32(sr), self._fp32(hr)))   # fp32 kernels with or without AMP
            else:
                effective = l["weight"] * l["function"](sr, hr)
            results.append(effective)
            self._log(log_dict, l["name"], effective)
        return results, log_dict
