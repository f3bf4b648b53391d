"""Glue shared by the network executors: one convolution layer bound to its packed weights, and
the autograd bridge that lets the reference-shaped training code (`loss.backward()`) drive the
hand-written forward / backward kernel schedules of a whole network as ONE autograd node.
"""
import torch

from . import hip, ops
from .flat import ALIGN, FlatParams


class ConvOp:
    """Forward, data-gradient and weight-gradient launches of one Conv2dHIP layer."""

    def __init__(self, mod, packer, need_dgrad=True, ups=False):
        self.mod, self.packer = mod, packer
        k, s = mod.kernel_size, mod.stride
        if k == 3 and s == 1:
            self.mode_f = ops.CONV_3x3_UP2 if ups else ops.CONV_3x3
            self.mode_d = ops.CONV_3x3
            pf, pd = ops.PACK_FWD, ops.PACK_DGRAD_3x3
        elif k == 4 and s == 2 and not ups:
            self.mode_f, self.mode_d = ops.CONV_4x4_S2, ops.DGRAD_4x4_S2
            pf, pd = ops.PACK_FWD_S2D, ops.PACK_DGRAD_S2
        else:
            raise NotImplementedError("conv k=%d s=%d is not on the SR hot path" % (k, s))
        self.i_f = packer.add(mod.weight, pf)
        self.i_d = packer.add(mod.weight, pd) if need_dgrad else None
        # nearest x2 + 3x3: the layer folded into its virtual 4x4 stride-2 convolution (ops.upconv_plan decides per pass and per call)
        self.ups = ups
        self.i_uf = packer.add(mod.weight, ops.PACK_UP2_DGRAD_S2) if ups else None
        self.i_ud = packer.add(mod.weight, ops.PACK_UP2_FWD_S2D) if (ups and need_dgrad) else None
        # deep layers that can meet a tiny spatial extent (discriminator tail): column-layout packings for the
        # im2col + split-K GEMM path (ops.conv_small)
        deep = mod.in_channels * k * k >= 2048 and not ups
        i_fc = packer.add(mod.weight, ops.PACK_COL_FWD) if deep else None
        i_dc = packer.add(mod.weight, ops.PACK_COL_DGRAD3) if (deep and need_dgrad and k == 3) else None
        # <= 4-channel image on either side of a 3x3 layer: taps folded into K (TNR_CONV_3x3_C4)
        img = k == 3 and s == 1 and not ups
        self.thin = img                 # <= 4 channels on one side: vector-ALU kernels (conv_thin.hip)
        i_f4 = packer.add(mod.weight, ops.PACK_C4_FWD) if (img and mod.in_channels <= 4) else None
        i_d4 = packer.add(mod.weight, ops.PACK_C4_DGRAD3) if (img and need_dgrad and mod.out_channels <= 4) else None
        # per direction (False: forward, True: data-gradient): the launch mode and the facts ops.conv_plan decides on
        cin, cout = mod.in_channels, mod.out_channels
        self.dirs = {False: (self.mode_f, ops.ConvLayer(k, s, cin, cout, False, ups, direct=self.i_f, c4=i_f4, col=i_fc)),
                     True: (self.mode_d, ops.ConvLayer(k, s, cin, cout, True, ups, direct=self.i_d, c4=i_d4, col=i_dc))}

    def _run(self, dgrad, x, y, epi):
        """One launch of this layer in the form ops.conv_plan names."""
        mode, layer = self.dirs[dgrad]
        wp = self.packer.get(layer.direct)
        form = ops.conv_plan(x, wp, y, mode, epi, layer=layer)[0]
        if form == "thin":
            ops.conv_thin(x, self.mod.weight, y, bias=None if dgrad else self.mod.bias, alpha=epi.get("alpha", 1.0), dgrad=dgrad)
        elif form == "c4":          # the whole 4-channel pixel of the NHWC4 image (3 channels + the zero pad)
            ops.conv(x if x.C == 4 else ops.View(x.buf), self.packer.get(layer.c4), y, mode=ops.CONV_3x3_C4, **epi)
        elif form == "im2col":
            ops.conv_small(x, self.packer.get(layer.col), y, layer.k, layer.stride, **epi)
        else:
            ops.conv(x, wp, y, mode=mode, **epi)

    def fwd(self, x, y, **epi):
        epi["bias"] = self.mod.bias
        self._run(False, x, y, epi)

    def fwd_up2(self, x, y, **epi):
        """An UP2 layer's forward in the form ops.upconv_plan names: folded, one four-tap stride-2 data-gradient launch over the folded
        weights (bias, activation and slope as in fwd); else fwd itself, the TNR_CONV_3x3_UP2 launch."""
        if "fwd" not in ops.upconv_plan(x)[0]:
            return self.fwd(x, y, **epi)
        ops.conv(x, self.packer.get(self.i_uf), y, mode=ops.DGRAD_4x4_S2, family=ops.UPFOLD_FAMILY, bias=self.mod.bias, **epi)

    def fwd_shuffle2(self, x, y, **epi):
        """This layer + nn.PixelShuffle(2) in one launch, y = the shuffled tensor (ops.conv_shuffle2); False: not available here."""
        return ops.conv_shuffle2(x, self.packer.get(self.i_f), y, layer=self.dirs[False][1], bias=self.mod.bias, **epi)

    def fwd_pool2(self, x, y, route=None, **epi):
        """This layer + its activation + nn.MaxPool2d(2, 2) in one launch, y = the pooled tensor (ops.conv_pool2); False: not available here."""
        if self.mode_f != ops.CONV_3x3:
            return False
        return ops.conv_pool2(x, self.packer.get(self.i_f), y, route=route, layer=self.dirs[False][1], bias=self.mod.bias, **epi)

    def dgrad(self, g, gx, **epi):
        """gx = conv_transpose(g); for an UP2 layer gx lives in the up-sampled domain."""
        self._run(True, g, gx, epi)

    def dgrad_up2(self, g, gx, mask=None, m_slope=0.2):
        """An UP2 layer's gradient in the LOW-resolution domain: gx = the 2 x 2 block sums of conv_transpose(g), times LeakyReLU'(mask)
        where the layer's input is an activation's output.  Folded: one four-tap stride-2 launch with the mask in its epilogue; else
        the 3x3 data-gradient into a high-resolution scratch and tnr_upsample2x_bwd."""
        if "dgrad" in ops.upconv_plan(gx)[0]:
            epi = dict(mask=mask, m_slope=m_slope) if mask is not None else {}
            ops.conv(g, self.packer.get(self.i_ud), gx, mode=ops.CONV_4x4_S2, family=ops.UPFOLD_FAMILY, **epi)
            return
        gup = ops.View(ops.new_act(g.N, g.H, g.W, gx.C, g.buf.device))
        self.dgrad(g, gup)
        ops.upsample2x_bwd(gup, gx, mask=mask, mslope=m_slope)

    def _wgrad_up2_folded(self, x, g, alpha, with_bias):
        """dW (+ db) += alpha * ... of an UP2 layer through the folded S: its weight gradient (x := g, g := x) into a workspace, the
        16 -> 9 tap unfold, and the bias gradient as the plain sum of g (S's own bias sum would be the sum of x)."""
        w, b = self.mod.weight, self.mod.bias
        cout, cin = w.shape[0], w.shape[1]
        n = cin * cout * 16
        dws = ops.WS.get("upfold_dw@%x" % hip.stream(), n * 4, x.buf.device).view(torch.float32)[:n].view(cin, cout, 4, 4)
        ops.wgrad_group([dict(x=g, g=x, dw=dws, db=None, alpha=1.0, beta=0.0)], mode=ops.CONV_4x4_S2, family=ops.UPFOLD_FAMILY)
        ops.upconv_wgrad_unfold(dws, w.grad, alpha=alpha, beta=1.0)
        if with_bias and b is not None:
            ops.bias_grad(g, b.grad, alpha=alpha, beta=1.0)

    def fwd_stage(self, x, y, fresh_from=None, **epi):
        """Stage descriptor of this layer's forward for ops.conv_chain."""
        return dict(x=x, wp=self.packer.get(self.i_f), y=y, mode=self.mode_f, bias=self.mod.bias, fresh_from=fresh_from, **epi)

    def wgrad_item(self, x, g, alpha=1.0, cin_begin=0, with_bias=True, reflect=False):
        """Descriptor of dW[:, cin_begin : cin_begin + x.C] (+ db) += alpha * (g (x) x) for ops.wgrad_group."""
        w = self.mod.weight
        db = self.mod.bias.grad if (with_bias and self.mod.bias is not None and cin_begin == 0) else None
        return dict(x=x, g=g, dw=w.grad, db=db, cin_begin=cin_begin, alpha=alpha, beta=1.0, reflect=reflect)

    def wgrad(self, x, g, alpha=1.0, cin_begin=0, with_bias=True, reflect=False):
        if self.ups and cin_begin == 0 and not reflect and "wgrad" in ops.upconv_plan(x)[0]:
            self._wgrad_up2_folded(x, g, alpha, with_bias)
            return
        if reflect:           # ReflectionPad2d(1) in front of the layer (TNR_CONV_3x3 on the matrix cores only)
            ops.wgrad_group([self.wgrad_item(x, g, alpha, cin_begin, with_bias, reflect=True)], mode=self.mode_f)
            return
        if self.thin and ops.IMAGE_C4 and cin_begin == 0 and x.N == g.N and (x.H, x.W) == (g.H, g.W):
            m = self.mod
            db = m.bias.grad if (with_bias and m.bias is not None) else None
            if m.in_channels <= 3 and x.ctot == 4 and x.coff == 0 and g.C in (16, 32, 64):      # image -> features
                ops.wgrad_thin(g, ops.View(x.buf), m.weight.grad, db, flip=False, alpha=alpha)
                return
            if m.out_channels <= 3 and g.ctot == 4 and g.coff == 0 and x.C in (16, 32, 64):     # features -> image
                ops.wgrad_thin(x, ops.View(g.buf), m.weight.grad, db, flip=True, alpha=alpha)
                return
        ops.wgrad_group([self.wgrad_item(x, g, alpha, cin_begin, with_bias)], mode=self.mode_f)


class SpectralNormState:
    """The spectrally normalised convolutions of one network (block.SpectralNormConv2dHIP) and their weight generations.

    `derived` holds, per layer, the normalised weight W / sigma that the packer and the convolution kernels read, followed by the record
    of the forward that made it (its u, v and sigma); `gws` is the workspace the weight-gradient kernels write dL/d(W / sigma) into.
    Every training-mode forward makes a new generation (one power iteration); a forward that will be differentiated keeps a copy of
    `derived`, and its backward puts that copy back first when a later forward has replaced it."""

    def __init__(self, mods, device):
        self.mods = list(mods)
        al = lambda n: (n + ALIGN - 1) // ALIGN * ALIGN
        offs, off, goff = [], 0, 0
        for m in self.mods:
            w = m.weight_orig
            rows, n = w.shape[0], w.numel()
            offs.append((off, off + al(n), off + al(n) + al(rows), off + al(n) + al(rows) + al(n // rows), goff))
            off, goff = off + al(n) + al(rows) + al(n // rows) + ALIGN, goff + al(n)
        self.derived = torch.zeros(off, dtype=torch.float32, device=device)
        self.gws = torch.zeros(goff, dtype=torch.float32, device=device)
        layers = []
        for m, (o_w, o_u, o_v, o_s, o_g) in zip(self.mods, offs):
            w = m.weight_orig
            rows, n = w.shape[0], w.numel()
            if m.weight_u.device != w.device or m.weight_v.device != w.device or w.device != self.derived.device:
                raise hip.HipEngineError("spectral norm: weight_orig, weight_u and weight_v must live on the engine's device")
            wn, g = self.derived[o_w:o_w + n].view(w.shape), self.gws[o_g:o_g + n].view(w.shape)
            m.bind_derived(wn, g)
            layers.append(dict(w=w, wn=wn, u=m.weight_u, v=m.weight_v, ru=self.derived[o_u:o_u + rows], rv=self.derived[o_v:o_v + n // rows],
                               sig=self.derived[o_s:o_s + 1], g=g, dw=w.grad))
        self.table = ops.SpectralNormTable(layers, device)
        self.gen, self._count, self._snap = None, 0, None

    def bound_to(self, mods):
        """Still describing these modules' tensors (module.to() / load_state_dict(assign=True) replace buffers)?"""
        mods = list(mods)
        return len(mods) == len(self.mods) and all(
            a is b and L["u"] is a.weight_u and L["v"] is a.weight_v and L["w"] is a.weight_orig and L["dw"].data_ptr() == a.weight_orig.grad.data_ptr()
            for a, b, L in zip(mods, self.mods, self.table.layers))

    def derive(self, iterate):
        ops.sn_forward(self.table, iterate, eps=self.mods[0].eps)
        self._count += 1
        self.gen = self._count

    def snapshot(self):
        if self._snap is None or self._snap[0] != self.gen:
            self._snap = (self.gen, self.derived.clone())
        return self._snap

    def restore(self, snap):
        """-> True when the live generation was replaced (the caller re-packs)."""
        if snap[0] == self.gen:
            return False
        self.derived.copy_(snap[1])
        self.gen = snap[0]
        return True

    def begin_backward(self):
        ops.fill(self.gws, 0.0)

    def finish_backward(self):
        ops.sn_backward(self.table)


class _NetFn(torch.autograd.Function):
    """Whole-network autograd node.  Parameters are listed as inputs only so that autograd knows the
    output depends on them; their gradients are accumulated by the engine straight into the flat
    gradient buffer (param.grad views), so backward returns None for them."""

    @staticmethod
    def forward(ctx, net, x, *params):
        # (grad mode is always off inside Function.forward; needs_input_grad already accounts for it)
        need_param_grad = any(ctx.needs_input_grad[2:])
        need_graph = ctx.needs_input_grad[1] or need_param_grad
        memoize = net.memoize and not net._has_sn        # a spectrally normalised net's repeated forward is not a repeat
        memo = net._memo_lookup(x) if (memoize and net.training) else None
        if memo is not None and memo[1] is not None:
            # same input values, same parameters as an earlier forward of this step: its output and saved activations ARE this
            # forward's; only the side effects of running it again (BatchNorm running statistics) are replayed
            out, saved = memo
            net.replay_forward_side_effects(saved)
            out = out.detach()
        else:
            out, saved = net.engine_forward(x, save=need_graph or (memoize and net.training))
            if memoize and net.training:
                net._memo_store(x, out, saved)
        ctx.net, ctx.saved, ctx.need_param_grad = net, (saved if need_graph else None), need_param_grad
        ctx.sn_gen = net._sn.snapshot() if (need_graph and net._sn is not None) else None
        return out

    @staticmethod
    def backward(ctx, gout):
        saved = ctx.saved
        if saved is None:
            raise RuntimeError("HIP engine: backward through a forward that saved no activations")
        ctx.saved = None
        sched = getattr(ctx.net, "_bucket_schedule", None)
        if sched is not None and ctx.need_param_grad:
            sched.begin_pass()                      # dp.BucketSchedule: buckets leave in the last accumulating pass
        sn = ctx.net._sn if ctx.sn_gen is not None else None
        if sn is not None:
            ctx.net._sn_restore(ctx.sn_gen)         # the weights, u, v and sigma of THIS forward
            ctx.sn_gen = None
            if ctx.need_param_grad:
                sn.begin_backward()
        gx = ctx.net.engine_backward(saved, gout, need_input_grad=ctx.needs_input_grad[1],
                                     need_param_grad=ctx.need_param_grad)
        if sn is not None and ctx.need_param_grad:
            sn.finish_backward()
        return (None, gx) + (None,) * (len(ctx.needs_input_grad) - 2)


class HipNet(torch.nn.Module):
    """Base class of the engine's networks: flat parameters + the autograd bridge."""

    # Forward memoization (off by default; the SR model switches it on for its discriminator): a training-mode forward whose
    # input tensor (same storage, same version counter) and parameter version match an earlier forward is not recomputed --
    # output and saved activations are shared, backward passes only read them.  SRModel.optimize_parameters shows the
    # discriminator the real batch and the generated batch twice between two discriminator updates (generator stage, then
    # discriminator stage on `fake.detach()`): 2 of its 4 forward passes per step are such repeats.  Entries hold a reference
    # to their input (its address cannot be recycled while the entry lives) and die with the parameter version.  A net with spectrally
    # normalised layers never memoises, whatever is set here: its second forward has done one more power iteration.
    memoize = False

    def _memo_key(self, x):
        fp = self.flat_params()
        return (fp.version, fp.flat._version), (x.data_ptr(), tuple(x.shape), tuple(x.stride()), x._version)

    def _memo_lookup(self, x):
        ver, key = self._memo_key(x)
        if self._memo_ver != ver:
            self._memo, self._memo_ver = {}, ver
        hit = self._memo.get(key)
        return None if hit is None else (hit[1], hit[2])

    def _memo_store(self, x, out, saved):
        ver, key = self._memo_key(x)
        if self._memo_ver != ver:
            self._memo, self._memo_ver = {}, ver
        self._memo[key] = (x.detach(), out, saved)        # (detached alias: pins the storage, not the autograd graph)

    def memo_clear(self):
        """Drop every memo entry (the models call this at the start of each training step: an entry is valid only between
        the stages of ONE step -- feeder slots are refilled by raw kernels that do not move the tensors' version counters)."""
        self._memo = {}

    def replay_forward_side_effects(self, saved):
        """Hook: what a repeated training-mode forward would change besides its outputs (BatchNorm running statistics)."""

    def _init_engine(self):
        self._memo, self._memo_ver = {}, None
        self._has_sn = any(getattr(m, "spectral_norm", False) for m in self.modules())
        self._flat = FlatParams(self)
        self._packer = None
        self._dense_packer = None
        self._packer_owner = None
        self._packed_version = None
        self._ops = None
        self._sn = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._flat.touch())

    def flat_params(self):
        return self._flat.ensure()

    def _refresh_derived(self):
        """Hook: tensors derived from the parameters that the packer reads (zero-extended taps, ...) are rebuilt here,
        right before the weights are re-packed."""

    def _prepare(self, x):
        hip.require_device(x)
        if x.dtype != torch.float32:
            raise hip.HipEngineError("the HIP engine computes in fp32; got %s" % x.dtype)
        fp = self.flat_params()
        if fp.flat.device != x.device:
            raise hip.HipEngineError("network is on %s but input on %s" % (fp.flat.device, x.device))
        sn_mods = [m for m in self.modules() if getattr(m, "spectral_norm", False)] if self._has_sn else []
        if self._packer is None or self._packer.device != x.device or self._packer_owner is not fp.flat or \
                (sn_mods and not self._sn.bound_to(sn_mods)):
            # (the derived weights are bound before _build_ops hands `mod.weight` to the packer)
            self._sn = SpectralNormState(sn_mods, x.device) if sn_mods else None
            self._packer = ops.WeightPacker(x.device)
            self._dense_packer = ops.DensePacker(x.device)
            self._packer_owner = fp.flat
            self._packed_version = None
            self._build_ops(self._packer)
        # parameters only change through FusedAdam.step / load_state_dict / re-flattening, all of which bump
        # fp.version: the D (4 forwards per step) and the frozen VGG are not re-packed needlessly
        # (fp.flat._version also moves on any in-place torch write through a parameter view)
        key = (fp.version, fp.flat._version)
        if self._sn is not None and (self.training or self._packed_version != key):
            # a new weight generation: one power iteration per training-mode forward (under no_grad too); in eval mode sigma from the
            # stored u and v, when the parameters moved or a backward put an older generation back
            self._sn.derive(iterate=self.training)
            self._packed_version = None
        if self._packed_version != key:
            self._refresh_derived()
            self._packer.run()
            self._dense_packer.run()
            self._packed_version = key

    def _sn_restore(self, snap):
        """Put a saved forward's weight generation back (its W / sigma, u, v, sigma) and re-pack, unless it is the live one."""
        if self._sn.restore(snap):
            self._refresh_derived()
            self._packer.run()
            self._dense_packer.run()
            self._packed_version = None         # an eval-mode forward re-derives before it runs

    def forward(self, x, **kw):
        x = x.contiguous()
        self._prepare(x)
        params = list(self.parameters())
        return _NetFn.apply(self, x, *params)
