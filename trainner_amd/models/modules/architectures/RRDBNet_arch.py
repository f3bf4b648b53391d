"""RRDBNet (ESRGAN generator) on the MI355X engine.

Same constructor, same state_dict keys and the same arithmetic as the reference's
codes/models/modules/architectures/RRDBNet_arch.py (RRDBNet :14-60, RRDB :62-96,
ResidualDenseBlock_5C :98-163), re-designed for CDNA4:

  * every dense block lives in ONE 192-channel NHWC buffer [x | x1 | x2 | x3 | x4]; conv_k reads
    channels [0, 64+32(k-1)) and writes its 32 channels in place, so the four torch.cat per block
    (:152-160) never happen;
  * bias, LeakyReLU(0.2), `x5*0.2 + x` and the RRDB-level `out*0.2 + x` are epilogues of the
    implicit-GEMM kernel (conv5 of RDB3 carries both residuals);
  * the nearest x2 of upconv_block is folded into the following conv's gather;
  * backward is a hand-written schedule.  The data-gradient of a dense block runs as a "gradient
    dense block", the mirror image of the forward: with the gradient buffer laid out
    [g5 | g4 | g3 | g2 | g1] the gradient of each feature group is ONE convolution over a growing
    channel prefix (K = 64..192, exactly the forward's shapes; LeakyReLU' fused as an epilogue mask)
    instead of a chain of read-modify-write accumulations; the transposed/flipped weight slices are
    packed by tnr_pack_dense_dgrad.  Weight gradients are deterministic split-K launches that write
    straight into the flat gradient buffer.
"""
import math

import torch
import torch.nn as nn

from .... import ops
from ....engine import ConvOp, HipNet
from ....ops import View, new_act
from . import block as B


class ResidualDenseBlock_5C(nn.Module):
    def __init__(self, nf=64, gc=32, act_type="leakyrelu"):
        super().__init__()
        self.conv1 = B.conv_block(nf, gc, 3, act_type=act_type)
        self.conv2 = B.conv_block(nf + gc, gc, 3, act_type=act_type)
        self.conv3 = B.conv_block(nf + 2 * gc, gc, 3, act_type=act_type)
        self.conv4 = B.conv_block(nf + 3 * gc, gc, 3, act_type=act_type)
        self.conv5 = B.conv_block(nf + 4 * gc, nf, 3, act_type=None)


class RRDB(nn.Module):
    def __init__(self, nf, gc=32, act_type="leakyrelu"):
        super().__init__()
        self.RDB1 = ResidualDenseBlock_5C(nf, gc, act_type)
        self.RDB2 = ResidualDenseBlock_5C(nf, gc, act_type)
        self.RDB3 = ResidualDenseBlock_5C(nf, gc, act_type)


class RRDBNet(HipNet):
    def __init__(self, in_nc, out_nc, nf, nb, nr=3, gc=32, upscale=4, norm_type=None, act_type="leakyrelu",
                 mode="CNA", upsample_mode="upconv", convtype="Conv2D", finalact=None, gaussian_noise=False,
                 plus=False):
        super().__init__()
        if nr != 3 or norm_type is not None or mode != "CNA" or convtype != "Conv2D" or finalact or plus:
            raise NotImplementedError("RRDBNet option outside the ESRGAN recipe is not implemented by the HIP engine")
        if upscale not in (2, 4, 8) or upsample_mode not in ("upconv", "pixelshuffle"):
            raise NotImplementedError("upscale %s / upsample mode [%s] is not found" % (upscale, upsample_mode))
        if nf % 32 or in_nc > 4 or out_nc > 4:
            raise NotImplementedError("HIP RRDBNet needs nf %% 32 == 0 and <= 4 image channels")
        self.in_nc, self.out_nc, self.nf, self.nb, self.gc = in_nc, out_nc, nf, nb, 32  # reference ignores gc (:24)
        self.upsample_mode, self.n_up = upsample_mode, int(math.log(upscale, 2))
        self.act, self.slope = B.act_code(act_type)
        # ESRGAN+ GaussianNoise at the end of every dense block (ResidualDenseBlock_5C.forward :160-163, block.py:587-600: sigma 0.1,
        # training mode only, gradient through both terms; on by default, options/defaults.py:59).  The draw is a counter-based
        # function of (noise_seed, training-forward count, block, element) evaluated inside the convolution epilogues
        # (csrc/gauss_noise.h): nothing is stored, backward regenerates it.  noise_seed None: torch.initial_seed() at the forward
        # (what util.set_random_seed pins); noise_sample0: index of this rank's first sample in the global batch.
        self.noise_sigma = 0.1 if gaussian_noise else 0.0
        self.noise_seed, self.noise_sample0, self._noise_calls = None, 0, 0

        fea_conv = B.conv_block(in_nc, nf, 3, act_type=None)
        trunk = [RRDB(nf, 32, act_type) for _ in range(nb)] + [B.conv_block(nf, nf, 3, act_type=None)]
        ups = []
        for _ in range(self.n_up):
            if upsample_mode == "upconv":
                ups.append(B.flat_sequential(B.Marker("nearest x2"), B.conv_block(nf, nf, 3, act_type=act_type)))
            else:
                ups.append(B.flat_sequential(B.conv_block(nf, nf * 4, 3, act_type=None), B.Marker("pixelshuffle x2"),
                                             B.Marker("act:" + act_type)))
        hr0 = B.conv_block(nf, nf, 3, act_type=act_type)
        hr1 = B.conv_block(nf, out_nc, 3, act_type=None)
        self.model = B.flat_sequential(fea_conv, B.ShortcutBlock(B.flat_sequential(*trunk)), *ups, hr0, hr1)
        self._init_engine()

    # ------------------------------------------------------------------------------ engine
    def _build_ops(self, packer):
        m = self.model
        o = {"fea": ConvOp(m[0], packer, need_dgrad=False)}
        sub = m[1].sub
        o["rdb"], o["rdb_dense"] = [], []
        for b in range(self.nb):
            for ri, r in enumerate((sub[b].RDB1, sub[b].RDB2, sub[b].RDB3)):
                convs = [getattr(r, "conv%d" % k)[0] for k in range(1, 6)]
                o["rdb"].append([ConvOp(c, packer, need_dgrad=False) for c in convs])
                s = 0.2 if ri == 2 else 1.0      # RDB3's output is scaled by the RRDB residual (x0.2)
                o["rdb_dense"].append(self._dense_packer.add_block([c.weight for c in convs], self.nf, self.gc, 0.2 * s))
        o["lr"] = ConvOp(sub[self.nb], packer)
        o["up"] = []
        idx = 2
        for _ in range(self.n_up):
            if self.upsample_mode == "upconv":
                o["up"].append(ConvOp(m[idx + 1], packer, ups=True))
            else:
                o["up"].append(ConvOp(m[idx], packer))
            idx += 3
        o["hr0"] = ConvOp(m[idx], packer)
        o["hr1"] = ConvOp(m[idx + 2], packer)
        self._ops = o

    def engine_forward(self, x, save):
        o, nf, gc = self._ops, self.nf, self.gc
        N, _, h, w = x.shape
        dev = x.device
        act, sl = self.act, self.slope
        cb = nf + 4 * gc
        lr = new_act(N, h, w, 4, dev)
        ops.nchw_to_nhwc(x, View(lr), Cpad=4)
        nrdb = 3 * self.nb
        nz = self._draw_noise(nrdb, h * w)         # per dense block: ops.Noise, or None (eval mode / sigma 0)
        nbuf = nrdb if save else min(nrdb, 4)
        bufs = [new_act(N, h, w, cb, dev) for _ in range(nbuf)]
        trunk = new_act(N, h, w, nf, dev)
        first = View(bufs[0], 0, nf) if nrdb else View(trunk)
        o["fea"].fwd(View(lr), first)
        fea_keep = first
        if not save and nrdb:
            # the ring of 4 buffers is recycled: keep fea for the ShortcutBlock add
            fea_keep = View(new_act(N, h, w, nf, dev))
            ops.axpby(fea_keep, first, 1.0, 0.0)
        for i in range(nrdb):
            buf = bufs[i % nbuf]
            convs = o["rdb"][i]
            # the five convolutions of the block as ONE launch (conv_chain.hip): conv_{k+1} first meets the
            # output of conv_k at input channel nf + gc*(k-1)
            st = []
            for k in range(4):
                cin = nf + gc * k
                st.append(convs[k].fwd_stage(View(buf, 0, cin), View(buf, cin, gc), fresh_from=(cin - gc if k else None),
                                             act=act, slope=sl))
            dst = View(bufs[(i + 1) % nbuf], 0, nf) if i + 1 < nrdb else View(trunk)
            nk = dict(noise=nz[i]) if nz else {}     # noise(x5*0.2 + x): the multiplier sits between the r1 and the r2 step
            if i % 3 == 2:   # RDB3 also closes the RRDB: noise(x5*0.2 + x)*0.2 + x_rrdb
                st.append(convs[4].fwd_stage(View(buf), dst, fresh_from=nf + 3 * gc, alpha=0.2, r1=View(buf, 0, nf),
                                             r2=View(bufs[(i - 2) % nbuf], 0, nf), alpha2=0.2, **nk))
            else:
                st.append(convs[4].fwd_stage(View(buf), dst, fresh_from=nf + 3 * gc, alpha=0.2, r1=View(buf, 0, nf), **nk))
            ops.dense_block(st)
        y0 = new_act(N, h, w, nf, dev)
        o["lr"].fwd(View(trunk), View(y0), r1=fea_keep)          # ShortcutBlock: fea + trunk(fea)
        cur, stages = View(y0), []
        for u in o["up"]:
            H2, W2 = cur.H * 2, cur.W * 2
            if self.upsample_mode == "upconv":
                nxt = View(new_act(N, H2, W2, nf, dev))
                u.fwd_up2(cur, nxt, act=act, slope=sl)
                stages.append((cur, nxt, None))
            else:
                nxt = View(new_act(N, H2, W2, nf, dev))
                t = None
                if not u.fwd_shuffle2(cur, nxt, act=act, slope=sl):      # the shuffle folded into the convolution's store where the kernel offers it
                    t = View(new_act(N, cur.H, cur.W, 4 * nf, dev))
                    u.fwd(cur, t, act=act, slope=sl)              # activation commutes with the shuffle
                    ops.depth_to_space(t, nxt)
                stages.append((cur, nxt, t))
            cur = nxt
        h0 = View(new_act(N, cur.H, cur.W, nf, dev))
        o["hr0"].fwd(cur, h0, act=act, slope=sl)
        o4 = new_act(N, cur.H, cur.W, 4, dev)
        o["hr1"].fwd(h0, View(o4, 0, self.out_nc))
        out = torch.empty((N, self.out_nc, cur.H, cur.W), dtype=torch.float32, device=dev)
        ops.nhwc_to_nchw(View(o4, 0, self.out_nc), out)
        saved = None
        if save:
            saved = dict(lr=lr, bufs=bufs, trunk=trunk, y0=y0, stages=stages, hr_in=cur, h0=h0, shape=(N, h, w), noise=nz)
        return out, saved

    def calibrate_dense_block_form(self, N, h, w, dp=None):
        """ops.calibrate_dense_block_form on a SCRATCH dense block of the training shape (N x h x w LR pixels): the first block's weights,
        random activations in a 192-channel buffer of its own, the output in a second buffer -- nothing the network keeps is touched.
        Called once by the model's constructor (every data-parallel rank at the same point)."""
        dev = next(self.parameters()).device
        if not self.nb or dev.type != "cuda":
            return ops.calibrate_dense_block_form(None, dp)
        nf, gc = self.nf, self.gc
        self._prepare(torch.empty(1, self.in_nc, 8, 8, device=dev))      # the packed layouts of the current weights (what a forward does first)
        buf, res = new_act(N, h, w, nf + 4 * gc, dev), new_act(N, h, w, nf, dev)
        out = new_act(N, h, w, nf, dev)
        buf.normal_(0.0, 0.5)
        res.normal_(0.0, 0.5)
        convs, st = self._ops["rdb"][0], []
        for k in range(4):
            cin = nf + gc * k
            st.append(convs[k].fwd_stage(View(buf, 0, cin), View(buf, cin, gc), fresh_from=(cin - gc if k else None), act=self.act, slope=self.slope))
        st.append(convs[4].fwd_stage(View(buf), View(out), fresh_from=nf + 3 * gc, alpha=0.2, r1=View(buf, 0, nf), r2=View(res), alpha2=0.2))
        return ops.calibrate_dense_block_form(st, dp)

    def _draw_noise(self, nrdb, hw):
        if not (self.training and self.noise_sigma != 0.0):
            return None
        seed = torch.initial_seed() if self.noise_seed is None else int(self.noise_seed)
        call, self._noise_calls = self._noise_calls, self._noise_calls + 1
        pix0 = self.noise_sample0 * hw
        return [ops.Noise(self.noise_sigma, ops.noise_key(seed, call, i), 1, pix0) for i in range(nrdb)]

    def _rdb_backward(self, convs, dense, buf, GP, s, gnext, extra, want_w, pend, nz_out=None):
        """Backward of one dense block as a 'gradient dense block' (mirror of the forward).
        GP: 192-ch gradient buffer whose [0:nf) holds the incoming gradient g (unscaled; the block's
        residual scale s and conv5's 0.2 are folded into the packed weights).  Fills GP[nf:] with the
        pre-activation gradients [g4 | g3 | g2 | g1] and writes the gradient w.r.t. the block input,
        + s*g (+ extra, the RRDB skip), into `gnext` (64-ch view).  nz_out: the noise multiplier of the tensor `gnext` is the
        gradient of (the previous dense block's noised output): what leaves is the gradient of its pre-noise value, m * (...)."""
        nf, gc, sl = self.nf, self.gc, self.slope
        dp = self._dense_packer
        st = []
        for t in range(4):                       # targets x4, x3, x2, x1: LeakyReLU' fused as mask
            cin = nf + t * gc
            xk = View(buf, nf + (3 - t) * gc, gc)
            st.append(dict(x=View(GP, 0, cin), wp=dp.get(dense[t]), y=View(GP, cin, gc), fresh_from=(cin - gc if t else None),
                           mask=xk, m_lo=0, m_hi=gc, m_slope=sl))
        g = View(GP, 0, nf)
        kw = dict(r2=extra, alpha2=1.0) if extra is not None else {}
        if nz_out is not None:
            kw["noise"] = nz_out.at(2)
        st.append(dict(x=View(GP), wp=dp.get(dense[4]), y=gnext, fresh_from=nf + 3 * gc, r1=g, beta1=s, **kw))
        ops.dense_block(st)                      # the block's data-gradient: one launch (conv_chain.hip), or four stages + a Winograd launch
        if want_w:
            # Weight gradients are only COLLECTED here and launched per RRDB (_flush_wgrads): conv5 as 64 x 64 channel
            # workgroup tiles; conv1..conv4 (32 couts; g_k lives at GP[nf + (3-k)*gc : +gc)) as 32 x 128 / 32 x 64 /
            # 32 x 32 pieces (96 inputs = 64 + 32, 160 = 128 + 32) -- every class has 9 accumulator tiles per wave and
            # no padded MFMA slot (wgrad_tile.hip), and the pieces of one class over the RRDB's three dense blocks
            # share a launch: 4 weight-gradient launches per RRDB instead of 9.
            pend.setdefault("c5", []).append(convs[4].wgrad_item(View(buf), g, alpha=0.2 * s))
            if gc == 32 and nf == 64:
                # conv4 + conv3 and conv2 + conv1 as COUT PAIRS: their gradients stand side by side in GP ([g4 | g3], [g2 | g1]) and
                # both layers of a pair read the channels the narrower one reads (x | x1 | x2 = 128, x = 64), so a pair is one
                # 64-cout job of conv5's tile class (tnr_wgrad_desc.cout_split): the RRDB's 64-cout work -- 3 x (conv5 + two pairs) --
                # is ONE launch, the two 32-channel remainders (conv4 over x3, conv2 over x1) a second one.
                for ka, kb in ((3, 2), (1, 0)):                # (wider layer first: its gradient comes first in GP)
                    cin = nf + gc * kb                         # channels both layers read
                    gpair = View(GP, nf + (3 - ka) * gc, 2 * gc)
                    it = convs[ka].wgrad_item(View(buf, 0, cin), gpair)
                    it["pair"] = (convs[kb].mod.weight.grad, None if it["db"] is None else convs[kb].mod.bias.grad, gc)
                    pend["c5"].append(it)
                    ga = View(GP, nf + (3 - ka) * gc, gc)
                    pend.setdefault(gc, []).append(convs[ka].wgrad_item(View(buf, cin, gc), ga, cin_begin=cin))
                return
            for k in (3, 2, 1, 0):
                cin = nf + gc * k
                gk = View(GP, nf + (3 - k) * gc, gc)
                big = 4 * gc if cin >= 4 * gc else 2 * gc
                pieces = [(0, big)] + ([(big, cin - big)] if cin > big else [])
                for lo, n in pieces:
                    pend.setdefault(n, []).append(convs[k].wgrad_item(View(buf, lo, n), gk, cin_begin=lo))

    @staticmethod
    def _flush_wgrads(pend):
        for items in pend.values():
            for i in range(0, len(items), ops.WGRAD_GROUP_MAX):
                ops.wgrad_group(items[i:i + ops.WGRAD_GROUP_MAX])
        pend.clear()

    def engine_backward(self, sv, gout, need_input_grad, need_param_grad):
        o, nf, gc, sl = self._ops, self.nf, self.gc, self.slope
        N, h, w = sv["shape"]
        gout = gout.contiguous()
        dev = gout.device
        W = need_param_grad
        cur, h0 = sv["hr_in"], sv["h0"]
        g4 = new_act(N, cur.H, cur.W, 4, dev)
        ops.nchw_to_nhwc(gout, View(g4), Cpad=4)
        gh0 = View(new_act(N, cur.H, cur.W, nf, dev))
        o["hr1"].dgrad(View(g4), gh0, mask=h0, m_slope=sl)
        sched = getattr(self, "_bucket_schedule", None) if W else None   # data-parallel gradient buckets (dp.py)

        def done(op):
            if sched is not None:
                sched.mark_done(op.mod.weight)

        if W:
            o["hr1"].wgrad(h0, View(g4, 0, self.out_nc))
            done(o["hr1"])
        gcur = View(new_act(N, cur.H, cur.W, nf, dev))
        last_stage = sv["stages"][-1] if sv["stages"] else None
        # gradient w.r.t. hr_in; it is an activation output only if an upsample stage produced it
        o["hr0"].dgrad(gh0, gcur, **(dict(mask=cur, m_slope=sl) if (last_stage and self.upsample_mode == "upconv") else {}))
        if W:
            o["hr0"].wgrad(cur, gh0)
            done(o["hr0"])
        for si in range(len(sv["stages"]) - 1, -1, -1):
            src, dst, t = sv["stages"][si]
            u = o["up"][si]
            prev_is_act = si > 0 and self.upsample_mode == "upconv"
            if self.upsample_mode == "upconv":
                # gcur = grad w.r.t. dst pre-activation (mask applied by the consumer's dgrad epilogue)
                if W:
                    u.wgrad(src, gcur)
                    done(u)
                gsrc = View(new_act(N, src.H, src.W, nf, dev))
                u.dgrad_up2(gcur, gsrc, mask=(src if prev_is_act else None), m_slope=sl)
            else:
                gt = View(new_act(N, src.H, src.W, 4 * nf, dev))
                ops.space_to_depth_bwd(gcur, gt, mask=dst, mslope=sl)
                if W:
                    u.wgrad(src, gt)
                    done(u)
                gsrc = View(new_act(N, src.H, src.W, nf, dev))
                u.dgrad(gt, gsrc)
            gcur = gsrc
        gy0 = gcur                                     # grad w.r.t. fea + trunk
        nrdb = 3 * self.nb
        cb = nf + 4 * gc
        # four rotating gradient buffers: the three dense blocks of an RRDB keep theirs until the RRDB's grouped
        # weight-gradient launches are enqueued; the fourth receives the gradient leaving the RRDB
        G = [new_act(N, h, w, cb, dev) for _ in range(4 if nrdb else 1)]
        if W:
            o["lr"].wgrad(View(sv["trunk"]), gy0)
            done(o["lr"])
        # ESRGAN+ noise (sv["noise"]): a dense block's incoming gradient is m * (gradient of its noised output).  Inside an RRDB the
        # producing launch applies m in its last epilogue (nz_out).  The gradient of an RRDB's output is needed twice -- times RDB3's m
        # as RDB3's input and plain for the RRDB skip (:96) -- so it is written plain to one of two 64-channel buffers P and the
        # multiplied copy is one elementwise launch (tnr_gauss_mult) per RRDB.
        nz = sv.get("noise")
        P = [View(new_act(N, h, w, nf, dev)) for _ in range(2)] if (nz and nrdb) else None
        pc = 0
        o["lr"].dgrad(gy0, P[0] if P else View(G[0], 0, nf))
        if P:
            ops.gauss_mult(View(G[0], 0, nf), P[0], nz[nrdb - 1])
        pin = 0                                        # buffer whose [0:nf) holds the incoming gradient
        pend = {}
        for b in range(self.nb - 1, -1, -1):
            q, r, t = (pin + 1) % 4, (pin + 2) % 4, (pin + 3) % 4
            bufs, convs, dense = sv["bufs"], o["rdb"], o["rdb_dense"]
            skip = P[pc] if P else View(G[pin], 0, nf)                    # plain gradient of the RRDB's output
            leave = P[pc ^ 1] if P else View(G[t], 0, nf)                 # plain gradient of the RRDB's input
            self._rdb_backward(convs[3 * b + 2], dense[3 * b + 2], bufs[3 * b + 2], G[pin], 0.2, View(G[q], 0, nf), None, W, pend,
                               nz[3 * b + 1] if nz else None)
            self._rdb_backward(convs[3 * b + 1], dense[3 * b + 1], bufs[3 * b + 1], G[q], 1.0, View(G[r], 0, nf), None, W, pend,
                               nz[3 * b] if nz else None)
            self._rdb_backward(convs[3 * b], dense[3 * b], bufs[3 * b], G[r], 1.0, leave, skip, W, pend)
            pin = t
            if P:
                pc ^= 1
                if b > 0:
                    ops.gauss_mult(View(G[t], 0, nf), leave, nz[3 * b - 1])
            if W:
                self._flush_wgrads(pend)
                done(convs[3 * b][0])                  # everything from this RRDB's first conv onwards is final
        gfea = P[pc] if P else View(G[pin], 0, nf)
        ops.axpby(gfea, gy0, 1.0, 1.0)                 # ShortcutBlock: both branches reach fea
        if W:
            o["fea"].wgrad(View(sv["lr"], 0, self.in_nc), gfea)
        gx = None
        if need_input_grad:
            raise NotImplementedError("gradient w.r.t. the LR input is not on the SR training path")
        return gx

    def forward(self, x, outm=None):
        if outm:
            raise NotImplementedError("finalcap/outm [%s] is not implemented by the HIP engine" % outm)
        return super().forward(x)
