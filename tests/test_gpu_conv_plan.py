"""ops.conv_plan names what the REAL library launches (-m gpu): every form of a single convolution at the smallest shape it exists at, driven
through engine.ConvOp behind a recording proxy of the loaded library, and its result against an fp64 convolution on the CPU under the bounds
the kernels already carry (tests/test_gpu_kernels.py): error <= 1.5 x the fp32 matrix core's on the same operands + 2e-7 of the output scale
for the direct forms, 3 x for the Winograd form, and the fp32 round-off tolerance 2e-5 x (scale + 1) for all of them."""
import types

import pytest
import torch
import torch.nn.functional as F

from tools import record_conv_plan as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Proxy:
    """The loaded library, noting the entries of the table (and tnr_conv_forward's descriptor fields at call time) and its three late answers."""

    def __init__(self, lib):
        self.lib, self.calls, self.said = lib, [], {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def entry(*args):
            R.note(self.calls, name, args)
            ret = fn(*args)
            if name in R.LATE:
                self.said[("splitk", "wino_ok", "stream_ok")[R.LATE.index(name)]] = ret > 0
            return ret
        return entry


# name: (how, k, stride, cin, cout, N, H, W, nearest-x2, the form under bf16x3, under the fp32 matrix core)
CASES = {
    "thin_64to3": ("fwd", 3, 1, 64, 3, 1, 16, 16, False, "thin", "thin"),
    "c4_3to64": ("fwd", 3, 1, 3, 64, 1, 16, 16, False, "c4", "c4"),
    "im2col_512to512": ("fwd", 3, 1, 512, 512, 2, 4, 4, False, "im2col", "im2col"),
    "wino_64to64": ("fwd", 3, 1, 64, 64, 1, 64, 64, False, "wino", "tile"),
    "wino_64to64_ragged": ("fwd", 3, 1, 64, 64, 1, 70, 66, False, "wino", "tile"),
    "stream_64to64": ("fwd", 3, 1, 64, 64, 1, 32, 32, False, "stream", "tile"),
    # the four-tap stream kernel tiles 32 pixels of the STRIDE-2 grid: at 32 -> 16 the library declines (the plan's "declined" row, conv_tile
    # runs), at 64 -> 32 the form exists
    "4x4s2_32to16": ("fwd", 4, 2, 64, 64, 1, 32, 32, False, "tile", "tile"),
    "4x4s2_32to16_dgrad": ("dgrad", 4, 2, 64, 64, 1, 32, 32, False, "tile", "tile"),
    "stream_4x4s2": ("fwd", 4, 2, 64, 64, 1, 64, 64, False, "stream", "tile"),
    "stream_4x4s2_dgrad": ("dgrad", 4, 2, 64, 64, 1, 64, 64, False, "stream", "tile"),
    "stream_shuffle": ("shuffle", 3, 1, 64, 256, 1, 32, 32, False, "stream", "tile"),
    "tile_64to32": ("fwd", 3, 1, 64, 32, 1, 32, 32, False, "tile", "tile"),
    "tile_up2": ("fwd", 3, 1, 64, 64, 1, 16, 16, True, "tile", "tile"),
    "shuffle_16_declined": ("shuffle", 3, 1, 64, 256, 1, 16, 16, False, "tile", "tile"),
    "shuffle_20to80_declined": ("shuffle", 3, 1, 20, 80, 1, 32, 32, False, "tile", "tile"),
}


def _rnd(*shape, seed):
    from oracle.detrand import uniform
    return uniform(shape, seed, -1.0, 1.0)


def _nhwc(t, ctot=None):
    """NCHW cpu -> NHWC device buffer of ctot channels (zero pad), as an ops.View of the first C."""
    from trainner_amd import ops
    N, C, H, W = t.shape
    buf = torch.zeros(N, H, W, ctot or C)
    buf[..., :C] = t.permute(0, 2, 3, 1)
    return ops.View(buf.to(DEV).contiguous(), 0, C)


@pytest.mark.parametrize("name", list(CASES))
def test_plan_names_what_the_library_launches(name, mma_mode, monkeypatch):
    from trainner_amd import engine, hip, ops
    how, k, stride, cin, cout, N, H, W, ups, form_x3, form_f32 = CASES[name]
    want = form_x3 if mma_mode == "bf16x3" else form_f32
    seed = 11 + cin + H
    w, b = _rnd(cout, cin, k, k, seed=seed) * (cin * k * k) ** -0.5, _rnd(cout, seed=seed + 1)
    mod = types.SimpleNamespace(kernel_size=k, stride=stride, in_channels=cin, out_channels=cout, weight=w.to(DEV), bias=b.to(DEV))
    packer = ops.WeightPacker(torch.device(DEV))
    op = engine.ConvOp(mod, packer, ups=ups)
    packer.run()
    w64, b64 = w.double(), b.double()
    if how == "dgrad":          # the gradient of the layer's output -> the gradient of its input
        xin = _rnd(N, cout, H // stride, W // stride, seed=seed + 2)
        ref = F.conv_transpose2d(xin.double(), w64, None, stride=stride, padding=1)
    else:
        xin = _rnd(N, cin, H, W, seed=seed + 2)
        up = F.interpolate(xin.double(), scale_factor=2.0, mode="nearest") if ups else xin.double()
        ref = F.conv2d(up, w64, b64, stride=stride, padding=1)
        if how == "shuffle":
            ref = F.pixel_shuffle(ref, 2)
    x = _nhwc(xin, 4 if xin.shape[1] <= 4 else None)
    ychan = ref.shape[1]

    def launch():
        """-> (the output view, the outcome string, conv_plan given the late answers the library gave during the launch)."""
        y = ops.View(torch.full((N, ref.shape[2], ref.shape[3], max(ychan, 4)), 7.0, device=DEV), 0, ychan)
        proxy = Proxy(hip.load())
        with monkeypatch.context() as m:
            m.setattr(hip, "load", lambda *a, **kw: proxy)
            ret = {"fwd": op.fwd, "dgrad": op.dgrad, "shuffle": op.fwd_shuffle2}[how](x, y)
            torch.cuda.synchronize()
        mode, layer = op.dirs[how == "dgrad"]
        epi = {} if how == "dgrad" else {"bias": mod.bias}
        plan = ops.conv_plan(x, packer.get(layer.direct), y, mode, epi, 2 if how == "shuffle" else 0, layer, **proxy.said)
        got = "+".join(proxy.calls) + ("" if ret is None else "=%s" % ret)
        return y, got, plan

    y, got, plan = launch()
    print(name, mma_mode, "plan", plan, "launched", got)
    assert plan[0] == want and R.plan_matches(ops, plan, got), (plan, got)
    if name.startswith("4x4s2_32to16") and mma_mode == "bf16x3":
        assert plan == ("tile", "declined")
    if "declined" in name or (how == "shuffle" and want != "stream"):          # the documented fallback: False, nothing launched, y untouched
        assert got == "=False" and float(y.buf.min()) == 7.0 and float(y.buf.max()) == 7.0
        return
    err = float((y.dense().permute(0, 3, 1, 2).double().cpu() - ref).abs().max())
    monkeypatch.setattr(ops, "MMA", hip.MMA_F32)          # the same operands on the fp32 matrix core
    if how == "shuffle":
        z = ops.View(torch.empty(N, H, W, cout, device=DEV))
        op.fwd(x, z)
        y32 = F.pixel_shuffle(z.dense().permute(0, 3, 1, 2), 2)
    else:
        y32 = launch()[0].dense().permute(0, 3, 1, 2)
    err32 = float((y32.double().cpu() - ref).abs().max())
    scale = float(ref.abs().max())
    print(name, mma_mode, "max err %.3e, fp32 matrix core %.3e, scale %.3e" % (err, err32, scale))
    # the fp64 reference binds every case on its own (the kernels' fp32 round-off tolerance, as in test_bf16x3_split_operand_mode): under the fp32
    # matrix core, and for the vector-ALU form, the second launch is the first one again and the relative bound alone could not fail
    assert err <= 2e-5 * (scale + 1.0), (name, err, scale)
    assert err <= (3.0 if plan[0] == "wino" else 1.5) * err32 + 2e-7 * scale
