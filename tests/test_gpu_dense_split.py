"""The split form of a residual dense block in TNR_MMA_BF16X3 (-m gpu): conv1 .. conv4 (or stages 1 .. 4 of the gradient mirror) as the
FOUR-stage plan of tnr_conv_sweep, the 64-wide last stage as a Winograd F(2x2, 3x3) launch (ops.dense_block, TNR_DENSE_SPLIT).
  * the four-stage sweep against four direct per-layer launches: bit for bit;
  * the whole split block against an fp64 evaluation of the same five convolutions and epilogues: the project's Winograd bound
    (<= 3 x the error of the one-launch form + 2e-7 of the scale), x1 .. x4 bit-equal to the one-launch form's;
  * determinism, and the policy of ops.dense_block.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NF, GC = 64, 32


def _bf16x3():
    from trainner_amd import hip, ops
    if ops.MMA != hip.MMA_BF16X3:
        pytest.skip("the split form exists in the bf16x3 arithmetic")
    return ops


def _rerun(ops, buf, out, fn):
    """`fn` on the block's buffers with everything the block produces cleared first."""
    buf[..., NF:].zero_()
    out.zero_()
    fn()
    torch.cuda.synchronize()
    return buf.clone(), out.clone()


@pytest.mark.parametrize("grad_shape", [False, True])
@pytest.mark.parametrize("shape", [(1, 8, 32), (1, 10, 20), (2, 40, 72), (4, 32, 32), (3, 128, 128)])
def test_four_stage_sweep_equals_per_layer_launches(shape, grad_shape, mma_mode):
    """conv_chain(stages[:4]) -- the four-stage plan of conv_sweep4_kernel -- against four direct per-layer launches, bit for bit, on
    the dense buffer: one tile, ragged tiles both ways, several images, and (3, 128, 128) = 768 tiles over 256 workgroups (several
    rounds of the dispenser, the last one full).  Three launches: the progress counters and the dispenser are re-used."""
    ops = _bf16x3()
    from tools.probes.sweep_check import block
    run = block(*shape, seed=41, grad_shape=grad_shape, with_r2=False)
    buf, out, st = run("layers")              # (per-layer direct kernels: the reference; st's views alias buf / out)
    ref = buf.clone()
    assert float(ref[..., NF:].abs().max()) > 0.0
    for rep in range(3):
        got, _ = _rerun(ops, buf, out, lambda: ops.conv_chain(st[:4]))
        assert torch.equal(got, ref), "dense buffer differs (rep %d)" % rep
    images = st[0]["wp"].owner.__dict__.get("_sweep_images", {})
    assert any(len(k) == 4 for k in images), "conv_chain(stages[:4]) did not take the four-stage sweep"
    assert ops.chain_error_flag() == 0


def _ref64(ops, st, buf, grad_shape):
    """fp64 evaluation (CPU) of the five stages `st` over the block input buf[..., :NF]: -> (x1 .. x4 as [N, H, W, 128], block output)."""
    packer = st[0]["wp"].owner
    cur = buf[..., :NF].double().cpu().permute(0, 3, 1, 2)

    def view64(v):
        return v.dense().double().cpu().permute(0, 3, 1, 2)

    for k in range(5):
        d = st[k]
        w = packer.jobs[k][0].double().cpu()
        b = d["bias"].double().cpu() if d.get("bias") is not None else None
        v = F.conv2d(cur, w, b, padding=1)
        if d.get("act", ops.ACT_NONE) == ops.ACT_LRELU:
            v = F.leaky_relu(v, d.get("slope", 0.2))
        if k < 4:
            if d.get("mask") is not None:
                v = v * torch.where(view64(d["mask"]) > 0, 1.0, d.get("m_slope", 0.2))
            cur = torch.cat([cur, v], 1)
            continue
        v = v * d.get("alpha", 1.0) + d.get("beta1", 1.0) * cur[:, :NF]
        nz = d.get("noise")
        m = None
        if nz is not None:
            mb = torch.empty_like(buf[..., :NF]).contiguous()
            ops.gauss_mult(ops.View(mb), None, nz)
            torch.cuda.synchronize()
            m = mb.double().cpu().permute(0, 3, 1, 2)
        if m is not None and nz.pos == 1:
            v = v * m
        if d.get("r2") is not None:
            v = v * d.get("alpha2", 1.0) + view64(d["r2"])
        if m is not None and nz.pos != 1:
            v = v * m
        return cur[:, NF:].permute(0, 2, 3, 1).contiguous(), v.permute(0, 2, 3, 1).contiguous()


SPLIT_CASES = [(shape, g, r2, False) for shape in ((2, 40, 72), (1, 64, 96)) for g in (False, True) for r2 in (True, False)] + \
              [((2, 40, 72), False, True, True), ((2, 40, 72), True, True, True)]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: "%dx%dx%d-%s-%s%s" % (*c[0], "grad" if c[1] else "fwd", "r2" if c[2] else "nor2", "-noise" if c[3] else ""))
def test_split_block_error_vs_fp64(case, mma_mode, monkeypatch):
    """The split form of a whole block against fp64: error of the block output and of x1 .. x4 <= 3 x the error of ops.conv_chain (the
    one-launch form) on the same inputs + 2e-7 of the scale -- the bound of test_conv3x3_winograd_form_error_vs_fp64 -- with
    x1 .. x4 bit-equal to conv_chain's, and two runs of the split form bit-identical."""
    ops = _bf16x3()
    from tools.probes.sweep_check import block
    shape, grad_shape, with_r2, noise = case
    nz = ops.Noise(0.1, ops.noise_key(1, 2, 3)) if noise else None
    run = block(*shape, seed=53, grad_shape=grad_shape, with_r2=with_r2, noise=nz)
    buf, out, st = run("layers")
    monkeypatch.setattr(ops, "DENSE_SPLIT", True)
    assert ops.dense_split_applies(st)
    r_mid, r_out = _ref64(ops, st, buf, grad_shape)
    c_buf, c_out = _rerun(ops, buf, out, lambda: ops.conv_chain(st))
    s_buf, s_out = _rerun(ops, buf, out, lambda: ops.dense_block(st))
    s_buf2, s_out2 = _rerun(ops, buf, out, lambda: ops.dense_block(st))
    assert torch.equal(s_buf, c_buf), "x1 .. x4 of the split form differ from conv_chain's"
    assert torch.equal(s_buf, s_buf2) and torch.equal(s_out, s_out2), "the split form is not deterministic"
    assert not torch.equal(s_out, c_out), "the last stage did not run in the Winograd form"

    def err(got, ref):
        d = (got.double().cpu() - ref).abs()
        return float(d.max()), float(d.pow(2).mean().sqrt())

    for what, got, base, ref in (("block output", s_out, c_out, r_out), ("x1..x4", s_buf[..., NF:], c_buf[..., NF:], r_mid)):
        scale = float(ref.abs().max())
        e_split, e_chain = err(got, ref), err(base, ref)
        print("%s %s: split max %.3e rms %.3e, conv_chain max %.3e rms %.3e, scale %.3f" % (case, what, *e_split, *e_chain, scale))
        assert e_split[0] <= 3.0 * e_chain[0] + 2e-7 * scale and e_split[1] <= 3.0 * e_chain[1] + 2e-7 * scale, (what, e_split, e_chain, scale)
    assert ops.chain_error_flag() == 0


def test_dense_block_policy(mma_mode, monkeypatch):
    """ops.dense_block takes the split form for a training-shaped block -- the same form for N = 2 and N = 4 at one grid -- and is
    conv_chain(stages) under bf16 operands, under the fp32 matrix-core arithmetic, with the agreed form "layers", with
    TNR_DENSE_SPLIT=0 and on CPU tensors."""
    ops = _bf16x3()
    from trainner_amd import hip
    from tools.probes.sweep_check import block
    monkeypatch.setattr(ops, "DENSE_SPLIT", True)
    calls = []
    real_chain, real_conv = ops.conv_chain, ops.conv
    monkeypatch.setattr(ops, "conv_chain", lambda stages: (calls.append(("chain", len(stages))), real_chain(stages))[1])
    monkeypatch.setattr(ops, "conv", lambda *a, **k: (calls.append(("conv", k.get("wino"))), real_conv(*a, **k))[1])

    def form(st):
        del calls[:]
        ops.dense_block(st)
        torch.cuda.synchronize()
        top = [c for c in calls if c[0] == "chain"][:1] + [c for c in calls if c == ("conv", True)]
        return top

    split, whole = [("chain", 4), ("conv", True)], [("chain", 5)]
    _, _, st2 = block(2, 32, 64, seed=3, grad_shape=False)("layers")
    _, _, st4 = block(4, 32, 64, seed=3, grad_shape=True)("layers")
    assert form(st2) == split and form(st4) == split
    assert ops.dense_split_applies(st2) and ops.dense_split_applies(st4)
    with monkeypatch.context() as m:
        m.setattr(ops, "MMA", hip.MMA_BF16)
        assert form(st2) == whole
    with monkeypatch.context() as m:
        m.setattr(ops, "MMA", hip.MMA_F32)
        assert form(st2) == whole
    with monkeypatch.context() as m:
        m.setitem(ops.SWEEP_AUTO_STATE, "choice", "layers")
        assert form(st2) == whole
    with monkeypatch.context() as m:
        m.setattr(ops, "DENSE_SPLIT", False)
        assert form(st2) == whole
    cpu = [dict(st, **{k: ops.View(v.buf.cpu(), v.coff, v.C) for k, v in st.items() if isinstance(v, ops.View)}) for st in st2]
    assert not ops.dense_split_applies(cpu)
    assert form(st2) == split
    assert ops.chain_error_flag() == 0


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("shape", [(1, 8, 32), (1, 10, 20)])
def test_plan_names_the_form_the_image_caches_show(shape, split, mma_mode, monkeypatch):
    """ops.dense_block_plan against what ops.dense_block then leaves on the block's packer: "split" = a four-stage sweep image plus the
    last stage's transform-domain stream, "sweep" = a five-stage sweep image alone, "chain" (the fp32 matrix core) = no sweep image."""
    from trainner_amd import hip, ops
    from tools.probes.sweep_check import block
    _, _, st = block(*shape, seed=7, grad_shape=False)("layers")
    monkeypatch.setattr(ops, "DENSE_SPLIT", split)
    form, why = ops.dense_block_plan(st)
    assert why is None and form == ("chain" if ops.MMA != hip.MMA_BF16X3 else "split" if split else "sweep")
    owner = st[0]["wp"].owner
    owner.__dict__.pop("_sweep_images", None)
    owner.__dict__.pop("_wq_images", None)
    ops.dense_block(st)
    torch.cuda.synchronize()
    sweeps = sorted(len(k) for k in owner.__dict__.get("_sweep_images", {}))
    wino = [k for k in owner.__dict__.get("_wq_images", {}) if isinstance(k, tuple) and k[0] == "wino"]
    assert sweeps == {"split": [4], "sweep": [5], "chain": []}[form]
    assert wino == ([("wino", st[4]["wp"].t.data_ptr())] if form == "split" else [])
    assert ops.chain_error_flag() == 0


def test_dense_split_switch_reads_the_environment():
    """TNR_DENSE_SPLIT=0 turns the form off for a process (a fresh interpreter: the switch is read at import)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for val, want in (("0", "False"), ("1", "True")):
        env = dict(os.environ, TNR_DENSE_SPLIT=val)
        r = subprocess.run([sys.executable, "-c", "from trainner_amd import ops; print(ops.DENSE_SPLIT)"], cwd=root, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == want, (r.stdout, r.stderr[-500:])
