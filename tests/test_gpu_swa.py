"""Stochastic weight averaging on the device (-m gpu): the launch tnr_swa_update_guarded through the C ABI, and the SR step with
`use_swa: true` through save / resume / swa_generator().

Kernel level.  Buffer lengths 1, 3, 255, 256, 1027 and one pass of the launch's grid + 257 elements (MAX_GRID blocks of
flat.CHUNK = 256 threads x 4 elements, read from the kernel's source: the grid-stride loop takes a second, short pass), plus 1027
elements behind pointers that are NOT 16-byte aligned (the launch's scalar form).  Every buffer is followed by 64 sentinel floats
that must keep their bits.  Two kinds of snapshots: `train`, base + 1e-3 x noise at scale 0.1, as weights move in training, and
`wide`, magnitudes 1e-6 .. 1e+2 with both signs.  8 updates from n_averaged = 0 and 3 from n_averaged = 1000 cover the three
branches of the lerp form (w = 1, w = 0.5, w < 0.5).  After every update the device buffer is compared with the fp64 running mean
under the project's rule for kernels without a derived bound (test_gpu_membound_kernels.yardstick: device error <= 2 x the error of
the fp32 restatement -- torch.lerp on the CPU, tests/swa_restate.py -- + 2e-7 x scale); no element is left out.  Exact, with
torch.equal: the first update is a copy, p == avg leaves avg alone, p is never written, a set fault latch keeps avg's bits.

Step level: the small SR configuration (nb 1, batch 2, crop 64) with swa_start_iter 2, six steps and a seventh."""
import os
import re

import pytest
import torch

import swa_restate
import test_gpu_step as TS
from oracle import detrand, fixtures as FX, ref_harness as R
from test_gpu_membound_kernels import yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 64


def _one_pass():
    """Elements one pass of the launch's grid covers: MAX_GRID blocks (csrc/optimizers.hip) x flat.CHUNK elements per block."""
    from trainner_amd import flat
    with open(os.path.join(ROOT, "trainner_amd", "csrc", "optimizers.hip")) as fh:
        src = fh.read()
    max_grid = int(re.search(r"constexpr int MAX_GRID = (\d+);", src).group(1))
    assert "grid_chunks(tnr_cdiv64(n, %d))" % flat.CHUNK in src          # the launch's grid: one block per CHUNK elements, capped
    return max_grid * flat.CHUNK


LENGTHS = {"n1": 1, "n3": 3, "n255": 255, "n256": 256, "n1027": 1027, "wrap": _one_pass() + 257}


def _snapshots(n, kind, count, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "train":
        base = 0.1 * torch.randn(n, generator=g)
        return [base + 1e-3 * torch.randn(n, generator=g) for _ in range(count)]
    mag = 10.0 ** (torch.rand(n, generator=g) * 8.0 - 6.0)
    base = mag * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)
    return [base * (1 + 1e-2 * torch.randn(n, generator=g)) for _ in range(count)]


def _launch(avg, p, n, n_averaged, fault=None):
    from trainner_amd import hip
    hip.check(hip.load().tnr_swa_update_guarded(avg.data_ptr(), p.data_ptr(), n, 1.0 / (n_averaged + 1), hip.ptr(fault), hip.stream()), "swa_update")


def _padded(t, shift=0):
    """t on the device, `shift` floats into an allocation, followed by SENT sentinel floats -> (view of the n elements, whole buffer)."""
    full = torch.full((shift + t.numel() + SENT,), -123.0, device=DEV)
    full[shift:shift + t.numel()] = t.to(DEV)
    return full[shift:shift + t.numel()], full


def _run_chain(name, n, kind, start, count, shift=0):
    snaps = _snapshots(n, kind, count + 1, 1000 * len(name) + n % 997 + start)
    first, snaps = snaps[0], snaps[1:]
    avg, avg_full = _padded(first, shift)
    assert (avg.data_ptr() % 16 != 0) == bool(shift)
    a64, a32 = first.double(), first.clone()
    bitwise = True
    for i, p_host in enumerate(snaps):
        na = start + i
        p, p_full = _padded(p_host, shift)
        p_before, avg_before = p_full.clone(), avg.clone()
        _launch(avg, p, n, na)
        torch.cuda.synchronize()
        a64 = swa_restate.mean64(a64, p_host, na)
        a32 = swa_restate.update32(a32, p_host, na, "lerp")
        yardstick("swa %s %s n_averaged %d" % (name, kind, na), avg, a64, a32)
        assert torch.equal(p_full, p_before)                                               # p is only read
        assert torch.equal(avg_full[:shift], torch.full((shift,), -123.0, device=DEV))
        assert torch.equal(avg_full[shift + n:], torch.full((SENT,), -123.0, device=DEV))     # nothing past the n elements
        if na == 0:
            assert torch.equal(avg, p)                                                      # w = 1: an exact copy
        bitwise = bitwise and torch.equal(avg, torch.lerp(avg_before, p, float(torch.tensor(1.0 / (na + 1), dtype=torch.float32))))
    print("SWA-LERP %s %s from %d: bit-identical to torch.lerp on the device: %s" % (name, kind, start, bitwise))
    # averaging a buffer with itself leaves its bits, whatever the weight
    keep = avg.clone()
    for na in (1, 2, 7, 1000):
        _launch(avg, keep.clone(), n, na)
    torch.cuda.synchronize()
    assert torch.equal(avg, keep)


@pytest.mark.parametrize("kind", ["train", "wide"])
@pytest.mark.parametrize("name", list(LENGTHS))
def test_launch_meets_the_fp64_mean(name, kind):
    n = LENGTHS[name]
    _run_chain(name, n, kind, 0, 8)
    _run_chain(name, n, kind, 1000, 3)


@pytest.mark.parametrize("kind", ["train", "wide"])
def test_launch_with_unaligned_pointers(kind):
    _run_chain("unaligned1027", 1027, kind, 0, 8, shift=1)
    _run_chain("unaligned1027", 1027, kind, 1000, 3, shift=3)


@pytest.mark.parametrize("name", ["n3", "n1027", "wrap"])
def test_fault_latch_keeps_the_average(name):
    """With the latch word set the average keeps its bits (it never absorbs a step that was not applied); cleared again, the same
    launch moves it.  Set and cleared as test_gpu_optimizers.test_fault_latch_blocks_every_optimizer does."""
    from trainner_amd import ops
    n = LENGTHS[name]
    a, p = _snapshots(n, "train", 2, 77)
    avg, avg_full = _padded(a)
    p, _ = _padded(p)
    before = avg_full.clone()
    word = ops.fault_word(avg.device)
    try:
        word.fill_(1)
        ops.swa_update(avg, p, 3)
        _launch(avg, p, n, 0, fault=word)
        torch.cuda.synchronize()
        assert torch.equal(avg_full, before)
    finally:
        word.zero_()
    ops.swa_update(avg, p, 3)
    torch.cuda.synchronize()
    assert not torch.equal(avg, before[:n]) and torch.equal(avg_full[n:], before[n:])


def test_launch_refuses_bad_arguments():
    from trainner_amd import hip
    lib = hip.load()
    t = torch.zeros(8, device=DEV)
    assert lib.tnr_swa_update_guarded(t.data_ptr(), t.data_ptr(), 0, 0.5, None, hip.stream()) != 0
    assert lib.tnr_swa_update_guarded(None, t.data_ptr(), 8, 0.5, None, hip.stream()) != 0
    assert lib.tnr_swa_update_guarded(t.data_ptr(), t.data_ptr(), 8, 0.0, None, hip.stream()) != 0
    assert lib.tnr_swa_update_guarded(t.data_ptr(), t.data_ptr(), 8, 1.5, None, hip.stream()) != 0


# ---------------------------------------------------------------------------------------------------------------- step level
KW = dict(nb=1, batch=2, crop=64, d_nf=16)
SWA_START = 2
REPL = [("use_swa: false", "use_swa: true"), ("  lr_steps: [50000, 100000]", "  lr_steps: [1, 100000]"),
        ("  niter: 500000", "  niter: 500000\n  swa_start_iter: %d\n  swa_lr: 5e-5\n  swa_anneal_epochs: 3" % SWA_START)]


def _yaml(tmp_path, resume_state=None):
    yml = R.esrgan_yaml(name="swa_gpu", out_root=str(tmp_path), gpu_ids="[0]", **KW)
    txt = open(yml).read()
    for a, b in REPL + ([("path:\n", "path:\n  resume_state: %s\n" % resume_state)] if resume_state else []):
        assert a in txt, a
        txt = txt.replace(a, b, 1)
    with open(yml, "w") as fh:
        fh.write(txt)
    return yml


def _train_step(m, s):
    LR, HR = detrand.synthetic_pair(KW["batch"], KW["crop"], 8100 + s)
    m.feed_data({"LR": LR, "HR": HR})
    m.optimize_parameters(s)


def test_sr_step_with_swa(tmp_path):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    opt = options.parse(_yaml(tmp_path), is_train=True)
    a = create_model(opt, verbose=False)
    g = detrand.fill_state_dict_({k: v.detach().cpu().clone() for k, v in a.netG.state_dict().items()}, 101)
    d = detrand.fill_state_dict_({k: v.detach().cpu().clone() for k, v in a.netD.state_dict().items()}, 202)
    f = FX.vgg_state(77)
    TS.load_initial(a, g, d, f)
    holder = a.netG.flat_params()
    assert a.swa and a.swa_start_iter == SWA_START and a.swa_model.flat.numel() == holder.flat.numel()
    # the learning rates of a twin on the host: torch.optim.Adam + the recipe's MultiStepLR + SWALR
    twin = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-4)
    sched = torch.optim.lr_scheduler.MultiStepLR(twin, [1, 100000], 0.5)
    swalr = torch.optim.swa_utils.SWALR(twin, swa_lr=5e-5, anneal_epochs=3, anneal_strategy="cos")
    import warnings
    a64 = a32 = None
    for s in range(1, 7):
        _train_step(a, s)
        snap = holder.flat.detach().cpu().clone()                      # G's flat parameters after the step
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a.update_learning_rate(s, warmup_iter=-1)
            (swalr if s > SWA_START else sched).step()
        assert a.optimizer_G.param_groups[0]["lr"] == twin.param_groups[0]["lr"], s
        assert a.get_current_learning_rate(s) == (swalr if s > SWA_START else sched).get_last_lr()[0], s
        if s > SWA_START:
            na = s - SWA_START - 1
            a64 = swa_restate.mean64(a64, snap, na)
            a32 = swa_restate.update32(a32, snap, na, "lerp")
            assert int(a.swa_model.n_averaged) == na + 1
            yardstick("swa SR step %d" % s, a.swa_model.flat, a64, a32)
        else:
            assert int(a.swa_model.n_averaged) == 0
    dict(a.get_current_log())
    assert int(a.swa_model.n_averaged) == 4 and a.swa_model.n_averaged.dtype == torch.int64
    assert a.optimizer_G.param_groups[0]["lr"] == 5e-5 and a.optimizer_G.param_groups[0]["swa_lr"] == 5e-5
    # ---- save / resume: a fresh model carries the same average bit for bit
    a.save(6)
    a.save_training_state(0, 6)
    models = opt["path"]["models"]
    assert sorted(os.listdir(models)) == ["6_D.pth", "6_G.pth", "6_swaG.pth"]
    state_path = os.path.join(opt["path"]["training_state"], "6.state")
    ropt = options.parse(_yaml(tmp_path, state_path), is_train=True)
    resume_state = torch.load(ropt["path"]["resume_state"], weights_only=False)
    assert len(resume_state["swa_scheduler"]) == 1
    options.check_resume(ropt)
    assert ropt["path"]["pretrain_model_swaG"].endswith("6_swaG.pth")
    b = create_model(ropt, verbose=False)
    b.resume_training(resume_state)
    b.update_schedulers(ropt["train"])
    assert torch.equal(b.swa_model.flat, a.swa_model.flat) and int(b.swa_model.n_averaged) == 4 and b.swa_model._n == 4
    assert b.swa_scheduler.state_dict() == a.swa_scheduler.state_dict()
    assert [g_["lr"] for g_ in b.optimizer_G.param_groups] == [g_["lr"] for g_ in a.optimizer_G.param_groups]
    # ---- swa_generator(): test() on the average == a generator loaded with the file's weights (`module.` stripped)
    sd = torch.load(os.path.join(models, "6_swaG.pth"), weights_only=False)
    assert list(sd)[0] == "n_averaged" and int(sd["n_averaged"]) == 4
    b.netG.load_state_dict({k[len("module."):]: v for k, v in sd.items() if k != "n_averaged"}, strict=True)
    LR = detrand.uniform((2, 3, 12, 20), 31, 0.0, 1.0)
    b.feed_data({"LR": LR}, need_HR=False)
    b.test()
    want = b.fake_H.detach().clone()
    before = holder.flat.detach().clone()
    a.feed_data({"LR": LR}, need_HR=False)
    a.test()
    trained = a.fake_H.detach().clone()
    with a.swa_generator():
        a.test()
        got = a.fake_H.detach().clone()
    assert torch.equal(got, want) and not torch.equal(got, trained)
    assert torch.equal(holder.flat, before) and a.netG.flat_params() is holder
    a.test()
    assert torch.equal(a.fake_H, trained)                       # the training weights are back in every derived image of them
    # ---- and training goes on
    _train_step(a, 7)
    a.update_learning_rate(7, warmup_iter=-1)
    log = dict(a.get_current_log())
    assert all(v == v for v in log.values()) and int(a.swa_model.n_averaged) == 5 and not torch.equal(holder.flat, before)


def test_shipped_recipe_with_use_swa_steps_past_swa_start_iter(tmp_path, monkeypatch):
    """The reference's options/sr/train_sr.yml with its `use_swa` switch turned on and nothing else changed: the four-line block
    under it (swa_start_iter_rel 0.75 of niter 5e5, swa_lr 1e-4, 10 anneal epochs, cos) constructs, and the steps on either side of
    swa_start_iter run (ESRGAN+ noise and use_amp on, as shipped): the first step past it averages and hands G to the SWA scheduler."""
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml, _ = TS.shipped_recipe(tmp_path, monkeypatch)

    def switch_on(tree):
        assert tree["use_swa"] is False and tree["train"]["swa_start_iter_rel"] == 0.75
        tree["use_swa"] = True

    opt = options.parse(FX.write_recipe("sr/train_sr.yml", str(tmp_path), edit=switch_on), is_train=True)
    start = opt["train"]["swa_start_iter"]
    assert start == 375000 and opt["use_swa"] is True
    torch.manual_seed(opt["train"]["manual_seed"])
    model = create_model(opt, verbose=False)
    assert model.swa and model.swa_start_iter == start and model.optimizer_G.param_groups[0]["swa_lr"] == 1e-4
    import warnings
    for s in (start, start + 1):
        LR, HR = detrand.synthetic_pair(opt["datasets"]["train"]["batch_size"], opt["datasets"]["train"]["crop_size"], 500 + s % 7)
        model.feed_data({"LR": LR, "HR": HR})
        model.optimize_parameters(s)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model.update_learning_rate(s, warmup_iter=opt["train"].get("warmup_iter") or -1)
        log = model.get_current_log()
        assert all(v == v and abs(v) < 1e4 for v in log.values()), log
        assert int(model.swa_model.n_averaged) == s - start
    assert torch.equal(model.swa_model.flat, model.netG.flat_params().flat)          # one update: the average is the step's weights
    assert model.get_current_learning_rate(start + 1) == model.swa_scheduler.get_last_lr()[0] == model.optimizer_G.param_groups[0]["lr"]
