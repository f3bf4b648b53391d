"""LPIPS validation metric on the device (csrc/lpips.hip + tnr_conv_forward) against the REAL reference's values
(tests/golden/lpips_squeeze.pt, tools/make_golden_lpips.py) and an fp64 torch restatement, in both fp32 arithmetics (mma_mode)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tools import make_golden_lpips as G

FX = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_squeeze.pt"), weights_only=False)
PAIRS = {p["name"]: p for p in FX["pairs"]}
TV = G.seeded_backbone_state(FX["seed"], FX["gain"])


def bound(ref):
    return 1e-4 * abs(ref) + 1e-6


def model():
    from trainner_amd.models.modules.LPIPS.perceptual_loss import PerceptualLoss
    m = PerceptualLoss(allow_random_init=True)
    m.load_torchvision_state(TV)
    m.load_heads(FX["lin"])
    return m


@pytest.mark.gpu
def test_golden_pairs(mma_mode):
    m = model()
    for p in FX["pairs"]:
        total, per_layer = m.distance_u8(p["img1"], p["img2"], crop=p["crop"], per_layer=True)
        assert total.dtype == torch.float64 and tuple(per_layer.shape) == (1, 7)
        t64, l64 = G.restate(TV, FX["lin"], p["img1"], p["img2"], crop=p["crop"])
        got = float(total[0])
        assert abs(got - p["total"]) <= bound(p["total"]), (p["name"], got, p["total"])
        assert abs(got - t64) <= bound(t64), (p["name"], got, t64)
        assert abs(got - float(per_layer[0].sum())) <= 1e-15
        for l in range(7):
            g = float(per_layer[0, l])
            assert abs(g - p["per_layer"][l]) <= bound(p["per_layer"][l]), (p["name"], l, g, p["per_layer"][l])
            assert abs(g - l64[l]) <= bound(l64[l]), (p["name"], l, g, l64[l])
    # +-1 in a dozen pixels: far below the bound above; nonzero and close to fp64
    p = PAIRS["pm1"]
    got = float(m.distance_u8(p["img1"], p["img2"], crop=p["crop"])[0])
    t64, _ = G.restate(TV, FX["lin"], p["img1"], p["img2"], crop=p["crop"])
    assert got > 0 and abs(got - t64) <= 5e-2 * t64, (got, t64)


@pytest.mark.gpu
def test_identity_symmetry_determinism(mma_mode):
    m = model()
    p = PAIRS["odd35x50"]
    a, b = p["img1"], p["img2"]
    assert float(m.distance_u8(a, a, crop=4)[0]) == 0.0
    assert float(m.distance_u8(PAIRS["same"]["img1"], PAIRS["same"]["img2"], crop=4)[0]) == 0.0
    d_ab = m.distance_u8(a, b, crop=4)
    d_ba = m.distance_u8(b, a, crop=4)
    assert abs(float(d_ab[0]) - float(d_ba[0])) <= 1e-7 * abs(float(d_ab[0]))
    t1, l1 = m.distance_u8(a, b, crop=4, per_layer=True)
    t2, l2 = m.distance_u8(a, b, crop=4, per_layer=True)
    assert torch.equal(t1, t2) and torch.equal(l1, l2)
    # a batch: per image within the golden bound (the batch may pick other conv forms than single images)
    A = torch.stack([PAIRS["even66"]["img1"], PAIRS["pm1"]["img1"], PAIRS["even66"]["img1"]])
    B = torch.stack([PAIRS["even66"]["img2"], PAIRS["pm1"]["img2"], PAIRS["even66"]["img1"]])
    tb = m.distance_u8(A.cuda(), B.cuda(), crop=4)
    assert abs(float(tb[0]) - PAIRS["even66"]["total"]) <= bound(PAIRS["even66"]["total"])
    assert abs(float(tb[1]) - PAIRS["pm1"]["total"]) <= bound(PAIRS["pm1"]["total"]) and float(tb[2]) == 0.0


@pytest.mark.gpu
def test_chunked_batch(mma_mode, monkeypatch):
    """A batch split into several chunks (one pair per chunk here) gives the values of the whole batch."""
    from trainner_amd.models.modules.LPIPS import networks_basic as NB
    m = model()
    A = torch.stack([PAIRS["even66"]["img1"], PAIRS["pm1"]["img1"], PAIRS["even66"]["img2"]]).cuda()
    B = torch.stack([PAIRS["even66"]["img2"], PAIRS["pm1"]["img2"], PAIRS["even66"]["img1"]]).cuda()
    whole = m.distance_u8(A, B, crop=4)
    monkeypatch.setattr(NB, "CHUNK_ELEMS", 1)
    chunked = m.distance_u8(A, B, crop=4)
    for x, y in zip(whole.tolist(), chunked.tolist()):
        assert abs(x - y) <= bound(y)


@pytest.mark.gpu
def test_amp_policy_does_not_change_lpips(mma_mode):
    from trainner_amd import hip, ops
    m = model()
    p = PAIRS["sq128"]
    base = m.distance_u8(p["img1"], p["img2"], crop=4, per_layer=True)
    prev, ops.MMA = ops.MMA, hip.MMA_BF16
    try:
        amp = m.distance_u8(p["img1"], p["img2"], crop=4, per_layer=True)
        assert ops.MMA == hip.MMA_BF16
    finally:
        ops.MMA = prev
    assert torch.equal(base[0], amp[0]) and torch.equal(base[1], amp[1])


@pytest.mark.gpu
def test_maxpool3s2_ceil_bit_identical(mma_mode):
    from trainner_amd import hip
    from trainner_amd.ops import View
    lib = hip.load()
    g = torch.Generator(device="cpu").manual_seed(5)
    for C_ in (64, 128, 256):
        for H in (3, 4, 15, 16, 31, 32, 67):
            for W in (3, 4, 15, 16, 31, 32, 67):
                x = torch.randn((2, H, W, C_), generator=g).cuda()
                want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, ceil_mode=True).permute(0, 2, 3, 1)
                ho, wo = hip.c_i(), hip.c_i()
                hip.check(lib.tnr_maxpool3s2_ceil_dims(H, W, C.byref(ho), C.byref(wo)))
                assert (ho.value, wo.value) == tuple(want.shape[1:3]), (H, W)
                y = torch.full((2, ho.value, wo.value, C_), float("nan"), device="cuda")
                hip.check(lib.tnr_maxpool3s2_ceil_fwd(View(x).c(), View(y).c(), 2, H, W, C_, hip.stream()))
                assert torch.equal(y, want.contiguous()), (H, W, C_)
    # channel windows of wider buffers (the Fire concat buffers)
    x = torch.randn((1, 16, 15, 128), generator=g).cuda()
    y = torch.zeros((1, 8, 7, 192), device="cuda")
    hip.check(lib.tnr_maxpool3s2_ceil_fwd(View(x, 64, 64).c(), View(y, 128, 64).c(), 1, 16, 15, 64, hip.stream()))
    want = F.max_pool2d(x[..., 64:].permute(0, 3, 1, 2), 3, 2, ceil_mode=True).permute(0, 2, 3, 1)
    assert torch.equal(y[..., 128:], want) and torch.count_nonzero(y[..., :128]) == 0


def _stem_ref(x_nchw, w, b):
    """fp64 ScalingLayer + conv 3x3 s2 + ReLU of fp32 [-1, 1] images."""
    shift = torch.tensor([-.030, -.088, -.188], dtype=torch.float64).view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], dtype=torch.float64).view(1, 3, 1, 1)
    return F.relu(F.conv2d((x_nchw.double() - shift) / scale, w.double(), b.double(), stride=2)).permute(0, 2, 3, 1)


@pytest.mark.gpu
def test_stem_kernel(mma_mode):
    from trainner_amd import hip
    from trainner_amd.ops import View
    lib = hip.load()
    g = torch.Generator(device="cpu").manual_seed(9)
    w = (torch.rand((64, 3, 3, 3), generator=g) - 0.5)
    b = (torch.rand(64, generator=g) - 0.5) * 0.2
    shift = torch.tensor([-.030, -.088, -.188]).cuda()
    scale = torch.tensor([.458, .448, .450]).cuda()
    wd, bd = w.cuda(), b.cuda()
    N, H, W, crop = 2, 29, 40, 3
    a8 = (torch.rand((N, H, W, 3), generator=g) * 256).floor().to(torch.uint8)
    b8 = (torch.rand((N, H, W, 3), generator=g) * 256).floor().to(torch.uint8)
    Ho, Wo = (H - 2 * crop - 3) // 2 + 1, (W - 2 * crop - 3) // 2 + 1
    y = torch.full((2 * N, Ho, Wo, 64), float("nan"), device="cuda")
    a8d, b8d = a8.cuda(), b8.cuda()                               # (device copies held for the launch)
    hip.check(lib.tnr_lpips_stem(a8d.data_ptr(), b8d.data_ptr(), 0, N, H, W, 3, crop, 0, shift.data_ptr(), scale.data_ptr(),
                                 wd.data_ptr(), bd.data_ptr(), View(y).c(), hip.stream()), "stem u8")
    imgs = torch.cat([a8, b8])[:, crop:H - crop, crop:W - crop, :]
    x = torch.from_numpy((imgs.numpy() / 127.5 - 1.0).astype(np.float32)).permute(0, 3, 1, 2)
    ref = _stem_ref(x, w, b)
    assert tuple(y.shape) == tuple(ref.shape)
    assert (y.cpu().double() - ref).abs().max().item() < 2e-5
    # fp32 NCHW inputs in [0, 1] with normalize (2 x - 1 first), no crop
    xa = torch.rand((N, 3, H, W), generator=g)
    xb = torch.rand((N, 3, H, W), generator=g)
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    y = torch.full((2 * N, Ho, Wo, 64), float("nan"), device="cuda")
    xad, xbd = xa.cuda(), xb.cuda()
    hip.check(lib.tnr_lpips_stem(xad.data_ptr(), xbd.data_ptr(), 1, N, H, W, 3, 0, 1, shift.data_ptr(), scale.data_ptr(),
                                 wd.data_ptr(), bd.data_ptr(), View(y).c(), hip.stream()), "stem f32")
    ref = _stem_ref(torch.cat([xa, xb]) * 2 - 1, w, b)
    assert (y.cpu().double() - ref).abs().max().item() < 2e-5


@pytest.mark.gpu
def test_head_kernel(mma_mode):
    from trainner_amd import hip
    from trainner_amd.ops import View
    lib = hip.load()
    g = torch.Generator(device="cpu").manual_seed(13)
    L, N = 3, 2
    shapes = [(33, 20, 64), (9, 7, 384), (2, 3, 512)]
    ws = torch.empty(lib.tnr_lpips_workspace_bytes(N, L) // 8, dtype=torch.float64, device="cuda")
    want = torch.zeros((N, L), dtype=torch.float64)
    keep = []
    for l, (H, W, C_) in enumerate(shapes):
        f = torch.relu(torch.randn((2 * N, H, W, C_), generator=g))
        f[1, :H // 2] = f[N + 1, :H // 2]                       # identical half: exact zero contributions
        f[0, 0, 0] = 0.0                                          # an all-zero feature vector (norm 0 + eps)
        w = torch.rand(C_, generator=g)
        fd, wd = f.cuda(), w.cuda()
        keep += [fd, wd]
        hip.check(lib.tnr_lpips_head(View(fd[:N]).c(), View(fd[N:]).c(), N, H, W, C_, wd.data_ptr(), l, L, ws.data_ptr(), ws.numel() * 8,
                                     hip.stream()), "head")
        f64 = f.double()
        nrm = f64 / (f64.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
        want[:, l] = ((nrm[:N] - nrm[N:]) ** 2 * w.double()).sum(-1).mean(dim=(1, 2))
    out = torch.empty(N, dtype=torch.float64, device="cuda")
    per = torch.empty((N, L), dtype=torch.float64, device="cuda")
    hip.check(lib.tnr_lpips_finalize(N, L, ws.data_ptr(), ws.numel() * 8, out.data_ptr(), per.data_ptr(), hip.stream()), "finalize")
    assert torch.allclose(per.cpu(), want, rtol=1e-12, atol=0), (per.cpu(), want)
    assert torch.allclose(out.cpu(), want.sum(1), rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_forward_on_tensors(mma_mode):
    """PerceptualLoss.forward(pred, target) on NCHW tensors in [-1, 1] (and [0, 1] with normalize) = the uint8 path's values."""
    m = model()
    p = PAIRS["even66"]
    crop = lambda t: t[4:-4, 4:-4, :]                              # noqa: E731
    a = torch.from_numpy((crop(p["img1"]).numpy() / 127.5 - 1.0).astype(np.float32)).permute(2, 0, 1)[None].contiguous().cuda()
    b = torch.from_numpy((crop(p["img2"]).numpy() / 127.5 - 1.0).astype(np.float32)).permute(2, 0, 1)[None].contiguous().cuda()
    d = m(b, a)
    assert d.shape == (1,) and float(d[0]) == float(m.distance_u8(p["img1"], p["img2"], crop=4)[0])
    dn = m((b + 1) / 2, (a + 1) / 2, normalize=True)
    assert abs(float(dn[0]) - p["total"]) <= bound(p["total"])


@pytest.mark.gpu
def test_metrics_dict_batch(mma_mode):
    from trainner_amd.utils.metrics import MetricsDict, calculate_lpips
    m = model()
    A = torch.stack([PAIRS["even66"]["img1"], PAIRS["pm1"]["img1"]]).cuda()
    B = torch.stack([PAIRS["even66"]["img2"], PAIRS["pm1"]["img2"]]).cuda()
    md = MetricsDict("psnr,ssim,lpips", lpips_model=m)
    plain = MetricsDict("psnr,ssim")
    got = md.calculate_metrics(A, B, crop_size=4)
    base = plain.calculate_metrics(A, B, crop_size=4)
    assert got["psnr"] == base["psnr"] and got["ssim"] == base["ssim"]
    per = m.distance_u8(A, B, crop=4)
    assert got["lpips"] == float(per[1]) and md.count == 2
    assert abs(md.lpips_sum - float(per.sum())) <= 1e-18
    avg, avg0 = md.get_averages(), plain.get_averages()
    assert avg["psnr"] == avg0["psnr"] and avg["ssim"] == avg0["ssim"]
    assert abs(avg["lpips"] - float(per.mean())) <= 1e-15 and md.count == 0
    assert abs(avg["lpips"] - (PAIRS["even66"]["total"] + PAIRS["pm1"]["total"]) / 2) <= bound(PAIRS["even66"]["total"])
    # the reference's calculate_lpips: a list of image pairs -> their mean
    c = calculate_lpips([PAIRS["even66"]["img1"].numpy(), PAIRS["odd35x50"]["img1"].numpy()],
                        [PAIRS["even66"]["img2"].numpy(), PAIRS["odd35x50"]["img2"].numpy()], model=m)
    full = [float(m.distance_u8(PAIRS[n]["img1"], PAIRS[n]["img2"])[0]) for n in ("even66", "odd35x50")]
    assert abs(c.item() - sum(full) / 2) <= 1e-15


def _weight_files(root, monkeypatch):
    hub = os.path.join(root, "torch_home")
    lp = os.path.join(root, "lpips_weights")
    os.makedirs(os.path.join(hub, "hub", "checkpoints"), exist_ok=True)
    os.makedirs(os.path.join(lp, "v0.1"), exist_ok=True)
    torch.save(TV, os.path.join(hub, "hub", "checkpoints", "squeezenet1_1-b8a52dc0.pth"))
    torch.save(FX["lin"], os.path.join(lp, "v0.1", "squeeze.pth"))
    monkeypatch.setenv("TORCH_HOME", hub)
    monkeypatch.setenv("TNR_LPIPS_WEIGHTS", lp)
    return hub, lp


@pytest.mark.gpu
def test_weight_resolution_on_device(tmp_path, monkeypatch, mma_mode):
    from trainner_amd.models.modules.LPIPS.perceptual_loss import LPIPSWeightsUnavailable, PerceptualLoss
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "empty_hub"))
    monkeypatch.delenv("TNR_LPIPS_WEIGHTS", raising=False)
    with pytest.raises(LPIPSWeightsUnavailable) as e:
        PerceptualLoss()
    assert isinstance(e.value, NotImplementedError) and "squeezenet1_1-b8a52dc0.pth" in str(e.value) and "squeeze.pth" in str(e.value)
    hub, lp = _weight_files(str(tmp_path), monkeypatch)
    m = PerceptualLoss()
    assert m.weights_source == {"net": os.path.join(hub, "hub", "checkpoints", "squeezenet1_1-b8a52dc0.pth"),
                                "lin": os.path.join(lp, "v0.1", "squeeze.pth")}
    p = PAIRS["odd35x50"]
    assert abs(float(m.distance_u8(p["img1"], p["img2"], crop=4)[0]) - p["total"]) <= bound(p["total"])


@pytest.mark.gpu
def test_shipped_recipe_metrics_score_model_output(tmp_path, monkeypatch, mma_mode):
    """options/sr/train_sr.yml's metrics 'psnr,ssim,lpips' with the two weight files present: the validation block of train.py
    (SRModel.test -> tensor2np -> MetricsDict(crop = scale)) scores LPIPS next to PSNR / SSIM."""
    import test_gpu_step as TS
    from oracle import detrand, fixtures as FXM
    from trainner_amd.dataops.common import tensor2np
    from trainner_amd.options import options
    from trainner_amd.utils.metrics import MetricsDict
    shipped = options.parse(FXM.write_recipe("sr/train_sr.yml", str(tmp_path / "recipe")), is_train=True)
    metrics = shipped["train"]["metrics"]
    assert metrics == "psnr,ssim,lpips"
    _weight_files(str(tmp_path), monkeypatch)
    md = MetricsDict(metrics)
    opt, sr_model = TS.build_engine_model(dict(nb=1, batch=1, crop=64, d_nf=16), tmp_path / "run")
    g = detrand.fill_state_dict_({k: v.detach().cpu().clone() for k, v in sr_model.netG.state_dict().items()}, 303)
    sr_model.netG.load_state_dict(g)
    LR, HR = detrand.synthetic_pair(1, 64, 77)
    sr_model.feed_data({"LR": LR, "HR": HR})
    sr_model.test()
    vis = sr_model.get_current_visuals()
    sr8, hr8 = tensor2np(vis["SR"].cuda()), tensor2np(vis["HR"].cuda())
    got = md.calculate_metrics(sr8, hr8, crop_size=opt["scale"])
    assert set(got) == {"psnr", "ssim", "lpips"}
    t64, _ = G.restate(TV, FX["lin"], sr8.cpu(), hr8.cpu(), crop=opt["scale"])
    assert got["lpips"] > 0 and abs(got["lpips"] - t64) <= bound(t64), (got["lpips"], t64)
    assert set(md.get_averages()) == {"psnr", "ssim", "lpips"}
