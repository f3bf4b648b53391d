"""Thin Python wrappers over the C ABI: NHWC views, packed weights, per-device workspaces.

Nothing here computes with torch; torch only allocates the buffers the kernels read and write.
"""
import collections
import ctypes as C
import math
import os

import torch

from . import hip
from .hip import (ACT_LRELU, ACT_NONE, ACT_RELU, CONV_1x1, CONV_3x3, CONV_3x3_C4, CONV_3x3_UP2, CONV_4x4_S2, CONV_7x7_C4, DGRAD_4x4_S2,  # noqa: F401
                  PACK_C4_DGRAD3, PACK_C4_FWD, PACK_COL_DGRAD3, PACK_COL_FWD, PACK_DENSE_DGRAD, PACK_DGRAD_3x3, PACK_DGRAD_S2, PACK_FWD, PACK_FWD_S2D, PACK_UP2_DGRAD_S2,
                  PACK_UP2_FWD_S2D, CView,
                  ConvDesc,
                  DensePackItem, PackItem, WgradDesc)


def round_up(a, b):
    return (a + b - 1) // b * b


class View:
    """Channels [coff, coff+C) of an fp32 NHWC buffer [N,H,W,Ctot]."""
    __slots__ = ("buf", "coff", "C")

    def __init__(self, buf, coff=0, C=None):
        assert buf.dim() == 4 and buf.dtype == torch.float32 and buf.is_contiguous()
        self.buf, self.coff = buf, coff
        self.C = buf.shape[3] - coff if C is None else C
        assert 0 <= coff and coff + self.C <= buf.shape[3]

    N = property(lambda s: s.buf.shape[0])
    H = property(lambda s: s.buf.shape[1])
    W = property(lambda s: s.buf.shape[2])
    ctot = property(lambda s: s.buf.shape[3])
    pixels = property(lambda s: s.buf.shape[0] * s.buf.shape[1] * s.buf.shape[2])

    def sub(self, off, C):
        return View(self.buf, self.coff + off, C)

    def c(self):
        return CView(self.buf.data_ptr(), self.buf.shape[3], self.coff)

    def dense(self):
        """torch view [N,H,W,C] of this window (debug / tests only)."""
        return self.buf[..., self.coff:self.coff + self.C]


def new_act(N, H, W, C, device):
    """Uninitialised NHWC activation buffer."""
    return torch.empty((N, H, W, C), dtype=torch.float32, device=device)


def cv(v):
    return hip.NULLVIEW if v is None else v.c()


# ----------------------------------------------------------------------------------------------
# workspaces (per device, grown on demand; all kernels of one engine run on one stream)
# ----------------------------------------------------------------------------------------------
class _Workspaces:
    def __init__(self):
        self.bufs = {}

    def get(self, name, nbytes, device):
        key = (name, str(device))
        t = self.bufs.get(key)
        if t is None or t.numel() * 8 < nbytes:
            n = max(int(nbytes * 1.25) // 8 + 1, 1024)
            t = torch.empty(n, dtype=torch.float64, device=device)
            self.bufs[key] = t
        return t


WS = _Workspaces()


# ----------------------------------------------------------------------------------------------
# weight packing
# ----------------------------------------------------------------------------------------------
class Packed:
    """A packed weight slab; `owner` = the packer whose run() rewrites it (owner.gen counts those runs), None for one-off packs."""
    __slots__ = ("t", "KoutP", "KinP", "kind", "owner")

    def __init__(self, t, KoutP, KinP, kind, owner=None):
        self.t, self.KoutP, self.KinP, self.kind, self.owner = t, KoutP, KinP, kind, owner


def pack_dims(Cout, Cin, kh, kw, kind):
    lib = hip.load()
    ko, ki, n = hip.c_i(), hip.c_i(), hip.c_l()
    hip.check(lib.tnr_pack_dims(Cout, Cin, kh, kw, kind, C.byref(ko), C.byref(ki), C.byref(n)), "pack_dims")
    return ko.value, ki.value, n.value


class WeightPacker:
    """One device table of pack jobs for a whole network; `run()` re-lays out every weight with a
    single launch (weights change every optimiser step)."""

    def __init__(self, device):
        self.device = device
        self.jobs = []          # (weight tensor, kind)
        self.packed = []
        self.table = None
        self.max_out = 0
        self.flat = None
        self.gen = 0            # completed run() calls (consumers of derived layouts -- the sweep images -- compare it)

    def add(self, w, kind):
        Cout, Cin, kh, kw = w.shape
        ko, ki, n = pack_dims(Cout, Cin, kh, kw, kind)
        self.jobs.append((w, kind, ko, ki, n))
        self.packed.append(None)
        self.table = None
        return len(self.jobs) - 1

    def _finalize(self):
        self.__dict__.pop("_sweep_images", None)       # derived layouts of the old slabs
        self.__dict__.pop("_wq_images", None)
        total = sum(round_up(j[4], 64) for j in self.jobs)
        self.flat = torch.empty(total, dtype=torch.float32, device=self.device)
        items = (PackItem * len(self.jobs))()
        off = 0
        for i, (w, kind, ko, ki, n) in enumerate(self.jobs):
            seg = self.flat[off:off + n]
            off += round_up(n, 64)
            Cout, Cin, kh, kw = w.shape
            items[i] = PackItem(w.data_ptr(), seg.data_ptr(), Cout, Cin, kh, kw, kind, ko, ki, n)
            self.packed[i] = Packed(seg, ko, ki, kind, self)
            self.max_out = max(self.max_out, n)
        raw = bytes(items)
        self.table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)
        self._ptrs = [j[0].data_ptr() for j in self.jobs]

    def get(self, idx):
        if self.table is None:
            self._finalize()
        return self.packed[idx]

    def run(self):
        if not self.jobs:
            return
        if self.table is None or any(j[0].data_ptr() != p for j, p in zip(self.jobs, self._ptrs)):
            self._finalize()
        hip.check(hip.load().tnr_pack_weights(self.table.data_ptr(), len(self.jobs), self.max_out, hip.stream()),
                  "pack_weights")
        self.gen += 1


class DensePacker:
    """Packs the 'gradient dense block' slabs (tnr_pack_dense_dgrad) of every dense block of a network
    with one launch.  add() takes the five conv weights of a block and the block's residual scale."""

    def __init__(self, device):
        self.device = device
        self.jobs = []          # (weights[5], t, nf, gc, scale5, ko, ki, n)
        self.packed = []
        self.table = None
        self.max_out = 0
        self.gen = 0

    def add_block(self, weights, nf, gc, scale5):
        """-> list of 5 job indices (t = 0..4)."""
        lib = hip.load()
        idx = []
        for t in range(5):
            ko, ki, n = hip.c_i(), hip.c_i(), hip.c_l()
            hip.check(lib.tnr_pack_dense_dims(nf, gc, t, C.byref(ko), C.byref(ki), C.byref(n)), "pack_dense_dims")
            self.jobs.append((list(weights), t, nf, gc, float(scale5), ko.value, ki.value, n.value))
            self.packed.append(None)
            idx.append(len(self.jobs) - 1)
        self.table = None
        return idx

    def _finalize(self):
        self.__dict__.pop("_sweep_images", None)
        self.__dict__.pop("_wq_images", None)          # (dense_block: the transform-domain stream of the mirror's last stage)
        total = sum(round_up(j[7], 64) for j in self.jobs)
        self.flat = torch.empty(total, dtype=torch.float32, device=self.device)
        items = (DensePackItem * len(self.jobs))()
        off = 0
        for i, (ws, t, nf, gc, sc, ko, ki, n) in enumerate(self.jobs):
            seg = self.flat[off:off + n]
            off += round_up(n, 64)
            it = DensePackItem()
            for k in range(5):
                it.w[k] = ws[k].data_ptr()
            it.wp, it.nf, it.gc, it.t, it.KoutP, it.KinP, it.scale5, it.n_out = seg.data_ptr(), nf, gc, t, ko, ki, sc, n
            items[i] = it
            self.packed[i] = Packed(seg, ko, ki, PACK_DENSE_DGRAD, self)
            self.max_out = max(self.max_out, n)
        self.table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(self.device)
        self._ptrs = [w.data_ptr() for j in self.jobs for w in j[0]]

    def get(self, idx):
        if self.table is None:
            self._finalize()
        return self.packed[idx]

    def run(self):
        if not self.jobs:
            return
        if self.table is None or [w.data_ptr() for j in self.jobs for w in j[0]] != self._ptrs:
            self._finalize()
        hip.check(hip.load().tnr_pack_dense_dgrad(self.table.data_ptr(), len(self.jobs), self.max_out, hip.stream()),
                  "pack_dense_dgrad")
        self.gen += 1


# ----------------------------------------------------------------------------------------------
# spectral normalisation (csrc/spectral_norm.hip)
# ----------------------------------------------------------------------------------------------
SN_ROWS_PER_TILE, SN_COLS_PER_TILE, SN_COLS_PER_SUM, SN_ROWS_PER_DOT, SN_CHUNK = 16, 1024, 256, 4, 4096
SN_EPS = 1e-12
_SN_FIELDS = ("w", "wn", "u", "v", "ru", "rv", "sig", "g", "dw")


class SpectralNormTable:
    """The device job table and tile tables of tnr_sn_forward / tnr_sn_backward for the wrapped layers of one network.
    layers: one dict per layer with the fp32 tensors w [rows, ...] (the parameter), wn (derived, same shape), u [rows], v [K], the record
    ru [rows], rv [K], sig [1], and for the backward g (gradient w.r.t. wn) and dw (the parameter's gradient); g / dw may be None for a
    table that is only run forward."""

    def __init__(self, layers, device):
        self.layers, self.device = list(layers), device
        self._ptrs = None

    def dims(self, i):
        w = self.layers[i]["w"]
        return w.shape[0], w.numel() // w.shape[0]

    def _build(self):
        words = hip.load().tnr_sn_job_words()
        assert words == 16
        n_t = n_s = n_g = n_c = 0
        geo = []
        for i in range(len(self.layers)):
            rows, K = self.dims(i)
            nrb, nch = (rows + SN_ROWS_PER_TILE - 1) // SN_ROWS_PER_TILE, (rows * K + SN_CHUNK - 1) // SN_CHUNK
            geo.append((rows, K, nrb, nch, n_t, n_g, n_s, n_c))
            n_t, n_g, n_s, n_c = n_t + nrb * K, n_g + nch, n_s + rows, n_c + (K + SN_COLS_PER_SUM - 1) // SN_COLS_PER_SUM
        self.ws64 = torch.zeros(n_t + n_g + n_c, dtype=torch.float64, device=self.device)
        self.ws32 = torch.zeros(n_s, dtype=torch.float32, device=self.device)
        jobs, wt, colt, rowt, chunks = [], [], [], [], []
        for i, (L, (rows, K, nrb, nch, o_t, o_g, o_s, o_c)) in enumerate(zip(self.layers, geo)):
            for f in _SN_FIELDS:
                t = L.get(f)
                assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.device == self.ws32.device), f
            assert L["wn"].numel() == rows * K and L["u"].numel() == L["ru"].numel() == rows and L["v"].numel() == L["rv"].numel() == K
            assert L.get("g") is None or L["g"].numel() == rows * K == L["dw"].numel()
            jobs.append([hip.ptr(L.get(f)) or 0 for f in _SN_FIELDS] +
                        [rows, K, self.ws64.data_ptr() + 8 * o_t, self.ws32.data_ptr() + 4 * o_s, self.ws64.data_ptr() + 8 * (n_t + o_g), nch,
                         self.ws64.data_ptr() + 8 * (n_t + n_g + o_c)])
            for b in range(nrb):
                wt += [(i, b * SN_ROWS_PER_TILE, k0, b) for k0 in range(0, K, SN_COLS_PER_TILE)]
            colt += [(i, k0, 0, c) for c, k0 in enumerate(range(0, K, SN_COLS_PER_SUM))]
            rowt += [(i, r0, 0, 0) for r0 in range(0, rows, SN_ROWS_PER_DOT)]
            chunks += [(i, c * SN_CHUNK, 0, c) for c in range(nch)]
        self.njobs, self.n_wt, self.n_col, self.n_row, self.nchunks = len(jobs), len(wt), len(colt), len(rowt), len(chunks)
        self.jobs = torch.tensor(jobs, dtype=torch.int64).reshape(-1, words).to(self.device)
        self.wt = torch.tensor(wt, dtype=torch.int32).reshape(-1, 4).to(self.device)
        self.colt = torch.tensor(colt, dtype=torch.int32).reshape(-1, 4).to(self.device)
        self.rowt = torch.tensor(rowt, dtype=torch.int32).reshape(-1, 4).to(self.device)
        self.chunks = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 4).to(self.device)
        self._ptrs = self._live_ptrs()

    def _live_ptrs(self):
        return [hip.ptr(L.get(f)) for L in self.layers for f in _SN_FIELDS]

    def ensure(self):
        if self._ptrs is None or self._ptrs != self._live_ptrs():
            self._build()
        return self


def sn_forward(table, iterate, eps=SN_EPS):
    """Every layer of the table: (iterate: v <- normalize(W^T u), u <- normalize(W v) in place;) sigma = u . (W v); wn = W / sigma; the
    record (ru, rv, sig) filled.  4 launches with iterate, else 2, whatever the layer count."""
    t = table.ensure()
    hip.check(hip.load().tnr_sn_forward(t.jobs.data_ptr(), t.njobs, t.wt.data_ptr(), t.n_wt, t.colt.data_ptr(), t.n_col, t.rowt.data_ptr(), t.n_row,
                                        t.chunks.data_ptr(), t.nchunks, int(bool(iterate)), eps, hip.stream()), "sn_forward")


def sn_backward(table):
    """Every layer of the table: dw += (g - <g, wn> ru rv^T) / sig.  2 launches."""
    t = table.ensure()
    assert all(L.get("g") is not None and L.get("dw") is not None for L in t.layers)
    hip.check(hip.load().tnr_sn_backward(t.jobs.data_ptr(), t.njobs, t.chunks.data_ptr(), t.nchunks, hip.stream()), "sn_backward")


# ----------------------------------------------------------------------------------------------
# convolution
# ----------------------------------------------------------------------------------------------
class ConvProfile:
    """Optional per-launch HIP-event timing of the implicit-GEMM kernels (bench.py's roofline leg).
    Events are recorded on the launch stream around every launch; nothing is synchronised until
    `summary()`."""

    def __init__(self):
        self.records = []      # (family, flops, start_event, end_event)

    def begin(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        return ev

    def end(self, family, flops, start, shape=None):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        self.records.append((family, flops, start, ev, shape))

    def summary(self, by_shape=False):
        torch.cuda.synchronize()
        out = {}
        for fam, flops, a, b, shape in self.records:
            key = (fam,) + tuple(shape or ()) if by_shape else fam
            d = out.setdefault(key, {"launches": 0, "flops": 0.0, "ms": 0.0})
            d["launches"] += 1
            d["flops"] += flops
            d["ms"] += a.elapsed_time(b)
        return out


PROFILE = None      # set to a ConvProfile() to time launches
# matrix-core arithmetic of every MFMA launch below.  hip.MMA_F32: v_mfma_f32_32x32x2_f32; hip.MMA_BF16X3: fp32 operands split
# exactly into three bf16 values, six partial products on the bf16 matrix core, fp32 accumulate (fp32-level accuracy at 6/16 of the
# matrix-core cycles; TNR_MMA=bf16x3); hip.MMA_BF16: operands ROUNDED to bf16 (`use_amp: true`, set by BaseModel.setup_amp)
FP32_MMA = {"f32": hip.MMA_F32, "bf16x3": hip.MMA_BF16X3}[os.environ.get("TNR_MMA", "bf16x3").lower()]
MMA = FP32_MMA


def _conv_desc(d, x, wp, y, mode=CONV_3x3, bias=None, act=ACT_NONE, slope=0.2, alpha=1.0, r1=None, r1_ch=None,
               beta1=1.0, r2=None, alpha2=1.0, mask=None, m_lo=0, m_hi=None, m_slope=0.2, reflect=False, noise=None):
    d.x = x.c()
    d.N, d.H, d.W, d.Cin = x.N, x.H, x.W, x.C
    d.wp, d.KinP, d.KoutP = wp.t.data_ptr(), wp.KinP, wp.KoutP
    d.y = y.c()
    d.Ho, d.Wo, d.Cout = y.H, y.W, y.C
    d.mode = mode
    d.bias = hip.ptr(bias)
    d.act, d.slope, d.alpha = act, slope, alpha
    d.r1 = cv(r1)
    d.r1_ch = (r1.C if r1_ch is None else r1_ch) if r1 is not None else 0
    d.beta1 = beta1
    d.r2 = cv(r2)
    d.alpha2 = alpha2
    d.m = cv(mask)
    d.m_lo = m_lo
    d.m_hi = (y.C if m_hi is None else m_hi)
    d.m_slope = m_slope
    d.mma = MMA
    d.pad_mode = 1 if reflect else 0          # TNR_CONV_3x3 only: ReflectionPad2d(1) borders instead of zeros
    if noise is not None:                      # Noise: the ESRGAN+ multiplier of tnr_conv_desc.noise_* (None: the fields stay zero)
        d.noise_sigma, d.noise_pos, d.noise_key0, d.noise_key1, d.noise_pix0 = noise.sigma, noise.pos, noise.key0, noise.key1, noise.pix0


class Noise:
    """ESRGAN+ GaussianNoise multiplier of one dense block (block.py:587-600): m = 1 + sigma * n(key, element).  pos: where a
    convolution epilogue applies it (1 after the r1 step = forward, 2 after the r2 step = backward); pix0: first pixel of this
    rank's shard in the global batch."""
    __slots__ = ("sigma", "pos", "key0", "key1", "pix0")

    def __init__(self, sigma, key, pos=1, pix0=0):
        self.sigma, self.pos, self.pix0 = float(sigma), pos, pix0 & 0xFFFFFFFF
        self.key0, self.key1 = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF

    def at(self, pos):
        n = Noise(self.sigma, 0, pos, self.pix0)
        n.key0, n.key1 = self.key0, self.key1
        return n


def noise_key(seed, call, block):
    """64-bit key of (seed, training forward `call`, dense block): splitmix64 over the three words, so that neighbouring calls /
    blocks share no structure the device-side counter hash (csrc/gauss_noise.h) would have to undo."""
    M = 0xFFFFFFFFFFFFFFFF

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    return mix(mix(mix(seed & M) ^ (call & M)) ^ (block & M))


def gauss_mult(dst, src, noise):
    """dst = (src or 1) * the noise multiplier field (tnr_gauss_mult); dst / src: views of `dst.C` channels."""
    hip.check(hip.load().tnr_gauss_mult(dst.c(), cv(src), dst.pixels, dst.C, noise.sigma, noise.key0, noise.key1, noise.pix0,
                                        hip.stream()), "gauss_mult")


IMAGE_C4 = os.environ.get("TNR_IMAGE_C4", "1") != "0"       # taps-in-K kernel for <= 4-channel image layers (A/B switch)
SMALL_GEMM = os.environ.get("TNR_SMALL_GEMM", "1") != "0"   # im2col + split-K GEMM for <= 4096-pixel layers (A/B switch)
S2_D4 = os.environ.get("TNR_S2_D4", "1") != "0"      # the four-tap layers (4x4 stride 2 and its data-gradient) on the weight-stream machinery too (A/B switch)
X3_D4 = os.environ.get("TNR_X3_D4", "1") != "0"      # TNR_MMA=bf16x3: 64-cout 3x3 layers take their weights as a pre-split stream (A/B switch)
_wq_oneoff = {}                 # weight-stream images of one-off packs (no owning packer): (key, stream) -> [image, None]
_sweep_images = {}              # sweep images of one-off packs: ((packed-weight pointers), stream) -> [image, None]
_ONEOFF_IMAGES = {"_wq_images": _wq_oneoff, "_sweep_images": _sweep_images}


def _stream_image(owner, attr, key, need, dev, pack):
    """The cache of every weight image derived from packed weights: -> ([image, generation], True if this call allocated it).
    owner: the packer whose run() rewrites those weights.  The image lives in owner.__dict__[attr][key] and is re-packed --
    pack(image pointer, need): one small launch -- when owner.gen has moved: once per optimiser step, once ever for the VGG.
    owner None (one-off packs): the image lives in the module-level cache of `attr` and is re-packed on EVERY call, on the CURRENT
    stream -- so it is kept per (key, stream): two streams must not share one -- and at most 64 of them are kept (least recently
    used out: the addresses change as tensors come and go).  An entry smaller than `need` bytes is replaced by a new one."""
    if owner is None:
        cache, gen, key = _ONEOFF_IMAGES[attr], None, (key, hip.stream())
    else:
        cache, gen = owner.__dict__.setdefault(attr, {}), owner.gen
    ent = cache.get(key)
    if owner is None and ent is not None:
        cache[key] = cache.pop(key)          # most recently used last
    fresh = ent is None or ent[0].numel() * 4 < need
    if fresh:
        ent = cache[key] = [torch.empty(need // 4, dtype=torch.float32, device=dev), None]
        if owner is None:
            while len(cache) > 64:
                cache.pop(next(iter(cache)))
    if gen is None or ent[1] != gen:
        pack(ent[0].data_ptr(), need)
        ent[1] = gen
    return ent, fresh


def _wq_image(lib, d, wp, dev, tag=None):
    """The pre-split weight stream of a launch (tnr_conv_desc.wq; None: the launch cannot use one).
    tag: a second stream of the same weights in another order (the pixel-shuffle store's) is cached under its own key."""
    need = lib.tnr_conv_wq_bytes(C.byref(d))
    if need <= 0:
        return None
    key = wp.t.data_ptr() if tag is None else (tag, wp.t.data_ptr())
    return _stream_image(wp.owner, "_wq_images", key, need, dev,
                         lambda img, nb: hip.check(lib.tnr_conv_wq_pack(C.byref(d), img, nb, hip.stream()), "conv_wq_pack"))[0][0]


# TNR_MMA=bf16x3: 64-cout 3x3 layers in the Winograd F(2x2, 3x3) form (csrc/conv_wino.hip): 2.25 x fewer matrix-core instructions for the
# same convolution, a few more fp32 roundings per element (error vs fp64 <= 3 x the fp32 matrix core's in the tests; NOT bit-identical
# to the direct kernels).  The transform + operand split of an input chunk is vector-ALU work per PIXEL that only 64 output channels per
# workgroup amortise (registers: 16 transform positions x 2 x 2 accumulator tiles), so the kernel is bound by it, not by the matrix
# core: x 1.19 (128 ch) / 1.26 (256) / 1.23-1.31 (512) over the direct weight-stream kernel, x 1.04-1.11 on the 64-channel layers
# (profiles/r09o_wino_blate_ab.txt; analysis DESIGN.md 3.9).  conv_chain never uses it (its per-layer fallback must stay
# bit-identical to the one-launch forms); dense_block may run a block's 64-wide last stage in it (TNR_DENSE_SPLIT).  TNR_WINO=0: off.
WINO = os.environ.get("TNR_WINO", "1") != "0"
WINO_MIN_CIN = int(os.environ.get("TNR_WINO_MIN_CIN", "64"))
WINO_MIN_PIXELS = int(os.environ.get("TNR_WINO_MIN_PIXELS", "4096"))


def _wino_image(lib, d, wp, dev):
    """The transform-domain weight stream of a launch (tnr_conv_desc.wq with wq_form = 1; None: the launch cannot run in the Winograd
    form).  Shares the dictionaries of _wq_image under a ("wino", weights) key."""
    need = lib.tnr_conv_wino_bytes(C.byref(d))
    if need <= 0:
        return None
    return _stream_image(wp.owner, "_wq_images", ("wino", wp.t.data_ptr()), need, dev,
                         lambda img, nb: hip.check(lib.tnr_conv_wino_pack(C.byref(d), img, nb, hip.stream()), "conv_wino_pack"))[0][0]
SHUFFLE_FOLD = os.environ.get("TNR_SHUFFLE_FOLD", "1") != "0"      # nn.PixelShuffle(2) folded into the convolution's store (A/B switch)
_LIVE = object()                # conv_plan / dense_block_plan: "read the module's state now" (the default of every what-if argument)
# what engine.ConvOp knows about its layer and the direction of a launch; direct / c4 / col: the packer's index of that packing, None where the layer owns none
ConvLayer = collections.namedtuple("ConvLayer", "k stride cin cout dgrad ups direct c4 col")
_STREAM_MMA = (hip.MMA_BF16X3, hip.MMA_BF16)
_FUSED = ("r1", "r2", "mask")
# mode -> (PROFILE family, taps per output pixel: one of the stride-2 data-gradient sees 4 of the 16)
_CONV_FAMILY = {CONV_3x3: ("conv_tile_3x3", 9), CONV_3x3_UP2: ("conv_tile_3x3_up2", 9), CONV_4x4_S2: ("conv_tile_4x4s2", 16), DGRAD_4x4_S2: ("conv_tile_dgrad4x4s2", 4),
                CONV_1x1: ("conv_tile_1x1", 1), CONV_3x3_C4: ("conv_tile_3x3_c4", 9), CONV_7x7_C4: ("conv_tile_7x7_c4", 49)}


def conv_plan(x, wp, y, mode=CONV_3x3, epi=None, shuffle=0, layer=None, wino=None, mma=_LIVE, splitk=True, wino_ok=True, stream_ok=True):
    """The form ONE convolution runs in right now -> (form, reason).  First matching row wins.  reason: None on the straight path, else why the FIRST
    better form was passed over: "switch", "arithmetic", "shape", "epilogue", "declined" (the library said no), "forbidden" (the caller's wino=False);
    two rows carry a word of their own: ("tile", "splitk") and ("wino", "forced").
    shuffle = 2 (conv + nn.PixelShuffle(2) in one store, y = the shuffled tensor) has one form:
      ("stream", None)    TNR_SHUFFLE_FOLD and TNR_X3_D4 on, device tensors; bf16x3 or bf16 operands; a 3x3 stride-1 layer, not nearest-x2, of exactly 4 y.C
                          outputs, no padding rows in its packing (KoutP == 4 y.C), y twice the size of x; tnr_conv_wq_bytes > 0.
      ("tile", why)       otherwise: the store is not folded, the caller runs conv + depth_to_space.
    The layer's rows (layer = a ConvLayer; a bare ops.conv has none):
      ("thin", None)      ops.conv_thin: a 3x3 stride-1 layer, not nearest-x2, <= 4 channels on the launch's OUTPUT side, y.C <= 4, TNR_IMAGE_C4 on, bias / alpha only.
      ("c4", why)         taps folded into K (TNR_CONV_3x3_C4): the layer owns the C4 packing, x starts a 4-channel buffer, TNR_IMAGE_C4 on.
      ("im2col", why)     ops.conv_small: the layer owns the column packing, TNR_SMALL_GEMM on, <= 4096 output pixels, a multiple of 8, x.C % 4 == 0, no r1 / r2 / mask / reflect.
    The launch's rows (tnr_conv_forward):
      ("tile", "splitk")  conv_tile over a split-K workspace, which excludes every weight stream: <= 16384 output pixels, KinP >= 512, tnr_conv_workspace_bytes > 0.
                          Always this word: _conv_launch asks the library when it reads it.
      ("c4", why)         mode is TNR_CONV_3x3_C4 / TNR_CONV_7x7_C4 (what the layer's row above, or a 7x7 image layer, launches).
      ("wino", None)      Winograd F(2x2, 3x3): TNR_CONV_3x3; TNR_WINO on, x.C >= WINO_MIN_CIN and y.pixels >= WINO_MIN_PIXELS -- or wino=True in their place:
                          ("wino", "forced") --; bf16x3; y.C % 64 == 0; tnr_conv_wino_bytes > 0.
      ("stream", why)     pre-split weight stream: TNR_X3_D4 on; TNR_CONV_3x3, or 4x4 stride 2 / its data-gradient with TNR_S2_D4 on; bf16x3 or bf16 operands; y.C % 64 == 0;
                          tnr_conv_wq_bytes > 0.
      ("tile", why)       conv_tile: everything else.
    Everything is read at call time; the keyword arguments ask a what-if instead: mma = the arithmetic, splitk / wino_ok / stream_ok = the library's three late
    answers, True until asked (_conv_launch asks and, on a decline, asks the plan again with that answer).
    Below, every row reads: the first condition that holds names why the row is passed over; none holds: the row is taken."""
    mma = MMA if mma is _LIVE else mma
    epi = epi or {}
    if shuffle:
        no = ((not (SHUFFLE_FOLD and X3_D4 and x.buf.is_cuda) and "switch")
              or (mma not in _STREAM_MMA and "arithmetic")
              or (layer is not None and (layer.k != 3 or layer.stride != 1 or layer.ups or layer.cout != 4 * y.C) and "shape")
              or ((wp.KoutP != 4 * y.C or y.H != 2 * x.H or y.W != 2 * x.W) and "shape")
              or (not stream_ok and "declined"))
        return ("tile", no) if no else ("stream", None)
    why = None          # of the first row passed over
    if layer is not None:
        if layer.k == 3 and layer.stride == 1 and not layer.ups and (layer.cin if layer.dgrad else layer.cout) <= 4 and y.C <= 4:
            why = ((not IMAGE_C4 and "switch")
                   or ((any(epi.get(n) is not None for n in _FUSED) or epi.get("act", ACT_NONE) != ACT_NONE) and "epilogue"))
            if not why:
                return "thin", None
        if layer.c4 is not None and x.ctot == 4 and x.coff == 0:
            if IMAGE_C4:
                return "c4", why
            why = why or "switch"
        if layer.col is not None:
            no = ((not SMALL_GEMM and "switch")
                  or ((y.pixels > 4096 or y.pixels % 8 or x.C % 4) and "shape")
                  or ((any(epi.get(n) is not None for n in _FUSED) or epi.get("reflect")) and "epilogue"))
            if not no:
                return "im2col", why
            why = why or no
    if splitk and wp.KinP >= 512 and y.pixels <= 16384:
        return "tile", "splitk"
    if mode in (CONV_3x3_C4, CONV_7x7_C4):
        return "c4", why
    if mode == CONV_3x3:
        no = ((wino is False and "forbidden")
              or (wino is None and not WINO and "switch")
              or (wino is None and (x.C < WINO_MIN_CIN or y.pixels < WINO_MIN_PIXELS) and "shape")
              or (mma != hip.MMA_BF16X3 and "arithmetic")
              or (y.C % 64 and "shape")
              or (not wino_ok and "declined"))
        if not no:
            return "wino", why or ("forced" if wino else None)
        why = why or no
    if mode in (CONV_3x3, CONV_4x4_S2, DGRAD_4x4_S2):
        no = ((not (X3_D4 and (S2_D4 or mode == CONV_3x3)) and "switch")
              or (mma not in _STREAM_MMA and "arithmetic")
              or (y.C % 64 and "shape")
              or (not stream_ok and "declined"))
        if not no:
            return "stream", why
        why = why or no
    return "tile", why


_DRY_PTR = 64                   # conv_launch_desc(dry=True): stands for a workspace / weight image of the size the library asked for; never dereferenced


def conv_launch_desc(x, wp, y, mode=CONV_3x3, wino=None, shuffle=0, epi=None, layer=None, dry=False):
    """The descriptor tnr_conv_forward gets for this launch -> (form, ConvDesc); (None, None): shuffle cannot be folded.  Descriptor; the
    library's late answers, each asked where conv_plan's answer hangs on it and fed back into the plan on a decline.
    dry: nothing is allocated or packed -- ws / wq hold a placeholder address with the byte count the library asked for -- so that
    conv_launch_class can be asked about views that have no memory behind them (x, wp, y: anything with the attributes read here)."""
    epi = epi or {}
    d, said = None, {}
    while True:
        form, why = conv_plan(x, wp, y, mode, epi, shuffle, layer, wino, **said)
        if shuffle and form != "stream":
            return None, None
        if d is None:
            lib, d = hip.load(), ConvDesc()
            _conv_desc(d, x, wp, y, mode, **epi)
            if shuffle:
                d.Ho, d.Wo, d.Cout, d.shuffle, d.m_hi = x.H, x.W, 4 * y.C, shuffle, 0
        if why == "splitk":
            need = lib.tnr_conv_workspace_bytes(C.byref(d))
            if need > 0:
                if dry:
                    d.ws, d.ws_bytes = _DRY_PTR, need
                else:
                    ws = WS.get("splitk@%x" % hip.stream(), need, x.buf.device)
                    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 8
                break
            said["splitk"] = False
        elif form == "wino":
            need = lib.tnr_conv_wino_bytes(C.byref(d)) if dry else 0
            img = None if dry else _wino_image(lib, d, wp, x.buf.device)
            if img is not None or need > 0:
                d.wq, d.wq_bytes, d.wq_form = (_DRY_PTR, need, 1) if dry else (img.data_ptr(), img.numel() * 4, 1)
                break
            assert wino is not True, "this launch cannot run in the Winograd form"
            said["wino_ok"] = False
        elif form == "stream":
            need = lib.tnr_conv_wq_bytes(C.byref(d)) if dry else 0
            img = None if dry else _wq_image(lib, d, wp, x.buf.device, tag="shuffle2" if shuffle else None)
            if img is not None or need > 0:
                d.wq, d.wq_bytes = (_DRY_PTR, need) if dry else (img.data_ptr(), img.numel() * 4)
                break
            said["stream_ok"] = False
        else:
            break
    return form, d


CONV_KERNELS = ("tile", "x3w8", "d4", "s2_d4", "wino")


def conv_launch_class(desc):
    """tnr_conv_launch_class of a ConvDesc (host only, no launch) -> dict: kernel (one of CONV_KERNELS), tw, th, nt, mt, tiles_x, tiles_y, ncb,
    tiles, ksplit and cap (the persistent grid's workgroups per CU; 0: one workgroup per tile)."""
    out = (C.c_int32 * 12)()
    hip.check(hip.load().tnr_conv_launch_class(C.byref(desc), C.byref(out)), "conv_launch_class")
    q = dict(zip(("kernel", "tw", "th", "nt", "mt", "tiles_x", "tiles_y", "ncb", "tiles", "ksplit", "cap"), out))
    q["kernel"] = CONV_KERNELS[q["kernel"]]
    return q


def _conv_launch(x, wp, y, mode, wino, shuffle, epi, layer=None, family=None):
    """The one tnr_conv_forward path (conv, conv_shuffle2) -> the form launched; None: shuffle cannot be folded and nothing ran.
    conv_launch_desc's descriptor; the launch; the PROFILE record."""
    form, d = conv_launch_desc(x, wp, y, mode, wino, shuffle, epi, layer)
    if d is None:
        return None
    lib = hip.load()
    t0 = PROFILE.begin() if PROFILE is not None else None
    hip.check(lib.tnr_conv_forward(C.byref(d), hip.stream()), "conv_forward")
    if PROFILE is not None:
        fam, taps = _CONV_FAMILY[mode]          # (the Winograd form: the algorithmic FLOP of the convolution it computes)
        PROFILE.end("conv_wino_3x3" if form == "wino" else (family or fam), 2.0 * d.N * d.Ho * d.Wo * taps * min(x.C, wp.KinP) * d.Cout, t0, (x.C, d.Cout, d.Ho, wp.kind))
    return form


def conv_shuffle2(x, wp, y, layer=None, **epi):
    """conv (nf -> 4 nf, 3x3) + nn.PixelShuffle(2) + the epilogue's activation in ONE launch (block.pixelshuffle_block, block.py:374-387):
    y is the SHUFFLED tensor [N, 2 H, 2 W, nf]; the [N, H, W, 4 nf] intermediate and the depth-to-space pass do not exist (tnr_conv_desc.shuffle).
    Returns False, and launches nothing, unless conv_plan with shuffle=2 says "stream": the caller then runs conv + depth_to_space."""
    return _conv_launch(x, wp, y, CONV_3x3, None, 2, epi, layer) is not None


def conv(x, wp, y, mode=CONV_3x3, wino=None, family=None, **epi):
    """One tnr_conv_forward launch in the form conv_plan names.  wino: None = the process policy (WINO and the layer's size), True / False =
    force / forbid the Winograd form for this launch.  family: the PROFILE family the launch is counted in instead of its mode's."""
    _conv_launch(x, wp, y, mode, wino, 0, epi, family=family)


# ----------------------------------------------------------------------------------------------
# conv + activation + nn.MaxPool2d(2, 2) in one launch: the pooled store of the Winograd form
# ----------------------------------------------------------------------------------------------
_NATIVE_CONV = conv             # (a test backend that replaces ops.conv has no pooled store: conv_pool2 then declines)
_FullRes = collections.namedtuple("_FullRes", "N H W C pixels")          # what conv_plan reads of an output view that is never allocated


def pool_fold_on():
    """TNR_POOL_FOLD (default 1, read at call time; A/B switch): 0 keeps conv and maxpool2_fwd / maxpool2_bwd as launches of their own."""
    return os.environ.get("TNR_POOL_FOLD", "1") != "0"


def conv_pool2(x, wp, y, route=None, layer=None, wino=None, **epi):
    """y [N, H / 2, W / 2, C] = maxpool2x2(act(conv3x3(x) + bias) * alpha) in ONE launch, bit for bit what conv + maxpool2_fwd store;
    the [N, H, W, C] map does not exist (tnr_conv_forward_pool2).  route: None, or a uint8 tensor of y's shape that receives the
    arg-max / sign bytes unpool2_bwd routes the gradient by.  An epilogue of the Winograd form: conv_plan's answers do not change.
    Returns False, and launches nothing, unless the native library is the backend, TNR_POOL_FOLD is on, conv_plan says "wino" for
    the unpooled launch (wino: as in conv) and the library agrees (tnr_conv_pool_ok): the caller then runs conv and maxpool2_fwd."""
    if conv is not _NATIVE_CONV or not x.buf.is_cuda or not pool_fold_on() or x.H % 2 or x.W % 2 or (y.N, y.H, y.W) != (x.N, x.H // 2, x.W // 2):
        return False
    full = _FullRes(x.N, x.H, x.W, y.C, x.N * x.H * x.W)
    if conv_plan(x, wp, full, CONV_3x3, epi, 0, layer, wino)[0] != "wino":
        return False
    lib, d = hip.load(), ConvDesc()
    _conv_desc(d, x, wp, y, CONV_3x3, **epi)
    d.Ho, d.Wo = x.H, x.W               # the descriptor of the UNPOOLED launch; only y is the pooled view
    if not lib.tnr_conv_pool_ok(C.byref(d)):
        return False
    img = _wino_image(lib, d, wp, x.buf.device)
    if img is None:
        return False
    d.wq, d.wq_bytes, d.wq_form = img.data_ptr(), img.numel() * 4, 1
    if route is not None:
        assert route.dtype == torch.uint8 and route.is_contiguous() and tuple(route.shape) == (y.N, y.H, y.W, y.C)
    t0 = PROFILE.begin() if PROFILE is not None else None
    hip.check(lib.tnr_conv_forward_pool2(C.byref(d), hip.ptr(route), hip.stream()), "conv_forward_pool2")
    if PROFILE is not None:             # (the convolution's own FLOP: the pooled store changes none of it)
        PROFILE.end("conv_wino_3x3", 2.0 * d.N * d.Ho * d.Wo * 9 * min(x.C, wp.KinP) * d.Cout, t0, (x.C, d.Cout, d.Ho, wp.kind))
    return True


# ----------------------------------------------------------------------------------------------
# nearest x2 + 3x3 (upconv_block) folded into the four-tap stride-2 launches
# ----------------------------------------------------------------------------------------------
UPFOLD_FAMILY = "conv_upfold"           # PROFILE family of the folded launches (all three passes), counted with the FLOP they execute (16 taps)
UPFOLD_PASSES = ("fwd", "dgrad", "wgrad")
# per axis: the 3x3 taps summed into folded tap k = 0..3 (csrc/common.h tnr_upfold_lo / tnr_upfold_hi)
UPFOLD_TAPS = ((2,), (1, 2), (0, 1), (0,))
# The passes TNR_UPCONV_FOLD=1 folds (upconv_plan): both gradients, NOT the forward.  The folded forward is the more accurate form against
# fp64 and 1.1 ms / step faster, but it moves the SR batch itself (1.7e-6 of its scale in the first step), and the GAN step amplifies a
# change that enters there far more than one that enters through a gradient: after 25 benchmark steps the outputs stand 5.6 % of the SR
# scale from the unfolded run's with it, 0.15 % without -- the process's two fp32 arithmetics stand 3.4 % apart (profiles/r30a_upconv_fold.txt).
_UPFOLD_DEFAULT = ("dgrad", "wgrad")


def upconv_plan(x, mma=_LIVE, switch=_LIVE):
    """Which passes of ONE `Upsample(nearest, x2) -> Conv2d(3, 1, 1)` layer run folded right now -> (passes, reason); x: the layer's
    LOW-resolution input view.  passes: the subset of UPFOLD_PASSES that runs as a four-tap stride-2 launch; the others keep the
    present launches (TNR_CONV_3x3_UP2, the 3x3 data-gradient + tnr_upsample2x_bwd, the x2 weight-gradient class).  reason: None
    when TNR_UPCONV_FOLD itself selects the passes, else why NOTHING is folded.
    The fold: nearest x2 followed by a zero-padded 3x3 convolution is the data-gradient of a virtual 4x4 stride-2
    padding-1 convolution S, W_S[ci][co] = the 16 sums of the 3x3 taps over {2}, {1,2}, {0,1}, {0} per axis, so
      "fwd"    is one TNR_DGRAD_4x4_S2 launch over the TNR_PACK_UP2_DGRAD_S2 packing (bias, activation as before);
      "dgrad"  is one TNR_CONV_4x4_S2 launch over the TNR_PACK_UP2_FWD_S2D packing: it sums the 2 x 2 block itself and carries the
               previous activation's mask in its epilogue (tnr_upsample2x_bwd does not run);
      "wgrad"  is the 4x4 stride-2 weight-gradient class into a workspace, tnr_upconv_wgrad_unfold (16 -> 9 taps), tnr_bias_grad.
    16 instead of 36 products per output pixel and channel pair; the results differ from the present launches at rounding level
    (weights summed before the product, 16 accumulation steps instead of 36) and are deterministic.
    First matching row wins:
      ((), "switch")       TNR_UPCONV_FOLD=0 (read at call time; switch=... asks a what-if).
      ((), "arithmetic")   the arithmetic is not bf16x3: TNR_MMA=f32 is the CPU reference's bit-parity class and stays on
                           TNR_CONV_3x3_UP2; `use_amp` (bf16 operands) stays there too -- one arithmetic question per change.
      ((), "device")       x is not a device tensor (the CPU stand-in of the tests re-states the present launches).
      (passes, None)       TNR_UPCONV_FOLD=1 (default): the passes of _UPFOLD_DEFAULT, i.e. the data gradient and the weight gradient -- the
                           forward stays on TNR_CONV_3x3_UP2, so the network's outputs for given weights are bit for bit the unfolded
                           ones; a comma list names the passes itself ("fwd,dgrad,wgrad": all three; A/B runs).
    The folded launches are ordinary 4x4 stride-2 launches to conv_plan: they land on its "stream" / "tile" rows, the stream kernel's
    decline for grids narrower than 32 pixels included."""
    sw = os.environ.get("TNR_UPCONV_FOLD", "1") if switch is _LIVE else str(switch)
    if sw == "0":
        return (), "switch"
    if (MMA if mma is _LIVE else mma) != hip.MMA_BF16X3:
        return (), "arithmetic"
    if not _on_device(x.buf):
        return (), "device"
    if sw == "1":
        return _UPFOLD_DEFAULT, None
    return tuple(p for p in UPFOLD_PASSES if p in sw.split(",")), None


def upconv_fold_table():
    """The library's 16 x 9 fold matrix (tnr_upconv_fold_table) as a float64 tensor: row ky*4 + kx, column ty*3 + tx."""
    out = (C.c_int32 * 144)()
    hip.check(hip.load().tnr_upconv_fold_table(C.byref(out)), "upconv_fold_table")
    return torch.tensor(list(out), dtype=torch.float64).view(16, 9)


def upconv_fold_weights(w):
    """[..., 3, 3] -> the folded [..., 4, 4] taps in the library's fp32 order (tnr_upfold_tap): inside a row over ascending kx first,
    then the row sums over ascending ky.  The channel swap of S is the packings' business, not this function's."""
    rows = []
    for ty in range(3):      # row sums: [..., 4] per 3x3 row
        rows.append(torch.stack([w[..., ty, t[0]] if len(t) == 1 else w[..., ty, t[0]] + w[..., ty, t[1]] for t in UPFOLD_TAPS], dim=-1))
    return torch.stack([rows[t[0]] if len(t) == 1 else rows[t[0]] + rows[t[1]] for t in UPFOLD_TAPS], dim=-2)


def upconv_unfold_grad(dF):
    """[..., 4, 4] gradients of the folded taps -> [..., 3, 3] in the library's fp32 order (tnr_upfold_grad): 3x3 tap t collects
    folded taps 2 - t and 3 - t per axis, inside a row over ascending kx first, then the two rows over ascending ky."""
    def row(ky):
        return torch.stack([dF[..., ky, 2 - tx] + dF[..., ky, 3 - tx] for tx in range(3)], dim=-1)
    return torch.stack([row(2 - ty) + row(3 - ty) for ty in range(3)], dim=-2)


def upconv_wgrad_unfold(dws, dw3, alpha=1.0, beta=1.0):
    """dw3 [Cout, Cin, 3, 3] = beta dw3 + alpha unfold(dws [Cin, Cout, 4, 4]) (tnr_upconv_wgrad_unfold)."""
    Cout, Cin = dw3.shape[0], dw3.shape[1]
    assert tuple(dws.shape) == (Cin, Cout, 4, 4) and dws.is_contiguous() and dw3.is_contiguous()
    hip.check(hip.load().tnr_upconv_wgrad_unfold(dws.data_ptr(), dw3.data_ptr(), Cout, Cin, alpha, beta, hip.stream()), "upconv_wgrad_unfold")


CHAIN_MAX = 6
# The process switches of the dense-block forms (A/B switches: each turns ONE thing off or on).  Which form a block runs in is decided
# by dense_block_plan below and nowhere else; DESIGN.md 3.2 has the table.
CONV_CHAIN = os.environ.get("TNR_CONV_CHAIN", "1") != "0"     # 0: one launch per layer
CONV_SWEEP = os.environ.get("TNR_CONV_SWEEP", "1") != "0"     # 0: tnr_conv_chain where tnr_conv_sweep would run
CHAIN_X3 = os.environ.get("TNR_CHAIN_X3", "1") == "1"   # 0: TNR_MMA=bf16x3 launches demote to the fp32 matrix core inside tnr_conv_chain
AMP_SWEEP = os.environ.get("TNR_AMP_SWEEP", "1") != "0"      # 0: use_amp (bf16 operands) keeps tnr_conv_chain instead of the sweep's bf16-operand form
# TNR_CHAIN_WITH_COLLECTIVES=1: keep the one-launch forms while gradient buckets are on the wire.  Measured next to a 4 x 64 MB RCCL
# all-reduce on a side stream (1-rank group, tools/chain_stress.py --rccl, profiles/r03j): bit-identical results, no wait ever timed out,
# +0.10 ms per dense-block launch (sweep 0.61 -> 0.71 ms, chain 1.01 -> 1.14 ms).  Off by default: with N > 1 ranks an RCCL kernel waits
# for its peers while it holds CUs the launch wants all of -- never exercised on hardware here.
CHAIN_WITH_COLLECTIVES = os.environ.get("TNR_CHAIN_WITH_COLLECTIVES", "0") == "1"
# Per-box calibration of the bf16x3 sweep against five per-layer launches (bit-identical results either way).  The sweep hands tiles over
# between workgroups through system-coherent stores / loads and agent-scope progress words: fabric traffic that never touches L2.  On two
# of ~25 boxes met in round 5 that path was slow -- the sweep alone ran 1.6 x slower (935-941 vs 587-606 us per launch at batch 16), every
# other kernel at its usual rate -- while the per-layer path (plain loads and stores, 686 us on a normal box) does not
# use it.  calibrate_dense_block_form times both forms ONCE, at model set-up, on a scratch block of the TRAINING shape (3 launches each,
# ~10 ms; never from inside a forward, whose first full-size call could be a validation or tiled-inference shape): "layers" if the sweep
# is more than 10 % slower.  Data-parallel ranks agree on ONE form (a rank that kept a slow sweep would be the step's straggler); every
# rank's own measurement is kept in SWEEP_AUTO_STATE["per_rank"] (bench.py prints it).  TNR_SWEEP_AUTO=0: the agreed form is ignored.
SWEEP_AUTO = os.environ.get("TNR_SWEEP_AUTO", "1") != "0"
SWEEP_AUTO_STATE = {"choice": None, "sweep_us": None, "layers_us": None}     # choice: None (not calibrated) | "sweep" | "layers"
# The split form: a block's 64-wide last stage -- 46 % of its multiply-adds -- as a Winograd F(2x2, 3x3) launch (2.25 x fewer matrix
# instructions; conv_wino.hip) behind a FOUR-stage sweep.  x1 .. x4 stay bit-identical to conv_chain's; the block output carries the Winograd
# form's error (<= 3 x the fp32 matrix core's against fp64, as everywhere that form runs) and is deterministic.  The five-stage sweep's time is
# set by the matrix core's dynamic energy, so the instructions removed are what pays.  Measured: DESIGN.md 3.2.
DENSE_SPLIT = os.environ.get("TNR_DENSE_SPLIT", "1") != "0"
COLLECTIVES_IN_FLIGHT = False   # True (dp.py) from the first gradient bucket handed to RCCL on the side stream until the compute stream has waited for all
COUNTERS = {"one_launch_next_to_collectives": 0, "per_layer_next_to_collectives": 0}      # dense blocks launched while gradient buckets were in flight
_cu_counts = {}


def _cus(dev):
    if dev not in _cu_counts:
        _cu_counts[dev] = torch.cuda.get_device_properties(dev).multi_processor_count
    return _cu_counts[dev]


def _on_device(buf):
    return buf.is_cuda


def _crowded(in_flight):
    return in_flight and not CHAIN_WITH_COLLECTIVES


def _chain_mma(mma):          # the arithmetic a one-launch form runs a launch of arithmetic `mma` in
    return hip.MMA_F32 if mma == hip.MMA_BF16X3 and not CHAIN_X3 else mma


def _eligible(stages):          # the shapes the one-launch kernels take
    return all(st.get("mode", CONV_3x3) == CONV_3x3 and st["y"].C % 32 == 0 and st["wp"].KoutP == st["y"].C for st in stages)


def _split_shape(stages):
    """The stricter shape rule of the split form: a function of the block's PER-IMAGE grid and channel counts, never of the batch size
    (data-parallel shards of one global batch pick the same form as one process would)."""
    x0 = stages[0]["x"]
    if not all(st.get("mode", CONV_3x3) == CONV_3x3 and not st.get("reflect") and st["wp"].KoutP == st["y"].C and st["wp"].KinP == st["x"].C for st in stages) \
            or stages[4]["y"].C != 64 or any(st["y"].C != 32 for st in stages[:4]) or x0.C % 16 or x0.C < 32 or stages[4]["x"].C != x0.C + 128:
        return False
    # the sweep keeps an image's 8 x 32 tiles co-resident (one workgroup per CU); the Winograd kernel wants an 8 x 8 grid at least
    return x0.H >= 8 and x0.W >= 8 and -(-x0.W // 32) * -(-x0.H // 8) <= _cus(x0.buf.device)


def dense_block_plan(stages, crowded=_LIVE, mma=_LIVE, choice=_LIVE, sweepable=True):
    """The form the dependent convolutions `stages` (1 .. CHAIN_MAX of them) run in right now -> (form, reason):
      ("layers", why)  one launch per stage.  why = "switch": TNR_CONV_CHAIN=0.  "shape": a stage the one-launch kernels do not take (_eligible).
                       "calibrated": the calibration (this box's or another rank's) chose per-layer launches -- heeded where the sweep would run, in
                       the bf16x3 arithmetic, on the device, unless TNR_SWEEP_AUTO=0.  "crowded": gradient buckets are on the wire (unless
                       TNR_CHAIN_WITH_COLLECTIVES=1) and the form that would run needs its whole grid co-resident, which RCCL's kernels on the same
                       CUs could delay: tnr_conv_chain.  The sweep DISPENSES its tiles in order (a waited-for tile
                       was either taken by a running workgroup or is the next to be dispensed): stage s of tile T reads stage s - 1 of T + tiles_x + 1,
                       so 4 (tiles_x + 1) + 1 resident workgroups guarantee progress (21 on the 128-wide trunk, never more than one image's tiles).
      ("chain", None)  tnr_conv_chain: every eligible list the sweep does not exist for.
      ("sweep", None)  tnr_conv_sweep: five stages in the bf16x3 arithmetic (unless TNR_CHAIN_X3=0) or under bf16 operands (unless TNR_AMP_SWEEP=0),
                       four stages in bf16x3 (a split block's first four); TNR_CONV_SWEEP=0: never.
      ("split", None)  dense_block only (conv_chain reads it as "sweep"): the four-stage sweep, then the last stage as a Winograd launch.  Five stages of
                       the bf16x3 sweep on the device, nothing crowded, _split_shape, unless TNR_DENSE_SPLIT=0.
    Everything is read at call time; the keyword arguments ask a what-if instead: crowded = buckets in flight, mma = the arithmetic, choice = the
    calibrated form, sweepable=False = tnr_conv_sweep declined this block; stages None = a well-shaped five-stage block on the device."""
    n = 5 if stages is None else len(stages)
    mma = _chain_mma(MMA if mma is _LIVE else mma)
    x3 = mma == hip.MMA_BF16X3
    if not CONV_CHAIN:
        return "layers", "switch"
    if stages is not None and not _eligible(stages):
        return "layers", "shape"
    on_device = stages is None or _on_device(stages[0]["x"].buf)
    sweep = sweepable and CONV_SWEEP and ((n in (4, 5) and x3) or (n == 5 and mma == hip.MMA_BF16 and AMP_SWEEP))
    if sweep and x3 and on_device and SWEEP_AUTO and (SWEEP_AUTO_STATE["choice"] if choice is _LIVE else choice) == "layers":
        return "layers", "calibrated"
    crowded = _crowded(COLLECTIVES_IN_FLIGHT if crowded is _LIVE else crowded)
    if crowded and not sweep:
        return "layers", "crowded"
    if not sweep:
        return "chain", None
    if DENSE_SPLIT and x3 and n == 5 and on_device and not crowded and stages is not None and _split_shape(stages):
        return "split", None
    return "sweep", None


def dense_split_applies(stages):
    return dense_block_plan(stages)[0] == "split"


def dense_block_form_applies(stages):
    """Is `stages` a block the calibration decides about: would it heed a calibrated "layers" in the step's fp32 arithmetic?"""
    return len(stages) == 5 and dense_block_plan(stages, mma=FP32_MMA, choice="layers") == ("layers", "calibrated")


def dense_blocks_overlap_collectives():
    """True when the dense blocks stay one launch each next to in-flight gradient buckets in the CURRENT arithmetic: the generator's
    all-reduce can then overlap its backward for free."""
    return not _crowded(True) or dense_block_plan(None, crowded=True, choice=None)[0] != "layers"


def g_buckets_leave_in_backward():
    """TNR_DP_OVERLAP_G: 0 (default) = the generator's gradient buckets go out at its optimizer step; auto = from inside its backward
    whenever the dense blocks stay one launch next to them; 1 = from inside its backward regardless (per-layer launches where needed)."""
    want = os.environ.get("TNR_DP_OVERLAP_G", "0")
    return want == "1" or (want == "auto" and dense_blocks_overlap_collectives())


_chain_epoch = {}


def _sweep_image(lib, descs, n, stages, dev):
    """The pre-split weight stream of a dense block for tnr_conv_sweep (None: not sweepable), keyed by the stages' packed weights."""
    need = lib.tnr_conv_sweep_image_bytes(descs, n)
    if need <= 0:
        return None
    owner = stages[0]["wp"].owner if all(st["wp"].owner is stages[0]["wp"].owner for st in stages) else None
    ent, _ = _stream_image(owner, "_sweep_images", tuple(st["wp"].t.data_ptr() for st in stages), need, dev,
                               lambda img, nb: hip.check(lib.tnr_conv_sweep_pack(descs, n, img, nb, hip.stream()), "conv_sweep_pack"))
    return ent[0]


def _stage_views(st):
    return [st[k] for k in ("x", "y", "r1", "r2", "mask") if st.get(k) is not None]


def _per_layer(stages, why=None):
    """One launch per stage, in the direct kernels: bit-identical to the one-launch forms (never the Winograd form)."""
    if why == "crowded":
        COUNTERS["per_layer_next_to_collectives"] += 1
    for st in stages:
        conv(wino=False, **{k: v for k, v in st.items() if k != "fresh_from"})


def _calibrate_dense_block(stages):
    """Time the one-launch form and the per-layer form of `stages` on the current stream and record this process's own choice.  The block
    is executed several times, which is only idempotent when no stage writes what another launch of the block reads: the LAST stage's
    output must not share a buffer with any input (the four inner stages write channel groups of the dense buffer that the block itself
    produces) -- asserted, not assumed."""
    global PROFILE
    out = stages[-1]["y"]
    for st in stages:
        for v in _stage_views(st):
            if v is not out and v.buf.data_ptr() == out.buf.data_ptr():
                lo, hi = max(v.coff, out.coff), min(v.coff + v.C, out.coff + out.C)
                assert hi <= lo, "calibration re-executes the block: its output must not alias an input (channels [%d, %d))" % (lo, hi)
    prof, PROFILE = PROFILE, None
    prev = SWEEP_AUTO_STATE["choice"]
    try:
        def timed(fn):
            fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(3):
                fn()
            b.record()
            torch.cuda.synchronize()
            return 1e3 * a.elapsed_time(b) / 3.0

        SWEEP_AUTO_STATE["choice"] = "sweep"                # (the timed calls below go through conv_chain itself)
        t_sweep, t_layers = timed(lambda: conv_chain(stages)), timed(lambda: _per_layer(stages))
        t_sweep = min(t_sweep, timed(lambda: conv_chain(stages)))          # (the clock may still be ramping at a process's first launches)
        prev = "layers" if t_sweep > 1.10 * t_layers else "sweep"
        SWEEP_AUTO_STATE.update(sweep_us=round(t_sweep, 1), layers_us=round(t_layers, 1))
    finally:
        SWEEP_AUTO_STATE["choice"] = prev
        PROFILE = prof


def calibrate_dense_block_form(stages, dp=None):
    """The explicit per-box calibration (see SWEEP_AUTO).  stages: a dense block over SCRATCH buffers of the training shape (None: nothing to
    time here -- a CPU stand-in run -- but the ranks still exchange their records).  dp: the
    data-parallel group -- every rank must call this at the same point (two small collectives).  Returns SWEEP_AUTO_STATE."""
    applies = bool(stages) and dense_block_form_applies(stages)
    if applies:
        prev, globals()["MMA"] = MMA, FP32_MMA               # (the fp32 arithmetic of the step, also when called inside an amp region)
        try:
            _calibrate_dense_block(stages)
        finally:
            globals()["MMA"] = prev
    SWEEP_AUTO_STATE["own_choice"] = SWEEP_AUTO_STATE["choice"]
    if dp is not None and dp.active:
        import torch.distributed as dist
        dev = stages[0]["x"].buf.device if (stages and stages[0]["x"].buf.is_cuda and dist.get_backend(dp.group) == "nccl") else torch.device("cpu")
        mine = torch.tensor([1.0 if SWEEP_AUTO_STATE["choice"] == "layers" else 0.0, float(SWEEP_AUTO_STATE["sweep_us"] or 0.0),
                             float(SWEEP_AUTO_STATE["layers_us"] or 0.0), 1.0 if applies else 0.0], dtype=torch.float32, device=dev)
        allr = [torch.zeros_like(mine) for _ in range(dp.world_size)]
        dist.all_gather(allr, mine, group=dp.group)
        rows = [t.cpu().tolist() for t in allr]
        SWEEP_AUTO_STATE["per_rank"] = [{"rank": r, "choice": (("layers" if v[0] else "sweep") if v[3] else None),
                                         "sweep_us": round(v[1], 1) or None, "layers_us": round(v[2], 1) or None} for r, v in enumerate(rows)]
        if any(v[3] for v in rows):
            SWEEP_AUTO_STATE["choice"] = "layers" if any(v[0] and v[3] for v in rows) else "sweep"       # all-reduce MAX, by hand
    if SWEEP_AUTO_STATE["choice"] is not None:
        import logging
        logging.getLogger("base").info("dense-block form: %s (this rank: sweep %s us, per-layer %s us%s)", SWEEP_AUTO_STATE["choice"],
                                       SWEEP_AUTO_STATE["sweep_us"], SWEEP_AUTO_STATE["layers_us"],
                                       "; ranks: %s" % SWEEP_AUTO_STATE["per_rank"] if "per_rank" in SWEEP_AUTO_STATE else "")
    return SWEEP_AUTO_STATE


def conv_chain(stages):
    """Dependent 3x3 convolutions over one pixel grid, in one launch where dense_block_plan allows it.  stages: dicts with the arguments of
    conv() (x, wp, y, bias, act, ..., mask) plus fresh_from: first input channel produced by the previous stage of this chain (None for the
    first stage).  Same results as calling conv() per stage.  tnr_conv_chain is the general one-launch form; tnr_conv_sweep reads every input
    channel chunk once per phase for all the stages that consume it and streams the weights pre-split (csrc/conv_sweep.hip)."""
    n = len(stages)
    assert 1 <= n <= CHAIN_MAX
    form, why = dense_block_plan(stages)
    if form == "layers":
        return _per_layer(stages, why)
    lib = hip.load()
    descs = (ConvDesc * n)()
    fresh = (C.c_int32 * n)()
    flops = 0.0
    for i, st in enumerate(stages):
        _conv_desc(descs[i], **{k: v for k, v in st.items() if k != "fresh_from"})
        descs[i].mma = _chain_mma(descs[i].mma)
        ff = st.get("fresh_from")
        fresh[i] = -1 if ff is None else ff
        flops += 2.0 * st["y"].pixels * 9 * min(st["x"].C, st["wp"].KinP) * st["y"].C
    dev = stages[0]["x"].buf.device
    fault_word(dev)
    need = lib.tnr_conv_chain_workspace_bytes(C.byref(descs[0]))
    key = ("chain", str(dev), hip.stream(), need)    # one counter set per (stream, tile grid)
    ws = WS.bufs.get(key)
    if ws is None:
        ws = torch.zeros(need // 4, dtype=torch.int32, device=dev)     # progress counters start at 0; last word = error flag
        WS.bufs[key] = ws
        _chain_epoch[key] = 0
    _chain_epoch[key] += 1
    if _chain_epoch[key] > 0x0FFFFFF0:                 # epoch wrap: stale counters would compare as already satisfied
        fill(ws[:-1].view(torch.float32), 0.0)         # (stream-ordered after every earlier launch on this stream)
        _chain_epoch[key] = 1
    image = _sweep_image(lib, descs, n, stages, dev) if form != "chain" else None
    if form != "chain" and image is None:
        # the one late fallback: a block the sweep does not cover after all (shapes, tiles per image) -> tnr_conv_chain, or per layer
        form, why = dense_block_plan(stages, sweepable=False)
        if form == "layers":
            return _per_layer(stages, why)
    if COLLECTIVES_IN_FLIGHT:
        COUNTERS["one_launch_next_to_collectives"] += 1
    t0 = PROFILE.begin() if PROFILE is not None else None
    if image is not None:
        hip.check(lib.tnr_conv_sweep(descs, n, image.data_ptr(), ws.data_ptr(), ws.numel() * 4, _chain_epoch[key], hip.stream()), "conv_sweep")
    else:
        hip.check(lib.tnr_conv_chain(descs, fresh, n, ws.data_ptr(), ws.numel() * 4, _chain_epoch[key], hip.stream()), "conv_chain")
    if PROFILE is not None:
        x0, yl = stages[0]["x"], stages[-1]["y"]
        PROFILE.end("conv_chain", flops, t0, (x0.C, yl.C, yl.H, stages[0]["wp"].kind))


def dense_block(stages):
    """A residual dense block's five convolutions (or the five of its gradient mirror): conv_chain(stages), or -- where
    dense_block_plan says "split" -- the four-stage sweep followed by the last stage in the Winograd form."""
    if not dense_split_applies(stages):
        return conv_chain(stages)
    last = {k: v for k, v in stages[4].items() if k != "fresh_from"}
    out = last["y"]
    for v in _stage_views(last):       # a Winograd tile reads a halo of its input (and residuals other workgroups' pixels never touch --
        if v is not out and v.buf.data_ptr() == out.buf.data_ptr():          # kept to the same rule): the output shares no channel with anything read
            assert min(v.coff + v.C, out.coff + out.C) <= max(v.coff, out.coff), "dense_block: the output view overlaps a view the last stage reads"
    conv_chain(stages[:4])
    conv(wino=True, **last)


_FAULT = None


def fault_word(device=None):
    """The engine's fault latch: one zero-initialised device word, registered with the library (tnr_set_fault_word) before the first
    one-launch dense block runs.  A bounded tile hand-off wait that gives up sets it; it is never cleared.  adam_step() launches
    behind it (a faulted step is not applied) and check_engine_errors() raises on it at the next host synchronisation."""
    global _FAULT
    if _FAULT is None:
        _FAULT = torch.zeros(1, dtype=torch.int32, device=device if device is not None else hip.engine_device())
        hip.check(hip.load().tnr_set_fault_word(_FAULT.data_ptr()), "set_fault_word")
    return _FAULT


def chain_error_flag():
    """Nonzero if a tile hand-off wait of tnr_conv_chain / tnr_conv_sweep ever gave up in this process (one host sync)."""
    bad = 0 if _FAULT is None else int(_FAULT.item() != 0)
    for key, ws in WS.bufs.items():       # (workspace tail words: only written while no latch was registered)
        if isinstance(key, tuple) and key[0] == "chain":
            bad += int(ws[-1].item() != 0)
    return bad


def conv_thin(x, w, y, bias=None, alpha=1.0, dgrad=False):
    """3x3 s1 p1 convolution with <= 4 output channels on the vector ALUs (tnr_conv_thin).  w is the layer's OIHW
    weight; dgrad=True computes the data-gradient of a layer with <= 4 INPUT channels (x = gradient of its output).
    The [tap][channel][4] weight layout is rebuilt on every call (a 2 304-element launch) so it is never stale."""
    lib = hip.load()
    Cout, Cin = w.shape[0], w.shape[1]
    red = Cout if dgrad else Cin
    n = lib.tnr_conv_thin_pack_floats(red)
    wp = WS.get("thin_w@%x" % hip.stream(), n * 4, x.buf.device)
    hip.check(lib.tnr_conv_thin_pack(w.data_ptr(), wp.data_ptr(), Cout, Cin, int(dgrad), hip.stream()), "conv_thin_pack")
    t0 = PROFILE.begin() if PROFILE is not None else None
    hip.check(lib.tnr_conv_thin(x.c(), x.N, x.H, x.W, x.C, wp.data_ptr(), y.c(), y.C, hip.ptr(bias), alpha, hip.stream()), "conv_thin")
    if PROFILE is not None:
        PROFILE.end("conv_thin", 2.0 * y.pixels * 9 * x.C * y.C, t0, (x.C, y.C, y.H, int(dgrad)))


def conv_thin7(x, w, y, pad=3, reflect=True, bias=None, alpha=1.0, dgrad=False):
    """7x7 stride-1 convolution with <= 4 output channels in one launch (tnr_conv_thin7): y[p] = sum_t w[t] x[p + t - pad] over y's own
    grid; reflect: ReflectionPad2d(pad) borders (y the size of x), else zeros outside x.  dgrad=True: the data-gradient of a layer with
    <= 4 INPUT channels (x = gradient of its output; pad = 6 and a (H + 6) x (W + 6) y give the gradient of its reflection-padded input)."""
    lib = hip.load()
    Cout, Cin = w.shape[0], w.shape[1]
    n = lib.tnr_conv_thin7_pack_floats(Cout if dgrad else Cin)
    wp = WS.get("thin7_w@%x" % hip.stream(), n * 4, x.buf.device)
    hip.check(lib.tnr_conv_thin7_pack(w.data_ptr(), wp.data_ptr(), Cout, Cin, int(dgrad), hip.stream()), "conv_thin7_pack")
    t0 = PROFILE.begin() if PROFILE is not None else None
    hip.check(lib.tnr_conv_thin7(x.c(), x.N, x.H, x.W, x.C, wp.data_ptr(), y.c(), y.H, y.W, y.C, pad, int(reflect), hip.ptr(bias), alpha,
                                 hip.stream()), "conv_thin7")
    if PROFILE is not None:
        PROFILE.end("conv_thin", 2.0 * y.pixels * 49 * x.C * y.C, t0, (x.C, y.C, y.H, 70 + int(dgrad)))


def wgrad_thin7(big, small4, dw, db, flip, rpad=0, off=0, alpha=1.0, beta=1.0):
    """Weight gradient of a 7x7 layer with <= 3 channels on one side in one launch (tnr_wgrad_thin7):
    flip=False: an image -> C layer (big = gradient of its output, small4 = its reflection-padded NHWC4 input, off = 0);
    flip=True: a C -> image layer (big = its input, read through ReflectionPad2d(rpad = 3); small4 = NHWC4 gradient of its output, off = -6)."""
    lib = hip.load()
    cs = dw.shape[0] if flip else dw.shape[1]
    need = lib.tnr_wgrad_thin7_workspace_bytes(big.N, big.H + 2 * rpad, big.C)
    ws = WS.get("wgrad_thin7@%x" % hip.stream(), need, big.buf.device)
    t0 = PROFILE.begin() if PROFILE is not None else None
    hip.check(lib.tnr_wgrad_thin7(big.c(), big.N, big.H, big.W, rpad, small4.c(), small4.H, small4.W, off, big.C, cs, int(flip),
                                  dw.data_ptr(), hip.ptr(db), alpha, beta, ws.data_ptr(), ws.numel() * 8, hip.stream()), "wgrad_thin7")
    if PROFILE is not None:
        PROFILE.end("wgrad_thin", 2.0 * big.N * (big.H + 2 * rpad) * (big.W + 2 * rpad) * 49 * big.C * cs, t0, (big.C, cs, big.H, 70 + int(flip)))


def conv_small(x, wp_col, y, k, stride, pad=1, **epi):
    """y = conv_kxk(x) through the patch matrix: tnr_im2col, then TNR_CONV_1x1 over [pixels][k*k*C] (split-K)."""
    M, K = y.pixels, k * k * x.C
    dev = x.buf.device
    col = WS.get("im2col@%x" % hip.stream(), M * K * 4, dev)
    hip.check(hip.load().tnr_im2col(x.c(), x.N, x.H, x.W, x.C, k, stride, pad, y.H, y.W, col.data_ptr(), hip.stream()), "im2col")
    wimg = 32 if M % 32 == 0 else (16 if M % 16 == 0 else 8)
    cimg = col.view(torch.float32)[:M * K].view(1, M // wimg, wimg, K)
    yimg = View(y.buf.view(1, M // wimg, wimg, y.ctot), y.coff, y.C)
    conv(View(cimg), wp_col, yimg, mode=CONV_1x1, **epi)


def conv_col(x, wp_col, y, k, stride=1, pad=1, **epi):
    """y = conv_kxk(x) (TNR_PACK_COL_FWD weights) or the stride-1 data-gradient conv_kxk(g, pad = k - 1 - p) with flipped /
    transposed weights (TNR_PACK_COL_DGRAD3) for kernel geometries without a direct MFMA tile (the PatchGAN's 4x4 stride-1
    layers): tnr_im2col into [N, Ho, Wo, k*k*C], then the 1x1 implicit-GEMM kernel over that image."""
    K = k * k * x.C
    if K % 16 or K != wp_col.KinP:
        raise hip.HipEngineError("conv_col: k*k*C = %d must be a multiple of 16 and match the packed weights (%d)" % (K, wp_col.KinP))
    M = y.pixels
    col = WS.get("im2col@%x" % hip.stream(), M * K * 4, x.buf.device)
    hip.check(hip.load().tnr_im2col(x.c(), x.N, x.H, x.W, x.C, k, stride, pad, y.H, y.W, col.data_ptr(), hip.stream()), "im2col")
    conv(View(col.view(torch.float32)[:M * K].view(y.N, y.H, y.W, K)), wp_col, y, mode=CONV_1x1, **epi)


WGRAD_GROUP_MAX = 12


def _wgrad_desc(d, x, g, dw, db, mode, cin_begin, alpha, beta, reflect=False, pair=None):
    d.x = x.c()
    d.N, d.H, d.W, d.Cin = x.N, x.H, x.W, x.C
    d.g = g.c()
    d.Ho, d.Wo, d.Cout = g.H, g.W, g.C
    d.mode = mode
    d.dw, d.cin_total, d.cin_begin = dw.data_ptr(), dw.shape[1], cin_begin
    d.db = hip.ptr(db)
    d.alpha, d.beta = alpha, beta
    d.mma = MMA
    d.pad_mode = 1 if reflect else 0
    if pair is not None:           # cout pair: g covers two layers' gradients, channels >= split belong to (dw2, db2)
        dw2, db2, split = pair
        d.dw2, d.cin_total2, d.cout_split, d.db2 = dw2.data_ptr(), dw2.shape[1], split, hip.ptr(db2)


def wgrad(x, g, dw, db=None, mode=CONV_3x3, cin_begin=0, alpha=1.0, beta=1.0, reflect=False):
    """dw (OIHW, full tensor) += alpha * sum g (x) x over input channels [cin_begin, cin_begin+x.C)."""
    wgrad_group([dict(x=x, g=g, dw=dw, db=db, cin_begin=cin_begin, alpha=alpha, beta=beta, reflect=reflect)], mode=mode)


def wgrad_group(items, mode=CONV_3x3, family=None):
    """Several weight gradients of one pixel geometry and one workgroup tile class in a single launch
    (tnr_conv_wgrad_group).  items: dicts with x, g, dw and optional db, cin_begin, alpha, beta, pair = (dw2, db2, cout_split).
    family: the PROFILE family the launch is counted in instead of "wgrad_tile"."""
    lib = hip.load()
    n = len(items)
    assert 1 <= n <= WGRAD_GROUP_MAX
    descs = (WgradDesc * n)()
    for d, it in zip(descs, items):
        _wgrad_desc(d, it["x"], it["g"], it["dw"], it.get("db"), mode, it.get("cin_begin", 0),
                    it.get("alpha", 1.0), it.get("beta", 1.0), it.get("reflect", False), it.get("pair"))
    dev = items[0]["x"].buf.device
    for i, d in enumerate(descs):
        need = lib.tnr_wgrad_workspace_bytes(C.byref(d))
        ws = WS.get("wgrad%d" % i, need, dev)
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 8
    if PROFILE is None:
        hip.check(lib.tnr_conv_wgrad_group(descs, n, hip.stream()), "conv_wgrad_group")
        return
    t0 = PROFILE.begin()
    hip.check(lib.tnr_conv_wgrad_group(descs, n, hip.stream()), "conv_wgrad_group")
    taps = 16 if mode == CONV_4x4_S2 else 9
    x0, g0 = items[0]["x"], items[0]["g"]
    flops = sum(2.0 * it["g"].pixels * taps * it["x"].C * it["g"].C for it in items)
    PROFILE.end(family or "wgrad_tile", flops, t0, (sum(it["x"].C for it in items) if n > 1 else x0.C, g0.C, g0.H, mode + 100 * (n - 1)))


def wgrad_tile_class(desc, group_jobs=0):
    """tnr_wgrad_tile_class of a WgradDesc (host only, no launch) -> dict of the kernel's template arguments mode / a_t / b_t / thg / bf / wps /
    db and ks, splits, tiles_per_split, lds, row (the index in the library's table of tile classes)."""
    out = (C.c_int32 * 12)()
    hip.check(hip.load().tnr_wgrad_tile_class(C.byref(desc), group_jobs, C.byref(out)), "wgrad_tile_class")
    return dict(zip(("mode", "a_t", "b_t", "thg", "bf", "wps", "db", "ks", "splits", "tiles_per_split", "lds", "row"), out))


def wgrad_thin(big, small4, dw, db, flip, alpha=1.0, beta=1.0):
    """Weight gradient of a 3x3 layer with <= 3 channels on one side on the vector ALUs (tnr_wgrad_thin): flip=False
    for a 3 -> C layer (big = gradient of its output, small4 = NHWC4 input image), flip=True for a C -> 3 layer
    (big = its input, small4 = NHWC4 gradient of its output)."""
    lib = hip.load()
    cs = dw.shape[0] if flip else dw.shape[1]
    need = lib.tnr_wgrad_thin_workspace_bytes(big.N, big.H, big.C)
    ws = WS.get("wgrad_thin@%x" % hip.stream(), need, big.buf.device)
    t0 = PROFILE.begin() if PROFILE is not None else None
    hip.check(lib.tnr_wgrad_thin(big.c(), small4.c(), big.N, big.H, big.W, big.C, cs, int(flip), dw.data_ptr(), hip.ptr(db),
                                 alpha, beta, ws.data_ptr(), ws.numel() * 8, hip.stream()), "wgrad_thin")
    if PROFILE is not None:
        PROFILE.end("wgrad_thin", 2.0 * big.pixels * 9 * big.C * cs, t0, (big.C, cs, big.H, int(flip)))


# ----------------------------------------------------------------------------------------------
# layout / resampling / elementwise
# ----------------------------------------------------------------------------------------------
def nchw_to_nhwc(src, dst, Cpad=None, scale=None, shift=None):
    N, Cc, H, W = src.shape
    assert src.is_contiguous() and src.dtype == torch.float32
    hip.check(hip.load().tnr_nchw_to_nhwc(src.data_ptr(), N, Cc, H, W, dst.c(), dst.C if Cpad is None else Cpad,
                                          hip.ptr(scale), hip.ptr(shift), hip.stream()), "nchw_to_nhwc")


def nhwc_to_nchw(src, dst, scale=None, accumulate=False):
    N, Cc, H, W = dst.shape
    assert dst.is_contiguous() and dst.dtype == torch.float32
    hip.check(hip.load().tnr_nhwc_to_nchw(src.c(), N, Cc, H, W, dst.data_ptr(), hip.ptr(scale), int(accumulate),
                                          hip.stream()), "nhwc_to_nchw")


def upsample2x_bwd(gup, gx, mask=None, mslope=0.2):
    hip.check(hip.load().tnr_upsample2x_bwd(gup.c(), gx.c(), gx.N, gx.H, gx.W, gx.C, cv(mask), mslope, hip.stream()),
              "upsample2x_bwd")


def depth_to_space(x, y):
    hip.check(hip.load().tnr_depth_to_space(x.c(), y.c(), x.N, x.H, x.W, y.C, hip.stream()), "depth_to_space")


def space_to_depth_bwd(gy, gx, mask=None, mslope=0.2):
    hip.check(hip.load().tnr_space_to_depth_bwd(gy.c(), gx.c(), gx.N, gx.H, gx.W, gy.C, cv(mask), mslope, hip.stream()),
              "space_to_depth_bwd")


def maxpool2_fwd(x, y):
    hip.check(hip.load().tnr_maxpool2_fwd(x.c(), y.c(), x.N, x.H, x.W, x.C, hip.stream()), "maxpool2_fwd")


def maxpool2_bwd(gy, x, gx):
    hip.check(hip.load().tnr_maxpool2_bwd(gy.c(), x.c(), gx.c(), x.N, x.H, x.W, x.C, hip.stream()), "maxpool2_bwd")


def unpool2_bwd(gy, route, gx):
    """maxpool2_bwd from the route bytes conv_pool2 wrote ([N, H / 2, W / 2, C] uint8) instead of the full-resolution activation."""
    assert route.dtype == torch.uint8 and route.is_contiguous() and tuple(route.shape) == (gy.N, gy.H, gy.W, gy.C)
    assert (gx.N, gx.H, gx.W, gx.C) == (gy.N, 2 * gy.H, 2 * gy.W, gy.C)
    hip.check(hip.load().tnr_unpool2_bwd(gy.c(), route.data_ptr(), gx.c(), gx.N, gx.H, gx.W, gx.C, hip.stream()), "unpool2_bwd")


def bilinear2x_fwd(x, y):
    """y [N,2H,2W,C] = bilinear x2 of x [N,H,W,C], align_corners=False."""
    hip.check(hip.load().tnr_bilinear2x_fwd(x.c(), y.c(), x.N, x.H, x.W, x.C, hip.stream()), "bilinear2x_fwd")


def bilinear2x_bwd(gy, gx=None, gz=None, mask=None, mslope=0.2):
    """adjoint of bilinear2x_fwd: gx = plain gradient and / or gz = gradient * LeakyReLU'(mask)."""
    ref = gx if gx is not None else gz
    hip.check(hip.load().tnr_bilinear2x_bwd(gy.c(), cv(gx), cv(gz), cv(mask), mslope, ref.N, ref.H, ref.W, ref.C, hip.stream()),
              "bilinear2x_bwd")


def add2(dst, a, b):
    hip.check(hip.load().tnr_add2(dst.c(), a.c(), b.c(), dst.pixels, dst.C, hip.stream()), "add2")


def mask_copy(dst, src, y, mslope=0.2):
    hip.check(hip.load().tnr_mask_copy(dst.c(), src.c(), y.c(), dst.pixels, dst.C, mslope, hip.stream()), "mask_copy")


# ----------------------------------------------------------------------------------------------
# image-to-image family: generic convolution (vector ALUs), padding helpers, tanh, GAN loss
# ----------------------------------------------------------------------------------------------
def gconv_fwd(x, w, y, bias=None, stride=1, pad=0, reflect=False, act=ACT_NONE, slope=0.2):
    """y = act(conv(x, w) + bias): any square kernel / stride, zero or reflection padding (tnr_gconv_fwd); w OIHW."""
    Cout, Cin, k, _ = w.shape
    t0 = PROFILE.begin() if PROFILE is not None else None
    hip.check(hip.load().tnr_gconv_fwd(x.c(), x.N, x.H, x.W, Cin, w.data_ptr(), hip.ptr(bias), y.c(), y.H, y.W, Cout, k, stride, pad,
                                       int(reflect), act, slope, hip.stream()), "gconv_fwd")
    if PROFILE is not None:
        PROFILE.end("gconv", 2.0 * y.pixels * k * k * Cin * Cout, t0, (Cin, Cout, y.H, k))


def gconv_dgrad(g, w, gx, stride=1, pad=0, reflect=False):
    Cout, Cin, k, _ = w.shape
    t0 = PROFILE.begin() if PROFILE is not None else None
    hip.check(hip.load().tnr_gconv_dgrad(g.c(), gx.N, gx.H, gx.W, Cin, w.data_ptr(), gx.c(), g.H, g.W, Cout, k, stride, pad, int(reflect),
                                         hip.stream()), "gconv_dgrad")
    if PROFILE is not None:
        PROFILE.end("gconv", 2.0 * g.pixels * k * k * Cin * Cout, t0, (Cin, Cout, g.H, k + 100))


def gconv_wgrad(x, g, dw, db=None, stride=1, pad=0, reflect=False, alpha=1.0, beta=1.0):
    Cout, Cin, k, _ = dw.shape
    lib = hip.load()
    ws = WS.get("gconv_wgrad@%x" % hip.stream(), lib.tnr_gconv_wgrad_workspace_bytes(Cout, Cin, k), x.buf.device)
    t0 = PROFILE.begin() if PROFILE is not None else None
    hip.check(lib.tnr_gconv_wgrad(x.c(), x.N, x.H, x.W, Cin, g.c(), g.H, g.W, Cout, k, stride, pad, int(reflect), dw.data_ptr(), hip.ptr(db),
                                  alpha, beta, ws.data_ptr(), ws.numel() * 8, hip.stream()), "gconv_wgrad")
    if PROFILE is not None:
        PROFILE.end("gconv", 2.0 * g.pixels * k * k * Cin * Cout, t0, (Cin, Cout, g.H, k + 200))


def bias_grad(g, db, alpha=1.0, beta=1.0):
    """db = beta db + alpha * sum over the pixels of g (per channel)."""
    ws = WS.get("bias_grad@%x" % hip.stream(), 512 * g.C * 8, g.buf.device)
    hip.check(hip.load().tnr_bias_grad(g.c(), g.pixels, g.C, db.data_ptr(), alpha, beta, ws.data_ptr(), ws.numel() * 8, hip.stream()), "bias_grad")


def pad2d(x, y, pad, reflect):
    """y [N, H + 2 pad, W + 2 pad, C] = x with a zero (reflect False) or reflected border."""
    hip.check(hip.load().tnr_pad2d(x.c(), y.c(), x.N, x.H, x.W, x.C, pad, int(reflect), hip.stream()), "pad2d")


def unpad2d(xp, y, pad, fold):
    """y [N,H,W,C] = centre crop of xp (fold False) or the adjoint of the reflection padding (fold True)."""
    hip.check(hip.load().tnr_unpad2d(xp.c(), y.c(), y.N, y.H, y.W, y.C, pad, int(fold), hip.stream()), "unpad2d")


def window2d(src, dst, oy, ox, acc=False):
    """dst[n, y, x, :] (+)= src[n, y + oy, x + ox, :] inside src, 0 outside (same N and C; zero-embedding at an offset / offset
    crop; acc: added to dst instead of replacing it)."""
    hip.check(hip.load().tnr_window2d(src.c(), src.H, src.W, dst.c(), dst.N, dst.H, dst.W, dst.C, oy, ox, int(acc), hip.stream()), "window2d")


def tanh_fwd(x, y):
    hip.check(hip.load().tnr_tanh_fwd(x.data_ptr(), y.data_ptr(), x.numel(), hip.stream()), "tanh_fwd")


def tanh_bwd(g, y, gx):
    hip.check(hip.load().tnr_tanh_bwd(g.data_ptr(), y.data_ptr(), gx.data_ptr(), g.numel(), hip.stream()), "tanh_bwd")


def gan_loss(pred, kind, target, out, grad=None):
    """GANLoss against a constant label: kind 0 vanilla (BCE with logits), 1 lsgan (MSE), 2 mean(pred); out[0] = mean loss."""
    hip.check(hip.load().tnr_gan_loss(pred.data_ptr(), pred.numel(), kind, float(target), out.data_ptr(), hip.ptr(grad), hip.stream()), "gan_loss")


def axpby(dst, src, a=1.0, b=1.0):
    """dst = a*src + b*dst"""
    hip.check(hip.load().tnr_axpby(dst.c(), src.c(), dst.pixels, dst.C, a, b, hip.stream()), "axpby")


def mask_mul(g, y, mslope=0.2):
    hip.check(hip.load().tnr_mask_mul(g.c(), y.c(), g.pixels, g.C, mslope, hip.stream()), "mask_mul")


def fill(t, value=0.0):
    hip.check(hip.load().tnr_fill(t.data_ptr(), t.numel(), value, hip.stream()), "fill")


# ----------------------------------------------------------------------------------------------
# batch norm / linear
# ----------------------------------------------------------------------------------------------
def bn_train_fwd(z, y, gamma, beta, running_mean, running_var, num_batches, save_mean, save_invstd,
                 momentum=0.1, eps=1e-5, act=ACT_LRELU, slope=0.2, stat64=None):
    """stat64: optional fp64 [2 C] tensor that receives the batch mean / unbiased variance of the running-statistics update
    (bn_replay_running re-applies it)."""
    lib = hip.load()
    ws = WS.get("bn", lib.tnr_bn_workspace_bytes(z.C), z.buf.device)
    hip.check(lib.tnr_bn_train_fwd_stats(z.c(), y.c(), z.pixels, z.C, gamma.data_ptr(), beta.data_ptr(),
                                         hip.ptr(running_mean), hip.ptr(running_var), hip.ptr(num_batches), momentum, eps,
                                         save_mean.data_ptr(), save_invstd.data_ptr(), hip.ptr(stat64), act, slope, ws.data_ptr(),
                                         hip.stream()), "bn_train_fwd")


def bn_replay_running(running_mean, running_var, num_batches, stat64, momentum=0.1):
    """The side effects of one more training-mode forward over the same batch (running statistics, batch counter)."""
    hip.check(hip.load().tnr_bn_replay_running(running_mean.data_ptr(), running_var.data_ptr(), hip.ptr(num_batches), stat64.data_ptr(),
                                               running_mean.numel(), momentum, hip.stream()), "bn_replay_running")


BN_MASK_FROM_Z = os.environ.get("TNR_BN_MASK_FROM_Z", "1") != "0"      # A/B switch


def bn_train_bwd(gy, y, z, gz, gamma, save_mean, save_invstd, dgamma=None, dbeta=None, acc_beta=1.0, mslope=0.2, beta=None):
    """Backward of y = act(BatchNorm_train(z)).  beta (the forward's shift) given: the activation mask is recomputed from z
    (tnr_bn_train_bwd_z: bit-identical, y is not read)."""
    lib = hip.load()
    ws = WS.get("bn", lib.tnr_bn_workspace_bytes(z.C), z.buf.device)
    if beta is not None and BN_MASK_FROM_Z:
        hip.check(lib.tnr_bn_train_bwd_z(gy.c(), z.c(), gz.c(), z.pixels, z.C, gamma.data_ptr(), beta.data_ptr(), save_mean.data_ptr(),
                                         save_invstd.data_ptr(), mslope, hip.ptr(dgamma), hip.ptr(dbeta), acc_beta, ws.data_ptr(),
                                         hip.stream()), "bn_train_bwd_z")
        return
    hip.check(lib.tnr_bn_train_bwd(gy.c(), y.c(), z.c(), gz.c(), z.pixels, z.C, gamma.data_ptr(),
                                   save_mean.data_ptr(), save_invstd.data_ptr(), mslope, hip.ptr(dgamma),
                                   hip.ptr(dbeta), acc_beta, ws.data_ptr(), hip.stream()), "bn_train_bwd")


def instnorm_fwd(z, y, save_mean, save_invstd, eps=1e-5, act=ACT_NONE, slope=0.0):
    """y = act(InstanceNorm2d(z)) (no affine, per image and channel statistics); save_mean / save_invstd: [N * C]."""
    lib = hip.load()
    ws = WS.get("instnorm", lib.tnr_instnorm_workspace_bytes(z.N, z.C), z.buf.device)
    hip.check(lib.tnr_instnorm_fwd(z.c(), y.c(), z.N, z.H * z.W, z.C, eps, save_mean.data_ptr(), save_invstd.data_ptr(), act, slope,
                                   ws.data_ptr(), hip.stream()), "instnorm_fwd")


def instnorm_bwd(gy, y, z, gz, save_mean, save_invstd, mslope=1.0):
    """gz = d loss / d z of instnorm_fwd from gy, the gradient of its (activated) output; mslope: the activation's negative slope
    (0 ReLU, 1 no activation), the gate is read from y."""
    lib = hip.load()
    ws = WS.get("instnorm", lib.tnr_instnorm_workspace_bytes(z.N, z.C), z.buf.device)
    hip.check(lib.tnr_instnorm_bwd(gy.c(), y.c(), z.c(), gz.c(), z.N, z.H * z.W, z.C, save_mean.data_ptr(), save_invstd.data_ptr(),
                                   mslope, ws.data_ptr(), hip.stream()), "instnorm_bwd")


def linear_fwd(x, w, b, y, act=ACT_NONE, slope=0.2):
    N, In = x.shape
    Out = w.shape[0]
    hip.check(hip.load().tnr_linear_fwd(x.data_ptr(), w.data_ptr(), hip.ptr(b), y.data_ptr(), N, In, Out, act, slope,
                                        hip.stream()), "linear_fwd")


def linear_bwd(x, w, gy, yact=None, gx=None, dw=None, db=None, acc_beta=1.0, mslope=0.2):
    N, In = x.shape
    Out = w.shape[0]
    gpre = WS.get("lin", N * Out * 4, x.device)
    hip.check(hip.load().tnr_linear_bwd(x.data_ptr(), w.data_ptr(), gy.data_ptr(), hip.ptr(yact), mslope, hip.ptr(gx),
                                        hip.ptr(dw), hip.ptr(db), N, In, Out, acc_beta, gpre.data_ptr(), hip.stream()),
              "linear_bwd")


# ----------------------------------------------------------------------------------------------
# losses / optimiser
# ----------------------------------------------------------------------------------------------
def _reduce_ws(dev):
    """The fp64 partials of the two-stage reductions, one buffer per stream: two streams may reduce at the same time."""
    return WS.get("reduce@%x" % hip.stream(), hip.load().tnr_reduce_workspace_bytes(), dev)


def _floats(seq, n=None):
    """Python floats (filter taps, level weights) as the ctypes array of n (default: all of them) fp32 values the library reads."""
    return (C.c_float * (len(seq) if n is None else n))(*seq)


def l1_mean_fwd(a, b, scale, out):
    hip.check(hip.load().tnr_l1_mean_fwd(a.data_ptr(), b.data_ptr(), a.numel(), scale, out.data_ptr(),
                                         _reduce_ws(a.device).data_ptr(), hip.stream()), "l1_mean_fwd")


def l1_mean_bwd(a, b, scale, gscale, ga, accumulate=False):
    hip.check(hip.load().tnr_l1_mean_bwd(a.data_ptr(), b.data_ptr(), a.numel(), scale, hip.ptr(gscale), ga.data_ptr(),
                                         int(accumulate), hip.stream()), "l1_mean_bwd")


# Image-space losses and filters (csrc/ssim_loss.hip, image_losses.hip, freqsep.hip).  x, y and every other image operand: fp32
# N x C x H x W in one dense layout (`layout` 0 NCHW-contiguous, 1 channels-last); taps: Python floats already rounded to fp32.
# A backward writes gx in x's layout, times gscale[0] (None = 1).
def ssim_fwd(x, y, layout, shave, taps, C1, C2, sums):
    """sums[n] (fp64 [N, 2]) = {sum ssim_map, sum cs_map} of image n."""
    lib = hip.load()
    N, Ch, H, W = x.shape
    arr, K = _floats(taps), len(taps)
    nbytes = lib.tnr_ssim_workspace_bytes(N, Ch, H, W, shave, K)
    ws = WS.get("ssim@%x" % hip.stream(), nbytes, x.device)
    hip.check(lib.tnr_ssim_fwd(x.data_ptr(), y.data_ptr(), N, Ch, H, W, layout, shave, arr, K, C1, C2, sums.data_ptr(), ws.data_ptr(),
                               ws.numel() * 8, hip.stream()), "ssim_fwd")


def ssim_bwd(x, y, layout, shave, taps, C1, C2, coef, gscale, gx, accumulate=False):
    N, Ch, H, W = x.shape
    arr, K = _floats(taps), len(taps)
    hip.check(hip.load().tnr_ssim_bwd(x.data_ptr(), y.data_ptr(), N, Ch, H, W, layout, shave, arr, K, C1, C2, coef.data_ptr(),
                                      hip.ptr(gscale), gx.data_ptr(), int(accumulate), hip.stream()), "ssim_bwd")


def avgpool2_pad_dims(H, W, shave=0):
    ho, wo = C.c_int32(), C.c_int32()
    hip.check(hip.load().tnr_avgpool2_pad_dims(H, W, shave, C.byref(ho), C.byref(wo)), "avgpool2_pad_dims")
    return ho.value, wo.value


def avgpool2_pad_fwd(x, y, layout, shave, xo, yo):
    N, Ch, H, W = x.shape
    hip.check(hip.load().tnr_avgpool2_pad_fwd(x.data_ptr(), y.data_ptr(), N, Ch, H, W, layout, shave, xo.data_ptr(), yo.data_ptr(),
                                              hip.stream()), "avgpool2_pad_fwd")


def avgpool2_pad_bwd(gcoarse, gfine, layout, shave):
    N, Ch, H, W = gfine.shape
    hip.check(hip.load().tnr_avgpool2_pad_bwd(gcoarse.data_ptr(), gfine.data_ptr(), N, Ch, H, W, layout, shave, hip.stream()),
              "avgpool2_pad_bwd")


def msssim_combine(sums, levels, N, counts, weights, mode, value, coef):
    cnt = (C.c_int64 * levels)(*counts)
    wts = _floats(weights, levels) if weights is not None else None
    hip.check(hip.load().tnr_msssim_combine(sums.data_ptr(), levels, N, cnt, wts, mode, value.data_ptr(), coef.data_ptr(),
                                            hip.stream()), "msssim_combine")


# HFEN / image-gradient / total-variation / difference-only pixel losses.  crit: one of the CRIT_* numbers; every forward writes
# loss (1 float) = scale * sum rho(e), every backward gx = scale * gscale[0] * d sum rho / dx.
CRIT_L1, CRIT_L2, CRIT_CB, CRIT_ELASTIC, CRIT_CLIPL1 = 0, 1, 2, 3, 4


def _imgloss_ws(x):
    N, Ch, H, W = x.shape
    return WS.get("imgloss@%x" % hip.stream(), hip.load().tnr_imgloss_workspace_bytes(N, Ch, H, W), x.device)


def filter_loss_fwd(x, y, layout, taps, K, crit, scale, loss, dmap=None):
    """taps: K * K Python floats, row-major.  dmap (x's shape and layout, or None) receives rho'(L * (x - y))."""
    N, Ch, H, W = x.shape
    ws = _imgloss_ws(x)
    hip.check(hip.load().tnr_filter_loss_fwd(x.data_ptr(), y.data_ptr(), N, Ch, H, W, layout, _floats(taps, K * K), K, crit,
                                             float(scale), loss.data_ptr(), hip.ptr(dmap), ws.data_ptr(), ws.numel() * 8, hip.stream()),
              "filter_loss_fwd")


def filter_loss_bwd(dmap, layout, taps, K, scale, gscale, gx, accumulate=False):
    N, Ch, H, W = dmap.shape
    hip.check(hip.load().tnr_filter_loss_bwd(dmap.data_ptr(), N, Ch, H, W, layout, _floats(taps, K * K), K, float(scale),
                                             hip.ptr(gscale), gx.data_ptr(), int(accumulate), hip.stream()), "filter_loss_bwd")


def fd_loss_fwd(x, y, layout, dirs, crit, scale, loss):
    """y None: the responses of x alone (total variation)."""
    N, Ch, H, W = x.shape
    ws = _imgloss_ws(x)
    hip.check(hip.load().tnr_fd_loss_fwd(x.data_ptr(), hip.ptr(y), N, Ch, H, W, layout, dirs, crit, float(scale), loss.data_ptr(),
                                         ws.data_ptr(), ws.numel() * 8, hip.stream()), "fd_loss_fwd")


def fd_loss_bwd(x, y, layout, dirs, crit, scale, gscale, gx, accumulate=False):
    N, Ch, H, W = x.shape
    hip.check(hip.load().tnr_fd_loss_bwd(x.data_ptr(), hip.ptr(y), N, Ch, H, W, layout, dirs, crit, float(scale), hip.ptr(gscale),
                                         gx.data_ptr(), int(accumulate), hip.stream()), "fd_loss_bwd")


def pointwise_loss_fwd(a, b, crit, scale, loss):
    hip.check(hip.load().tnr_pointwise_loss_fwd(a.data_ptr(), b.data_ptr(), a.numel(), crit, float(scale), loss.data_ptr(),
                                                _reduce_ws(a.device).data_ptr(), hip.stream()), "pointwise_loss_fwd")


def pointwise_loss_bwd(a, b, crit, scale, gscale, ga, accumulate=False):
    hip.check(hip.load().tnr_pointwise_loss_bwd(a.data_ptr(), b.data_ptr(), a.numel(), crit, float(scale), hip.ptr(gscale), ga.data_ptr(),
                                                int(accumulate), hip.stream()), "pointwise_loss_bwd")


def overflow_loss_fwd(x, scale, loss):
    """loss (1 float) = scale * sum log(|x - clamp(x, 0, 1)| + 1) over a dense x of any rank."""
    hip.check(hip.load().tnr_overflow_loss_fwd(x.data_ptr(), x.numel(), float(scale), loss.data_ptr(), _reduce_ws(x.device).data_ptr(),
                                               hip.stream()), "overflow_loss_fwd")


def overflow_loss_bwd(x, scale, gscale, gx, accumulate=False):
    hip.check(hip.load().tnr_overflow_loss_bwd(x.data_ptr(), x.numel(), float(scale), hip.ptr(gscale), gx.data_ptr(), int(accumulate),
                                               hip.stream()), "overflow_loss_bwd")


# Pooled pixel losses (csrc/pooled_losses.hip): crit over k x k box averages (with `uv` over their two BT.601 chroma planes), and the
# five-level multi-scale sum.  crit: a CRIT_* above or CRIT_L1COS (over the channel vector of a cell).  One launch each way; the
# forwards' workspace starts with a ticket word that the kernels expect and leave at zero, so it is allocated zeroed and kept per
# stream handle.  The trade-off: zeroing the word before every forward would be a second enqueue per loss, which the one-launch form
# exists to avoid; instead a forward whose call reports an error drops its workspace, so the next one starts from a fresh zeroed
# buffer.  A launch that dies on the device without an error from the call takes the context with it.  A stream handle reused after
# its stream was destroyed gets the old buffer back, whose ticket is zero between launches.
CRIT_L1COS = 5
_POOLED_WS = {}


def _pooled_ws(x):
    key = (hip.stream(), str(x.device))
    t = _POOLED_WS.get(key)
    if t is None:
        t = _POOLED_WS[key] = torch.zeros(hip.load().tnr_pooled_workspace_bytes() // 8 + 1, dtype=torch.float64, device=x.device)
    return key, t


def _pooled_check(rc, key, what):
    if rc != 0:
        _POOLED_WS.pop(key, None)
    hip.check(rc, what)


def pooled_forward_blocks(pool_blocks=0, ms_blocks=0):
    """The largest grids of the two forwards, process-wide (0: the default): for measurements and tests of the multi-band paths."""
    hip.check(hip.load().tnr_pooled_forward_blocks(int(pool_blocks), int(ms_blocks)), "pooled_forward_blocks")


def pool_loss_fwd(x, y, layout, k, uv, crit, loss):
    """loss (1 float) = the mean-reduced crit of the k x k box averages of x and y (`uv`: of their chroma planes, C == 3)."""
    N, Ch, H, W = x.shape
    key, ws = _pooled_ws(x)
    _pooled_check(hip.load().tnr_pool_loss_fwd(x.data_ptr(), y.data_ptr(), N, Ch, H, W, layout, int(k), int(bool(uv)), crit, loss.data_ptr(),
                                               ws.data_ptr(), ws.numel() * 8, hip.stream()), key, "pool_loss_fwd")


def pool_loss_bwd(x, y, layout, k, uv, crit, gscale, gx, accumulate=False):
    N, Ch, H, W = x.shape
    hip.check(hip.load().tnr_pool_loss_bwd(x.data_ptr(), y.data_ptr(), N, Ch, H, W, layout, int(k), int(bool(uv)), crit, hip.ptr(gscale),
                                           gx.data_ptr(), int(accumulate), hip.stream()), "pool_loss_bwd")


def multiscale_loss_fwd(x, y, layout, crit, loss):
    """loss (1 float) = sum over five levels of w_i * the mean-reduced crit of the 2^i x 2^i box averages, w = 1, .5, .25, .125, .125."""
    N, Ch, H, W = x.shape
    key, ws = _pooled_ws(x)
    _pooled_check(hip.load().tnr_multiscale_loss_fwd(x.data_ptr(), y.data_ptr(), N, Ch, H, W, layout, crit, loss.data_ptr(), ws.data_ptr(),
                                                     ws.numel() * 8, hip.stream()), key, "multiscale_loss_fwd")


def multiscale_loss_bwd(x, y, layout, crit, gscale, gx, accumulate=False):
    N, Ch, H, W = x.shape
    hip.check(hip.load().tnr_multiscale_loss_bwd(x.data_ptr(), y.data_ptr(), N, Ch, H, W, layout, crit, hip.ptr(gscale), gx.data_ptr(),
                                                 int(accumulate), hip.stream()), "multiscale_loss_bwd")


# Spatial profile losses (csrc/spl_loss.hip).  mask: the families of derived planes the SPLoss traces run on; loss: 5 floats, one per
# family in the order of the bits and their sum; coef (spl_coef): the per-line backward coefficients the forward leaves.
SPL_RGB, SPL_YUV, SPL_DIMG, SPL_DYUV = 1, 2, 4, 8
SPL_CPL, SPL_GPL = SPL_RGB | SPL_YUV | SPL_DYUV, SPL_DIMG


def spl_coef(x, mask):
    N, Ch, H, W = x.shape
    return torch.empty(hip.load().tnr_spl_coef_bytes(N, Ch, H, W, mask) // 4, dtype=torch.float32, device=x.device)


def spl_loss_fwd(x, y, layout, mask, denorm, loss, coef):
    lib = hip.load()
    N, Ch, H, W = x.shape
    ws = WS.get("spl@%x" % hip.stream(), lib.tnr_spl_workspace_bytes(N, Ch, H, W, mask), x.device)
    hip.check(lib.tnr_spl_loss_fwd(x.data_ptr(), y.data_ptr(), N, Ch, H, W, layout, mask, int(bool(denorm)), loss.data_ptr(), coef.data_ptr(),
                                   ws.data_ptr(), ws.numel() * 8, hip.stream()), "spl_loss_fwd")


def spl_loss_bwd(x, y, layout, mask, denorm, coef, gscale, gx, accumulate=False):
    """gscale: 4 floats on the device, one per family (None = all 1)."""
    N, Ch, H, W = x.shape
    hip.check(hip.load().tnr_spl_loss_bwd(x.data_ptr(), y.data_ptr(), N, Ch, H, W, layout, mask, int(bool(denorm)), coef.data_ptr(),
                                          hip.ptr(gscale), gx.data_ptr(), int(accumulate), hip.stream()), "spl_loss_bwd")


# Frequency separation: the zero-padded 9 x 9 low-pass L from its 9 separable taps and the separator high-pass
# clamp((x - L x + 1) / 2, 0, 1); one launch each.
def freqsep_low(x, layout, taps9, out, gscale=None, accumulate=False):
    """out (+)= gscale[0] * (L x): FilterLow's forward and, L being its own adjoint, its backward."""
    N, Ch, H, W = x.shape
    hip.check(hip.load().tnr_freqsep_low(x.data_ptr(), N, Ch, H, W, layout, _floats(taps9, 9), hip.ptr(gscale), out.data_ptr(),
                                         int(accumulate), hip.stream()), "freqsep_low")


def freqsep_high_fwd(x, layout, taps9, out):
    N, Ch, H, W = x.shape
    hip.check(hip.load().tnr_freqsep_high_fwd(x.data_ptr(), N, Ch, H, W, layout, _floats(taps9, 9), out.data_ptr(), hip.stream()),
              "freqsep_high_fwd")


def freqsep_high_bwd(g, o, layout, taps9, gx, gscale=None, accumulate=False):
    """gx (+)= gscale[0] * (g' - L g'), g' = 0.5 g where the forward's saved output o is strictly inside (0, 1)."""
    N, Ch, H, W = g.shape
    hip.check(hip.load().tnr_freqsep_high_bwd(g.data_ptr(), o.data_ptr(), N, Ch, H, W, layout, _floats(taps9, 9), hip.ptr(gscale),
                                              gx.data_ptr(), int(accumulate), hip.stream()), "freqsep_high_bwd")


# DiffAugment (csrc/diffaug.hip): out = cutout_mask . Geo(Colour(x)).  params: fp32 [N, 8] on the device (the int fields written through
# an int32 view), geo: the 9 host integers {kind, flip, rot, offy, offx, inh, inw, color, cutout} (dataops/diffaug.py builds both).
def _diffaug_ws(x):
    return WS.get("diffaug@%x" % hip.stream(), hip.load().tnr_diffaug_workspace_bytes(x.shape[0]), x.device)


def diffaug_mean(src, layout, params, geo, backward=False):
    """-> the workspace with the fp64 partial sums of src[n] (forward) or of the pulled-back gradient (backward); one launch."""
    N, Ch, H, W = src.shape
    ws = _diffaug_ws(src)
    hip.check(hip.load().tnr_diffaug_mean(src.data_ptr(), N, Ch, H, W, layout, params.data_ptr(), (C.c_int32 * 9)(*geo), int(backward),
                                          ws.data_ptr(), ws.numel() * 8, hip.stream()), "diffaug_mean")
    return ws


def diffaug_fwd(x, layout, params, geo, ws, out):
    N, Ch, H, W = x.shape
    hip.check(hip.load().tnr_diffaug_fwd(x.data_ptr(), N, Ch, H, W, layout, params.data_ptr(), (C.c_int32 * 9)(*geo), hip.ptr(ws),
                                         out.data_ptr(), hip.stream()), "diffaug_fwd")


def diffaug_bwd(g, layout, params, geo, ws, gx):
    N, Ch, H, W = g.shape
    hip.check(hip.load().tnr_diffaug_bwd(g.data_ptr(), N, Ch, H, W, layout, params.data_ptr(), (C.c_int32 * 9)(*geo), hip.ptr(ws),
                                         gx.data_ptr(), hip.stream()), "diffaug_bwd")


# Batch augmentations (csrc/batchaug.hip).  prm: the 10 host integers {inside, outside, y0, x0, bh, bw, p0 .. p3}
# (dataops/batchaug.py builds them); x2 / r / col may be None where no region needs them.
def batchaug_mix(x, layout, prm, a, b, out, x2=None, r=None, col=None):
    N, Ch, H, W = x.shape
    hip.check(hip.load().tnr_batchaug_mix(x.data_ptr(), hip.ptr(x2), hip.ptr(r), hip.ptr(col), N, Ch, H, W, layout,
                                          (C.c_int32 * 10)(*prm), float(a), float(b), out.data_ptr(), hip.stream()), "batchaug_mix")


def batchaug_mask(x, layout, mask, s, out):
    """out = x * mask[n, y // s, x // s]; mask: uint8 N x (H / s) x (W / s), contiguous, on x's device."""
    N, Ch, H, W = x.shape
    hip.check(hip.load().tnr_batchaug_mask(x.data_ptr(), mask.data_ptr(), N, Ch, H, W, layout, int(s), out.data_ptr(), hip.stream()),
              "batchaug_mask")


# Gram matrix of an activation view and its gradient (csrc/gram.hip).  Always on the fp32 activations and in the fp32 arithmetic of
# TNR_MMA (FP32_MMA), also under `use_amp`: stricter than the reference, whose autocast runs the bmm in half precision.
def gram_fwd(x, scale, G):
    lib, dev = hip.load(), x.buf.device
    nbytes = lib.tnr_gram_workspace_bytes(x.N, x.H, x.W, x.C)
    ws = WS.get("gram@%x" % hip.stream(), nbytes, dev)
    hip.check(lib.tnr_gram_fwd(x.c(), x.N, x.H, x.W, x.C, scale, FP32_MMA, G.data_ptr(), ws.data_ptr(), ws.numel() * 8, hip.stream()),
              "gram_fwd")


def gram_bwd(x, S, scale, dx, accumulate=False):
    hip.check(hip.load().tnr_gram_bwd(x.c(), S.data_ptr(), x.N, x.H, x.W, x.C, scale, FP32_MMA, dx.c(), int(accumulate), hip.stream()),
              "gram_bwd")


# Contextual loss of two activation views and its gradient (csrc/contextual.hip).  Like the Gram matrix: on the fp32 activations and in
# the arithmetic of TNR_MMA, also under `use_amp`.
def _cx_ws(name, nbytes, dev, dtype=torch.float32):
    return WS.get("cx_%s@%x" % (name, hip.stream()), nbytes, dev).view(dtype)


def cx_sums(y, idx, P, sums):
    """sums[c] = sum of y over batch and (pooled) positions, sums[C] = the count: C + 1 floats a data-parallel group may all-reduce."""
    lib, dev = hip.load(), y.buf.device
    nbytes = lib.tnr_cx_sums_workspace_bytes(y.N, P, y.C)
    ws = WS.get("cx_sums@%x" % hip.stream(), nbytes, dev)
    hip.check(lib.tnr_cx_sums(y.c(), y.N, y.H, y.W, y.C, hip.ptr(idx), P, sums.data_ptr(), ws.data_ptr(), ws.numel() * 8, hip.stream()), "cx_sums")


def cx_prepare(x, idx, P, sums, xh, nrm):
    hip.check(hip.load().tnr_cx_prepare(x.c(), x.N, x.H, x.W, x.C, hip.ptr(idx), P, sums.data_ptr(), xh.data_ptr(), nrm.data_ptr(), hip.stream()),
              "cx_prepare")


def cx_layer(x, y, idx_x=None, idx_y=None, inv_x=None, b=1.0, h=0.5, dx=None, group=None, probe=None):
    """The contextual loss of the views x (SR tap) and y (HR tap): -> {'loss' (0-d), 'CS', 'rowmin', 'argmin', 'colmax', 'argmax'}.
    idx_x / idx_y: int32 device lists of the P pooled positions of each operand (None: all H W), inv_x: int32 [H W] map position -> slot
    or -1 (needed with idx_x when `dx` is given).  With the view `dx` the gradient kernels run too and d loss / d x is written into it
    (zeros at unsampled positions); without it they do not run.  `probe`, a dict, receives a copy of the distance matrix [N, P, P]
    (tests).  `group`: the data-parallel group whose ranks share the channel mean."""
    lib, dev, st = hip.load(), x.buf.device, hip.stream()
    N, C = x.N, x.C
    P = x.H * x.W if idx_x is None else idx_x.numel()
    Py = y.H * y.W if idx_y is None else idx_y.numel()
    if y.N != N or y.C != C or Py != P:
        raise ValueError("cx_layer: operands of %d x %d x %d and %d x %d x %d (images x positions x channels)" % (N, P, C, y.N, Py, y.C))
    for t in (idx_x, idx_y, inv_x):
        assert t is None or (t.dtype == torch.int32 and t.is_cuda and t.is_contiguous())
    sums = torch.empty(C + 1, dtype=torch.float32, device=dev)
    cx_sums(y, idx_y, P, sums)
    if group is not None:
        group.all_reduce_sum(sums)
    feat = _cx_ws("feat", 3 * N * P * C * 4, dev)
    xh, yh, dxh = feat[:N * P * C], feat[N * P * C:2 * N * P * C], feat[2 * N * P * C:3 * N * P * C]
    nrm_x = torch.empty(N * P, dtype=torch.float32, device=dev)
    nrm_y = torch.empty(N * P, dtype=torch.float32, device=dev)
    cx_prepare(x, idx_x, P, sums, xh, nrm_x)
    cx_prepare(y, idx_y, P, sums, yh, nrm_y)
    D = _cx_ws("matrix", lib.tnr_cx_matrix_bytes(N, P), dev)
    hip.check(lib.tnr_cx_distance(xh.data_ptr(), yh.data_ptr(), N, P, C, FP32_MMA, D.data_ptr(), st), "cx_distance")
    if probe is not None:
        ld = (P + 3) // 4 * 4
        probe["d"] = D[:N * P * ld].view(N, P, ld)[:, :, :P].clone()
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    out = {"rowmin": torch.empty((N, P), **f32), "argmin": torch.empty((N, P), **i32), "colmax": torch.empty((N, P), **f32),
           "argmax": torch.empty((N, P), **i32), "CS": torch.empty(N, **f32), "loss": torch.empty((), **f32)}
    rowE, gcoef = torch.empty((N, P), **f32), torch.empty(N, **f32)
    colpack = torch.empty((N, P), dtype=torch.int64, device=dev)
    hip.check(lib.tnr_cx_rows(D.data_ptr(), N, P, float(b), float(h), out["rowmin"].data_ptr(), out["argmin"].data_ptr(), rowE.data_ptr(),
                              colpack.data_ptr(), st), "cx_rows")
    hip.check(lib.tnr_cx_finalize(colpack.data_ptr(), N, P, out["colmax"].data_ptr(), out["argmax"].data_ptr(), out["CS"].data_ptr(),
                                  gcoef.data_ptr(), out["loss"].data_ptr(), st), "cx_finalize")
    if dx is not None:
        if idx_x is not None and inv_x is None:
            raise ValueError("cx_layer: a pooled gradient needs the inverse index map")
        cx_grad(D, xh, yh, dxh, nrm_x, N, P, C, h, out, rowE, gcoef, inv_x, dx)
    return out


def cx_grad(D, xh, yh, dxh, nrm_x, N, P, C, h, out, rowE, gcoef, inv_x, dx):
    """The three gradient launches of cx_layer (a function of its own so that a test can see whether they ran)."""
    lib, st = hip.load(), hip.stream()
    dwin = torch.empty((N, P), dtype=torch.float32, device=D.device)
    hip.check(lib.tnr_cx_grad_rows(D.data_ptr(), xh.data_ptr(), yh.data_ptr(), N, P, C, float(h), out["rowmin"].data_ptr(), out["argmin"].data_ptr(),
                                   rowE.data_ptr(), out["argmax"].data_ptr(), gcoef.data_ptr(), dwin.data_ptr(), st), "cx_grad_rows")
    hip.check(lib.tnr_cx_grad_gemm(D.data_ptr(), yh.data_ptr(), N, P, C, FP32_MMA, dxh.data_ptr(), st), "cx_grad_gemm")
    hip.check(lib.tnr_cx_norm_bwd(dxh.data_ptr(), xh.data_ptr(), nrm_x.data_ptr(), N, dx.H, dx.W, C, P, hip.ptr(inv_x), dx.c(), st), "cx_norm_bwd")


def ragan_phase_a(pf, pr, sums):
    hip.check(hip.load().tnr_ragan_phase_a(pf.data_ptr(), pr.data_ptr(), pf.numel(), sums.data_ptr(), _reduce_ws(pf.device).data_ptr(), hip.stream()), "ragan_a")


def ragan_phase_b(pf, pr, stage, sums):
    hip.check(hip.load().tnr_ragan_phase_b(pf.data_ptr(), pr.data_ptr(), pf.numel(), stage, sums.data_ptr(), _reduce_ws(pf.device).data_ptr(), hip.stream()),
              "ragan_b")


def ragan_phase_c(pf, pr, stage, weight, sums, out, gf, gr):
    hip.check(hip.load().tnr_ragan_phase_c(pf.data_ptr(), pr.data_ptr(), pf.numel(), stage, float(weight), sums.data_ptr(),
                                           out.data_ptr(), hip.ptr(gf), hip.ptr(gr), hip.stream()), "ragan_c")


def scale_by(dst, src, gscale):
    hip.check(hip.load().tnr_scale_by(dst.data_ptr(), src.data_ptr(), src.numel(), gscale.data_ptr(), hip.stream()),
              "scale_by")


def sumsq(g, out):
    hip.check(hip.load().tnr_sumsq(g.data_ptr(), g.numel(), out.data_ptr(), _reduce_ws(g.device).data_ptr(), hip.stream()),
              "sumsq")


def clip_by_norm(g, sumsq_t, max_norm):
    hip.check(hip.load().tnr_clip_by_norm(g.data_ptr(), g.numel(), sumsq_t.data_ptr(), max_norm, hip.stream()),
              "clip_by_norm")


def adam_step(p, g, m, v, step_size, b1, b2, bc2_sqrt, eps, wd=0.0):
    """One Adam launch over a flat buffer, behind the fault latch: if a tile hand-off of this process ever timed out, the update is
    NOT applied (the weights stay those of the last healthy step until check_engine_errors() raises)."""
    hip.check(hip.load().tnr_adam_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), step_size, b1,
                                               b2, bc2_sqrt, eps, wd, fault_word(p.device).data_ptr(), hip.stream()), "adam_step")


# ---------------------------------------------------------------------------------- the optimisers beside Adam (csrc/optimizers.hip)
# `table` is the flat buffer's SegTable (trainner_amd/flat.py).  Hyper-parameters arrive as the reference's classes name them; the few
# per-step scalars (bias corrections, N_sma, lamb) are formed here in Python doubles exactly as those classes form them.
def _tbl(table):
    return table.chunks.data_ptr(), table.nchunks


def _tbl_rows(table):
    need = hip.load().tnr_optim_workspace_bytes(table.nseg, table.nrows)
    assert table.ws.numel() >= need, "SegTable workspace is smaller than tnr_optim_workspace_bytes"
    return (table.chunks.data_ptr(), table.nchunks, table.segs.data_ptr(), table.nseg, table.rowseg.data_ptr(), table.nrows,
            table.ws.data_ptr(), table.ws.numel())


def sgd_step(p, g, buf, table, lr, momentum=0.0, wd=0.0):
    """torch.optim.SGD over a flat buffer, one launch behind the fault latch.  buf is None exactly when momentum is 0."""
    hip.check(hip.load().tnr_sgd_step_guarded(p.data_ptr(), g.data_ptr(), hip.ptr(buf), *_tbl(table), lr, momentum, wd,
                                              fault_word(p.device).data_ptr(), hip.stream()), "sgd_step")


def rmsprop_step(p, g, square_avg, table, lr, alpha, eps, wd=0.0):
    """torch.optim.RMSprop (not centered, no momentum) over a flat buffer, one launch behind the fault latch."""
    hip.check(hip.load().tnr_rmsprop_step_guarded(p.data_ptr(), g.data_ptr(), square_avg.data_ptr(), *_tbl(table), lr, alpha, eps, wd,
                                                  fault_word(p.device).data_ptr(), hip.stream()), "rmsprop_step")


def madgrad_step(p, g, grad_sum_sq, s, x0, table, lr, eps, k, momentum, decay=0.0, decay_type="AdamW"):
    """MADGRAD step number k (0-based) over a flat buffer, one launch behind the fault latch.  x0 is None exactly when momentum is 0."""
    lr = lr + eps                                   # the reference's own quirk (madgrad.py:87)
    lamb = lr * math.pow(k + 1, 0.5)
    hip.check(hip.load().tnr_madgrad_step_guarded(p.data_ptr(), g.data_ptr(), grad_sum_sq.data_ptr(), s.data_ptr(), hip.ptr(x0), *_tbl(table),
                                                  lamb, eps, decay, 1 - lr * decay, int(decay_type == "AdamW"), momentum,
                                                  fault_word(p.device).data_ptr(), hip.stream()), "madgrad_step")


def adamp_step(p, g, m, v, table, lr, b1, b2, eps, t, nesterov=False, delta=0.1, wd_ratio=0.1, wd=0.0):
    """AdamP step number t (1-based) over a flat buffer: 4 launches, the projection decision stays on the device."""
    hip.check(hip.load().tnr_adamp_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), *_tbl_rows(table),
                                                lr / (1 - b1 ** t), b1, b2, math.sqrt(1 - b2 ** t), eps, int(bool(nesterov)), delta, wd,
                                                1 - lr * wd * 1, 1 - lr * wd * wd_ratio, fault_word(p.device).data_ptr(), hip.stream()),
              "adamp_step")


def sgdp_step(p, g, buf, table, lr, momentum, dampening, eps, nesterov=False, delta=0.1, wd_ratio=0.1, wd=0.0):
    """SGDP over a flat buffer: 4 launches, the projection decision stays on the device."""
    hip.check(hip.load().tnr_sgdp_step_guarded(p.data_ptr(), g.data_ptr(), buf.data_ptr(), *_tbl_rows(table), lr, momentum, dampening, eps,
                                               int(bool(nesterov)), delta, wd, 1 - lr * wd * 1 / (1 - momentum) if wd > 0 else 1.0,
                                               1 - lr * wd * wd_ratio / (1 - momentum) if wd > 0 else 1.0,
                                               fault_word(p.device).data_ptr(), hip.stream()), "sgdp_step")


def ranger_scalars(t, b1, b2, nsma_threshold):
    """(rectified, step_size) of Ranger's step t (ranger.py:162-175)."""
    beta2_t = b2 ** t
    n_max = 2 / (1 - b2) - 1
    n_sma = n_max - 2 * t * beta2_t / (1 - beta2_t)
    if n_sma > nsma_threshold:
        return True, math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - b1 ** t)
    return False, 1.0 / (1 - b1 ** t)


def ranger_step(p, g, m, v, slow, table, lr, b1, b2, eps, wd, t, k=6, alpha=0.5, nsma_threshold=5, use_gc=True, gc_conv_only=False):
    """Ranger step number t (1-based) over a flat buffer: the row means of the gradient, then one launch with the centralised gradient,
    the (rectified) Adam update and, on every k-th step, the lookahead."""
    rect, step_size = ranger_scalars(t, b1, b2, nsma_threshold)
    gc_min_dim = (3 if gc_conv_only else 1) if use_gc else (1 << 30)
    hip.check(hip.load().tnr_ranger_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), slow.data_ptr(), *_tbl_rows(table),
                                                 gc_min_dim, b1, b2, eps, wd, step_size * lr, int(rect), int(t % k == 0), alpha,
                                                 fault_word(p.device).data_ptr(), hip.stream()), "ranger_step")


def swa_update(avg, p, n_averaged):
    """Stochastic weight averaging over a flat buffer: avg <- lerp(avg, p, fp32(1 / (n_averaged + 1))), n_averaged the host count of
    the updates made so far (0: avg becomes a copy of p).  One launch behind the fault latch."""
    assert avg.numel() == p.numel() and avg.dtype == p.dtype == torch.float32 and avg.is_contiguous() and p.is_contiguous()
    hip.check(hip.load().tnr_swa_update_guarded(avg.data_ptr(), p.data_ptr(), p.numel(), 1.0 / (int(n_averaged) + 1),
                                                fault_word(p.device).data_ptr(), hip.stream()), "swa_update")
