// RRDBNet's x3 up-conv layer (upscale 3: nearest x3, then a 3x3 pad-1 convolution nf -> nf, then LeakyReLU) as the transposed 5x5 stride-3
// padding-1 convolution of the LOW-resolution tensor it is exactly, borders included.  LR pixel i reaches the HR outputs
// 3i - 1 + k through folded tap k = 0..4 (common.h tnr_fold_*, 5 taps); by output phase (o mod 3) an output reads the LR neighbours
// {i - 1, i}, {i}, {i, i + 1} per axis: 4 + 2 + 4 + 2 + 1 + 2 + 4 + 2 + 4 = 25 products per LR pixel and channel pair against the 81 of the
// layer written out in the HR domain.  The up-sampled tensor never exists, in any of the three passes.
//   forward : y[3I + a, 3J + b] = act(bias + sum over the phase's taps of K[ky][kx] x[I + dy, J + dx])             nine GEMMs per LR tile
//   dgrad   : gx[i, j] = sum_k K[ky][kx]^T g[3i - 1 + ky, 3j - 1 + kx]  (* LeakyReLU'(mask))                        K = 25 nf
//   wgrad   : dK[ky][kx][ci][co] = sum over LR pixels x[I + dy, J + dx, ci] g[3I + a, 3J + b, co], then the 25 -> 9 unfold
// Forward and data gradient on mma_pixel.h's tile convention (an 8 x 16 LR tile per workgroup, the lane owns a pixel), every workgroup with
// all nf produced channels.  The activations are staged in LDS once (forward: the tile + a one-pixel zero halo; data gradient:
// the (3 * 8 + 2) x (3 * 16 + 2) gradient window in chunks of 16 channels) in the operand format of the arithmetic -- fp32, bf16, or the exact
// hi / mid / lo bf16 planes.  The folded weights do not fit LDS (25 x 64 x 64: 410 KB in fp32); TNR_PACK_UP3_* lays them out as ready A
// fragments in consumption order (already split for TNR_MMA_BF16X3, already rounded for TNR_MMA_BF16), so a wave streams them from L2 with one
// coalesced 16-byte load per lane and fragment, one step (a tap x 16 reduced channels) ahead of the matrix core; the main loop has no barrier.
// Sums: a tap's (forward) | a tap row's (data gradient) steps grow in one accumulation chain, then added to the running sum.
#include "mma_pixel.h"

namespace {

constexpr int U3_FH = MP_TH + 2, U3_FW = MP_TW + 2;        // forward: the staged tile with its halo, 180 pixels
constexpr int U3_GH = 3 * MP_TH + 2, U3_GW = 3 * MP_TW + 2; // data gradient: the staged window of g, 26 x 50 = 1300 pixels
constexpr int U3_WG_SLABS = 20;                            // weight gradient: pixel-block slabs per folded tap (25 x 20 workgroups)

// fragments of step s from the packed image (pack_api.hip: fp32 region [s][8-group][half][row][4], then bf16 region [s][plane][half][row][8 bf16])
template <int NT, int MMA>
__device__ __forceinline__ void u3_load_w(MpFrag<NT, MMA> &w, const float *wp, const int s, const int li, const int half) {
    constexpr int NF = NT * 32, KS = NF / 16;
    if constexpr (MMA == TNR_MMA_F32) {
        const float *base = wp + (size_t)s * 16 * NF;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int nn = 0; nn < NT; ++nn) w.f[g][nn] = *reinterpret_cast<const f32x4 *>(base + ((g * 2 + half) * NF + nn * 32 + li) * 4);
    } else {
        const float *base = wp + (size_t)25 * KS * NF * 16 + (size_t)s * 24 * NF;
#pragma unroll
        for (int p = 0; p < mp_planes(MMA); ++p)
#pragma unroll
            for (int nn = 0; nn < NT; ++nn) w.b[p][nn] = *reinterpret_cast<const tnr_bf16x8 *>(base + ((p * 2 + half) * NF + nn * 32 + li) * 4);
    }
}

// ------------------------------------------------------------------------------------------------ forward
struct Up3FwdK {
    const float *x; int x_ct, x_co, N, H, W;  // LR input view
    const float *wp;                          // TNR_PACK_UP3_FWD
    float *y; int y_ct, y_co;                 // HR output view [N, 3H, 3W, nf]
    const float *bias; float ns;              // act(v) = max(v, 0) + ns min(v, 0)
    int tiles_x, tiles_y;
};

// LDS pixel stride: nf + 4 floats | nf + 8 bf16, an odd number of 16-byte units, so the 16-byte reads of 8 consecutive pixels meet 8 bank groups
template <int NT, int MMA> constexpr int up3_fwd_lds() {
    constexpr int NF = NT * 32, px = U3_FH * U3_FW;
    return MMA == TNR_MMA_F32 ? px * (NF + 4) * 4 : px * (NF + 8) * 2 * mp_planes(MMA);
}

template <int NT, int MMA>
__global__ void __launch_bounds__(256) up3_fwd_kernel(const Up3FwdK a) {
    constexpr int NF = NT * 32, KS = NF / 16, NPIX = U3_FH * U3_FW;
    constexpr int PSF = NF + 4, PSB = NF + 8, PLANE = NPIX * PSB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *s_f = reinterpret_cast<float *>(smem);
    __bf16 *s_b = reinterpret_cast<__bf16 *>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, half = lane >> 5;
    int bid = blockIdx.x;
    const int tx = bid % a.tiles_x;
    bid /= a.tiles_x;
    const int ty = bid % a.tiles_y;
    const int n = bid / a.tiles_y;
    const int y0 = ty * MP_TH, x0 = tx * MP_TW;
    const int ly = 2 * wave + (li >> 4), lx = li & 15;              // mma_pixel.h: the lane's pixel of the tile

    MpFrag<NT, MMA> cur, nxt;
    u3_load_w<NT, MMA>(cur, a.wp, 0, li, half);
    nxt = cur;

    // ---- the LR tile and its halo, once; zeros outside the image (= the layer's zero padding seen from the LR domain)
    for (int i = tid; i < NPIX * (NF / 4); i += 256) {
        const int p = i / (NF / 4), c4 = i - p * (NF / 4);
        const int r = p / U3_FW, c = p - r * U3_FW;
        const int Y = y0 - 1 + r, X = x0 - 1 + c;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (Y >= 0 && Y < a.H && X >= 0 && X < a.W) v = *reinterpret_cast<const f32x4 *>(a.x + (((size_t)n * a.H + Y) * a.W + X) * a.x_ct + a.x_co + c4 * 4);
        mp_stage4<MMA>(v, s_f + p * PSF + c4 * 4, s_b + p * PSB + c4 * 4, PLANE);
    }
    __syncthreads();

    const int abase = (ly + 1) * U3_FW + lx + 1;                    // the lane's LR pixel in the staged tile
    const bool inside = y0 + ly < a.H && x0 + lx < a.W;
    int s = 0;
#pragma unroll 1
    for (int ph = 0; ph < 9; ++ph) {
        const int pa = ph / 3, pb = ph - pa * 3;
        f32x16 acc[NT];
        mp_zero<NT>(acc);
#pragma unroll 1
        for (int t = 0; t < tnr_up3_ntaps(pa) * tnr_up3_ntaps(pb); ++t) {
            int dy, dx, ky, kx;
            tnr_up3_phase_tap(pa, t / tnr_up3_ntaps(pb), &dy, &ky);
            tnr_up3_phase_tap(pb, t % tnr_up3_ntaps(pb), &dx, &kx);
            const int pix = abase + dy * U3_FW + dx;
            f32x16 part[NT];                                        // one tap's nf products, then added to the phase's sum
            mp_zero<NT>(part);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks, ++s) {
                if (s + 1 < 25 * KS) u3_load_w<NT, MMA>(nxt, a.wp, s + 1, li, half);
                mp_step<NT, MMA>(part, cur, s_f + pix * PSF + ks * 16, s_b + pix * PSB + ks * 16, PLANE, half);
                cur = nxt;
            }
            mp_add<NT>(acc, part);
        }
        // ---- this phase's pixel (3 (y0 + ly) + pa, 3 (x0 + lx) + pb)
        if (inside) {
            float *yp = a.y + (((size_t)n * 3 * a.H + 3 * (y0 + ly) + pa) * 3 * a.W + 3 * (x0 + lx) + pb) * a.y_ct + a.y_co;
#pragma unroll
            for (int nn = 0; nn < NT; ++nn)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int co = nn * 32 + q * 8 + half * 4;
                    const f32x4 v = {acc[nn][4 * q], acc[nn][4 * q + 1], acc[nn][4 * q + 2], acc[nn][4 * q + 3]};
                    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
                    if (a.bias != nullptr) bv = *reinterpret_cast<const f32x4 *>(a.bias + co);
                    *reinterpret_cast<f32x4 *>(yp + co) = tnr_bias_act4(v, bv, a.ns, 1.f);
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ data gradient
struct Up3DgradK {
    const float *g; int g_ct, g_co, N, H, W;  // HR gradient view [N, 3H, 3W, nf]; H, W: the LR extent
    const float *wp;                          // TNR_PACK_UP3_DGRAD
    float *gx; int gx_ct, gx_co;
    const float *m; int m_ct, m_co; float m_slope;
    int tiles_x, tiles_y;
};

// one 16-channel chunk of the window: 64 bytes per pixel in fp32, 32 bytes per pixel and plane in the bf16 forms (83 KB | 42 KB | 125 KB)
template <int MMA> constexpr int up3_dgrad_lds() {
    constexpr int px = U3_GH * U3_GW;
    return MMA == TNR_MMA_F32 ? px * 64 : px * 32 * mp_planes(MMA);
}

template <int NT, int MMA>
__global__ void __launch_bounds__(256) up3_dgrad_kernel(const Up3DgradK a) {
    constexpr int NF = NT * 32, KS = NF / 16, NPIX = U3_GH * U3_GW, PLANE = NPIX * 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *s_f = reinterpret_cast<float *>(smem);
    __bf16 *s_b = reinterpret_cast<__bf16 *>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, half = lane >> 5;
    int bid = blockIdx.x;
    const int tx = bid % a.tiles_x;
    bid /= a.tiles_x;
    const int ty = bid % a.tiles_y;
    const int n = bid / a.tiles_y;
    const int y0 = ty * MP_TH, x0 = tx * MP_TW;
    const int ly = 2 * wave + (li >> 4), lx = li & 15;              // mma_pixel.h: the lane's pixel of the tile
    const int Hh = 3 * a.H, Wh = 3 * a.W;

    MpFrag<NT, MMA> cur, nxt;
    u3_load_w<NT, MMA>(cur, a.wp, 0, li, half);
    nxt = cur;

    const int abase = 3 * ly * U3_GW + 3 * lx;                      // the lane's LR pixel: its window starts at (3 ly, 3 lx)
    f32x16 acc[NT];
    mp_zero<NT>(acc);
    int s = 0;
#pragma unroll 1
    for (int ks = 0; ks < KS; ++ks) {
        if (ks) __syncthreads();                                    // the previous chunk's window is read
        // ---- channels 16 ks .. + 15 of the window: HR rows 3 y0 - 1 .. 3 (y0 + 8), zeros outside the HR image
        for (int i = tid; i < NPIX * 4; i += 256) {
            const int p = i >> 2, c4 = i & 3;
            const int r = p / U3_GW, c = p - r * U3_GW;
            const int Y = 3 * y0 - 1 + r, X = 3 * x0 - 1 + c;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (Y >= 0 && Y < Hh && X >= 0 && X < Wh)
                v = *reinterpret_cast<const f32x4 *>(a.g + (((size_t)n * Hh + Y) * Wh + X) * a.g_ct + a.g_co + ks * 16 + c4 * 4);
            mp_stage4<MMA>(v, s_f + p * 16 + c4 * 4, s_b + p * 16 + c4 * 4, PLANE);
        }
        __syncthreads();
#pragma unroll 1
        for (int ky = 0; ky < 5; ++ky) {
            f32x16 part[NT];                                        // one row of taps (80 products), then added to the running sum
            mp_zero<NT>(part);
#pragma unroll
            for (int kx = 0; kx < 5; ++kx, ++s) {
                if (s + 1 < 25 * KS) u3_load_w<NT, MMA>(nxt, a.wp, s + 1, li, half);
                const int pix = abase + ky * U3_GW + kx;
                mp_step<NT, MMA>(part, cur, s_f + pix * 16, s_b + pix * 16, PLANE, half);
                cur = nxt;
            }
            mp_add<NT>(acc, part);
        }
    }
    if (y0 + ly < a.H && x0 + lx < a.W) {
        const size_t pixel = ((size_t)n * a.H + y0 + ly) * a.W + x0 + lx;
        float *gp = a.gx + pixel * a.gx_ct + a.gx_co;
#pragma unroll
        for (int nn = 0; nn < NT; ++nn)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ci = nn * 32 + q * 8 + half * 4;
                f32x4 v = {acc[nn][4 * q], acc[nn][4 * q + 1], acc[nn][4 * q + 2], acc[nn][4 * q + 3]};
                if (a.m != nullptr) {                               // LeakyReLU' of the activation that produced the layer's input
                    const f32x4 mv = *reinterpret_cast<const f32x4 *>(a.m + pixel * a.m_ct + a.m_co + ci);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = mv[e] > 0.f ? v[e] : v[e] * a.m_slope;
                }
                *reinterpret_cast<f32x4 *>(gp + ci) = v;
            }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct Up3WgradK {
    const float *x; int x_ct, x_co, N, H, W;
    const float *g; int g_ct, g_co;
    float *ws;                                // [slab][25][ci][co]
    int tiles_x, tiles_y, tiles, slabs;
};

template <int NT> constexpr int up3_wgrad_lds() { return 2 * MP_TPIX * NT * 32 * 4; }

// Workgroup (tap k = ky * 5 + kx, slab): dK[k] over the tiles slab, slab + slabs, ...  Per tile it stages the tap's two operands -- x of the
// tile shifted by the tap's LR offset (zeros outside the image) and g at the tap's phase of the tile's 3 x 3 blocks -- and every wave
// multiplies its two tile rows (32 pixels = 16 steps of v_mfma_f32_32x32x2_f32) into all nf x nf accumulators, kept in registers over the
// workgroup's tiles.  The four waves' sums are then added in wave order through LDS: the order in which every partial sum grows is fixed.
template <int NT>
__global__ void __launch_bounds__(256) up3_wgrad_kernel(const Up3WgradK a) {
    constexpr int NF = NT * 32, TPIX = MP_TPIX;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *s_x = reinterpret_cast<float *>(smem);
    float *s_g = s_x + TPIX * NF;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, half = lane >> 5;
    const int ky = blockIdx.x / 5, kx = blockIdx.x - ky * 5;
    // output 3i - 1 + k = 3I + a: phase a = (k + 2) mod 3, LR source i = I + d
    const int pa = (ky + 2) % 3, pb = (kx + 2) % 3;
    const int dy = ky == 0 ? 1 : (ky == 4 ? -1 : 0), dx = kx == 0 ? 1 : (kx == 4 ? -1 : 0);
    const int Hh = 3 * a.H, Wh = 3 * a.W;

    f32x16 acc[NT][NT];
#pragma unroll
    for (int ib = 0; ib < NT; ++ib) mp_zero<NT>(acc[ib]);

    for (int tile = blockIdx.y; tile < a.tiles; tile += a.slabs) {
        int q = tile;
        const int tx = q % a.tiles_x;
        q /= a.tiles_x;
        const int ty = q % a.tiles_y;
        const int n = q / a.tiles_y;
        const int y0 = ty * MP_TH, x0 = tx * MP_TW;
        __syncthreads();
        for (int i = tid; i < TPIX * (NF / 4); i += 256) {
            const int p = i / (NF / 4), c4 = i - p * (NF / 4);
            const int I = y0 + p / MP_TW, J = x0 + p % MP_TW;
            f32x4 xv = {0.f, 0.f, 0.f, 0.f}, gv = {0.f, 0.f, 0.f, 0.f};
            if (I < a.H && J < a.W) {
                gv = *reinterpret_cast<const f32x4 *>(a.g + (((size_t)n * Hh + 3 * I + pa) * Wh + 3 * J + pb) * a.g_ct + a.g_co + c4 * 4);
                const int Y = I + dy, X = J + dx;
                if (Y >= 0 && Y < a.H && X >= 0 && X < a.W) xv = *reinterpret_cast<const f32x4 *>(a.x + (((size_t)n * a.H + Y) * a.W + X) * a.x_ct + a.x_co + c4 * 4);
            }
            *reinterpret_cast<f32x4 *>(s_x + p * NF + c4 * 4) = xv;
            *reinterpret_cast<f32x4 *>(s_g + p * NF + c4 * 4) = gv;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < 16; ++kk) {
            const int pix = wave * 32 + 2 * kk + half;
            float av[NT], bv[NT];
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                av[b] = s_x[pix * NF + b * 32 + li];
                bv[b] = s_g[pix * NF + b * 32 + li];
            }
#pragma unroll
            for (int ib = 0; ib < NT; ++ib)
#pragma unroll
                for (int jb = 0; jb < NT; ++jb) acc[ib][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ib], bv[jb], acc[ib][jb], 0, 0, 0);
        }
    }
    // ---- the four waves' sums through LDS ([wave][ci][co], inside the staging area), added in wave order
    __syncthreads();
    float *s_r = reinterpret_cast<float *>(smem);
#pragma unroll
    for (int ib = 0; ib < NT; ++ib)
#pragma unroll
        for (int jb = 0; jb < NT; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ib * 32 + (r >> 2) * 8 + half * 4 + (r & 3);
                s_r[(wave * NF + ci) * NF + jb * 32 + li] = acc[ib][jb][r];
            }
    __syncthreads();
    float *slab = a.ws + ((size_t)blockIdx.y * 25 + blockIdx.x) * NF * NF;
    for (int i = tid; i < NF * NF; i += 256) slab[i] = ((s_r[i] + s_r[NF * NF + i]) + s_r[2 * NF * NF + i]) + s_r[3 * NF * NF + i];
}

struct Up3UnfoldK {
    const float *ws; int slabs, nf;
    float *dw; float alpha, beta;
};

// one thread per (3x3 tap, ci, co): per folded tap the slabs in index order, then the folded taps (2 - t .. 4 - t per axis) in ascending (ky, kx)
__global__ void __launch_bounds__(256) up3_wgrad_unfold_kernel(const Up3UnfoldK a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, nn = a.nf * a.nf;
    if (i >= 9 * nn) return;
    const int t = i / nn, cc = i - t * nn, ci = cc / a.nf, co = cc - ci * a.nf;
    const int ty = t / 3, tx = t - ty * 3;
    float sum = 0.f;
    for (int ky = 2 - ty; ky <= 4 - ty; ++ky)
        for (int kx = 2 - tx; kx <= 4 - tx; ++kx) {
            const float *src = a.ws + (size_t)(ky * 5 + kx) * nn + cc;
            float p = 0.f;
            for (int sl = 0; sl < a.slabs; ++sl) p += src[(size_t)sl * 25 * nn];
            sum += p;
        }
    const size_t o = ((size_t)co * a.nf + ci) * 9 + t;
    a.dw[o] = (a.beta != 0.f ? a.beta * a.dw[o] : 0.f) + a.alpha * sum;
}

// ------------------------------------------------------------------------------------------------ host side
int up3_geometry(const char *who, int N, int H, int W, int nf, int *tiles_x, int *tiles_y, int64_t *tiles) {
    const int rc = mp_geometry(who, N, H, W, 3, tiles_x, tiles_y, tiles);
    if (rc != TNR_OK) return rc;
    TNR_REQUIRE(nf == 32 || nf == 64, "%s: nf must be 32 or 64 (got %d)", who, nf);
    return TNR_OK;
}

int up3_wgrad_slabs(int64_t tiles) { return tiles < U3_WG_SLABS ? (int)tiles : U3_WG_SLABS; }

}  // namespace

extern "C" int tnr_upconv3_fwd(tnr_view x, int32_t N, int32_t H, int32_t W, const float *wp, tnr_view y, int32_t nf, const float *bias,
                               int32_t act, float slope, int32_t mma, void *stream) {
    Up3FwdK k;
    int64_t tiles;
    const int rc = up3_geometry("upconv3_fwd", N, H, W, nf, &k.tiles_x, &k.tiles_y, &tiles);
    if (rc != TNR_OK) return rc;
    TNR_REQUIRE(wp && mp_view_ok(x, nf) && mp_view_ok(y, nf), "upconv3_fwd: bad views");
    TNR_REQUIRE(mp_mma_ok(mma), "upconv3_fwd: bad mma %d", mma);
    TNR_REQUIRE(act == TNR_ACT_NONE || act == TNR_ACT_LRELU || act == TNR_ACT_RELU, "upconv3_fwd: bad activation %d", act);
    k.x = x.ptr; k.x_ct = x.ctot; k.x_co = x.coff; k.N = N; k.H = H; k.W = W; k.wp = wp;
    k.y = y.ptr; k.y_ct = y.ctot; k.y_co = y.coff;
    k.bias = bias; k.ns = act == TNR_ACT_LRELU ? slope : (act == TNR_ACT_RELU ? 0.f : 1.f);
    static int cus = 0;
#define U3_FWD(NT, MMA) tnr_kernel_lds(up3_fwd_kernel<NT, MMA>, up3_fwd_lds<NT, MMA>())
    return mp_launch(&cus, "upconv3_fwd", {MP_MODES(U3_FWD, 1), MP_MODES(U3_FWD, 2)}, (nf == 64 ? 3 : 0) + mma, dim3((unsigned)tiles), &k, stream);
#undef U3_FWD
}

extern "C" int tnr_upconv3_dgrad(tnr_view g, int32_t N, int32_t H, int32_t W, const float *wp, tnr_view gx, int32_t nf, tnr_view mask,
                                 float m_slope, int32_t mma, void *stream) {
    Up3DgradK k;
    int64_t tiles;
    const int rc = up3_geometry("upconv3_dgrad", N, H, W, nf, &k.tiles_x, &k.tiles_y, &tiles);
    if (rc != TNR_OK) return rc;
    TNR_REQUIRE(wp && mp_view_ok(g, nf) && mp_view_ok(gx, nf) && (mask.ptr == nullptr || mp_view_ok(mask, nf)), "upconv3_dgrad: bad views");
    TNR_REQUIRE(mp_mma_ok(mma), "upconv3_dgrad: bad mma %d", mma);
    k.g = g.ptr; k.g_ct = g.ctot; k.g_co = g.coff; k.N = N; k.H = H; k.W = W; k.wp = wp;
    k.gx = gx.ptr; k.gx_ct = gx.ctot; k.gx_co = gx.coff;
    k.m = mask.ptr; k.m_ct = mask.ctot; k.m_co = mask.coff; k.m_slope = m_slope;
    static int cus = 0;
#define U3_DG(NT, MMA) tnr_kernel_lds(up3_dgrad_kernel<NT, MMA>, up3_dgrad_lds<MMA>())
    return mp_launch(&cus, "upconv3_dgrad", {MP_MODES(U3_DG, 1), MP_MODES(U3_DG, 2)}, (nf == 64 ? 3 : 0) + mma, dim3((unsigned)tiles), &k, stream);
#undef U3_DG
}

extern "C" int64_t tnr_upconv3_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t nf) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)up3_wgrad_slabs(mp_tiles(N, H, W)) * 25 * nf * nf * (int64_t)sizeof(float);
}

extern "C" int tnr_upconv3_wgrad(tnr_view x, tnr_view g, int32_t N, int32_t H, int32_t W, int32_t nf, float *dw, float alpha, float beta,
                                 float *ws, int64_t ws_bytes, void *stream) {
    Up3WgradK k;
    int64_t tiles;
    int rc = up3_geometry("upconv3_wgrad", N, H, W, nf, &k.tiles_x, &k.tiles_y, &tiles);
    if (rc != TNR_OK) return rc;
    TNR_REQUIRE(dw && ws && mp_view_ok(x, nf) && mp_view_ok(g, nf), "upconv3_wgrad: bad arguments");
    TNR_REQUIRE(tnr_upconv3_wgrad_workspace_bytes(N, H, W, nf) <= ws_bytes, "upconv3_wgrad: workspace too small");
    k.x = x.ptr; k.x_ct = x.ctot; k.x_co = x.coff; k.N = N; k.H = H; k.W = W;
    k.g = g.ptr; k.g_ct = g.ctot; k.g_co = g.coff;
    k.ws = ws; k.tiles = (int)tiles; k.slabs = up3_wgrad_slabs(tiles);
    static int cus = 0;
#define U3_WG(NT) tnr_kernel_lds(up3_wgrad_kernel<NT>, up3_wgrad_lds<NT>())
    rc = mp_launch(&cus, "upconv3_wgrad", {U3_WG(1), U3_WG(2)}, nf == 64 ? 1 : 0, dim3(25, (unsigned)k.slabs), &k, stream);
#undef U3_WG
    if (rc != TNR_OK) return rc;
    Up3UnfoldK u;
    u.ws = ws; u.slabs = k.slabs; u.nf = nf; u.dw = dw; u.alpha = alpha; u.beta = beta;
    hipLaunchKernelGGL(up3_wgrad_unfold_kernel, dim3(tnr_cdiv(9 * nf * nf, 256)), dim3(256), 0, (hipStream_t)stream, u);
    return tnr_check_launch("upconv3_wgrad_unfold");
}
