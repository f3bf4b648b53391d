// The image-to-image decoders' up-conv layer (upsample_mode: upconv -- nearest x2, then a 3x3 pad-1 convolution Cin -> Cout, no activation:
// a norm layer follows) as the transposed 4x4 stride-2 padding-1 convolution of the LOW-resolution tensor it is, borders included.
// LR pixel i reaches the HR outputs 2i - 1 + k through folded tap k = 0..3 (common.h tnr_fold_*, 4 taps); an output of parity a = o mod 2 reads the
// two LR neighbours I - 1 + a + u, u = 0, 1, through folded tap 3 - a - 2u per axis: 4 x 4 = 16 products per LR pixel and channel pair
// against the 36 of the layer written out in the HR domain.  The up-sampled tensor never exists, in any of the three passes.
//   forward : y[2I + a, 2J + b] = bias + sum over the parity's 2 x 2 taps of F[ky][kx] x[I + dy, J + dx]        four GEMMs per staged LR tile
//   dgrad   : gx[i, j] = sum_k F[ky][kx]^T g[2i - 1 + ky, 2j - 1 + kx]                                         K = 16 Cout, LR domain directly
//   wgrad   : dF[ky][kx][ci][co] = sum over LR pixels x[I + dy, J + dx, ci] g[2I + a, 2J + b, co], then the 16 -> 9 unfold
// Channel counts are multiples of 4, Cout <= 512, Cin <= 2048 (the decoders run Cin = Cout, 2 Cout and 4 Cout, 32 .. 512 produced channels;
// the thin layers next to the image run through the same kernels with their rows / reduced channels zero-extended to 32 / 16).
// Forward and data gradient on mma_pixel.h's tile convention (an 8 x 16 LR tile per workgroup, the lane owns a pixel), a workgroup with 32 NT
// produced channels.  The activations go through LDS in chunks of the reduced channels (forward: 32 channels of the tile + a
// one-pixel zero halo, read by all four parities; data gradient: 16 channels of the (2 * 8 + 2) x (2 * 16 + 2) gradient window) in the operand
// format of the arithmetic -- fp32, bf16, or the exact hi / mid / lo bf16 planes.  The folded weights (16 Cin Cout: up to 33 MB in fp32) never
// enter LDS: tnr_upconv_i2i_pack lays them out as ready A fragments in consumption order (already split for TNR_MMA_BF16X3, already rounded for
// TNR_MMA_BF16), and a wave streams them from L2 with one coalesced 16-byte load per lane and fragment, one step (a tap x 16 reduced channels)
// ahead of the matrix core.  Sums: one step per accumulation chain on the matrix core, then VALU fp32 into the chunk's partial sum, then into
// the running sum (DESIGN.md 29 "Summation").  The tap loops are rolled on purpose: no instance spills (DESIGN.md 29 "Registers").  A wave whose two tile rows lie below the image streams nothing (the 1 x 1 .. 4 x 4 end of the U-Net: the layer is
// weight-bound there, and the launcher hands out 32-channel row blocks instead of 64 so that twice as many CUs stream disjoint weight slices).
#include "mma_pixel.h"

namespace {

constexpr int UI_FW = MP_TW + 2, UI_FPIX = (MP_TH + 2) * UI_FW;   // forward: the staged tile with its halo, 180 pixels
constexpr int UI_FCK = 32;                                    // forward: reduced channels per LDS fill
constexpr int UI_FPSF = UI_FCK + 4, UI_FPSB = UI_FCK + 8;     // LDS pixel strides (floats | bf16): an odd number of 16-byte units
constexpr int UI_GW = 2 * MP_TW + 2, UI_GPIX = (2 * MP_TH + 2) * UI_GW;   // data gradient: the staged window of g, 18 x 34 = 612 pixels
constexpr int UI_GPSF = 20, UI_GPSB = 24;                     // 16 channels + pad: 80 | 48 bytes
constexpr int UI_MAX_COUT = 512, UI_MAX_CIN = 2048;

// floats of one step (a tap x 16 reduced channels) of one 32-row block in the packed image
__host__ __device__ constexpr int ui_unit(int mma) { return mma == TNR_MMA_F32 ? 512 : (mma == TNR_MMA_BF16 ? 256 : 768); }

// fragments of step s; `wp` points at the workgroup's first 32-row block: [step][row block][fp32: 8-group][half][row][4] | [plane][half][row][8 bf16]
template <int NT, int MMA>
__device__ __forceinline__ void ui_load_w(MpFrag<NT, MMA> &w, const float *wp, const int s, const int R32, const int li, const int half) {
    constexpr int UNIT = ui_unit(MMA);
    const float *base = wp + (size_t)s * R32 * UNIT;
    if constexpr (MMA == TNR_MMA_F32) {
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int nn = 0; nn < NT; ++nn) w.f[g][nn] = *reinterpret_cast<const f32x4 *>(base + nn * UNIT + ((g * 2 + half) * 32 + li) * 4);
    } else {
#pragma unroll
        for (int p = 0; p < mp_planes(MMA); ++p)
#pragma unroll
            for (int nn = 0; nn < NT; ++nn) w.b[p][nn] = *reinterpret_cast<const tnr_bf16x8 *>(base + nn * UNIT + ((p * 2 + half) * 32 + li) * 4);
    }
}

// ------------------------------------------------------------------------------------------------ weight image
// Step order.  Forward (rows = Cout, reduced = Cin): s = ((chunk * 4 + parity) * 4 + neighbour) * 2 + half-chunk, parity = 2a + b, neighbour =
// 2uy + ux, folded tap (3 - a - 2uy, 3 - b - 2ux), reduced channels 32 chunk + 16 half-chunk + 0..15.  Data gradient (rows = Cin, reduced =
// Cout): s = chunk * 16 + ky * 4 + kx, reduced channels 16 chunk + 0..15.  Rows and reduced channels past the layer's own are zeros.
struct UiPackK {
    const float *w; float *out;
    int Cout, Cin, dgrad, R32;
    long long total;                          // threads: steps x rows x 2
};

template <int MMA>
__global__ void __launch_bounds__(256) ui_pack_kernel(const UiPackK a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.total) return;
    const int k8 = (int)(i & 1), rows = a.R32 * 32;
    const long long q = i >> 1;
    const int row = (int)(q % rows);
    const int s = (int)(q / rows);
    int ky, kx, kbase;
    if (!a.dgrad) {
        const int ks = s & 1, t = (s >> 1) & 3, p = (s >> 3) & 3, c = s >> 5;
        ky = 3 - (p >> 1) - 2 * (t >> 1);
        kx = 3 - (p & 1) - 2 * (t & 1);
        kbase = c * UI_FCK + ks * 16 + k8 * 8;
    } else {
        const int t = s & 15, c = s >> 4;
        ky = t >> 2;
        kx = t & 3;
        kbase = c * 16 + k8 * 8;
    }
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = kbase + j;
        const int co = a.dgrad ? k : row, ci = a.dgrad ? row : k;
        float v = 0.f;
        if (co < a.Cout && ci < a.Cin) v = tnr_fold_tap(a.w + ((size_t)co * a.Cin + ci) * 9, 4, ky, kx);
        if (j < 4) lo[j] = v; else hi[j - 4] = v;
    }
    constexpr int UNIT = ui_unit(MMA);
    float *dst = a.out + ((size_t)s * a.R32 + (row >> 5)) * UNIT;
    const int r = row & 31;
    if constexpr (MMA == TNR_MMA_F32) {
        *reinterpret_cast<f32x4 *>(dst + ((k8 * 2 + 0) * 32 + r) * 4) = lo;
        *reinterpret_cast<f32x4 *>(dst + ((k8 * 2 + 1) * 32 + r) * 4) = hi;
    } else {
        __bf16 *db = reinterpret_cast<__bf16 *>(dst);
#pragma unroll
        for (int p = 0; p < mp_planes(MMA); ++p) {
            tnr_bf16x4 pl, ph;
            f32x4 rl, rh;
            tnr_pk_level(lo, pl, rl);
            tnr_pk_level(hi, ph, rh);
            __bf16 *o = db + ((p * 2 + k8) * 32 + r) * 8;
            *reinterpret_cast<tnr_bf16x4 *>(o) = pl;
            *reinterpret_cast<tnr_bf16x4 *>(o + 4) = ph;
            lo = rl;
            hi = rh;
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward
struct UiFwdK {
    const float *x; int x_ct, x_co, N, H, W, Cin;    // LR input view
    const float *wp; int R32;                        // the forward image, its 32-row blocks
    float *y; int y_ct, y_co, Cout;                  // HR output view [N, 2H, 2W, Cout]
    const float *bias;
    int tiles_x, tiles_y;
};

template <int MMA> constexpr int ui_fwd_lds() {
    return MMA == TNR_MMA_F32 ? UI_FPIX * UI_FPSF * 4 : UI_FPIX * UI_FPSB * 2 * mp_planes(MMA);
}

template <int NT, int MMA>
__global__ void __launch_bounds__(256) ui_fwd_kernel(const UiFwdK a) {
    constexpr int PLANE = UI_FPIX * UI_FPSB;
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
    const int rb0 = blockIdx.y * NT;
    const float *wp = a.wp + (size_t)rb0 * ui_unit(MMA);
    const bool wave_on = y0 + 2 * wave < a.H;                       // wave-uniform: a wave below the image neither streams nor multiplies
    const int chunks = (a.Cin + UI_FCK - 1) / UI_FCK, steps = chunks * 32;

    MpFrag<NT, MMA> cur, nxt;
    ui_load_w<NT, MMA>(cur, wp, 0, a.R32, li, half);
    nxt = cur;

    const int ly = 2 * wave + (li >> 4), lx = li & 15;              // mma_pixel.h: the lane's pixel of the tile
    const int abase = (ly + 1) * UI_FW + lx + 1;                    // the lane's LR pixel in the staged tile
    f32x16 acc[4][NT];                                              // the four output parities of the lane's pixel
#pragma unroll
    for (int p = 0; p < 4; ++p) mp_zero<NT>(acc[p]);

#pragma unroll 1
    for (int c = 0; c < chunks; ++c) {
        if (c) __syncthreads();                                     // the previous chunk is read
        // ---- 32 channels of the LR tile and its halo; zeros outside the image (= the layer's zero padding seen from the LR domain)
        for (int i = tid; i < UI_FPIX * (UI_FCK / 4); i += 256) {
            const int p = i >> 3, c4 = i & 7;
            const int r = p / UI_FW, cc = p - r * UI_FW;
            const int Y = y0 - 1 + r, X = x0 - 1 + cc, ch = c * UI_FCK + c4 * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (Y >= 0 && Y < a.H && X >= 0 && X < a.W && ch < a.Cin)
                v = *reinterpret_cast<const f32x4 *>(a.x + (((size_t)n * a.H + Y) * a.W + X) * a.x_ct + a.x_co + ch);
            mp_stage4<MMA>(v, s_f + p * UI_FPSF + c4 * 4, s_b + p * UI_FPSB + c4 * 4, PLANE);
        }
        __syncthreads();
        if (wave_on) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                f32x16 part[NT];                                    // the chunk's 4 taps x 32 channels of this parity, then added to its running sum
                mp_zero<NT>(part);
                // the parity's 4 neighbours x 2 half-chunks as a ROLLED loop: unrolled, the scheduler hoists every step's fragment and LDS loads
                // to the top and the body spills (3 KB of scratch per lane at NT = 2); rolled, one step's operands are live at a time
#pragma unroll 1
                for (int u = 0; u < 8; ++u) {
                    const int t = u >> 1, ks = u & 1;
                    const int pix = abase + ((t >> 1) - 1 + (p >> 1)) * UI_FW + (t & 1) - 1 + (p & 1);
                    const int s = c * 32 + p * 8 + u;
                    if (s + 1 < steps) ui_load_w<NT, MMA>(nxt, wp, s + 1, a.R32, li, half);
                    f32x16 st[NT];                                  // one step = one accumulation chain on the matrix core; the sums above it in VALU fp32
                    mp_zero<NT>(st);
                    mp_step<NT, MMA>(st, cur, s_f + pix * UI_FPSF + ks * 16, s_b + pix * UI_FPSB + ks * 16, PLANE, half);
                    mp_add<NT>(part, st);
                    cur = nxt;
                }
                mp_add<NT>(acc[p], part);
            }
        }
    }
    // ---- pixel (2 (y0 + ly) + a, 2 (x0 + lx) + b) of every parity
    if (wave_on && y0 + ly < a.H && x0 + lx < a.W) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float *yp = a.y + (((size_t)n * 2 * a.H + 2 * (y0 + ly) + (p >> 1)) * 2 * a.W + 2 * (x0 + lx) + (p & 1)) * a.y_ct + a.y_co;
#pragma unroll
            for (int nn = 0; nn < NT; ++nn)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int co = (rb0 + nn) * 32 + q * 8 + half * 4;
                    if (co >= a.Cout) continue;
                    f32x4 v = {acc[p][nn][4 * q], acc[p][nn][4 * q + 1], acc[p][nn][4 * q + 2], acc[p][nn][4 * q + 3]};
                    if (a.bias != nullptr) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += a.bias[co + e];
                    }
                    *reinterpret_cast<f32x4 *>(yp + co) = v;
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ data gradient
struct UiDgradK {
    const float *g; int g_ct, g_co, N, H, W, Cout;   // HR gradient view [N, 2H, 2W, Cout]; H, W: the LR extent
    const float *wp; int R32;                        // the data-gradient image, its 32-row blocks (rows = Cin)
    float *gx; int gx_ct, gx_co, Cin;
    int tiles_x, tiles_y;
};

template <int MMA> constexpr int ui_dgrad_lds() {
    return MMA == TNR_MMA_F32 ? UI_GPIX * UI_GPSF * 4 : UI_GPIX * UI_GPSB * 2 * mp_planes(MMA);
}

template <int NT, int MMA>
__global__ void __launch_bounds__(256) ui_dgrad_kernel(const UiDgradK a) {
    constexpr int PLANE = UI_GPIX * UI_GPSB;
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
    const int Hh = 2 * a.H, Wh = 2 * a.W;
    const int rb0 = blockIdx.y * NT;
    const float *wp = a.wp + (size_t)rb0 * ui_unit(MMA);
    const bool wave_on = y0 + 2 * wave < a.H;
    const int chunks = (a.Cout + 15) / 16, steps = chunks * 16;

    MpFrag<NT, MMA> cur, nxt;
    ui_load_w<NT, MMA>(cur, wp, 0, a.R32, li, half);
    nxt = cur;

    const int ly = 2 * wave + (li >> 4), lx = li & 15;              // mma_pixel.h: the lane's pixel of the tile
    const int abase = 2 * ly * UI_GW + 2 * lx;                      // the lane's LR pixel: its 4 x 4 window starts at (2 ly, 2 lx)
    f32x16 acc[NT];
    mp_zero<NT>(acc);
#pragma unroll 1
    for (int c = 0; c < chunks; ++c) {
        if (c) __syncthreads();
        // ---- channels 16 c .. + 15 of the window: HR rows 2 y0 - 1 .. 2 (y0 + 8), zeros outside the HR image
        for (int i = tid; i < UI_GPIX * 4; i += 256) {
            const int p = i >> 2, c4 = i & 3;
            const int r = p / UI_GW, cc = p - r * UI_GW;
            const int Y = 2 * y0 - 1 + r, X = 2 * x0 - 1 + cc, ch = c * 16 + c4 * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (Y >= 0 && Y < Hh && X >= 0 && X < Wh && ch < a.Cout)
                v = *reinterpret_cast<const f32x4 *>(a.g + (((size_t)n * Hh + Y) * Wh + X) * a.g_ct + a.g_co + ch);
            mp_stage4<MMA>(v, s_f + p * UI_GPSF + c4 * 4, s_b + p * UI_GPSB + c4 * 4, PLANE);
        }
        __syncthreads();
        if (wave_on) {
            f32x16 part[NT];                                        // the chunk's 16 taps x 16 channels, then added to the running sum
            mp_zero<NT>(part);
#pragma unroll 1
            for (int t = 0; t < 16; ++t) {                          // (rolled for the same reason as the forward's tap loop)
                const int s = c * 16 + t, pix = abase + (t >> 2) * UI_GW + (t & 3);
                if (s + 1 < steps) ui_load_w<NT, MMA>(nxt, wp, s + 1, a.R32, li, half);
                f32x16 st[NT];                                      // (as in the forward: one step per matrix-core accumulation chain)
                mp_zero<NT>(st);
                mp_step<NT, MMA>(st, cur, s_f + pix * UI_GPSF, s_b + pix * UI_GPSB, PLANE, half);
                mp_add<NT>(part, st);
                cur = nxt;
            }
            mp_add<NT>(acc, part);
        }
    }
    if (wave_on && y0 + ly < a.H && x0 + lx < a.W) {
        float *gp = a.gx + (((size_t)n * a.H + y0 + ly) * a.W + x0 + lx) * a.gx_ct + a.gx_co;
#pragma unroll
        for (int nn = 0; nn < NT; ++nn)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ci = (rb0 + nn) * 32 + q * 8 + half * 4;
                if (ci >= a.Cin) continue;
                *reinterpret_cast<f32x4 *>(gp + ci) = f32x4{acc[nn][4 * q], acc[nn][4 * q + 1], acc[nn][4 * q + 2], acc[nn][4 * q + 3]};
            }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct UiWgradK {
    const float *x; int x_ct, x_co, N, H, W, Cin;
    const float *g; int g_ct, g_co, Cout;
    float *ws;                                // [slab][16][CinP][CoutP]
    int CinP, CoutP, nbi, nbo;
    int tiles_x, tiles_y, tiles, slabs;
};

template <int NI, int NO> constexpr int ui_wgrad_lds() {
    constexpr int stage = MP_TPIX * (NI + NO) * 32 * 4, reduce = 4 * NI * 32 * NO * 32 * 4;
    return stage > reduce ? stage : reduce;
}

// Workgroup (folded tap, block of 32 NI reduced-side channels, block of 32 NO produced channels, slab): dF[tap] of its block over the tiles
// slab, slab + slabs, ...  Per tile it stages the tap's two operands -- x of the tile shifted by the tap's LR offset (zeros outside the image)
// and g at the tap's parity of the tile's 2 x 2 blocks -- and every wave multiplies its two tile rows (32 pixels = 16 steps of
// v_mfma_f32_32x32x2_f32, fp32 in every arithmetic mode) into the block's accumulators, kept in registers over the workgroup's tiles.  The four
// waves' sums are then added in wave order through LDS: the order in which every partial sum grows is fixed.
template <int NI, int NO>
__global__ void __launch_bounds__(256) ui_wgrad_kernel(const UiWgradK a) {
    constexpr int CI = NI * 32, CO = NO * 32, TPIX = MP_TPIX;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *s_x = reinterpret_cast<float *>(smem);
    float *s_g = s_x + TPIX * CI;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, half = lane >> 5;
    int bid = blockIdx.x;
    const int co0 = (bid % a.nbo) * CO;
    bid /= a.nbo;
    const int ci0 = (bid % a.nbi) * CI;
    const int tap = bid / a.nbi, ky = tap >> 2, kx = tap & 3;
    // output 2i - 1 + k = 2I + a: parity a = (k + 1) mod 2, LR source i = I + d
    const int pa = (ky + 1) & 1, pb = (kx + 1) & 1;
    const int dy = ky == 0 ? 1 : (ky == 3 ? -1 : 0), dx = kx == 0 ? 1 : (kx == 3 ? -1 : 0);
    const int Hh = 2 * a.H, Wh = 2 * a.W;

    f32x16 acc[NI][NO];
#pragma unroll
    for (int ib = 0; ib < NI; ++ib) mp_zero<NO>(acc[ib]);

    for (int tile = blockIdx.y; tile < a.tiles; tile += a.slabs) {
        int q = tile;
        const int tx = q % a.tiles_x;
        q /= a.tiles_x;
        const int ty = q % a.tiles_y;
        const int n = q / a.tiles_y;
        const int y0 = ty * MP_TH, x0 = tx * MP_TW;
        __syncthreads();
        for (int i = tid; i < TPIX * (CI / 4); i += 256) {
            const int p = i / (CI / 4), c4 = i - p * (CI / 4);
            const int I = y0 + p / MP_TW, J = x0 + p % MP_TW, Y = I + dy, X = J + dx, ch = ci0 + c4 * 4;
            f32x4 xv = {0.f, 0.f, 0.f, 0.f};
            if (I < a.H && J < a.W && Y >= 0 && Y < a.H && X >= 0 && X < a.W && ch < a.Cin)
                xv = *reinterpret_cast<const f32x4 *>(a.x + (((size_t)n * a.H + Y) * a.W + X) * a.x_ct + a.x_co + ch);
            *reinterpret_cast<f32x4 *>(s_x + p * CI + c4 * 4) = xv;
        }
        for (int i = tid; i < TPIX * (CO / 4); i += 256) {
            const int p = i / (CO / 4), c4 = i - p * (CO / 4);
            const int I = y0 + p / MP_TW, J = x0 + p % MP_TW, ch = co0 + c4 * 4;
            f32x4 gv = {0.f, 0.f, 0.f, 0.f};
            if (I < a.H && J < a.W && ch < a.Cout)
                gv = *reinterpret_cast<const f32x4 *>(a.g + (((size_t)n * Hh + 2 * I + pa) * Wh + 2 * J + pb) * a.g_ct + a.g_co + ch);
            *reinterpret_cast<f32x4 *>(s_g + p * CO + c4 * 4) = gv;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < 16; ++kk) {
            const int pix = wave * 32 + 2 * kk + half;
            float av[NI], bv[NO];
#pragma unroll
            for (int b = 0; b < NI; ++b) av[b] = s_x[pix * CI + b * 32 + li];
#pragma unroll
            for (int b = 0; b < NO; ++b) bv[b] = s_g[pix * CO + b * 32 + li];
#pragma unroll
            for (int ib = 0; ib < NI; ++ib)
#pragma unroll
                for (int jb = 0; jb < NO; ++jb) acc[ib][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ib], bv[jb], acc[ib][jb], 0, 0, 0);
        }
    }
    // ---- the four waves' sums through LDS ([wave][ci][co], inside the staging area), added in wave order
    __syncthreads();
    float *s_r = reinterpret_cast<float *>(smem);
#pragma unroll
    for (int ib = 0; ib < NI; ++ib)
#pragma unroll
        for (int jb = 0; jb < NO; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ib * 32 + (r >> 2) * 8 + half * 4 + (r & 3);
                s_r[(wave * CI + ci) * CO + jb * 32 + li] = acc[ib][jb][r];
            }
    __syncthreads();
    float *slab = a.ws + ((size_t)blockIdx.y * 16 + tap) * a.CinP * a.CoutP;
    for (int i = tid; i < CI * CO; i += 256) {
        const int ci = i / CO, co = i - ci * CO;
        slab[(size_t)(ci0 + ci) * a.CoutP + co0 + co] = ((s_r[i] + s_r[CI * CO + i]) + s_r[2 * CI * CO + i]) + s_r[3 * CI * CO + i];
    }
}

struct UiUnfoldK {
    const float *ws; int slabs, Cin, Cout, CinP, CoutP;
    float *dw; float alpha, beta;
};

// one thread per (3x3 tap, ci, co): per folded tap the slabs in index order, then the four folded taps (2 - t, 3 - t per axis) in tnr_upfold_grad's order
__global__ void __launch_bounds__(256) ui_wgrad_unfold_kernel(const UiUnfoldK a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, cc = a.Cin * a.Cout;
    if (i >= 9 * cc) return;
    const int t = i / cc, r = i - t * cc, ci = r / a.Cout, co = r - ci * a.Cout;
    const int ty = t / 3, tx = t - ty * 3;
    const size_t tap_stride = (size_t)a.CinP * a.CoutP;
    auto tap = [&](int ky, int kx) {
        const float *src = a.ws + (size_t)(ky * 4 + kx) * tap_stride + (size_t)ci * a.CoutP + co;
        float p = 0.f;
        for (int sl = 0; sl < a.slabs; ++sl) p += src[(size_t)sl * 16 * tap_stride];
        return p;
    };
    const int ky = 2 - ty, kx = 2 - tx;
    const float sum = (tap(ky, kx) + tap(ky, kx + 1)) + (tap(ky + 1, kx) + tap(ky + 1, kx + 1));
    const size_t o = ((size_t)co * a.Cin + ci) * 9 + t;
    a.dw[o] = (a.beta != 0.f ? a.beta * a.dw[o] : 0.f) + a.alpha * sum;
}

// ------------------------------------------------------------------------------------------------ host side
// the built channel classes: multiples of 4 (16-byte channel groups), 4 <= Cout <= 512, 4 <= Cin <= 2048 -- one test for launchers and size queries
bool ui_channels_ok(int Cin, int Cout) {
    return Cout >= 4 && Cout <= UI_MAX_COUT && Cout % 4 == 0 && Cin >= 4 && Cin <= UI_MAX_CIN && Cin % 4 == 0;
}

int ui_geometry(const char *who, int N, int H, int W, int Cin, int Cout, int *tiles_x, int *tiles_y, int64_t *tiles) {
    const int rc = mp_geometry(who, N, H, W, 2, tiles_x, tiles_y, tiles);
    if (rc != TNR_OK) return rc;
    TNR_REQUIRE(ui_channels_ok(Cin, Cout),
                "%s: built for 4 <= Cout <= %d and 4 <= Cin <= %d, both multiples of 4 (got %d -> %d)", who, UI_MAX_COUT, UI_MAX_CIN, Cin, Cout);
    return TNR_OK;
}

int ui_steps(int Cout, int Cin, int dgrad) { return dgrad ? tnr_cdiv(Cout, 16) * 16 : tnr_cdiv(Cin, UI_FCK) * 32; }
int ui_rows32(int Cout, int Cin, int dgrad) { return tnr_cdiv(dgrad ? Cin : Cout, 32); }

// 64-channel row blocks reuse every staged pixel twice as often; 32-channel blocks put twice as many workgroups on the weight stream.  The
// first wins as soon as the 64-channel grid alone covers the CUs; below that the launch is weight-bound (few tiles, wide channels).
int ui_row_blocks(int R32, int64_t tiles, int cus) { return (R32 % 2 == 0 && tiles * (R32 / 2) >= cus) ? 2 : 1; }

// weight gradient: 32- or 64-channel blocks per side, and enough tile slabs that the 16-tap grid reaches ~1024 workgroups
int ui_wgrad_blocks(int C) { return tnr_cdiv(C, 32) % 2 == 0 ? 2 : 1; }
int ui_wgrad_slabs(int64_t tiles, int Cin, int Cout) {
    const int nb = (tnr_cdiv(Cin, 32) / ui_wgrad_blocks(Cin)) * (tnr_cdiv(Cout, 32) / ui_wgrad_blocks(Cout));
    int64_t s = 1024 / (16 * (int64_t)nb);
    if (s < 1) s = 1;
    if (s > 32) s = 32;
    return (int)(s < tiles ? s : tiles);
}

}  // namespace

extern "C" int64_t tnr_upconv_i2i_pack_floats(int32_t Cout, int32_t Cin, int32_t dgrad, int32_t mma) {
    if (!ui_channels_ok(Cin, Cout) || !mp_mma_ok(mma)) return 0;
    return (int64_t)ui_steps(Cout, Cin, dgrad) * ui_rows32(Cout, Cin, dgrad) * ui_unit(mma);
}

extern "C" int tnr_upconv_i2i_pack(const float *w, int32_t Cout, int32_t Cin, int32_t dgrad, int32_t mma, float *out, int64_t out_floats,
                                   void *stream) {
    TNR_REQUIRE(w && out && (reinterpret_cast<uintptr_t>(out) & 15) == 0, "upconv_i2i_pack: bad pointers");
    TNR_REQUIRE(ui_channels_ok(Cin, Cout),
                "upconv_i2i_pack: built for 4 <= Cout <= %d and 4 <= Cin <= %d, both multiples of 4 (got %d -> %d)", UI_MAX_COUT, UI_MAX_CIN, Cin, Cout);
    TNR_REQUIRE(mp_mma_ok(mma), "upconv_i2i_pack: bad mma %d", mma);
    TNR_REQUIRE(tnr_upconv_i2i_pack_floats(Cout, Cin, dgrad, mma) <= out_floats, "upconv_i2i_pack: image buffer too small");
    UiPackK k;
    k.w = w; k.out = out; k.Cout = Cout; k.Cin = Cin; k.dgrad = dgrad != 0; k.R32 = ui_rows32(Cout, Cin, dgrad);
    k.total = (long long)ui_steps(Cout, Cin, dgrad) * k.R32 * 32 * 2;
    const dim3 grid((unsigned)tnr_cdiv64(k.total, 256));
    hipStream_t st = (hipStream_t)stream;
    if (mma == TNR_MMA_F32) hipLaunchKernelGGL(ui_pack_kernel<TNR_MMA_F32>, grid, dim3(256), 0, st, k);
    else if (mma == TNR_MMA_BF16) hipLaunchKernelGGL(ui_pack_kernel<TNR_MMA_BF16>, grid, dim3(256), 0, st, k);
    else hipLaunchKernelGGL(ui_pack_kernel<TNR_MMA_BF16X3>, grid, dim3(256), 0, st, k);
    return tnr_check_launch("upconv_i2i_pack");
}

extern "C" int tnr_upconv_i2i_fwd(tnr_view x, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *wp, tnr_view y, int32_t Cout,
                                  const float *bias, int32_t mma, void *stream) {
    UiFwdK k;
    int64_t tiles;
    int rc = ui_geometry("upconv_i2i_fwd", N, H, W, Cin, Cout, &k.tiles_x, &k.tiles_y, &tiles);
    if (rc != TNR_OK) return rc;
    TNR_REQUIRE(wp && mp_view_ok(x, Cin) && mp_view_ok(y, Cout), "upconv_i2i_fwd: bad views");
    TNR_REQUIRE(mp_mma_ok(mma), "upconv_i2i_fwd: bad mma %d", mma);
    k.x = x.ptr; k.x_ct = x.ctot; k.x_co = x.coff; k.N = N; k.H = H; k.W = W; k.Cin = Cin;
    k.wp = wp; k.R32 = ui_rows32(Cout, Cin, 0);
    k.y = y.ptr; k.y_ct = y.ctot; k.y_co = y.coff; k.Cout = Cout; k.bias = bias;
    static int cus = 0;
#define UI_FWD(NT, MMA) tnr_kernel_lds(ui_fwd_kernel<NT, MMA>, ui_fwd_lds<MMA>())
    const std::initializer_list<tnr_kernel_lds> table = {MP_MODES(UI_FWD, 1), MP_MODES(UI_FWD, 2)};
#undef UI_FWD
    rc = tnr_kernel_setup(&cus, "upconv_i2i_fwd", table);           // (the row-block choice reads the CU count)
    if (rc != TNR_OK) return rc;
    const int nt = ui_row_blocks(k.R32, tiles, cus);
    return mp_launch_entry("upconv_i2i_fwd", table, (nt == 2 ? 3 : 0) + mma, dim3((unsigned)tiles, (unsigned)(k.R32 / nt)), &k, stream);
}

extern "C" int tnr_upconv_i2i_dgrad(tnr_view g, int32_t N, int32_t H, int32_t W, int32_t Cout, const float *wp, tnr_view gx, int32_t Cin,
                                    int32_t mma, void *stream) {
    UiDgradK k;
    int64_t tiles;
    int rc = ui_geometry("upconv_i2i_dgrad", N, H, W, Cin, Cout, &k.tiles_x, &k.tiles_y, &tiles);
    if (rc != TNR_OK) return rc;
    TNR_REQUIRE(wp && mp_view_ok(g, Cout) && mp_view_ok(gx, Cin), "upconv_i2i_dgrad: bad views");
    TNR_REQUIRE(mp_mma_ok(mma), "upconv_i2i_dgrad: bad mma %d", mma);
    k.g = g.ptr; k.g_ct = g.ctot; k.g_co = g.coff; k.N = N; k.H = H; k.W = W; k.Cout = Cout;
    k.wp = wp; k.R32 = ui_rows32(Cout, Cin, 1);
    k.gx = gx.ptr; k.gx_ct = gx.ctot; k.gx_co = gx.coff; k.Cin = Cin;
    static int cus = 0;
#define UI_DG(NT, MMA) tnr_kernel_lds(ui_dgrad_kernel<NT, MMA>, ui_dgrad_lds<MMA>())
    const std::initializer_list<tnr_kernel_lds> table = {MP_MODES(UI_DG, 1), MP_MODES(UI_DG, 2)};
#undef UI_DG
    rc = tnr_kernel_setup(&cus, "upconv_i2i_dgrad", table);
    if (rc != TNR_OK) return rc;
    const int nt = ui_row_blocks(k.R32, tiles, cus);
    return mp_launch_entry("upconv_i2i_dgrad", table, (nt == 2 ? 3 : 0) + mma, dim3((unsigned)tiles, (unsigned)(k.R32 / nt)), &k, stream);
}

extern "C" int64_t tnr_upconv_i2i_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || !ui_channels_ok(Cin, Cout)) return 0;
    return (int64_t)ui_wgrad_slabs(mp_tiles(N, H, W), Cin, Cout) * 16 * tnr_round_up(Cin, 32) * tnr_round_up(Cout, 32) * (int64_t)sizeof(float);
}

extern "C" int tnr_upconv_i2i_wgrad(tnr_view x, tnr_view g, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, float *dw, float alpha,
                                    float beta, float *ws, int64_t ws_bytes, void *stream) {
    UiWgradK k;
    int64_t tiles;
    int rc = ui_geometry("upconv_i2i_wgrad", N, H, W, Cin, Cout, &k.tiles_x, &k.tiles_y, &tiles);
    if (rc != TNR_OK) return rc;
    TNR_REQUIRE(dw && ws && mp_view_ok(x, Cin) && mp_view_ok(g, Cout), "upconv_i2i_wgrad: bad arguments");
    TNR_REQUIRE(tnr_upconv_i2i_wgrad_workspace_bytes(N, H, W, Cin, Cout) <= ws_bytes, "upconv_i2i_wgrad: workspace too small");
    k.x = x.ptr; k.x_ct = x.ctot; k.x_co = x.coff; k.N = N; k.H = H; k.W = W; k.Cin = Cin;
    k.g = g.ptr; k.g_ct = g.ctot; k.g_co = g.coff; k.Cout = Cout;
    k.ws = ws; k.CinP = tnr_round_up(Cin, 32); k.CoutP = tnr_round_up(Cout, 32);
    const int ni = ui_wgrad_blocks(Cin), no = ui_wgrad_blocks(Cout);
    k.nbi = k.CinP / (32 * ni); k.nbo = k.CoutP / (32 * no);
    k.tiles = (int)tiles; k.slabs = ui_wgrad_slabs(tiles, Cin, Cout);
    static int cus = 0;
#define UI_WG(NI, NO) tnr_kernel_lds(ui_wgrad_kernel<NI, NO>, ui_wgrad_lds<NI, NO>())
    rc = mp_launch(&cus, "upconv_i2i_wgrad", {UI_WG(1, 1), UI_WG(1, 2), UI_WG(2, 1), UI_WG(2, 2)}, (ni - 1) * 2 + (no - 1),
                   dim3((unsigned)(16 * k.nbi * k.nbo), (unsigned)k.slabs), &k, stream);
#undef UI_WG
    if (rc != TNR_OK) return rc;
    UiUnfoldK u;
    u.ws = ws; u.slabs = k.slabs; u.Cin = Cin; u.Cout = Cout; u.CinP = k.CinP; u.CoutP = k.CoutP; u.dw = dw; u.alpha = alpha; u.beta = beta;
    hipLaunchKernelGGL(ui_wgrad_unfold_kernel, dim3(tnr_cdiv(9 * Cin * Cout, 256)), dim3(256), 0, (hipStream_t)stream, u);
    return tnr_check_launch("upconv_i2i_wgrad_unfold");
}
