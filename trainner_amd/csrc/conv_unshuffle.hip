// The generator's first layer behind a pixel unshuffle (use_unshuffle; block.SpaceToDepth 'pt' = F.pixel_unshuffle(x, s) in front of
// RRDBNet's 3x3 pad-1 fea conv, [nf, 3 s^2, 3, 3]) as ONE convolution over the RGB image itself: window (3s) x (3s), stride s,
// padding s, read from the NHWC4 buffer the engine already keeps the image in.  No unshuffled tensor is ever stored.
//   forward : y[n, Y, X, co] = bias[co] + sum_{wy, wx, c} Wwin[co][wy][wx][c] * img[n, (Y - 1) s + wy, (X - 1) s + wx, c]
//             Wwin[co][dy s + i][dx s + j][c] = W[co][c s^2 + i s + j][dy][dx]   (zeros outside the image and for the pad channel c = 3)
//   wgrad   : dWwin[wy][wx][c][co] = sum_{n, Y, X} img[n, (Y - 1) s + wy, (X - 1) s + wx, c] * g[n, Y, X, co], db = sum g
// Both on the matrix cores with the window folded into the reduction (forward: K = (3s)^2 * 4 = 144 | 576) or into the rows
// (weight gradient: M = 27 s^2 = 108 | 432, reduced over pixels).  A workgroup owns an 8 x 16 tile of output pixels (the forward on
// mma_pixel.h's tile convention: the lane owns a pixel; its step reads the weights from LDS too and stays written here) and stages that tile's image halo, ((T + 2) s)^2 pixels of 16 bytes, ONCE: a window row of 3s pixels is contiguous there, so a K step of the bf16
// matrix core (16 values = 4 pixels; a lane half takes 2 pixels = 8 values) is one 16-byte LDS read per plane.
#include "mma_pixel.h"

namespace {

constexpr int UW_GRID = 256;                  // weight gradient: persistent workgroups (= partial slabs), one per CU

template <int S> struct UGeom {
    static constexpr int WS = 3 * S;                          // window side in image pixels
    static constexpr int K = WS * WS * 4;                     // forward reduction: (wy, wx, 4 channels)
    static constexpr int KSTEPS = K / 16;                     // 9 | 36
    static constexpr int TH = (MP_TH + 2) * S, TW = (MP_TW + 2) * S, NPIX = TH * TW;      // staged image halo
    static constexpr int M = WS * WS * 3;                     // weight-gradient rows: (wy, wx, 3 channels); row M = the bias sum
    static constexpr int NMT = (M + 1 + 31) / 32;             // 32-row blocks: 4 | 14
};

// ------------------------------------------------------------------------------------------------ forward
constexpr int UF_CHUNK = 3;                   // K steps of weights staged per LDS fill (48 of K: 9 and 36 are multiples)

struct UnshufK {
    const float *x; int N, H, W;              // NHWC4 image
    const float *wp;                          // TNR_PACK_UNSHUFFLE_FWD: [K / 8][nf][8]
    float *y; int y_ct, y_co, Ho, Wo;
    const float *bias;
    int tiles_x, tiles_y;
};

template <int S, int NT, int MMA> constexpr int unshuffle_fwd_lds() {
    constexpr int np = mp_planes(MMA);
    constexpr int img = MMA == TNR_MMA_F32 ? UGeom<S>::NPIX * 16 : UGeom<S>::NPIX * 8 * np;
    constexpr int units = MMA == TNR_MMA_F32 ? UF_CHUNK * 2 * 2 : UF_CHUNK * np * 2;      // 16-byte units per output channel
    return img + units * NT * 32 * 16;
}

// LDS: the image halo -- TNR_MMA_F32: [pixel] float4; bf16 forms: [plane][pixel] of 4 bf16 (TNR_MMA_BF16X3: the exact hi / mid / lo
// split, made once per pixel where the halo is staged) -- and one chunk of weights as 16-byte units [K step][plane][lane half][cout]
// (TNR_MMA_F32: [8-value group][lane half][cout]): consecutive lanes read consecutive units.  The packed weights (K x nf floats:
// 37 KB at s = 2, 147 KB at s = 4, more than fits beside the halo) stream from L2 in chunks of 48 K values; the next chunk's loads
// are in flight while the matrix core works on this one.
template <int S, int NT, int MMA>
__global__ void __launch_bounds__(256) conv_unshuffle_kernel(const UnshufK a) {
    using G = UGeom<S>;
    constexpr int NF = NT * 32;
    constexpr bool F32 = MMA == TNR_MMA_F32;
    constexpr int NP = MMA == TNR_MMA_BF16X3 ? 3 : 1;
    constexpr int IMG_BYTES = F32 ? G::NPIX * 16 : G::NPIX * 8 * NP;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f32x4 *s_imgf = reinterpret_cast<f32x4 *>(smem);
    tnr_bf16x4 *s_imgb = reinterpret_cast<tnr_bf16x4 *>(smem);
    f32x4 *s_w = reinterpret_cast<f32x4 *>(smem + IMG_BYTES);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, half = lane >> 5;
    int bid = blockIdx.x;
    const int tx = bid % a.tiles_x;
    bid /= a.tiles_x;
    const int ty = bid % a.tiles_y;
    const int n = bid / a.tiles_y;
    const int y0 = ty * MP_TH, x0 = tx * MP_TW;

    // ---- weights: item = (8-value group gi of the chunk, cout j) = 2 float4
    constexpr int ITEMS = UF_CHUNK * 2 * NF, R = (ITEMS + 255) / 256;
    f32x4 wreg[R][2];
    auto load_w = [&](int chunk) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int it = tid + r * 256;
            if (it < ITEMS) {
                const float *src = a.wp + ((size_t)chunk * ITEMS + it) * 8;
                wreg[r][0] = *reinterpret_cast<const f32x4 *>(src);
                wreg[r][1] = *reinterpret_cast<const f32x4 *>(src + 4);
            }
        }
    };
    auto store_w = [&]() {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int it = tid + r * 256;
            if (it < ITEMS) {
                const int gi = it / NF, j = it - gi * NF;
                if constexpr (F32) {
                    s_w[(gi * 2 + 0) * NF + j] = wreg[r][0];
                    s_w[(gi * 2 + 1) * NF + j] = wreg[r][1];
                } else {
                    const int ks = gi >> 1, h = gi & 1;
                    tnr_bf16x8 pl[3];
                    if constexpr (NP == 3) tnr_split_bf16x3(wreg[r][0], wreg[r][1], pl);
                    else pl[0] = tnr_pack_bf16(wreg[r][0], wreg[r][1]);
#pragma unroll
                    for (int p = 0; p < NP; ++p) *reinterpret_cast<tnr_bf16x8 *>(s_w + ((ks * NP + p) * 2 + h) * NF + j) = pl[p];
                }
            }
        }
    };
    load_w(0);

    // ---- the image halo, once: rows (y0 - 1) s .. (y0 + MP_TH + 1) s - 1, zeros outside the image (= the layer's zero padding)
    {
        const int iy0 = (y0 - 1) * S, ix0 = (x0 - 1) * S;
        for (int p = tid; p < G::NPIX; p += 256) {
            const int r = p / G::TW, c = p - r * G::TW;
            const int Y = iy0 + r, X = ix0 + c;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (Y >= 0 && Y < a.H && X >= 0 && X < a.W) v = *reinterpret_cast<const f32x4 *>(a.x + (((size_t)n * a.H + Y) * a.W + X) * 4);
            if constexpr (F32) {
                s_imgf[p] = v;
            } else {
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) {
                    tnr_bf16x4 pk;
                    f32x4 res;
                    tnr_pk_level(v, pk, res);
                    s_imgb[pl * G::NPIX + p] = pk;
                    v = res;
                }
            }
        }
    }

    // this lane's output pixel (the B operand's column) and the first pixel of its window in the halo
    const int ly = 2 * wave + (li >> 4), lx = li & 15;
    const int abase = ly * S * G::TW + lx * S;
    f32x16 acc[NT];
#pragma unroll
    for (int nn = 0; nn < NT; ++nn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nn][r] = 0.f;

    constexpr int NCH = G::KSTEPS / UF_CHUNK;
#pragma unroll 1
    for (int chunk = 0; chunk < NCH; ++chunk) {
        __syncthreads();                      // (first trip: nothing to wait for) the previous chunk's fragments are read
        store_w();
        __syncthreads();                      // (first trip: the halo too)
        if (chunk + 1 < NCH) load_w(chunk + 1);
        // a chunk's 48 products grow in an accumulator of their own that is then added to the running sum: one fp32 chain over all of
        // K = 576 drifts 2-3 x further from the fp64 sum than the blocked sums of a CPU convolution
        f32x16 part[NT];
#pragma unroll
        for (int nn = 0; nn < NT; ++nn)
#pragma unroll
            for (int r = 0; r < 16; ++r) part[nn][r] = 0.f;
        if constexpr (F32) {
#pragma unroll
            for (int gi = 0; gi < UF_CHUNK * 2; ++gi) {
                const int p = (chunk * UF_CHUNK * 2 + gi) * 2 + half;          // window pixel of this lane half
                const int wy = p / G::WS, wx = p - wy * G::WS;
                const f32x4 av = s_imgf[abase + wy * G::TW + wx];
                f32x4 bv[NT];
#pragma unroll
                for (int nn = 0; nn < NT; ++nn) bv[nn] = s_w[(gi * 2 + half) * NF + nn * 32 + li];
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int nn = 0; nn < NT; ++nn) part[nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[nn][m], av[m], part[nn], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < UF_CHUNK; ++ks) {
                const int p = (chunk * UF_CHUNK + ks) * 4 + 2 * half;           // first of this lane half's two window pixels (same row: 3s is even)
                const int wy = p / G::WS, wx = p - wy * G::WS;
                tnr_bf16x8 ca[NP], cb[NT][NP];
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) ca[pl] = *reinterpret_cast<const tnr_bf16x8 *>(s_imgb + pl * G::NPIX + abase + wy * G::TW + wx);
#pragma unroll
                for (int nn = 0; nn < NT; ++nn)
#pragma unroll
                    for (int pl = 0; pl < NP; ++pl) cb[nn][pl] = *reinterpret_cast<const tnr_bf16x8 *>(s_w + ((ks * NP + pl) * 2 + half) * NF + nn * 32 + li);
                if constexpr (NP == 3) {
                    // the six kept partial products, smallest first (as in conv_body.h)
                    constexpr int TA[6] = {0, 2, 1, 0, 1, 0}, TB[6] = {2, 0, 1, 1, 0, 0};
#pragma unroll
                    for (int q = 0; q < 6; ++q)
#pragma unroll
                        for (int nn = 0; nn < NT; ++nn) part[nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cb[nn][TB[q]], ca[TA[q]], part[nn], 0, 0, 0);
                } else {
#pragma unroll
                    for (int nn = 0; nn < NT; ++nn) part[nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cb[nn][0], ca[0], part[nn], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int nn = 0; nn < NT; ++nn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nn][r] += part[nn][r];
    }

    // ---- store: the weights were the A operand, so a lane holds, for ITS pixel, output channels 8 q + 4 half .. + 3 of every block
    const int oy = y0 + ly, ox = x0 + lx;
    if (oy < a.Ho && ox < a.Wo) {
        float *yp = a.y + (((size_t)n * a.Ho + oy) * a.Wo + ox) * a.y_ct + a.y_co;
#pragma unroll
        for (int nn = 0; nn < NT; ++nn)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co = nn * 32 + q * 8 + half * 4;
                f32x4 v = {acc[nn][4 * q], acc[nn][4 * q + 1], acc[nn][4 * q + 2], acc[nn][4 * q + 3]};
                if (a.bias != nullptr) v += *reinterpret_cast<const f32x4 *>(a.bias + co);
                *reinterpret_cast<f32x4 *>(yp + co) = v;
            }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct UWgradK {
    const float *x; int N, H, W;              // NHWC4 image
    const float *g; int g_ct, g_co, Ho, Wo;   // gradient of the layer's output
    float *ws;                                // [workgroup][M + 1][nf]
    int tiles_x, tiles_y, tiles;
};

template <int S, int NT> constexpr int unshuffle_wgrad_lds() { return UGeom<S>::NPIX * 16 + MP_TH * MP_TW * NT * 32 * 4; }

// D[m][co] += A[m][pixel] B[pixel][co] with v_mfma_f32_32x32x2_f32 (fp32 products, fp32 accumulate): m = (wy (3s) + wx) 3 + c is
// a row of the window, A[m][pixel] = the halo value at the pixel's window origin + (wy, wx), channel c -- one 4-byte LDS read per
// lane and instruction, a lane's offset fixed for the whole launch --, B = the tile of g.  Row M reads the constant 1: the bias
// gradient comes out of the same instructions.  Wave w owns the 32-row blocks w, w + 4, ... for all nf columns and keeps their
// accumulators in registers over ALL tiles of its (persistent) workgroup; tiles are dealt out round-robin, so the order in which
// every partial sum grows is fixed: equal inputs give equal bits.
template <int S, int NT>
__global__ void __launch_bounds__(256) wgrad_unshuffle_kernel(const UWgradK a) {
    using G = UGeom<S>;
    constexpr int NF = NT * 32, MTW = (G::NMT + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *s_img = reinterpret_cast<float *>(smem);
    float *s_g = reinterpret_cast<float *>(smem + G::NPIX * 16);

    const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int aoff[MTW];
    float fill[MTW];
    bool real[MTW];
#pragma unroll
    for (int t = 0; t < MTW; ++t) {
        const int m = (wave + 4 * t) * 32 + li;
        real[t] = m < G::M;
        fill[t] = m == G::M ? 1.f : 0.f;
        const int wp_ = m / 3, c = m - wp_ * 3, wy = wp_ / G::WS, wx = wp_ - wy * G::WS;
        aoff[t] = real[t] ? (wy * G::TW + wx) * 4 + c : 0;
    }
    f32x16 acc[MTW][NT];
#pragma unroll
    for (int t = 0; t < MTW; ++t)
#pragma unroll
        for (int nn = 0; nn < NT; ++nn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][nn][r] = 0.f;

    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        int q = tile;
        const int tx = q % a.tiles_x;
        q /= a.tiles_x;
        const int ty = q % a.tiles_y;
        const int n = q / a.tiles_y;
        const int y0 = ty * MP_TH, x0 = tx * MP_TW;
        __syncthreads();
        const int iy0 = (y0 - 1) * S, ix0 = (x0 - 1) * S;
        for (int p = tid; p < G::NPIX; p += 256) {
            const int r = p / G::TW, c = p - r * G::TW;
            const int Y = iy0 + r, X = ix0 + c;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (Y >= 0 && Y < a.H && X >= 0 && X < a.W) v = *reinterpret_cast<const f32x4 *>(a.x + (((size_t)n * a.H + Y) * a.W + X) * 4);
            *reinterpret_cast<f32x4 *>(s_img + p * 4) = v;
        }
        for (int i = tid; i < MP_TH * MP_TW * (NF / 4); i += 256) {      // g of the tile; zeros beyond the output grid
            const int pix = i / (NF / 4), c4 = i - pix * (NF / 4);
            const int oy = y0 + pix / MP_TW, ox = x0 + pix % MP_TW;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (oy < a.Ho && ox < a.Wo) v = *reinterpret_cast<const f32x4 *>(a.g + (((size_t)n * a.Ho + oy) * a.Wo + ox) * a.g_ct + a.g_co + c4 * 4);
            *reinterpret_cast<f32x4 *>(s_g + pix * NF + c4 * 4) = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int ly = 0; ly < MP_TH; ++ly) {
#pragma unroll
            for (int kx = 0; kx < MP_TW / 2; ++kx) {
                const int lx = 2 * kx + half;                               // this lane half's pixel of the K step
                const int pixoff = (ly * S * G::TW + lx * S) * 4;
                float bv[NT];
#pragma unroll
                for (int nn = 0; nn < NT; ++nn) bv[nn] = s_g[(ly * MP_TW + lx) * NF + nn * 32 + li];
#pragma unroll
                for (int t = 0; t < MTW; ++t) {
                    if (wave + 4 * t < G::NMT) {                           // wave-uniform
                        const float raw = s_img[pixoff + aoff[t]];
                        const float av = real[t] ? raw : fill[t];
#pragma unroll
                        for (int nn = 0; nn < NT; ++nn) acc[t][nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[nn], acc[t][nn], 0, 0, 0);
                    }
                }
            }
        }
    }
    // ---- this workgroup's slab: row m = block * 32 + 8 (r / 4) + 4 half + r % 4, column = nn * 32 + li
    float *slab = a.ws + (size_t)blockIdx.x * (G::M + 1) * NF;
#pragma unroll
    for (int t = 0; t < MTW; ++t) {
        if (wave + 4 * t < G::NMT) {
#pragma unroll
            for (int nn = 0; nn < NT; ++nn)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = (wave + 4 * t) * 32 + (r >> 2) * 8 + half * 4 + (r & 3);
                    if (m <= G::M) slab[(size_t)m * NF + nn * 32 + li] = acc[t][nn][r];
                }
        }
    }
}

struct UWgradRedK {
    const float *ws; int grid, nf, s;
    float *dw; float *db; float alpha, beta;
};

// one thread per (row m, cout): the workgroup slabs in index order (four interleaved chains), then window row -> OIHW:
// (wy, wx, c) = (dy s + i, dx s + j, c) -> dW[co][c s^2 + i s + j][dy][dx]; row M -> db[co]
__global__ void __launch_bounds__(256) wgrad_unshuffle_reduce_kernel(const UWgradRedK a) {
    const int ws_ = 3 * a.s, M = ws_ * ws_ * 3;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (M + 1) * a.nf) return;
    const int m = i / a.nf, co = i - m * a.nf;
    const size_t stride = (size_t)(M + 1) * a.nf;
    const float *src = a.ws + i;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
    int g = 0;
    for (; g + 3 < a.grid; g += 4) {
        p0 += src[(size_t)g * stride];
        p1 += src[(size_t)(g + 1) * stride];
        p2 += src[(size_t)(g + 2) * stride];
        p3 += src[(size_t)(g + 3) * stride];
    }
    for (; g < a.grid; ++g) p0 += src[(size_t)g * stride];
    const float sum = (p0 + p1) + (p2 + p3);
    if (m < M) {
        const int wpix = m / 3, c = m - wpix * 3, wy = wpix / ws_, wx = wpix - wy * ws_;
        const int dy = wy / a.s, iy = wy - dy * a.s, dx = wx / a.s, jx = wx - dx * a.s;
        const size_t o = (((size_t)co * 3 * a.s * a.s + c * a.s * a.s + iy * a.s + jx) * 3 + dy) * 3 + dx;
        a.dw[o] = (a.beta != 0.f ? a.beta * a.dw[o] : 0.f) + a.alpha * sum;
    } else if (a.db != nullptr) {
        a.db[co] = (a.beta != 0.f ? a.beta * a.db[co] : 0.f) + a.alpha * sum;
    }
}

int unshuffle_wgrad_grid(int64_t tiles) { return tiles < UW_GRID ? (int)tiles : UW_GRID; }

int unshuffle_geometry(const char *who, tnr_view x, int N, int H, int W, int nf, int s, int *tiles_x, int *tiles_y, int64_t *tiles) {
    TNR_REQUIRE(x.ptr && N > 0 && H > 0 && W > 0, "%s: bad arguments", who);
    TNR_REQUIRE(x.ctot == 4 && x.coff == 0, "%s: the input is the NHWC4 image (3 channels + pad)", who);
    TNR_REQUIRE(s == 2 || s == 4, "%s: unshuffle scale must be 2 or 4 (got %d)", who, s);
    TNR_REQUIRE(H % s == 0 && W % s == 0, "%s: image %d x %d is no multiple of the unshuffle scale %d", who, H, W, s);
    TNR_REQUIRE(nf == 32 || nf == 64, "%s: nf must be 32 or 64 (got %d)", who, nf);
    return mp_geometry(who, N, H / s, W / s, 1, tiles_x, tiles_y, tiles);
}

}  // namespace

extern "C" int tnr_conv_unshuffle_fwd(tnr_view x, int32_t N, int32_t H, int32_t W, const float *wp, tnr_view y, int32_t nf, int32_t s,
                                      const float *bias, int32_t mma, void *stream) {
    UnshufK k;
    int64_t tiles;
    const int rc = unshuffle_geometry("conv_unshuffle_fwd", x, N, H, W, nf, s, &k.tiles_x, &k.tiles_y, &tiles);
    if (rc != TNR_OK) return rc;
    TNR_REQUIRE(wp && y.ptr && (y.ctot % 4) == 0 && (y.coff % 4) == 0 && y.coff + nf <= y.ctot, "conv_unshuffle_fwd: bad output view");
    TNR_REQUIRE(mp_mma_ok(mma), "conv_unshuffle_fwd: bad mma %d", mma);
    k.x = x.ptr; k.N = N; k.H = H; k.W = W; k.wp = wp;
    k.y = y.ptr; k.y_ct = y.ctot; k.y_co = y.coff; k.Ho = H / s; k.Wo = W / s;
    k.bias = bias;
    static int cus = 0;
#define U_FWD(S, NT, MMA) tnr_kernel_lds(conv_unshuffle_kernel<S, NT, MMA>, unshuffle_fwd_lds<S, NT, MMA>())
    return mp_launch(&cus, "conv_unshuffle_fwd", {MP_MODES(U_FWD, 2, 1), MP_MODES(U_FWD, 2, 2), MP_MODES(U_FWD, 4, 1), MP_MODES(U_FWD, 4, 2)},
                     ((s == 4 ? 2 : 0) + (nf == 64 ? 1 : 0)) * 3 + mma, dim3((unsigned)tiles), &k, stream);
#undef U_FWD
}

extern "C" int64_t tnr_wgrad_unshuffle_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t nf, int32_t s) {
    if (s != 2 && s != 4) return 0;
    const int64_t tiles = mp_tiles(N, H / s, W / s);
    return (int64_t)unshuffle_wgrad_grid(tiles) * (27 * s * s + 1) * nf * (int64_t)sizeof(float);
}

extern "C" int tnr_wgrad_unshuffle(tnr_view g, tnr_view x, int32_t N, int32_t H, int32_t W, int32_t nf, int32_t s, float *dw, float *db,
                                   float alpha, float beta, float *ws, int64_t ws_bytes, void *stream) {
    UWgradK k;
    int64_t tiles;
    int rc = unshuffle_geometry("wgrad_unshuffle", x, N, H, W, nf, s, &k.tiles_x, &k.tiles_y, &tiles);
    if (rc != TNR_OK) return rc;
    TNR_REQUIRE(g.ptr && dw && ws && (g.ctot % 4) == 0 && (g.coff % 4) == 0 && g.coff + nf <= g.ctot, "wgrad_unshuffle: bad arguments");
    TNR_REQUIRE(tnr_wgrad_unshuffle_workspace_bytes(N, H, W, nf, s) <= ws_bytes, "wgrad_unshuffle: workspace too small");
    k.x = x.ptr; k.N = N; k.H = H; k.W = W;
    k.g = g.ptr; k.g_ct = g.ctot; k.g_co = g.coff; k.Ho = H / s; k.Wo = W / s;
    k.ws = ws; k.tiles = (int)tiles;
    const int grid = unshuffle_wgrad_grid(tiles);
    static int cus = 0;
#define U_WG(S, NT) tnr_kernel_lds(wgrad_unshuffle_kernel<S, NT>, unshuffle_wgrad_lds<S, NT>())
    rc = mp_launch(&cus, "wgrad_unshuffle", {U_WG(2, 1), U_WG(2, 2), U_WG(4, 1), U_WG(4, 2)}, (s == 4 ? 2 : 0) + (nf == 64 ? 1 : 0), dim3(grid), &k, stream);
#undef U_WG
    if (rc != TNR_OK) return rc;
    UWgradRedK r;
    r.ws = ws; r.grid = grid; r.nf = nf; r.s = s;
    r.dw = dw; r.db = db; r.alpha = alpha; r.beta = beta;
    hipLaunchKernelGGL(wgrad_unshuffle_reduce_kernel, dim3(tnr_cdiv((27 * s * s + 1) * nf, 256)), dim3(256), 0, (hipStream_t)stream, r);
    return tnr_check_launch("wgrad_unshuffle_reduce");
}
