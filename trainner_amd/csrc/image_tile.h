// What the image-loss translation units (ssim_loss.hip, image_losses.hip, spl_loss.hip, pooled_losses.hip, freqsep.hip) share: the view
// of a dense fp32 image batch, the argument checks and the 16-byte-path test of their entry points, the block -> tile decode, the staging
// of a tile with a zero halo in LDS, the difference-only criteria and the final sum over the blocks' fp64 partials.  The kernels stay in their files (DESIGN.md sections 11-13).
#pragma once
#include "common.h"

struct ImView {                                          // the (shaved) h x w region of an N x C x H x W batch in either dense layout
    int64_t sN, sC, sH, sW, off;                         // off: the region's first pixel
    int N, C, h, w;
};

static inline ImView make_view(int N, int C, int H, int W, int layout, int shave = 0) {
    ImView v;
    v.sN = (int64_t)C * H * W;
    if (layout == 0) {
        v.sC = (int64_t)H * W; v.sH = W; v.sW = 1;
    } else {
        v.sC = 1; v.sH = (int64_t)W * C; v.sW = C;
    }
    v.off = (int64_t)shave * v.sH + (int64_t)shave * v.sW;
    v.N = N; v.C = C; v.h = H - 2 * shave; v.w = W - 2 * shave;
    return v;
}

static inline int check_dense(const char *what, int N, int C, int H, int W, int layout) {
    TNR_REQUIRE(N > 0 && C >= 1 && H > 0 && W > 0, "%s: bad shape %d x %d x %d x %d", what, N, C, H, W);
    TNR_REQUIRE(layout == 0 || layout == 1, "%s: layout must be 0 (NCHW) or 1 (channels-last)", what);
    return TNR_OK;
}

// check_dense, then the launch geometry of one workgroup per TW x TH tile of every (n, c) plane of H x W positions
static inline int check_batch(const char *what, int N, int C, int H, int W, int layout, int TW, int TH, int64_t *blocks, int *tilesX,
                              int *tilesY) {
    if (int rc = check_dense(what, N, C, H, W, layout)) return rc;
    *tilesY = tnr_cdiv(H, TH);
    *tilesX = tnr_cdiv(W, TW);
    *blocks = (int64_t)N * C * *tilesY * *tilesX;
    TNR_REQUIRE(*blocks < (1ll << 31), "%s: batch too large", what);
    return TNR_OK;
}

static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// 16-byte loads / stores in the stencil kernels: NCHW rows that start on a 16-byte boundary and split into whole groups of four
static inline int vec_rows(int layout, int W, const void *a, const void *b = nullptr, const void *c = nullptr) {
    return layout == 0 && (W & 3) == 0 && aligned16(a) && (!b || aligned16(b)) && (!c || aligned16(c));
}

template <int TW, int TH>
__device__ __forceinline__ void tile_of_block(const ImView &g, int tilesX, int tilesY, int *n, int *c, int *y0, int *x0) {
    int b = blockIdx.x;
    const int tx = b % tilesX; b /= tilesX;
    const int ty = b % tilesY; b /= tilesY;
    *c = b % g.C; *n = b / g.C;
    *y0 = ty * TH; *x0 = tx * TW;
}

// Fills NT LDS tiles (row stride ST floats) with the IH x IW pixels whose first is image position (y0 - HALO, x0 - HALO) of the plane
// at `base`; positions outside the h x w region hold 0.  px(a, v) loads what the tiles get for the pixel at offset a, or with `vec`
// (see vec_rows) for the aligned group of four pixels that starts there, into v[0 .. NT).  The groups of a row start at column
// x0 - GX0 (GX0 a multiple of 4, >= HALO), each wholly inside or wholly outside the image; element k of group gq is staged column
// 4 gq + HALO - GX0 + k and is kept when it is one of the first QW (>= IW, <= ST) columns of the row.  A group that begins a
// 16-byte slot of LDS (HALO = GX0, nothing dropped) is stored as one.  256 threads; the caller synchronises.
template <int IH, int IW, int HALO, int ST, int GX0, int QW, int NT, class Px>
__device__ __forceinline__ void stage_tile(const ImView &g, int64_t base, int y0, int x0, int vec, float *const (&dst)[NT], const Px &px) {
    if (vec) {
        constexpr int NG = (GX0 + IW - HALO + 3) / 4, SH = HALO - GX0;
        for (int i = threadIdx.x; i < IH * NG; i += 256) {
            const int r = i / NG, gq = i - r * NG;
            const int yy = y0 - HALO + r, xg = x0 - GX0 + 4 * gq;
            f32x4 v[NT] = {};                            // zero padding
            if (yy >= 0 && yy < g.h && xg >= 0 && xg < g.w) px(base + (int64_t)yy * g.sH + xg, v);
            const int q = 4 * gq + SH;
            if constexpr (SH == 0 && QW >= 4 * NG) {
#pragma unroll
                for (int t = 0; t < NT; ++t) *(f32x4 *)(dst[t] + r * ST + q) = v[t];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if ((SH + k >= 0 || q + k >= 0) && (QW >= 4 * NG + SH || q + k < QW)) {
#pragma unroll
                        for (int t = 0; t < NT; ++t) dst[t][r * ST + q + k] = v[t][k];
                    }
            }
        }
    } else {
        for (int i = threadIdx.x; i < IH * IW; i += 256) {
            const int r = i / IW, q = i - r * IW;
            const int yy = y0 - HALO + r, xx = x0 - HALO + q;
            float v[NT] = {};                            // zero padding
            if (yy >= 0 && yy < g.h && xx >= 0 && xx < g.w) px(base + (int64_t)yy * g.sH + (int64_t)xx * g.sW, v);
#pragma unroll
            for (int t = 0; t < NT; ++t) dst[t][r * ST + q] = v[t];
        }
    }
}

// The criteria of the difference alone (image_losses.hip, pooled_losses.hip): rho(e) and d rho / d e as autograd gives it
// (sign(0) = 0, the clamp passes the gradient on the closed interval)
enum { CRIT_L1 = TNR_CRIT_L1, CRIT_L2 = TNR_CRIT_L2, CRIT_CB = TNR_CRIT_CB, CRIT_ELASTIC = TNR_CRIT_ELASTIC, CRIT_CLIPL1 = TNR_CRIT_CLIPL1 };

__device__ __forceinline__ float sgn(float e) { return e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f); }

__device__ __forceinline__ float rho(float e, int crit) {
    const float a = fabsf(e);
    switch (crit) {
    case CRIT_L1: return a;
    case CRIT_L2: return e * e;
    case CRIT_CB: return sqrtf(e * e + 1e-12f);
    case CRIT_ELASTIC: return 0.2f * (e * e) + 0.8f * a;
    default: return fminf(a, 10.f);                      // clipl1: clamp(|e|, 0, 10)
    }
}

__device__ __forceinline__ float drho(float e, int crit) {
    switch (crit) {
    case CRIT_L1: return sgn(e);
    case CRIT_L2: return 2.f * e;
    case CRIT_CB: return e / sqrtf(e * e + 1e-12f);
    case CRIT_ELASTIC: return 0.4f * e + 0.8f * sgn(e);
    default: return fabsf(e) <= 10.f ? sgn(e) : 0.f;
    }
}

// NS interleaved sums over `count` fp64 slots each (p[NS i + j]), strided over the 256 threads and then summed in the block's fixed
// order: the second stage of every "one partial per block" reduction.  out[0 .. NS) is valid in thread 0.
template <int NS, class Count>
__device__ __forceinline__ void sum_partials(const double *__restrict__ p, Count count, double *sh, double *out) {
    double acc[NS] = {};
    for (Count i = threadIdx.x; i < count; i += 256)
#pragma unroll
        for (int j = 0; j < NS; ++j) acc[j] += p[NS * i + j];
#pragma unroll
    for (int j = 0; j < NS; ++j) out[j] = tnr_block_sum256(acc[j], sh);
}
