// DiffAugment on the discriminator inputs (codes/dataops/diffaug.py): the composite of one call,
//
//     out = cutout_mask . Geo( Colour(x) )
//
// of a fp32 image batch N x C x H x W (C <= 4) in either dense layout, value and adjoint.  The draws come from the host module
// (trainner_amd/dataops/diffaug.py): one DaImage per image on the device, the batch-wide ones (DaGeo) as kernel arguments.
//
//   Colour   s = x + b;  s = (s - mean_C s) sat + mean_C s;  s = (s - m) con + m,  m = mean_CHW(x) + b  (saturation keeps the channel
//            mean, brightness shifts it).  Affine in x given the draws, so the backward needs nothing from the forward.
//   Geo      one of identity / per-image integer translation / zoom_in (crop, bilinear up) / zoom_out (zero padding, bilinear down),
//            then a batch-wide horizontal flip, then a batch-wide rot90 by +1 or -1 (H = W).  Every map is separable: per axis an
//            output coordinate reads at most two taps (i0, w0), (i1, w1); a tap outside the image reads 0 (the padding is applied
//            AFTER the colour map).  Bilinear indices and weights follow ATen's align_corners=False rule in fp32.
//   Cutout   per-image box of (round(H/2), round(W/2)) at (oy - ch/2, ox - cw/2), both ends clamped into the image: the clamped
//            indices of the reference still zero the border row / column they land on.
//
//   diffaug_sum<false>   per-block fp64 partials of sum x[n]                        (forward, only with `color`)
//   diffaug_fwd          the fused pass: one thread = the C channels of one output pixel
//   diffaug_sum<true>    per-block fp64 partials of sum P[n], P = Geo^T(mask . g), formed over the OUTPUTS (the in-range tap
//                        weights of an output sum to what it hands to P): no P tensor exists
//   diffaug_bwd          gx = Colour^T(P) in gather form: one thread = one source pixel, which loops over the contiguous range of
//                        outputs whose taps name it (a range from the inverse of the monotone index map, widened by one and then
//                        tested with the forward's own tap function, so the two cannot disagree)
//
// No atomics; the partials are summed in a fixed order by every block that needs the mean: two runs are bit-identical.  Policies
// without `color` and without a zoom are pure copies and zeros.
#include "image_tile.h"

namespace {

enum { GEO_IDENT = 0, GEO_TRANSL = 1, GEO_ZOOM_IN = 2, GEO_ZOOM_OUT = 3 };
constexpr int MAXB = 64;                                 // partial sums per image

struct DaImage {                                         // 32 bytes per image, written by the host module
    float b, sat, con;                                   // brightness shift, saturation and contrast factors
    int ty, tx;                                          // translation: out(y, x) = in(y + ty, x + tx)
    int oy, ox;                                          // cutout offsets as drawn
    int pad;
};

struct DaGeo {
    int kind, flip, rot;                                 // rot: 0, +1, -1 (torch.rot90's k)
    int offy, offx;                                      // zoom_in: the crop's first row / column; zoom_out: -top, -left
    int inh, inw;                                        // zoom_in: the crop's size; zoom_out: the padded size
    int color, cutout;
    int ch, cw;                                          // cutout box
    int tw_log2;                                         // width of the thread grid (256 threads): 64 x 4, or 16 x 16 under rotation
    float scy, scx, ivy, ivx;                            // zooms: (float)in / (float)out per axis (ATen's scale) and its inverse
};
constexpr int ROWS = 4;                                  // rows of the thread grid per block: a thread handles ROWS pixels of one column

struct Tap {
    int i0, i1;                                          // image coordinates, possibly outside [0, size)
    float w0, w1;
};

// ATen's area_pixel_compute_source_index / guard_index_and_lambda, align_corners=False
__device__ __forceinline__ Tap zoom_tap(int d, float scale, int in, int off) {
    float src = scale * ((float)d + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    int i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    float l1 = src - (float)i0;
    l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
    const int i1 = i0 + 1 < in ? i0 + 1 : in - 1;
    return Tap{i0 + off, i1 + off, 1.f - l1, l1};
}

// final output position (Y, X) -> the position (y, x) of Geo's first map that it shows (undo the rotation, then the flip)
__device__ __forceinline__ void unrotate(const DaGeo &q, int S, int W, int Y, int X, int *y, int *x) {
    int yy = Y, xx = X;
    if (q.rot == 1) { yy = X; xx = S - 1 - Y; }          // rot90(a, 1)[i][j] = a[j][S - 1 - i]
    else if (q.rot == -1) { yy = S - 1 - X; xx = Y; }    // rot90(a, -1)[i][j] = a[S - 1 - j][i]
    if (q.flip) xx = W - 1 - xx;
    *y = yy; *x = xx;
}

// the inverse: where position (y, x) of the first map lands
__device__ __forceinline__ void rotate(const DaGeo &q, int S, int W, int y, int x, int *Y, int *X) {
    if (q.flip) x = W - 1 - x;
    if (q.rot == 1) { *Y = S - 1 - x; *X = y; }
    else if (q.rot == -1) { *Y = x; *X = S - 1 - y; }
    else { *Y = y; *X = x; }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ float cut_mask(const DaGeo &q, const DaImage &p, int H, int W, int Y, int X) {
    if (!q.cutout) return 1.f;
    const int ylo = clampi(p.oy - q.ch / 2, 0, H - 1), yhi = clampi(p.oy + q.ch - 1 - q.ch / 2, 0, H - 1);
    const int xlo = clampi(p.ox - q.cw / 2, 0, W - 1), xhi = clampi(p.ox + q.cw - 1 - q.cw / 2, 0, W - 1);
    return (Y >= ylo && Y <= yhi && X >= xlo && X <= xhi) ? 0.f : 1.f;
}

// the per-image sum of the partials (sh: MAXB doubles), by the same tree in every block; valid in all threads
__device__ __forceinline__ double image_sum(const double *__restrict__ part, int n, int nb, double *sh) {
    const int t = threadIdx.x;
    if (t < MAXB) sh[t] = t < nb ? part[(int64_t)n * MAXB + t] : 0.0;
    __syncthreads();
#pragma unroll
    for (int s = MAXB / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

template <int C>
__device__ __forceinline__ void load_px(const float *__restrict__ x, const ImView &g, int64_t base, int y, int xx, float (&v)[C]) {
    const int64_t a = base + (int64_t)y * g.sH + (int64_t)xx * g.sW;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = x[a + c * g.sC];
}

template <int C>
__device__ __forceinline__ void colour(float (&s)[C], const DaImage &p, float m) {
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        s[c] = s[c] + p.b;
        sum += s[c];
    }
    const float mc = sum / (float)C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        s[c] = (s[c] - mc) * p.sat + mc;
        s[c] = (s[c] - m) * p.con + m;
    }
}

// Colour(x) at image position (y, x), 0 outside the image
template <int C>
__device__ __forceinline__ void tap_px(const float *__restrict__ x, const ImView &g, int64_t base, int y, int xx, const DaGeo &q,
                                       const DaImage &p, float m, float (&v)[C]) {
    if (y < 0 || y >= g.h || xx < 0 || xx >= g.w) {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = 0.f;
        return;
    }
    load_px<C>(x, g, base, y, xx, v);
    if (q.color) colour<C>(v, p, m);
}

// block -> image n, the thread's column X and its first row Y0; its rows are Y0 + r * th, r < ROWS.  Returns th
__device__ __forceinline__ int tile_pixel(const DaGeo &q, int tilesX, int tilesY, int *n, int *Y0, int *X) {
    const int tw = 1 << q.tw_log2, th = 256 >> q.tw_log2;
    int b = blockIdx.x;
    const int tx = b % tilesX; b /= tilesX;
    const int ty = b % tilesY; b /= tilesY;
    *n = b;
    *Y0 = ty * th * ROWS + ((int)threadIdx.x >> q.tw_log2);
    *X = tx * tw + ((int)threadIdx.x & (tw - 1));
    return th;
}

template <int C>
__global__ __launch_bounds__(256) void diffaug_fwd(const float *__restrict__ x, ImView g, const DaImage *__restrict__ prm, DaGeo q,
                                                   const double *__restrict__ part, int nb, int tilesX, int tilesY,
                                                   float *__restrict__ out) {
    __shared__ double sh[MAXB];
    int n, Y0, X;
    const int th = tile_pixel(q, tilesX, tilesY, &n, &Y0, &X);
    const DaImage p = prm[n];
    float m = 0.f;
    if (q.color) m = (float)(image_sum(part, n, nb, sh) / ((double)C * g.h * g.w)) + p.b;
    if (X >= g.w) return;
    const int64_t base = (int64_t)n * g.sN;
    for (int r = 0; r < ROWS; ++r) {
        const int Y = Y0 + r * th;
        if (Y >= g.h) break;
        int y, xx;
        unrotate(q, g.h, g.w, Y, X, &y, &xx);
        float v[C];
        if (q.kind <= GEO_TRANSL) {
            if (q.kind == GEO_TRANSL) { y += p.ty; xx += p.tx; }
            tap_px<C>(x, g, base, y, xx, q, p, m, v);
        } else {
            const Tap ty = zoom_tap(y, q.scy, q.inh, q.offy), tx = zoom_tap(xx, q.scx, q.inw, q.offx);
            float v00[C], v01[C], v10[C], v11[C];
            tap_px<C>(x, g, base, ty.i0, tx.i0, q, p, m, v00);
            tap_px<C>(x, g, base, ty.i0, tx.i1, q, p, m, v01);
            tap_px<C>(x, g, base, ty.i1, tx.i0, q, p, m, v10);
            tap_px<C>(x, g, base, ty.i1, tx.i1, q, p, m, v11);
#pragma unroll
            for (int c = 0; c < C; ++c)
                v[c] = ty.w0 * (tx.w0 * v00[c] + tx.w1 * v01[c]) + ty.w1 * (tx.w0 * v10[c] + tx.w1 * v11[c]);
        }
        const int64_t a = base + (int64_t)Y * g.sH + (int64_t)X * g.sW;
        if (q.cutout) {
            const float mk = cut_mask(q, p, g.h, g.w, Y, X);
#pragma unroll
            for (int c = 0; c < C; ++c) out[a + c * g.sC] = v[c] * mk;
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) out[a + c * g.sC] = v[c];
        }
    }
}

// the weight with which the output coordinate d of one axis reads image coordinate s (0 when it does not); `hit` says whether a tap
// names s at all
__device__ __forceinline__ float axis_weight(int kind, int d, float scale, int in, int off, int t, int s, bool *hit) {
    if (kind <= GEO_TRANSL) {
        *hit = d + t == s;
        return 1.f;
    }
    const Tap k = zoom_tap(d, scale, in, off);
    float w = 0.f;
    *hit = false;
    if (k.i0 == s) { w = k.w0; *hit = true; }
    if (k.i1 == s) { w = *hit ? w + k.w1 : k.w1; *hit = true; }
    return w;
}

// the range of output coordinates whose taps can name image coordinate s: src(d) = scale (d + 0.5) - 0.5 within (s' - 1, s' + 1),
// s' = s - off, widened by one on either side (the exact test is axis_weight's)
__device__ __forceinline__ void axis_range(int kind, int out, float inv, int in, int off, int t, int s, int *lo, int *hi) {
    if (kind <= GEO_TRANSL) {
        *lo = *hi = s - t;
        if (*lo < 0 || *lo >= out) { *lo = 0; *hi = -1; }
        return;
    }
    const int sl = s - off;
    if (sl < 0 || sl >= in) { *lo = 0; *hi = -1; return; }
    const int a = (int)floorf(((float)sl - 0.5f) * inv - 0.5f) - 1, b = (int)ceilf(((float)sl + 1.5f) * inv - 0.5f) + 1;
    *lo = sl == 0 ? 0 : (a < 0 ? 0 : a);                 // src is clamped at 0: every output below reads tap 0
    *hi = sl == in - 1 ? out - 1 : (b > out - 1 ? out - 1 : b);
}

template <int C>
__global__ __launch_bounds__(256) void diffaug_bwd(const float *__restrict__ go, ImView g, const DaImage *__restrict__ prm, DaGeo q,
                                                   const double *__restrict__ part, int nb, int tilesX, int tilesY,
                                                   float *__restrict__ gx) {
    __shared__ double sh[MAXB];
    int n, sy0, sx;
    const int th = tile_pixel(q, tilesX, tilesY, &n, &sy0, &sx);
    const DaImage p = prm[n];
    float MP = 0.f;
    if (q.color) MP = (float)(image_sum(part, n, nb, sh) / ((double)C * g.h * g.w));
    if (sx >= g.w) return;
    const int64_t base = (int64_t)n * g.sN;
    int xlo, xhi;
    axis_range(q.kind, g.w, q.ivx, q.inw, q.offx, p.tx, sx, &xlo, &xhi);
    for (int r = 0; r < ROWS; ++r) {
        const int sy = sy0 + r * th;
        if (sy >= g.h) break;
        int ylo, yhi;
        axis_range(q.kind, g.h, q.ivy, q.inh, q.offy, p.ty, sy, &ylo, &yhi);
        float P[C];
#pragma unroll
        for (int c = 0; c < C; ++c) P[c] = 0.f;
        for (int y = ylo; y <= yhi; ++y) {
            bool hy;
            const float wy = axis_weight(q.kind, y, q.scy, q.inh, q.offy, p.ty, sy, &hy);
            if (!hy) continue;
            for (int xx = xlo; xx <= xhi; ++xx) {
                bool hx;
                const float wx = axis_weight(q.kind, xx, q.scx, q.inw, q.offx, p.tx, sx, &hx);
                if (!hx) continue;
                int Y, X;
                rotate(q, g.h, g.w, y, xx, &Y, &X);
                float v[C];
                load_px<C>(go, g, base, Y, X, v);
                if (q.cutout) {
                    const float mk = cut_mask(q, p, g.h, g.w, Y, X);
#pragma unroll
                    for (int c = 0; c < C; ++c) v[c] = v[c] * mk;
                }
                if (q.kind <= GEO_TRANSL) {
#pragma unroll
                    for (int c = 0; c < C; ++c) P[c] = v[c];
                } else {
                    const float w = wy * wx;
#pragma unroll
                    for (int c = 0; c < C; ++c) P[c] = P[c] + w * v[c];
                }
            }
        }
        if (q.color) {
            // contrast: con P, and (1 - con) mean_CHW(P) to every element; saturation: sat u + (1 - sat) mean_C u; brightness: identity
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                P[c] = p.con * P[c];
                sum += P[c];
            }
            const float mc = sum / (float)C, k = (1.f - p.con) * MP;
#pragma unroll
            for (int c = 0; c < C; ++c) P[c] = (p.sat * P[c] + (1.f - p.sat) * mc) + k;
        }
        const int64_t a = base + (int64_t)sy * g.sH + (int64_t)sx * g.sW;
#pragma unroll
        for (int c = 0; c < C; ++c) gx[a + c * g.sC] = P[c];
    }
}

// the sum of the in-range tap weights of output coordinate d: what that output hands on to P along this axis
__device__ __forceinline__ float axis_inrange(int kind, int d, float scale, int in, int off, int t, int size) {
    if (kind <= GEO_TRANSL) return (d + t >= 0 && d + t < size) ? 1.f : 0.f;
    const Tap k = zoom_tap(d, scale, in, off);
    float w = 0.f;
    if (k.i0 >= 0 && k.i0 < size) w = k.w0;
    if (k.i1 >= 0 && k.i1 < size) w = w + k.w1;
    return w;
}

// part[n][b]: block b's fp64 share of sum x[n] (BWD = false) or of sum Geo^T(mask . g)[n] (BWD = true); grid (nb, N)
template <int C, bool BWD>
__global__ __launch_bounds__(256) void diffaug_sum(const float *__restrict__ src, ImView g, const DaImage *__restrict__ prm, DaGeo q,
                                                   double *__restrict__ part) {
    __shared__ double sh[256];
    const int n = blockIdx.y;
    const int64_t base = (int64_t)n * g.sN;
    const int64_t hw = (int64_t)g.h * g.w;
    double acc = 0.0;
    DaImage p = {};
    if (BWD) p = prm[n];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
        const int Y = (int)(i / g.w), X = (int)(i - (int64_t)Y * g.w);
        float v[C];
        load_px<C>(src, g, base, Y, X, v);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) s += v[c];
        if (BWD) {
            int y, xx;
            unrotate(q, g.h, g.w, Y, X, &y, &xx);
            const float w = axis_inrange(q.kind, y, q.scy, q.inh, q.offy, p.ty, g.h) * axis_inrange(q.kind, xx, q.scx, q.inw, q.offx, p.tx, g.w);
            s = s * (w * cut_mask(q, p, g.h, g.w, Y, X));
        }
        acc += (double)s;
    }
    const double r = tnr_block_sum256(acc, sh);
    if (threadIdx.x == 0) part[(int64_t)n * MAXB + blockIdx.x] = r;
}

int sum_blocks(int H, int W) {
    const int64_t b = tnr_cdiv64((int64_t)H * W, 256 * 4);
    return (int)(b < 1 ? 1 : (b > MAXB ? MAXB : b));
}

int check_geo(const char *what, int N, int C, int H, int W, int layout, const int32_t *geo, DaGeo *q, int *tilesX, int *tilesY,
              int64_t *blocks) {
    if (int rc = check_dense(what, N, C, H, W, layout)) return rc;
    TNR_REQUIRE(C <= 4, "%s: at most 4 channels, got %d", what, C);
    TNR_REQUIRE(geo, "%s: null geometry record", what);
    q->kind = geo[0]; q->flip = geo[1]; q->rot = geo[2]; q->offy = geo[3]; q->offx = geo[4]; q->inh = geo[5]; q->inw = geo[6];
    q->color = geo[7]; q->cutout = geo[8];
    TNR_REQUIRE(q->kind >= GEO_IDENT && q->kind <= GEO_ZOOM_OUT, "%s: unknown geometric kind %d", what, q->kind);
    TNR_REQUIRE(q->rot >= -1 && q->rot <= 1 && (q->flip == 0 || q->flip == 1), "%s: bad flip / rotation (%d, %d)", what, q->flip, q->rot);
    TNR_REQUIRE(q->rot == 0 || H == W, "%s: rotate needs H = W, got %d x %d", what, H, W);
    if (q->kind == GEO_ZOOM_IN)                           // the crop lies inside the image
        TNR_REQUIRE(q->inh >= 1 && q->inw >= 1 && q->offy >= 0 && q->offx >= 0 && q->offy + q->inh <= H && q->offx + q->inw <= W,
                    "%s: zoom_in crop %d x %d at (%d, %d) leaves the %d x %d image", what, q->inh, q->inw, q->offy, q->offx, H, W);
    if (q->kind == GEO_ZOOM_OUT)                          // the image lies inside the padded frame
        TNR_REQUIRE(q->offy <= 0 && q->offx <= 0 && q->inh >= H - q->offy && q->inw >= W - q->offx && q->inh <= 4 * H && q->inw <= 4 * W,
                    "%s: zoom_out frame %d x %d with the image at (%d, %d) does not hold the %d x %d image", what, q->inh, q->inw,
                    -q->offy, -q->offx, H, W);
    q->ch = (int)(H * 0.5 + 0.5); q->cw = (int)(W * 0.5 + 0.5);
    q->tw_log2 = q->rot ? 4 : 6;
    *tilesX = tnr_cdiv(W, 1 << q->tw_log2);
    *tilesY = tnr_cdiv(H, (256 >> q->tw_log2) * ROWS);
    q->scy = q->scx = q->ivy = q->ivx = 1.f;
    if (q->kind >= GEO_ZOOM_IN) {
        q->scy = (float)q->inh / (float)H; q->scx = (float)q->inw / (float)W;
        q->ivy = (float)H / (float)q->inh; q->ivx = (float)W / (float)q->inw;
    }
    *blocks = (int64_t)N * *tilesX * *tilesY;
    TNR_REQUIRE(*blocks < (1ll << 31), "%s: batch too large", what);
    return TNR_OK;
}

#define DA_DISPATCH_C(C, ...)                                  \
    switch (C) {                                               \
        case 1: { constexpr int CC = 1; __VA_ARGS__; } break;  \
        case 2: { constexpr int CC = 2; __VA_ARGS__; } break;  \
        case 3: { constexpr int CC = 3; __VA_ARGS__; } break;  \
        default: { constexpr int CC = 4; __VA_ARGS__; } break; \
    }

}  // namespace

extern "C" int64_t tnr_diffaug_workspace_bytes(int32_t N) { return N > 0 ? (int64_t)N * MAXB * 8 : 0; }

extern "C" int tnr_diffaug_mean(const float *src, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const void *params,
                                const int32_t *geo, int32_t backward, void *ws, int64_t ws_bytes, void *stream) {
    const char *what = "diffaug_mean";
    DaGeo q;
    int tilesX, tilesY;
    int64_t blocks;
    if (int rc = check_geo(what, N, C, H, W, layout, geo, &q, &tilesX, &tilesY, &blocks)) return rc;
    TNR_REQUIRE(src && ws && (!backward || params), "%s: null pointer", what);
    TNR_REQUIRE(ws_bytes >= tnr_diffaug_workspace_bytes(N), "%s: workspace of %lld bytes, need %lld", what, (long long)ws_bytes,
                (long long)tnr_diffaug_workspace_bytes(N));
    TNR_REQUIRE(N <= 65535, "%s: batch too large", what);
    const dim3 grid((unsigned)sum_blocks(H, W), (unsigned)N);
    const ImView g = make_view(N, C, H, W, layout);
    if (backward) {
        DA_DISPATCH_C(C, hipLaunchKernelGGL((diffaug_sum<CC, true>), grid, dim3(256), 0, (hipStream_t)stream, src, g,
                                             (const DaImage *)params, q, (double *)ws));
    } else {
        DA_DISPATCH_C(C, hipLaunchKernelGGL((diffaug_sum<CC, false>), grid, dim3(256), 0, (hipStream_t)stream, src, g,
                                             (const DaImage *)params, q, (double *)ws));
    }
    return tnr_check_launch(what);
}

extern "C" int tnr_diffaug_fwd(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const void *params,
                               const int32_t *geo, const void *ws, float *out, void *stream) {
    const char *what = "diffaug_fwd";
    DaGeo q;
    int tilesX, tilesY;
    int64_t blocks;
    if (int rc = check_geo(what, N, C, H, W, layout, geo, &q, &tilesX, &tilesY, &blocks)) return rc;
    TNR_REQUIRE(x && out && params && x != out, "%s: null or aliased pointer", what);
    TNR_REQUIRE(!q.color || ws, "%s: `color` needs the partial sums of tnr_diffaug_mean", what);
    const ImView g = make_view(N, C, H, W, layout);
    DA_DISPATCH_C(C, hipLaunchKernelGGL((diffaug_fwd<CC>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, g,
                                         (const DaImage *)params, q, (const double *)ws, sum_blocks(H, W), tilesX, tilesY, out));
    return tnr_check_launch(what);
}

extern "C" int tnr_diffaug_bwd(const float *g_out, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const void *params,
                               const int32_t *geo, const void *ws, float *gx, void *stream) {
    const char *what = "diffaug_bwd";
    DaGeo q;
    int tilesX, tilesY;
    int64_t blocks;
    if (int rc = check_geo(what, N, C, H, W, layout, geo, &q, &tilesX, &tilesY, &blocks)) return rc;
    TNR_REQUIRE(g_out && gx && params && g_out != gx, "%s: null or aliased pointer", what);
    TNR_REQUIRE(!q.color || ws, "%s: `color` needs the partial sums of tnr_diffaug_mean", what);
    const ImView g = make_view(N, C, H, W, layout);
    DA_DISPATCH_C(C, hipLaunchKernelGGL((diffaug_bwd<CC>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g_out, g,
                                         (const DaImage *)params, q, (const double *)ws, sum_blocks(H, W), tilesX, tilesY, gx));
    return tnr_check_launch(what);
}
