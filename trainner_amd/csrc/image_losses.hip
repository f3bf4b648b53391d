// Image-space training losses of the form  stencil -> pointwise criterion rho -> sum  (codes/models/modules/loss.py: HFENLoss :173-224,
// TVLoss :227-299, GradientLoss :302-325 and the difference-only pixel criteria :47-58,328-343,387-402) for fp32 image batches,
// value and d/dX.
//
//   filter_kernel<0>   HFEN forward: one workgroup = one 64 x 16 tile of one (n, c) plane.  d = x - y with a 7-pixel zero halo is staged in
//                      LDS once, every thread forms four neighbouring responses e = L * d (15 x 15 taps from the kernel arguments), adds
//                      rho(e) into the block's fp64 partial and, when a gradient is wanted, stores rho'(e)
//                      (the stencil kernels load and store 16 bytes at a time where NCHW rows split into aligned groups of four)
//   filter_kernel<1>   HFEN backward: the same stencil with the flipped taps over the stored rho'(e) map, times scale * gscale
//   fd_fwd_kernel      finite differences (dataops/filters.py:722-777, quirks included) of x and of y, rho of their difference, partial sum
//   fd_bwd_kernel      gathers every pixel's gradient from the responses of its 3 x 3 neighbourhood, recomputed from x and y in LDS
//   point_*_kernel     rho(a - b) over a flat dense range (pixel_criterion other than l1)
//   overflow_*_kernel  log(|x - clamp(x, 0, 1)| + 1) over a flat dense range (OFLoss :527-542)
//   sum_kernel         the blocks' partials in a fixed order -> loss = scale * sum
//
// All reductions are fixed-order (one fp64 slot per block, then one block): two runs are bit-identical.  No float atomics.
#include "image_tile.h"

namespace {

constexpr int FK = 15, FR = FK / 2;                      // filter taps per side (smaller odd filters are centred and zero-padded)
constexpr int TW = 64, TH = 16;                          // tile of every stencil kernel; thread = 4 neighbouring columns of one row
constexpr int FIW = TW + 2 * FR, FIH = TH + 2 * FR;      // 78 x 30 staged differences
constexpr int FST = 81;                                  // LDS row stride: = 1 mod 4, so the 4 rows of a wave start on banks 0, 1, 2, 3
constexpr int DST = TW + 3;                              // finite-difference tiles: 66 columns staged, stride 67

struct FilterTaps {
    float w[FK * FK];
};

__global__ __launch_bounds__(256) void sum_kernel(const double *__restrict__ partial, int64_t count, double scale, float *__restrict__ loss) {
    __shared__ double sh[256];
    double acc;
    sum_partials<1>(partial, count, sh, &acc);
    if (threadIdx.x == 0) *loss = (float)(acc * scale);
}

// what stage_tile stores for the filter: the difference x - y, or (BWD) the rho'(e) map
template <int BWD>
struct DiffPixel {
    const float *x, *y;
    template <class V>
    __device__ __forceinline__ void operator()(int64_t a, V (&v)[1]) const {
        v[0] = *(const V *)(x + a);
        if (!BWD) v[0] -= *(const V *)(y + a);
    }
};

// BWD = 0: src = x, y != nullptr, e = L * (x - y); partial[block] = sum rho(e); dmap (nullable) = rho'(e).
// BWD = 1: src = the rho'(e) map, out = (accumulate ? out : 0) + mul * (L * src) with the taps already flipped by the host.
template <int BWD>
__global__ __launch_bounds__(256) void filter_kernel(const float *__restrict__ src, const float *__restrict__ y, ImView g, FilterTaps taps,
                                                     int crit, int tilesX, int tilesY, double *__restrict__ partial,
                                                     float *__restrict__ out, float scale, const float *__restrict__ gscale, int accumulate,
                                                     int vec) {
    __shared__ float sD[FIH * FST];
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    int n, c, y0, x0;
    tile_of_block<TW, TH>(g, tilesX, tilesY, &n, &c, &y0, &x0);
    const int64_t base = (int64_t)n * g.sN + (int64_t)c * g.sC;
    // with 16-byte loads: the 20 aligned groups of four columns x0 - 8 .. x0 + 71 of every staged row.  Group gq lands on LDS columns
    // 4 gq - 1 .. 4 gq + 2; column -1 is dropped, column 78 falls into the row's padding (FST = 81)
    float *const tile[1] = {sD};
    stage_tile<FIH, FIW, FR, FST, 8, FIW + 1>(g, base, y0, x0, vec, tile, DiffPixel<BWD>{src, y});
    __syncthreads();
    const int row = tid >> 4, col = (tid & 15) * 4;
    float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
#pragma unroll
    for (int ky = 0; ky < FK; ++ky) {
        float v[FK + 3];
#pragma unroll
        for (int j = 0; j < FK + 3; ++j) v[j] = sD[(row + ky) * FST + col + j];
#pragma unroll
        for (int kx = 0; kx < FK; ++kx) {
            const float w = taps.w[ky * FK + kx];
            e0 = fmaf(w, v[kx], e0);
            e1 = fmaf(w, v[kx + 1], e1);
            e2 = fmaf(w, v[kx + 2], e2);
            e3 = fmaf(w, v[kx + 3], e3);
        }
    }
    const float e[4] = {e0, e1, e2, e3};
    const int yy = y0 + row;
    double acc = 0;
    float mul = 0.f;
    if (BWD) mul = scale * (gscale ? *gscale : 1.f);
    if (vec && yy < g.h && x0 + col < g.w) {             // the thread's four columns are one aligned group inside the image
        f32x4 *o = out ? (f32x4 *)(out + base + (int64_t)yy * g.sH + x0 + col) : nullptr;
        f32x4 r;
        if (BWD) {
            r.x = mul * e0; r.y = mul * e1; r.z = mul * e2; r.w = mul * e3;
            if (accumulate) r = *o + r;
            *o = r;
        } else {
            acc = (((double)rho(e0, crit) + (double)rho(e1, crit)) + (double)rho(e2, crit)) + (double)rho(e3, crit);
            if (o) {
                r.x = drho(e0, crit); r.y = drho(e1, crit); r.z = drho(e2, crit); r.w = drho(e3, crit);
                *o = r;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = x0 + col + j;
            if (yy >= g.h || xx >= g.w) continue;
            const int64_t a = base + (int64_t)yy * g.sH + (int64_t)xx * g.sW;
            if (BWD) {
                const float gv = mul * e[j];
                out[a] = accumulate ? out[a] + gv : gv;
            } else {
                acc += (double)rho(e[j], crit);
                if (out) out[a] = drho(e[j], crit);
            }
        }
    }
    if (!BWD) {
        acc = tnr_block_sum256(acc, sh);
        if (tid == 0) partial[blockIdx.x] = acc;
    }
}

// The four finite-difference responses at image position (i, j) from a staged tile in which positions outside the image hold 0:
// s points at the pixel, st is the row stride.  dx is zeroed in the last column, dy and dp in the last row; dn is not zeroed and
// dp = right - bottom sees the zero `right` of the last column (dataops/filters.py:766-777).
struct Fd4 {
    float dx, dy, dp, dn;
};
__device__ __forceinline__ Fd4 fd_resp(const float *s, int st, int i, int j, int H, int W) {
    const float v = s[0], right = s[1], bottom = s[st], botright = s[st + 1];
    Fd4 r;
    r.dx = j == W - 1 ? 0.f : right - v;
    r.dy = i == H - 1 ? 0.f : bottom - v;
    r.dp = i == H - 1 ? 0.f : right - bottom;
    r.dn = botright - v;
    return r;
}

// what stage_tile stores for the finite differences: x and y (zeros when there is no y) in two tiles
struct PairPixel {
    const float *x, *y;
    template <class V>
    __device__ __forceinline__ void operator()(int64_t a, V (&v)[2]) const {
        v[0] = *(const V *)(x + a);
        if (y) v[1] = *(const V *)(y + a);
    }
};

// stages rows y0 - UP .. y0 + TH and columns x0 - UP .. x0 + TW of x and of y.  With 16-byte loads: the 18 aligned groups of four
// columns x0 - 4 .. x0 + 67 of every staged row; element k of group gq is staged column 4 gq - 4 + UP + k, kept when it is one of the
// TW + 1 + UP columns the tile holds
template <int UP>
__device__ __forceinline__ void fd_stage(const float *__restrict__ x, const float *__restrict__ y, const ImView &g, int64_t base, int y0, int x0,
                                         int vec, float *sX, float *sY) {
    float *const tiles[2] = {sX, sY};
    stage_tile<TH + 1 + UP, TW + 1 + UP, UP, DST, 4, TW + 1 + UP>(g, base, y0, x0, vec, tiles, PairPixel{x, y});
}

// the responses' differences e = dir(x) - dir(y) at (i, j); s indexes the staged tiles at that pixel
__device__ __forceinline__ Fd4 fd_err(const float *sX, const float *sY, int s, int i, int j, int H, int W) {
    const Fd4 a = fd_resp(sX + s, DST, i, j, H, W), b = fd_resp(sY + s, DST, i, j, H, W);
    Fd4 e;
    e.dx = a.dx - b.dx; e.dy = a.dy - b.dy; e.dp = a.dp - b.dp; e.dn = a.dn - b.dn;
    return e;
}

__global__ __launch_bounds__(256) void fd_fwd_kernel(const float *__restrict__ x, const float *__restrict__ y, ImView g, int dirs, int crit,
                                                     int tilesX, int tilesY, double *__restrict__ partial, int vec) {
    __shared__ float sX[(TH + 1) * DST], sY[(TH + 1) * DST];
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    int n, c, y0, x0;
    tile_of_block<TW, TH>(g, tilesX, tilesY, &n, &c, &y0, &x0);
    fd_stage<0>(x, y, g, (int64_t)n * g.sN + (int64_t)c * g.sC, y0, x0, vec, sX, sY);
    __syncthreads();
    double acc = 0;
    for (int i = tid; i < TH * TW; i += 256) {
        const int r = i / TW, q = i % TW;
        const int yy = y0 + r, xx = x0 + q;
        if (yy >= g.h || xx >= g.w) continue;
        const Fd4 e = fd_err(sX, sY, r * DST + q, yy, xx, g.h, g.w);
        float v = rho(e.dx, crit) + rho(e.dy, crit);     // zeroed responses still count rho(0) (cb: 1e-6 each)
        if (dirs == 4) v += rho(e.dp, crit) + rho(e.dn, crit);
        acc += (double)v;
    }
    acc = tnr_block_sum256(acc, sh);
    if (tid == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void fd_bwd_kernel(const float *__restrict__ x, const float *__restrict__ y, ImView g, int dirs, int crit,
                                                     int tilesX, int tilesY, float scale, const float *__restrict__ gscale,
                                                     float *__restrict__ gx, int accumulate, int vec) {
    __shared__ float sX[(TH + 2) * DST], sY[(TH + 2) * DST];
    const int tid = threadIdx.x;
    int n, c, y0, x0;
    tile_of_block<TW, TH>(g, tilesX, tilesY, &n, &c, &y0, &x0);
    const int64_t base = (int64_t)n * g.sN + (int64_t)c * g.sC;
    fd_stage<1>(x, y, g, base, y0, x0, vec, sX, sY);
    __syncthreads();
    const float mul = scale * (gscale ? *gscale : 1.f);
    const int H = g.h, W = g.w;
    for (int t = tid; t < TH * TW; t += 256) {
        const int r = t / TW, q = t % TW;
        const int i = y0 + r, j = x0 + q;
        if (i >= H || j >= W) continue;
        const int s = (r + 1) * DST + q + 1;             // the pixel itself in the staged tiles (one halo row / column before it)
        float gv = 0.f;
        {                                                // responses placed on (i, j): the pixel is the subtrahend of dx, dy, dn
            const Fd4 e = fd_err(sX, sY, s, i, j, H, W);
            if (j < W - 1) gv -= drho(e.dx, crit);
            if (i < H - 1) gv -= drho(e.dy, crit);
            if (dirs == 4) gv -= drho(e.dn, crit);
        }
        if (j >= 1) {                                    // (i, j - 1): the pixel is `right` of dx and of dp
            const Fd4 e = fd_err(sX, sY, s - 1, i, j - 1, H, W);
            gv += drho(e.dx, crit);
            if (dirs == 4 && i < H - 1) gv += drho(e.dp, crit);
        }
        if (i >= 1) {                                    // (i - 1, j): the pixel is `bottom` of dy and of dp
            const Fd4 e = fd_err(sX, sY, s - DST, i - 1, j, H, W);
            gv += drho(e.dy, crit);
            if (dirs == 4) gv -= drho(e.dp, crit);
        }
        if (dirs == 4 && i >= 1 && j >= 1) {             // (i - 1, j - 1): the pixel is `botright` of dn
            const Fd4 e = fd_err(sX, sY, s - DST - 1, i - 1, j - 1, H, W);
            gv += drho(e.dn, crit);
        }
        gv *= mul;
        const int64_t a = base + (int64_t)i * g.sH + (int64_t)j * g.sW;
        gx[a] = accumulate ? gx[a] + gv : gv;
    }
}

constexpr int PT_BLOCKS = 1024;                          // partial slots of the flat criterion (tnr_reduce_workspace_bytes holds 2048)

__global__ __launch_bounds__(256) void point_fwd_kernel(const float *__restrict__ a, const float *__restrict__ b, int64_t n, int vec, int crit,
                                                        double *__restrict__ partial) {
    __shared__ double sh[256];
    double acc = 0;
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    if (vec) {
        const int64_t n4 = n >> 2;
        for (int64_t i = t0; i < n4; i += step) {
            const f32x4 va = ((const f32x4 *)a)[i], vb = ((const f32x4 *)b)[i];
            const float r = (rho(va.x - vb.x, crit) + rho(va.y - vb.y, crit)) + (rho(va.z - vb.z, crit) + rho(va.w - vb.w, crit));
            acc += (double)r;
        }
        for (int64_t i = (n4 << 2) + t0; i < n; i += step) acc += (double)rho(a[i] - b[i], crit);
    } else {
        for (int64_t i = t0; i < n; i += step) acc += (double)rho(a[i] - b[i], crit);
    }
    acc = tnr_block_sum256(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void point_bwd_kernel(const float *__restrict__ a, const float *__restrict__ b, int64_t n, int vec, int crit,
                                                        float scale, const float *__restrict__ gscale, float *__restrict__ ga, int accumulate) {
    const float mul = scale * (gscale ? *gscale : 1.f);
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    int64_t tail = 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        for (int64_t i = t0; i < n4; i += step) {
            const f32x4 va = ((const f32x4 *)a)[i], vb = ((const f32x4 *)b)[i];
            f32x4 r;
            r.x = mul * drho(va.x - vb.x, crit); r.y = mul * drho(va.y - vb.y, crit);
            r.z = mul * drho(va.z - vb.z, crit); r.w = mul * drho(va.w - vb.w, crit);
            if (accumulate) r += ((const f32x4 *)ga)[i];
            ((f32x4 *)ga)[i] = r;
        }
        tail = n4 << 2;
    }
    for (int64_t i = tail + t0; i < n; i += step) {
        const float r = mul * drho(a[i] - b[i], crit);
        ga[i] = accumulate ? ga[i] + r : r;
    }
}

// OFLoss: log(|x - clamp(x, 0, 1)| + 1); its derivative sign(d) / (|d| + 1) is 0 on the closed interval, where d is exactly 0
__device__ __forceinline__ float overflow_of(float v) { return v - fminf(fmaxf(v, 0.f), 1.f); }

__global__ __launch_bounds__(256) void overflow_fwd_kernel(const float *__restrict__ x, int64_t n, int vec, double *__restrict__ partial) {
    __shared__ double sh[256];
    double acc = 0;
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    int64_t tail = 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        for (int64_t i = t0; i < n4; i += step) {
            const f32x4 v = ((const f32x4 *)x)[i];
            const float r = (log1pf(fabsf(overflow_of(v.x))) + log1pf(fabsf(overflow_of(v.y)))) +
                            (log1pf(fabsf(overflow_of(v.z))) + log1pf(fabsf(overflow_of(v.w))));
            acc += (double)r;
        }
        tail = n4 << 2;
    }
    for (int64_t i = tail + t0; i < n; i += step) acc += (double)log1pf(fabsf(overflow_of(x[i])));
    acc = tnr_block_sum256(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void overflow_bwd_kernel(const float *__restrict__ x, int64_t n, int vec, float scale,
                                                           const float *__restrict__ gscale, float *__restrict__ gx, int accumulate) {
    const float mul = scale * (gscale ? *gscale : 1.f);
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    const auto d = [mul](float v) {
        const float e = overflow_of(v);
        return mul * sgn(e) / (fabsf(e) + 1.f);
    };
    int64_t tail = 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        for (int64_t i = t0; i < n4; i += step) {
            const f32x4 v = ((const f32x4 *)x)[i];
            f32x4 r;
            r.x = d(v.x); r.y = d(v.y); r.z = d(v.z); r.w = d(v.w);
            if (accumulate) r += ((const f32x4 *)gx)[i];
            ((f32x4 *)gx)[i] = r;
        }
        tail = n4 << 2;
    }
    for (int64_t i = tail + t0; i < n; i += step) {
        const float r = d(x[i]);
        gx[i] = accumulate ? gx[i] + r : r;
    }
}

int check_crit(const char *what, int crit) {
    TNR_REQUIRE(crit >= CRIT_L1 && crit <= CRIT_CLIPL1, "%s: unknown criterion %d", what, crit);
    return TNR_OK;
}

// K x K host taps -> the centred 15 x 15 table, flipped in both axes for the adjoint
int make_taps(const char *what, const float *taps, int K, int flip, FilterTaps *t) {
    TNR_REQUIRE(taps && K >= 1 && K <= FK && (K & 1), "%s: the filter must have an odd number of taps per side <= %d (got %d)", what, FK, K);
    for (int i = 0; i < FK * FK; ++i) t->w[i] = 0.f;
    const int o = (FK - K) / 2;
    for (int r = 0; r < K; ++r)
        for (int q = 0; q < K; ++q) t->w[(o + r) * FK + o + q] = flip ? taps[(K - 1 - r) * K + (K - 1 - q)] : taps[r * K + q];
    return TNR_OK;
}

}  // namespace

extern "C" int64_t tnr_imgloss_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)N * C * tnr_cdiv(H, TH) * tnr_cdiv(W, TW) * (int64_t)sizeof(double);
}

extern "C" int tnr_filter_loss_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout,
                                   const float *taps, int32_t K, int32_t crit, double scale, float *loss, float *dmap, void *ws,
                                   int64_t ws_bytes, void *stream) {
    int64_t blocks;
    int tilesX, tilesY;
    if (int rc = check_batch("filter_loss_fwd", N, C, H, W, layout, TW, TH, &blocks, &tilesX, &tilesY)) return rc;
    if (int rc = check_crit("filter_loss_fwd", crit)) return rc;
    TNR_REQUIRE(x && y && loss, "filter_loss_fwd: null pointer");
    TNR_REQUIRE(ws && ws_bytes >= tnr_imgloss_workspace_bytes(N, C, H, W), "filter_loss_fwd: workspace missing or too small");
    FilterTaps t;
    if (int rc = make_taps("filter_loss_fwd", taps, K, 0, &t)) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(filter_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, s, x, y, make_view(N, C, H, W, layout), t, (int)crit, tilesX,
                       tilesY, (double *)ws, dmap, 0.f, (const float *)nullptr, 0, vec_rows(layout, W, x, y, dmap));
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, s, (const double *)ws, blocks, scale, loss);
    return tnr_check_launch("filter_loss_fwd");
}

extern "C" int tnr_filter_loss_bwd(const float *dmap, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const float *taps, int32_t K,
                                   double scale, const float *gscale, float *gx, int32_t accumulate, void *stream) {
    int64_t blocks;
    int tilesX, tilesY;
    if (int rc = check_batch("filter_loss_bwd", N, C, H, W, layout, TW, TH, &blocks, &tilesX, &tilesY)) return rc;
    TNR_REQUIRE(dmap && gx && dmap != gx, "filter_loss_bwd: null or aliased pointer");
    FilterTaps t;
    if (int rc = make_taps("filter_loss_bwd", taps, K, 1, &t)) return rc;
    hipLaunchKernelGGL(filter_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dmap, (const float *)nullptr,
                       make_view(N, C, H, W, layout), t, 0, tilesX, tilesY, (double *)nullptr, gx, (float)scale, gscale, (int)accumulate,
                       vec_rows(layout, W, dmap, gx, nullptr));
    return tnr_check_launch("filter_loss_bwd");
}

extern "C" int tnr_fd_loss_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t dirs,
                               int32_t crit, double scale, float *loss, void *ws, int64_t ws_bytes, void *stream) {
    int64_t blocks;
    int tilesX, tilesY;
    if (int rc = check_batch("fd_loss_fwd", N, C, H, W, layout, TW, TH, &blocks, &tilesX, &tilesY)) return rc;
    if (int rc = check_crit("fd_loss_fwd", crit)) return rc;
    TNR_REQUIRE(x && loss && (dirs == 2 || dirs == 4), "fd_loss_fwd: null pointer or dirs not 2 / 4");
    TNR_REQUIRE(ws && ws_bytes >= tnr_imgloss_workspace_bytes(N, C, H, W), "fd_loss_fwd: workspace missing or too small");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fd_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, make_view(N, C, H, W, layout), (int)dirs, (int)crit, tilesX,
                       tilesY, (double *)ws, vec_rows(layout, W, x, y, nullptr));
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, s, (const double *)ws, blocks, scale, loss);
    return tnr_check_launch("fd_loss_fwd");
}

extern "C" int tnr_fd_loss_bwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t dirs,
                               int32_t crit, double scale, const float *gscale, float *gx, int32_t accumulate, void *stream) {
    int64_t blocks;
    int tilesX, tilesY;
    if (int rc = check_batch("fd_loss_bwd", N, C, H, W, layout, TW, TH, &blocks, &tilesX, &tilesY)) return rc;
    if (int rc = check_crit("fd_loss_bwd", crit)) return rc;
    TNR_REQUIRE(x && gx && x != gx && (dirs == 2 || dirs == 4), "fd_loss_bwd: null or aliased pointer, or dirs not 2 / 4");
    hipLaunchKernelGGL(fd_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, make_view(N, C, H, W, layout), (int)dirs,
                       (int)crit, tilesX, tilesY, (float)scale, gscale, gx, (int)accumulate, vec_rows(layout, W, x, y, nullptr));
    return tnr_check_launch("fd_loss_bwd");
}

extern "C" int tnr_pointwise_loss_fwd(const float *a, const float *b, int64_t n, int32_t crit, double scale, float *loss, void *ws,
                                      void *stream) {
    TNR_REQUIRE(a && b && loss && ws && n > 0, "pointwise_loss_fwd: bad arguments");
    if (int rc = check_crit("pointwise_loss_fwd", crit)) return rc;
    const int vec = aligned16(a) && aligned16(b);
    int64_t nb = tnr_cdiv64(vec ? tnr_cdiv64(n, 4) : n, 256);
    if (nb > PT_BLOCKS) nb = PT_BLOCKS;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(point_fwd_kernel, dim3((unsigned)nb), dim3(256), 0, s, a, b, n, vec, (int)crit, (double *)ws);
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, s, (const double *)ws, nb, scale, loss);
    return tnr_check_launch("pointwise_loss_fwd");
}

extern "C" int tnr_pointwise_loss_bwd(const float *a, const float *b, int64_t n, int32_t crit, double scale, const float *gscale, float *ga,
                                      int32_t accumulate, void *stream) {
    TNR_REQUIRE(a && b && ga && n > 0, "pointwise_loss_bwd: bad arguments");
    if (int rc = check_crit("pointwise_loss_bwd", crit)) return rc;
    const int vec = aligned16(a) && aligned16(b) && aligned16(ga);
    int64_t nb = tnr_cdiv64(vec ? tnr_cdiv64(n, 4) : n, 256);
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(point_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, a, b, n, vec, (int)crit, (float)scale, gscale, ga,
                       (int)accumulate);
    return tnr_check_launch("pointwise_loss_bwd");
}

extern "C" int tnr_overflow_loss_fwd(const float *x, int64_t n, double scale, float *loss, void *ws, void *stream) {
    TNR_REQUIRE(x && loss && ws && n > 0, "overflow_loss_fwd: bad arguments");
    const int vec = aligned16(x);
    int64_t nb = tnr_cdiv64(vec ? tnr_cdiv64(n, 4) : n, 256);
    if (nb > PT_BLOCKS) nb = PT_BLOCKS;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(overflow_fwd_kernel, dim3((unsigned)nb), dim3(256), 0, s, x, n, vec, (double *)ws);
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, s, (const double *)ws, nb, scale, loss);
    return tnr_check_launch("overflow_loss_fwd");
}

extern "C" int tnr_overflow_loss_bwd(const float *x, int64_t n, double scale, const float *gscale, float *gx, int32_t accumulate,
                                     void *stream) {
    TNR_REQUIRE(x && gx && x != gx && n > 0, "overflow_loss_bwd: bad arguments");
    const int vec = aligned16(x) && aligned16(gx);
    int64_t nb = tnr_cdiv64(vec ? tnr_cdiv64(n, 4) : n, 256);
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(overflow_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, n, vec, (float)scale, gscale, gx,
                       (int)accumulate);
    return tnr_check_launch("overflow_loss_bwd");
}
