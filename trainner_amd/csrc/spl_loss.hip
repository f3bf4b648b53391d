// Spatial profile losses (codes/models/modules/loss.py: SPLoss :741-757, GPLoss :616-649, CPLoss :652-707) for fp32 image batches, value
// and d/dX.
//
// One SPLoss trace of a tensor D (N x K x H x W) against its counterpart from y is  -(sum of the cosines of every column of every plane
// + the same over rows) / (H N), each cosine formed with F.normalize's clamp  x / max(|x|, 1e-12).  The traces of GPLoss and CPLoss
// run on DERIVED planes of the image pair, grouped into four families selected by a mask:
//     RGB    the C channels themselves (after denorm when flagged)                    C planes
//     YUV    rgb_to_yuv of the image (dataops/colors.py:66, BT.601 constants)         3 planes, C == 3
//     DIMG   dx and dy of the image (dataops/filters.py:722-746)                      2 C planes
//     DYUV   dx and dy of the YUV image                                               6 planes, C == 3
// cpl = RGB | YUV | DYUV, gpl = DIMG.  All selected planes share three launches:
//   stats_kernel     one workgroup = a band of 4 stacked 64 x 16 tiles of one image, one tile at a time: all channels with the one-pixel
//                    halo right and below staged in LDS once; every derived plane is formed in registers and leaves its
//                    (Sxx, Syy, Sxy) per row segment of the tile and per column segment of the band in the workspace (a wave reads
//                    along W; columns are summed over the wave's 4 rows by cross-lane adds, over the 4 waves through LDS and over
//                    the band's tiles in LDS accumulators)
//   finalize_kernel  one thread per line: the segments in a fixed order, the cosine, and the two backward coefficients
//                    alpha = 1 / (nx ny), beta = Sxy / (nx^3 ny)  (nx below eps: alpha = 1 / (eps ny), beta = 0: the clamp passes no
//                    gradient to the norm); the cosines reduced per family, times -1 / (H N)
//   grad_kernel      gather form: a tile of x, y with a one-pixel halo all round plus the coefficients of its rows and columns in LDS;
//                    every derived-plane element's g_d = (alpha_row + alpha_col) y_d - (beta_row + beta_col) x_d, then the adjoints in
//                    registers (the differences with the reference's zeroed last column / row, the transposed YUV matrix, the denorm
//                    mask x 0.5), one store of gx
// All sums are fp64 in a fixed order, no atomics: two runs are bit-identical.
#include "image_tile.h"

namespace {

constexpr int TW = 64, TH = 16;                          // tile; thread = 4 neighbouring columns of one row
constexpr int RT = 4;                                    // tiles per band of the statistics launch (column segments are RT * TH rows)
constexpr int ST = TW + 3;                               // LDS row stride of the staged tiles (66 columns at most)
constexpr int MAXP = 18;                                 // derived planes with every family on (C = 3)
constexpr float WR = 0.299f, WB = 0.114f, WG = 0.587f, UC = 0.493f, VC = 0.877f;
constexpr double EPS = 1e-12;

enum { F_RGB = TNR_SPL_RGB, F_YUV = TNR_SPL_YUV, F_DIMG = TNR_SPL_DIMG, F_DYUV = TNR_SPL_DYUV, F_ALL = 15 };

struct Planes {                                          // first plane of each family (-1: not selected) and their number
    int rgb, yuv, dimg, dyuv, P;
};

__host__ __device__ inline Planes planes_of(int C, int mask) {
    Planes p;
    int n = 0;
    p.rgb = mask & F_RGB ? n : -1;   n += mask & F_RGB ? C : 0;
    p.yuv = mask & F_YUV ? n : -1;   n += mask & F_YUV ? 3 : 0;
    p.dimg = mask & F_DIMG ? n : -1; n += mask & F_DIMG ? 2 * C : 0;
    p.dyuv = mask & F_DYUV ? n : -1; n += mask & F_DYUV ? 6 : 0;
    p.P = n;
    return p;
}

__device__ __forceinline__ int family_of(const Planes &pl, int p) {
    if (pl.dyuv >= 0 && p >= pl.dyuv) return 3;
    if (pl.dimg >= 0 && p >= pl.dimg) return 2;
    if (pl.yuv >= 0 && p >= pl.yuv) return 1;
    return 0;
}

__device__ __forceinline__ float dn1(float v) { return fminf(fmaxf((v + 1.f) * 0.5f, 0.f), 1.f); }

// what stage_tile stores: every channel of x, then of y (denormed on load when flagged), in 2 C tiles
template <int C>
struct AllChannels {
    const float *x, *y;
    int64_t sC;
    int denorm;
    __device__ __forceinline__ float dn(float v) const { return denorm ? dn1(v) : v; }
    __device__ __forceinline__ f32x4 dn(f32x4 v) const {
        if (denorm) { v.x = dn1(v.x); v.y = dn1(v.y); v.z = dn1(v.z); v.w = dn1(v.w); }
        return v;
    }
    template <class V>
    __device__ __forceinline__ void operator()(int64_t a, V (&v)[2 * C]) const {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            v[c] = dn(*(const V *)(x + a + c * sC));
            v[C + c] = dn(*(const V *)(y + a + c * sC));
        }
    }
};

// the K components of the base image of a family group at one staged position: the channels, or their YUV
template <int C, bool YUV>
__device__ __forceinline__ void base_at(const float *s, int at, float (&o)[YUV ? 3 : C]) {
    if constexpr (YUV) {
        const float r = s[at], g = s[(TH + 2) * ST + at], b = s[2 * (TH + 2) * ST + at];
        const float yv = WR * r + WG * g + WB * b;
        o[0] = yv; o[1] = (b - yv) * UC + 0.5f; o[2] = (r - yv) * VC + 0.5f;
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = s[c * (TH + 2) * ST + at];
    }
}

__device__ __forceinline__ void decode_tile(int tilesX, int tilesY, int *n, int *ty, int *tx) {
    int b = blockIdx.x;
    *tx = b % tilesX; b /= tilesX;
    *ty = b % tilesY; *n = b / tilesY;
}

struct StatsOut {
    double *row;                                         // the workspace's row part
    double (*acc)[TW][3];                                // the band's column sums per plane (LDS)
    int n, P, H, W, tilesX, tx, y0, x0;
};

// (Sxx, Syy, Sxy) of plane p over the thread's 4 elements -> the row segment (16 lanes) and the column segments (the wave's 4 rows by
// cross-lane adds, the 4 waves through `red`, added to the band's accumulator).  Elements outside the image come in as 0.
// 256 threads; one barrier: the caller alternates between the two halves of `red`.
__device__ __forceinline__ void plane_sums(const float (&xd)[4], const float (&yd)[4], int p, const StatsOut &o, double (*red)[TW][3]) {
    const int tid = threadIdx.x, row = tid >> 4, col = (tid & 15) * 4, wave = tid >> 6;
    double c[4][3], rs[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double a = xd[j], b = yd[j];
        c[j][0] = a * a; c[j][1] = b * b; c[j][2] = a * b;
#pragma unroll
        for (int k = 0; k < 3; ++k) rs[k] += c[j][k];
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) rs[k] += __shfl_xor(rs[k], m, 64);
    const int yy = o.y0 + row;
    if ((tid & 15) == 0 && yy < o.H) {
        double *w = o.row + ((((int64_t)o.n * o.P + p) * o.H + yy) * o.tilesX + o.tx) * 3;
        w[0] = rs[0]; w[1] = rs[1]; w[2] = rs[2];
    }
#pragma unroll
    for (int m = 16; m < 64; m <<= 1)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) c[j][k] += __shfl_xor(c[j][k], m, 64);
    if ((tid & 63) < 16) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) red[wave][col + j][k] = c[j][k];
    }
    __syncthreads();
    if (tid < TW) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o.acc[p][tid][k] += ((red[0][tid][k] + red[1][tid][k]) + red[2][tid][k]) + red[3][tid][k];
    }
}

// the plain planes (first plane pP, or -1) and the difference planes (dx from pD, dy from pD + K, or -1) of one base image
template <int C, bool YUV>
__device__ __forceinline__ void stats_group(const float *sX, const float *sY, int pP, int pD, const StatsOut &o, double (*red)[4][TW][3],
                                            int *flip) {
    constexpr int K = YUV ? 3 : C;
    const int tid = threadIdx.x, row = tid >> 4, col = (tid & 15) * 4;
    const int yy = o.y0 + row;
    float bx[2][5][K], by[2][5][K];                      // rows yy, yy + 1; columns xx .. xx + 4
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            if (r == 1 && j == 4) continue;
            base_at<C, YUV>(sX, (row + r) * ST + col + j, bx[r][j]);
            base_at<C, YUV>(sY, (row + r) * ST + col + j, by[r][j]);
        }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float xd[4], yd[4];
        if (pP >= 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = yy < o.H && o.x0 + col + j < o.W;
                xd[j] = in ? bx[0][j][k] : 0.f; yd[j] = in ? by[0][j][k] : 0.f;
            }
            plane_sums(xd, yd, pP + k, o, red[*flip]); *flip ^= 1;
        }
        if (pD >= 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {                // dx: zero in the last column
                const bool in = yy < o.H && o.x0 + col + j < o.W - 1;
                xd[j] = in ? bx[0][j + 1][k] - bx[0][j][k] : 0.f; yd[j] = in ? by[0][j + 1][k] - by[0][j][k] : 0.f;
            }
            plane_sums(xd, yd, pD + k, o, red[*flip]); *flip ^= 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {                // dy: zero in the last row
                const bool in = yy < o.H - 1 && o.x0 + col + j < o.W;
                xd[j] = in ? bx[1][j][k] - bx[0][j][k] : 0.f; yd[j] = in ? by[1][j][k] - by[0][j][k] : 0.f;
            }
            plane_sums(xd, yd, pD + K + k, o, red[*flip]); *flip ^= 1;
        }
    }
}

template <int C>
__global__ __launch_bounds__(256) void spl_stats_kernel(const float *__restrict__ x, const float *__restrict__ y, ImView g, int mask, int denorm,
                                                        int tilesX, int bands, double *__restrict__ wsRow, double *__restrict__ wsCol,
                                                        int vec) {
    constexpr int PC = C == 3 ? MAXP : 3 * C;            // planes at most for this channel count
    __shared__ float sT[2 * C][(TH + 2) * ST];           // rows 0 .. TH hold the tile and the halo row below it
    __shared__ double red[2][4][TW][3];
    __shared__ double acc[PC][TW][3];
    const int tid = threadIdx.x;
    const Planes pl = planes_of(C, mask);
    StatsOut o;
    int band;
    o.row = wsRow; o.acc = acc; o.P = pl.P; o.H = g.h; o.W = g.w; o.tilesX = tilesX;
    decode_tile(tilesX, bands, &o.n, &band, &o.tx);
    o.x0 = o.tx * TW;
    if (tid < TW)                                        // column tid of every plane belongs to thread tid alone
        for (int p = 0; p < pl.P; ++p) acc[p][tid][0] = acc[p][tid][1] = acc[p][tid][2] = 0;
    float *dst[2 * C];
#pragma unroll
    for (int t = 0; t < 2 * C; ++t) dst[t] = sT[t];
    float *const(&tiles)[2 * C] = dst;
    for (int it = 0; it < RT; ++it) {
        o.y0 = (band * RT + it) * TH;
        if (o.y0 >= g.h) break;
        __syncthreads();                                 // the tile of the previous round has been read
        // no halo on the left: with 16-byte loads the 17 aligned groups of four columns x0 .. x0 + 67 of every row, column 64 the last kept
        stage_tile<TH + 1, TW + 1, 0, ST, 0, TW + 1>(g, (int64_t)o.n * g.sN, o.y0, o.x0, vec, tiles, AllChannels<C>{x, y, g.sC, denorm});
        __syncthreads();
        int flip = 0;
        stats_group<C, false>(sT[0], sT[C], pl.rgb, pl.dimg, o, red, &flip);
        if constexpr (C == 3) {
            if (mask & (F_YUV | F_DYUV)) stats_group<C, true>(sT[0], sT[C], pl.yuv, pl.dyuv, o, red, &flip);
        }
    }
    if (tid < TW && o.x0 + tid < g.w)
        for (int p = 0; p < pl.P; ++p) {
            double *w = wsCol + ((((int64_t)o.n * pl.P + p) * bands + band) * g.w + o.x0 + tid) * 3;
            w[0] = acc[p][tid][0]; w[1] = acc[p][tid][1]; w[2] = acc[p][tid][2];
        }
}

// One thread per line l of (n, p): rows 0 .. H - 1, then columns.  coef[2 line] = (alpha, beta); part[block][4] = the block's cosine sums
// per family.
__global__ __launch_bounds__(256) void spl_finalize_kernel(const double *__restrict__ wsRow, const double *__restrict__ wsCol, int N, int C,
                                                           int H, int W, int mask, int tilesX, int bands, float *__restrict__ coef,
                                                           double *__restrict__ part) {
    __shared__ double sh[256];
    const Planes pl = planes_of(C, mask);
    const int64_t lines = (int64_t)N * pl.P * (H + W), L = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double fam[4] = {0, 0, 0, 0};
    if (L < lines) {
        const int64_t np = L / (H + W);
        const int l = (int)(L - np * (H + W));
        double s[3] = {0, 0, 0};
        if (l < H) {
            const double *w = wsRow + (np * H + l) * tilesX * 3;
            for (int t = 0; t < tilesX; ++t)
                for (int k = 0; k < 3; ++k) s[k] += w[3 * t + k];
        } else {
            const double *w = wsCol + (np * bands * W + (l - H)) * 3;
            for (int t = 0; t < bands; ++t)
                for (int k = 0; k < 3; ++k) s[k] += w[(int64_t)t * W * 3 + k];
        }
        const double nx = sqrt(s[0]), ny = fmax(sqrt(s[1]), EPS), nxc = fmax(nx, EPS);
        const double alpha = 1.0 / (nxc * ny);
        coef[2 * L] = (float)alpha;
        coef[2 * L + 1] = nx < EPS ? 0.f : (float)(s[2] * alpha / (nxc * nxc));
        fam[family_of(pl, (int)(np % pl.P))] = s[2] * alpha;
    }
    double out[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) out[f] = tnr_block_sum256(fam[f], sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int f = 0; f < 4; ++f) part[4 * (int64_t)blockIdx.x + f] = out[f];
}

// loss[f] = -(family f's cosines) / (H N), loss[4] = their sum
__global__ __launch_bounds__(256) void spl_sum_kernel(const double *__restrict__ part, int64_t count, double scale, float *__restrict__ loss) {
    __shared__ double sh[256];
    double acc[4];
    sum_partials<4>(part, count, sh, acc);
    if (threadIdx.x == 0) {
        for (int f = 0; f < 4; ++f) loss[f] = (float)(acc[f] * scale);
        loss[4] = (float)((((acc[0] + acc[1]) + acc[2]) + acc[3]) * scale);
    }
}

struct GradCtx {
    const float *cf;                                     // staged coefficients: [p][TH + 1 rows from y0 - 1, TW + 1 columns from x0 - 1][2]
    int H, W;
};
constexpr int CFN = TH + 1 + TW + 1;

// g_d of plane p at tile row r / column q (-1 .. ) for the derived values xd, yd
__device__ __forceinline__ float g_of(const GradCtx &c, int p, int r, int q, float xd, float yd) {
    const float *a = c.cf + (p * CFN + r + 1) * 2, *b = c.cf + (p * CFN + TH + 1 + q + 1) * 2;
    return (a[0] + b[0]) * yd - (a[1] + b[1]) * xd;
}

// d (family sums) / d (base image component k) at the pixel (i, j) = tile (r, q): the plain planes times gsP, the difference planes
// through their adjoint (nothing through the zeroed last column of dx and last row of dy) times gsD
template <int C, bool YUV>
__device__ __forceinline__ void grad_group(const float *sX, const float *sY, const GradCtx &c, int pP, int pD, float gsP, float gsD, int r,
                                           int q, int i, int j, float (&G)[YUV ? 3 : C]) {
    constexpr int K = YUV ? 3 : C;
    const int at = (r + 1) * ST + q + 1;
    float x0[K], y0[K];
    base_at<C, YUV>(sX, at, x0);
    base_at<C, YUV>(sY, at, y0);
#pragma unroll
    for (int k = 0; k < K; ++k) G[k] = 0.f;
    if (pP >= 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) G[k] = gsP * g_of(c, pP + k, r, q, x0[k], y0[k]);
    }
    if (pD >= 0) {
        float t[K], xn[K], yn[K];
#pragma unroll
        for (int k = 0; k < K; ++k) t[k] = 0.f;
        if (j >= 1) {                                    // dx at (i, j - 1): the pixel is `right`
            base_at<C, YUV>(sX, at - 1, xn); base_at<C, YUV>(sY, at - 1, yn);
#pragma unroll
            for (int k = 0; k < K; ++k) t[k] += g_of(c, pD + k, r, q - 1, x0[k] - xn[k], y0[k] - yn[k]);
        }
        if (j < c.W - 1) {                               // dx at (i, j): the pixel is the subtrahend
            base_at<C, YUV>(sX, at + 1, xn); base_at<C, YUV>(sY, at + 1, yn);
#pragma unroll
            for (int k = 0; k < K; ++k) t[k] -= g_of(c, pD + k, r, q, xn[k] - x0[k], yn[k] - y0[k]);
        }
        if (i >= 1) {                                    // dy at (i - 1, j): the pixel is `bottom`
            base_at<C, YUV>(sX, at - ST, xn); base_at<C, YUV>(sY, at - ST, yn);
#pragma unroll
            for (int k = 0; k < K; ++k) t[k] += g_of(c, pD + K + k, r - 1, q, x0[k] - xn[k], y0[k] - yn[k]);
        }
        if (i < c.H - 1) {                               // dy at (i, j)
            base_at<C, YUV>(sX, at + ST, xn); base_at<C, YUV>(sY, at + ST, yn);
#pragma unroll
            for (int k = 0; k < K; ++k) t[k] -= g_of(c, pD + K + k, r, q, xn[k] - x0[k], yn[k] - y0[k]);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) G[k] += gsD * t[k];
    }
}

template <int C>
__global__ __launch_bounds__(256) void spl_grad_kernel(const float *__restrict__ x, const float *__restrict__ y, ImView g, int mask, int denorm,
                                                       int tilesX, int tilesY, const float *__restrict__ coef,
                                                       const float *__restrict__ gscale, float scale, float *__restrict__ gx, int accumulate,
                                                       int vec) {
    __shared__ float sT[2 * C][(TH + 2) * ST];
    __shared__ float sCf[MAXP * CFN * 2];
    const int tid = threadIdx.x;
    const Planes pl = planes_of(C, mask);
    int n, ty, tx;
    decode_tile(tilesX, tilesY, &n, &ty, &tx);
    const int y0 = ty * TH, x0 = tx * TW, H = g.h, W = g.w;
    const int64_t base = (int64_t)n * g.sN;
    float *dst[2 * C];
#pragma unroll
    for (int t = 0; t < 2 * C; ++t) dst[t] = sT[t];
    float *const(&tiles)[2 * C] = dst;
    stage_tile<TH + 2, TW + 2, 1, ST, 4, TW + 2>(g, base, y0, x0, vec, tiles, AllChannels<C>{x, y, g.sC, denorm});
    for (int e = tid; e < pl.P * CFN; e += 256) {        // the coefficients of rows y0 - 1 .. y0 + TH - 1 and columns x0 - 1 .. x0 + TW - 1
        const int p = e / CFN, l = e - p * CFN;
        const int line = l <= TH ? y0 - 1 + l : H + x0 - 1 + (l - TH - 1);
        const bool in = l <= TH ? (line >= 0 && line < H) : (line >= H && line < H + W);
        float a = 0.f, b = 0.f;
        if (in) {
            const float *w = coef + (((int64_t)n * pl.P + p) * (H + W) + line) * 2;
            a = w[0]; b = w[1];
        }
        sCf[2 * e] = a; sCf[2 * e + 1] = b;
    }
    __syncthreads();
    float gs[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) gs[f] = gscale ? gscale[f] : 1.f;
    const GradCtx ctx{sCf, H, W};
    const int r = tid >> 4, q0 = (tid & 15) * 4, i = y0 + r;
    if (i >= H) return;
    float out[C][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = x0 + q0 + k;
        float G[C];
#pragma unroll
        for (int c = 0; c < C; ++c) G[c] = 0.f;
        if (j < W) {
            grad_group<C, false>(sT[0], sT[C], ctx, pl.rgb, pl.dimg, gs[0], gs[2], r, q0 + k, i, j, G);
            if constexpr (C == 3) {
                if (mask & (F_YUV | F_DYUV)) {
                    float Y[3];
                    grad_group<C, true>(sT[0], sT[C], ctx, pl.yuv, pl.dyuv, gs[1], gs[3], r, q0 + k, i, j, Y);
                    const float gy = Y[0] - UC * Y[1] - VC * Y[2];          // the transposed rgb -> yuv matrix
                    G[0] += WR * gy + VC * Y[2];
                    G[1] += WG * gy;
                    G[2] += WB * gy + UC * Y[1];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) out[c][k] = scale * G[c];
    }
    if (vec && x0 + q0 < W) {                            // the thread's four columns are one aligned group inside the image
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int64_t a = base + c * g.sC + (int64_t)i * g.sH + x0 + q0;
            f32x4 v;
            v.x = out[c][0]; v.y = out[c][1]; v.z = out[c][2]; v.w = out[c][3];
            if (denorm) {                                // d clamp((x + 1) / 2, 0, 1) / dx = 0.5 on the closed interval
                const f32x4 raw = *(const f32x4 *)(x + a);
                v.x *= raw.x >= -1.f && raw.x <= 1.f ? 0.5f : 0.f; v.y *= raw.y >= -1.f && raw.y <= 1.f ? 0.5f : 0.f;
                v.z *= raw.z >= -1.f && raw.z <= 1.f ? 0.5f : 0.f; v.w *= raw.w >= -1.f && raw.w <= 1.f ? 0.5f : 0.f;
            }
            if (accumulate) v += *(const f32x4 *)(gx + a);
            *(f32x4 *)(gx + a) = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = x0 + q0 + k;
            if (j >= W) continue;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int64_t a = base + c * g.sC + (int64_t)i * g.sH + (int64_t)j * g.sW;
                float v = out[c][k];
                if (denorm) {
                    const float raw = x[a];
                    v *= raw >= -1.f && raw <= 1.f ? 0.5f : 0.f;
                }
                gx[a] = accumulate ? gx[a] + v : v;
            }
        }
    }
}

struct Geometry {
    int64_t blocks, statBlocks, lines, rowSlots, colSlots, finBlocks;
    int tilesX, tilesY, bands;
    Planes pl;
};

int spl_geometry(const char *what, int N, int C, int H, int W, int layout, int mask, Geometry *geo) {
    if (int rc = check_dense(what, N, C, H, W, layout)) return rc;
    TNR_REQUIRE(mask > 0 && mask <= F_ALL, "%s: the family mask must select at least one of RGB 1, YUV 2, DIMG 4, DYUV 8 (got %d)", what, mask);
    TNR_REQUIRE(C <= 4, "%s: at most 4 channels (got %d)", what, C);
    TNR_REQUIRE(!(mask & (F_YUV | F_DYUV)) || C == 3, "%s: the YUV families need 3 channels (got %d)", what, C);
    if (int rc = check_batch(what, N, 1, H, W, layout, TW, TH, &geo->blocks, &geo->tilesX, &geo->tilesY)) return rc;
    geo->pl = planes_of(C, mask);
    geo->lines = (int64_t)N * geo->pl.P * (H + W);
    geo->rowSlots = (int64_t)N * geo->pl.P * H * geo->tilesX;
    geo->bands = tnr_cdiv(geo->tilesY, RT);
    geo->statBlocks = (int64_t)N * geo->bands * geo->tilesX;
    geo->colSlots = (int64_t)N * geo->pl.P * geo->bands * W;
    geo->finBlocks = tnr_cdiv64(geo->lines, 256);
    TNR_REQUIRE(geo->finBlocks < (1ll << 31), "%s: batch too large", what);
    return TNR_OK;
}

int64_t ws_bytes_of(const Geometry &geo) { return ((geo.rowSlots + geo.colSlots) * 3 + geo.finBlocks * 4) * (int64_t)sizeof(double); }

template <int C>
void launch_stats(const Geometry &geo, hipStream_t s, const float *x, const float *y, const ImView &g, int mask, int denorm, double *row,
                  double *col, int vec) {
    hipLaunchKernelGGL(spl_stats_kernel<C>, dim3((unsigned)geo.statBlocks), dim3(256), 0, s, x, y, g, mask, denorm, geo.tilesX, geo.bands, row,
                       col, vec);
}

template <int C>
void launch_grad(const Geometry &geo, hipStream_t s, const float *x, const float *y, const ImView &g, int mask, int denorm, const float *coef,
                 const float *gscale, float scale, float *gx, int accumulate, int vec) {
    hipLaunchKernelGGL(spl_grad_kernel<C>, dim3((unsigned)geo.blocks), dim3(256), 0, s, x, y, g, mask, denorm, geo.tilesX, geo.tilesY, coef, gscale,
                       scale, gx, accumulate, vec);
}

}  // namespace

extern "C" int64_t tnr_spl_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t mask) {
    Geometry geo;
    if (N <= 0 || C <= 0 || C > 4 || H <= 0 || W <= 0 || mask <= 0 || mask > F_ALL) return 0;
    if (spl_geometry("spl_workspace_bytes", N, C, H, W, 0, mask, &geo)) return 0;
    return ws_bytes_of(geo);
}

extern "C" int64_t tnr_spl_coef_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t mask) {
    Geometry geo;
    if (N <= 0 || C <= 0 || C > 4 || H <= 0 || W <= 0 || mask <= 0 || mask > F_ALL) return 0;
    if (spl_geometry("spl_coef_bytes", N, C, H, W, 0, mask, &geo)) return 0;
    return geo.lines * 2 * (int64_t)sizeof(float);
}

extern "C" int tnr_spl_loss_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t mask,
                                int32_t denorm, float *loss, float *coef, void *ws, int64_t ws_bytes, void *stream) {
    Geometry geo;
    if (int rc = spl_geometry("spl_loss_fwd", N, C, H, W, layout, mask, &geo)) return rc;
    TNR_REQUIRE(x && y && loss && coef, "spl_loss_fwd: null pointer");
    TNR_REQUIRE(ws && ws_bytes >= ws_bytes_of(geo), "spl_loss_fwd: workspace missing or too small");
    hipStream_t s = (hipStream_t)stream;
    double *row = (double *)ws, *col = row + geo.rowSlots * 3, *part = col + geo.colSlots * 3;
    const ImView g = make_view(N, C, H, W, layout);
    const int vec = vec_rows(layout, W, x, y, nullptr);
    switch (C) {
    case 1: launch_stats<1>(geo, s, x, y, g, mask, denorm != 0, row, col, vec); break;
    case 2: launch_stats<2>(geo, s, x, y, g, mask, denorm != 0, row, col, vec); break;
    case 3: launch_stats<3>(geo, s, x, y, g, mask, denorm != 0, row, col, vec); break;
    default: launch_stats<4>(geo, s, x, y, g, mask, denorm != 0, row, col, vec); break;
    }
    hipLaunchKernelGGL(spl_finalize_kernel, dim3((unsigned)geo.finBlocks), dim3(256), 0, s, (const double *)row, (const double *)col, (int)N,
                       (int)C, (int)H, (int)W, (int)mask, geo.tilesX, geo.bands, coef, part);
    hipLaunchKernelGGL(spl_sum_kernel, dim3(1), dim3(256), 0, s, (const double *)part, geo.finBlocks, -1.0 / ((double)H * N), loss);
    return tnr_check_launch("spl_loss_fwd");
}

extern "C" int tnr_spl_loss_bwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t mask,
                                int32_t denorm, const float *coef, const float *gscale, float *gx, int32_t accumulate, void *stream) {
    Geometry geo;
    if (int rc = spl_geometry("spl_loss_bwd", N, C, H, W, layout, mask, &geo)) return rc;
    TNR_REQUIRE(x && y && coef && gx && gx != x && gx != y, "spl_loss_bwd: null or aliased pointer");
    const ImView g = make_view(N, C, H, W, layout);
    const int vec = vec_rows(layout, W, x, y, gx);
    const float scale = (float)(-1.0 / ((double)H * N));
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
    case 1: launch_grad<1>(geo, s, x, y, g, mask, denorm != 0, coef, gscale, scale, gx, accumulate != 0, vec); break;
    case 2: launch_grad<2>(geo, s, x, y, g, mask, denorm != 0, coef, gscale, scale, gx, accumulate != 0, vec); break;
    case 3: launch_grad<3>(geo, s, x, y, g, mask, denorm != 0, coef, gscale, scale, gx, accumulate != 0, vec); break;
    default: launch_grad<4>(geo, s, x, y, g, mask, denorm != 0, coef, gscale, scale, gx, accumulate != 0, vec); break;
    }
    return tnr_check_launch("spl_loss_bwd");
}
