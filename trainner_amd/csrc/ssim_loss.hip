// SSIM / MS-SSIM training losses (codes/models/modules/ssim.py, dataops/filters.py:417-448) for fp32 image batches in [0, 1]:
// value and d/dX, fused so that nothing but X, Y and gX crosses HBM at full size.
//
//   ssim_fwd_kernel      one workgroup = one 32 x 32 tile of the SSIM map of one (n, c) plane: X and Y with their K-1 halo are
//                        staged in LDS once, the five moment maps (X, Y, XX, YY, XY) take the row pass and the column pass inside
//                        the workgroup, only {sum ssim_map, sum cs_map} of the tile leaves (fp64, one slot per block)
//   ssim_sum_kernel      per image: the blocks' partials in a fixed order -> {sum ssim_map, sum cs_map}
//   ssim_bwd_kernel      one workgroup = one 16 x 32 tile of gX: moments recomputed on the tile with a DOUBLE halo (2(K-1)), the three
//                        coefficient maps formed in LDS, then the transposed window (full correlation), row pass and column pass
//   pool_fwd/bwd_kernel  F.avg_pool2d(kernel 2, padding (H % 2, W % 2), count_include_pad) between MS-SSIM levels, X and Y together
//   combine_kernel       relu, powers, product over levels, batch mean; the per-image scalars the backward launches read
//
// All reductions are fixed-order (per-block slots, then one block per image): a step is reproducible run to run.  No float atomics.
#include "image_tile.h"

namespace {

constexpr int SS_KMAX = 11;      // window taps (odd, <= 11)
constexpr int SS_MAXLEV = 8;     // MS-SSIM levels

struct SsWin {
    float w[SS_KMAX];
    int K;
};
struct SsLevels {
    double count[SS_MAXLEV];     // elements per image of the level's maps (C * oh * ow)
    double expo[SS_MAXLEV];      // exponent of the level's factor
    int levels;
};

// the five moments at one map position -> the two maps' values (ssim.py:160-186); s1neg: the sigma1_sq clamp acted
struct SsPoint {
    float lum, cs, B1, B2;
    bool s1neg;
};
__device__ __forceinline__ SsPoint ss_point(float mu1, float mu2, float e11, float e22, float e12, float C1, float C2) {
    const float mu1sq = mu1 * mu1, mu2sq = mu2 * mu2, mu12 = mu1 * mu2;
    float s1 = e11 - mu1sq, s2 = e22 - mu2sq;
    const float s12 = e12 - mu12;
    SsPoint p;
    p.s1neg = s1 < 0.f;
    if (s1 < 0.f) s1 = 0.f;
    if (s2 < 0.f) s2 = 0.f;
    p.B2 = s1 + s2 + C2;
    p.cs = (2.f * s12 + C2) / p.B2;
    p.B1 = mu1sq + mu2sq + C1;
    p.lum = (2.f * mu12 + C1) / p.B1;
    return p;
}

constexpr int FT = 32;                                  // forward tile (FT x FT map positions)
constexpr int FI = FT + SS_KMAX - 1;

__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float *__restrict__ X, const float *__restrict__ Y, ImView g, SsWin win,
                                                       float C1, float C2, int tilesX, int tilesY, double *__restrict__ partial) {
    __shared__ float sX[FI * FI], sY[FI * FI];
    __shared__ float sR[5][FI * FT];
    __shared__ double sh[256];
    const int K = win.K, tid = threadIdx.x;
    int n, c, y0, x0;
    tile_of_block<FT, FT>(g, tilesX, tilesY, &n, &c, &y0, &x0);
    const int oh = g.h - K + 1, ow = g.w - K + 1;
    const int th = min(FT, oh - y0), tw = min(FT, ow - x0);
    const int ih = th + K - 1, iw = tw + K - 1;          // rows y0 .. y0+ih-1 <= h-1, columns likewise: all inside the region
    const int64_t base = g.off + (int64_t)n * g.sN + (int64_t)c * g.sC;
    for (int i = tid; i < ih * iw; i += 256) {
        const int r = i / iw, q = i - r * iw;
        const int64_t a = base + (int64_t)(y0 + r) * g.sH + (int64_t)(x0 + q) * g.sW;
        sX[r * FI + q] = X[a];
        sY[r * FI + q] = Y[a];
    }
    __syncthreads();
    for (int i = tid; i < ih * FT; i += 256) {           // row pass (filters.py:446: along W first)
        const int r = i / FT, col = i % FT;
        if (col >= tw) continue;
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
        for (int k = 0; k < K; ++k) {
            const float wk = win.w[k], x = sX[r * FI + col + k], y = sY[r * FI + col + k];
            m1 = fmaf(wk, x, m1);
            m2 = fmaf(wk, y, m2);
            e11 = fmaf(wk, x * x, e11);
            e22 = fmaf(wk, y * y, e22);
            e12 = fmaf(wk, x * y, e12);
        }
        sR[0][i] = m1; sR[1][i] = m2; sR[2][i] = e11; sR[3][i] = e22; sR[4][i] = e12;
    }
    __syncthreads();
    double as = 0, ac = 0;
    for (int i = tid; i < th * FT; i += 256) {           // column pass, then the maps
        const int r = i / FT, col = i % FT;
        if (col >= tw) continue;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < K; ++k) {
            const float wk = win.w[k];
#pragma unroll
            for (int j = 0; j < 5; ++j) m[j] = fmaf(wk, sR[j][(r + k) * FT + col], m[j]);
        }
        const SsPoint p = ss_point(m[0], m[1], m[2], m[3], m[4], C1, C2);
        as += (double)(p.lum * p.cs);
        ac += (double)p.cs;
    }
    as = tnr_block_sum256(as, sh);
    ac = tnr_block_sum256(ac, sh);
    if (tid == 0) {
        partial[(size_t)blockIdx.x * 2] = as;
        partial[(size_t)blockIdx.x * 2 + 1] = ac;
    }
}

__global__ __launch_bounds__(256) void ssim_sum_kernel(const double *__restrict__ partial, int per_image, double *__restrict__ sums) {
    __shared__ double sh[256];
    double a[2];
    sum_partials<2>(partial + (size_t)blockIdx.x * per_image * 2, per_image, sh, a);
    if (threadIdx.x == 0) {
        sums[blockIdx.x * 2] = a[0];
        sums[blockIdx.x * 2 + 1] = a[1];
    }
}

constexpr int BH = 16, BW = 32;                          // backward tile of gX
constexpr int BCH = BH + SS_KMAX - 1, BCW = BW + SS_KMAX - 1;            // coefficient tile (one halo)
constexpr int BIH = BH + 2 * SS_KMAX - 2, BIW = BW + 2 * SS_KMAX - 2;    // input tile (double halo)

__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float *__restrict__ X, const float *__restrict__ Y, ImView g, SsWin win,
                                                       float C1, float C2, const float *__restrict__ coef,
                                                       const float *__restrict__ gscale, float *__restrict__ gX, int accumulate,
                                                       int shave, int tilesX, int tilesY) {
    __shared__ float sX[BIH * BIW], sY[BIH * BIW];
    __shared__ float sR[5][BIH * BCW];                   // row-passed moments; later the row-passed coefficient maps
    __shared__ float sC[3][BCH * BCW];
    const int K = win.K, tid = threadIdx.x;
    int n, c, y0, x0;
    tile_of_block<BW, BH>(g, tilesX, tilesY, &n, &c, &y0, &x0);
    const int oh = g.h - K + 1, ow = g.w - K + 1;
    const int H = g.h + 2 * shave, W = g.w + 2 * shave;
    const int ry0 = y0 - shave, rx0 = x0 - shave;                // tile origin in region coordinates (may be negative)
    const int iy0 = ry0 - (K - 1), ix0 = rx0 - (K - 1);          // origin of the input tile and of the coefficient tile
    const int ih = BH + 2 * K - 2, iw = BW + 2 * K - 2, ch = BH + K - 1, cw = BW + K - 1;
    const int64_t base = g.off + (int64_t)n * g.sN + (int64_t)c * g.sC;
    const float gs = gscale ? *gscale : 1.f;
    const float ws = coef[2 * n] * gs, wc = coef[2 * n + 1] * gs;
    for (int i = tid; i < ih * iw; i += 256) {
        const int r = i / iw, q = i - r * iw;
        const int y = iy0 + r, x = ix0 + q;
        float vx = 0.f, vy = 0.f;
        if (y >= 0 && y < g.h && x >= 0 && x < g.w) {
            const int64_t a = base + (int64_t)y * g.sH + (int64_t)x * g.sW;
            vx = X[a];
            vy = Y[a];
        }
        sX[r * BIW + q] = vx;
        sY[r * BIW + q] = vy;
    }
    __syncthreads();
    for (int i = tid; i < ih * cw; i += 256) {           // row pass of the moments, exactly the forward's expression
        const int r = i / cw, col = i - r * cw;
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
        for (int k = 0; k < K; ++k) {
            const float wk = win.w[k], x = sX[r * BIW + col + k], y = sY[r * BIW + col + k];
            m1 = fmaf(wk, x, m1);
            m2 = fmaf(wk, y, m2);
            e11 = fmaf(wk, x * x, e11);
            e22 = fmaf(wk, y * y, e22);
            e12 = fmaf(wk, x * y, e12);
        }
        const int o = r * BCW + col;
        sR[0][o] = m1; sR[1][o] = m2; sR[2][o] = e11; sR[3][o] = e22; sR[4][o] = e12;
    }
    __syncthreads();
    for (int i = tid; i < ch * cw; i += 256) {           // column pass -> coefficient maps at map position (iy0 + r, ix0 + col)
        const int r = i / cw, col = i - r * cw;
        const int qy = iy0 + r, qx = ix0 + col;
        float u = 0.f, bb = 0.f, cc = 0.f;
        if (qy >= 0 && qy < oh && qx >= 0 && qx < ow) {
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < K; ++k) {
                const float wk = win.w[k];
#pragma unroll
                for (int j = 0; j < 5; ++j) m[j] = fmaf(wk, sR[j][(r + k) * BCW + col], m[j]);
            }
            const SsPoint p = ss_point(m[0], m[1], m[2], m[3], m[4], C1, C2);
            const float dcs = ws * p.lum + wc;                              // d loss / d cs_map
            cc = dcs * 2.f / p.B2;                                          // d / d sigma12
            bb = p.s1neg ? 0.f : -dcs * p.cs / p.B2;                        // d / d sigma1_sq (0 where the clamp acted)
            const float a = ws * p.cs * 2.f * (m[1] - p.lum * m[0]) / p.B1; // d / d mu1 through the luminance term
            u = a - 2.f * m[0] * bb - m[1] * cc;
        }
        const int o = r * BCW + col;
        sC[0][o] = u; sC[1][o] = bb; sC[2][o] = cc;
    }
    __syncthreads();
    float *sT = &sR[0][0];                               // [3][ch * BW]: 3 * 26 * 32 floats, inside sR
    for (int i = tid; i < ch * BW; i += 256) {           // transposed window, row pass: T[p] = sum_k w[k] coef[p - k]
        const int r = i / BW, col = i % BW;
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
        for (int k = 0; k < K; ++k) {
            const float wk = win.w[k];
            const int o = r * BCW + col + K - 1 - k;
            t0 = fmaf(wk, sC[0][o], t0);
            t1 = fmaf(wk, sC[1][o], t1);
            t2 = fmaf(wk, sC[2][o], t2);
        }
        sT[i] = t0; sT[BCH * BW + i] = t1; sT[2 * BCH * BW + i] = t2;
    }
    __syncthreads();
    float *gplane = gX + (int64_t)n * g.sN + (int64_t)c * g.sC;
    for (int i = tid; i < BH * BW; i += 256) {           // column pass and the three terms of gX
        const int r = i / BW, col = i % BW;
        const int fy = y0 + r, fx = x0 + col;              // full-image coordinates
        if (fy >= H || fx >= W) continue;
        const int py = fy - shave, px = fx - shave;
        const int64_t a = (int64_t)fy * g.sH + (int64_t)fx * g.sW;
        if (py < 0 || py >= g.h || px < 0 || px >= g.w) {            // the shaved border carries no gradient
            if (!accumulate) gplane[a] = 0.f;
            continue;
        }
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
        for (int k = 0; k < K; ++k) {
            const float wk = win.w[k];
            const int o = (r + K - 1 - k) * BW + col;
            t0 = fmaf(wk, sT[o], t0);
            t1 = fmaf(wk, sT[BCH * BW + o], t1);
            t2 = fmaf(wk, sT[2 * BCH * BW + o], t2);
        }
        const int s = (r + K - 1) * BIW + col + K - 1;
        const float gv = t0 + 2.f * sX[s] * t1 + sY[s] * t2;
        gplane[a] = accumulate ? gplane[a] + gv : gv;
    }
}

__global__ void pool_fwd_kernel(const float *__restrict__ X, const float *__restrict__ Y, ImView g, int ho, int wo,
                                float *__restrict__ Xo, float *__restrict__ Yo) {
    const int64_t total = (int64_t)g.N * g.C * ho * wo;
    const int ph = g.h & 1, pw = g.w & 1;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(e % wo), oy = (int)((e / wo) % ho);
        const int64_t nc = e / ((int64_t)wo * ho);
        const int c = (int)(nc % g.C), n = (int)(nc / g.C);
        const int64_t base = g.off + (int64_t)n * g.sN + (int64_t)c * g.sC;
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int y = 2 * oy - ph + dy, x = 2 * ox - pw + dx;
                if (y >= 0 && y < g.h && x >= 0 && x < g.w) {       // padded zeros count in the divisor (count_include_pad)
                    const int64_t a = base + (int64_t)y * g.sH + (int64_t)x * g.sW;
                    sx += X[a];
                    sy += Y[a];
                }
            }
        Xo[e] = sx * 0.25f;
        Yo[e] = sy * 0.25f;
    }
}

__global__ void pool_bwd_kernel(const float *__restrict__ gc, ImView g, int ho, int wo, float *__restrict__ gf) {
    const int64_t total = (int64_t)g.N * g.C * g.h * g.w;
    const int ph = g.h & 1, pw = g.w & 1;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(e % g.w), y = (int)((e / g.w) % g.h);
        const int64_t nc = e / ((int64_t)g.w * g.h);
        const int c = (int)(nc % g.C), n = (int)(nc / g.C);
        const int64_t a = g.off + (int64_t)n * g.sN + (int64_t)c * g.sC + (int64_t)y * g.sH + (int64_t)x * g.sW;
        gf[a] += 0.25f * gc[(nc * ho + (y + ph) / 2) * wo + (x + pw) / 2];
    }
}

// mode 0: SSIM, the mean of the map over the batch.  mode 1: MS-SSIM with normalize='relu', option 1 (ssim.py:394-399).
__global__ __launch_bounds__(256) void combine_kernel(const double *__restrict__ sums, int N, SsLevels lv, int mode,
                                                      float *__restrict__ value, float *__restrict__ coef) {
    __shared__ double sh[256];
    const int L = lv.levels;
    double acc = 0;
    for (int n = threadIdx.x; n < N; n += 256) {
        if (mode == 0) {
            acc += sums[2 * n] / lv.count[0];
            coef[2 * n] = (float)(1.0 / (lv.count[0] * (double)N));
            coef[2 * n + 1] = 0.f;
            continue;
        }
        double f[SS_MAXLEV], ms = 1.0;
        for (int l = 0; l < L; ++l) {
            const double v = sums[((size_t)l * N + n) * 2 + (l == L - 1 ? 0 : 1)] / lv.count[l];
            f[l] = v > 0.0 ? v : 0.0;                                // relu
            ms *= f[l] > 0.0 ? pow(f[l], lv.expo[l]) : 0.0;
        }
        acc += ms;
        for (int l = 0; l < L; ++l) {
            // a factor the relu zeroed makes the image's value 0 and every one of its gradients 0 (never inf * 0)
            const double d = ms > 0.0 ? lv.expo[l] * ms / f[l] / (lv.count[l] * (double)N) : 0.0;
            coef[((size_t)l * N + n) * 2 + 0] = l == L - 1 ? (float)d : 0.f;
            coef[((size_t)l * N + n) * 2 + 1] = l == L - 1 ? 0.f : (float)d;
        }
    }
    acc = tnr_block_sum256(acc, sh);
    if (threadIdx.x == 0) *value = (float)(acc / (double)N);
}

// SSIM's conditions on top of the dense-batch check: both operands, 1..4 channels, something left after the shave
int check_image(const char *what, const void *x, const void *y, int N, int C, int H, int W, int layout, int shave) {
    TNR_REQUIRE(x && y, "%s: null pointer", what);
    if (int rc = check_dense(what, N, C, H, W, layout)) return rc;
    TNR_REQUIRE(C <= 4, "%s: bad shape %d x %d x %d x %d (1..4 channels)", what, N, C, H, W);
    TNR_REQUIRE(shave >= 0 && H - 2 * shave >= 1 && W - 2 * shave >= 1, "%s: nothing left of %d x %d after shave %d", what, H, W, shave);
    return TNR_OK;
}

int make_window(const char *what, const float *taps, int K, int h, int w, SsWin *win) {
    TNR_REQUIRE(taps && K >= 1 && K <= SS_KMAX && (K & 1), "%s: the window must have an odd number of taps <= %d (got %d)", what, SS_KMAX, K);
    TNR_REQUIRE(K <= h && K <= w, "%s: a %d-tap window does not fit a %d x %d image", what, K, h, w);
    for (int k = 0; k < SS_KMAX; ++k) win->w[k] = k < K ? taps[k] : 0.f;
    win->K = K;
    return TNR_OK;
}

unsigned pool_grid(int64_t n) {
    const int64_t b = tnr_cdiv64(n, 256);
    return (unsigned)(b > 8192 ? 8192 : b);
}

}  // namespace

extern "C" int64_t tnr_ssim_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t shave, int32_t K) {
    const int oh = H - 2 * shave - K + 1, ow = W - 2 * shave - K + 1;
    if (N <= 0 || C <= 0 || oh <= 0 || ow <= 0) return 0;
    return (int64_t)N * C * tnr_cdiv(oh, FT) * tnr_cdiv(ow, FT) * 2 * (int64_t)sizeof(double);
}

extern "C" int tnr_ssim_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t shave,
                            const float *taps, int32_t K, float C1, float C2, double *sums, void *ws, int64_t ws_bytes, void *stream) {
    if (int rc = check_image("ssim_fwd", x, y, N, C, H, W, layout, shave)) return rc;
    const ImView g = make_view(N, C, H, W, layout, shave);
    SsWin win;
    if (int rc = make_window("ssim_fwd", taps, K, g.h, g.w, &win)) return rc;
    TNR_REQUIRE(sums && ws && ws_bytes >= tnr_ssim_workspace_bytes(N, C, H, W, shave, K), "ssim_fwd: workspace missing or too small");
    int64_t blocks;
    int tilesX, tilesY;
    if (int rc = check_batch("ssim_fwd", N, C, g.h - K + 1, g.w - K + 1, layout, FT, FT, &blocks, &tilesX, &tilesY)) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ssim_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, g, win, C1, C2, tilesX, tilesY, (double *)ws);
    hipLaunchKernelGGL(ssim_sum_kernel, dim3(N), dim3(256), 0, s, (const double *)ws, C * tilesY * tilesX, sums);
    return tnr_check_launch("ssim_fwd");
}

extern "C" int tnr_ssim_bwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t shave,
                            const float *taps, int32_t K, float C1, float C2, const float *coef, const float *gscale, float *gx,
                            int32_t accumulate, void *stream) {
    if (int rc = check_image("ssim_bwd", x, y, N, C, H, W, layout, shave)) return rc;
    const ImView g = make_view(N, C, H, W, layout, shave);
    SsWin win;
    if (int rc = make_window("ssim_bwd", taps, K, g.h, g.w, &win)) return rc;
    TNR_REQUIRE(coef && gx, "ssim_bwd: null pointer");
    int64_t blocks;
    int tilesX, tilesY;
    if (int rc = check_batch("ssim_bwd", N, C, H, W, layout, BW, BH, &blocks, &tilesX, &tilesY)) return rc;
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, g, win, C1, C2, coef, gscale, gx,
                       (int)accumulate, (int)shave, tilesX, tilesY);
    return tnr_check_launch("ssim_bwd");
}

extern "C" int tnr_avgpool2_pad_dims(int32_t H, int32_t W, int32_t shave, int32_t *Ho, int32_t *Wo) {
    const int h = H - 2 * shave, w = W - 2 * shave;
    TNR_REQUIRE(Ho && Wo && h >= 1 && w >= 1, "avgpool2_pad_dims: bad arguments");
    *Ho = (h + 2 * (h & 1) - 2) / 2 + 1;
    *Wo = (w + 2 * (w & 1) - 2) / 2 + 1;
    return TNR_OK;
}

extern "C" int tnr_avgpool2_pad_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout,
                                    int32_t shave, float *xo, float *yo, void *stream) {
    if (int rc = check_image("avgpool2_pad_fwd", x, y, N, C, H, W, layout, shave)) return rc;
    TNR_REQUIRE(xo && yo, "avgpool2_pad_fwd: null pointer");
    const ImView g = make_view(N, C, H, W, layout, shave);
    TNR_REQUIRE(g.h >= 2 && g.w >= 2, "avgpool2_pad_fwd: a %d x %d image cannot be pooled", g.h, g.w);
    int ho, wo;
    tnr_avgpool2_pad_dims(H, W, shave, &ho, &wo);
    hipLaunchKernelGGL(pool_fwd_kernel, dim3(pool_grid((int64_t)N * C * ho * wo)), dim3(256), 0, (hipStream_t)stream, x, y, g, ho, wo, xo, yo);
    return tnr_check_launch("avgpool2_pad_fwd");
}

extern "C" int tnr_avgpool2_pad_bwd(const float *gcoarse, float *gfine, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout,
                                    int32_t shave, void *stream) {
    if (int rc = check_image("avgpool2_pad_bwd", gcoarse, gfine, N, C, H, W, layout, shave)) return rc;
    const ImView g = make_view(N, C, H, W, layout, shave);
    TNR_REQUIRE(g.h >= 2 && g.w >= 2, "avgpool2_pad_bwd: a %d x %d image cannot be pooled", g.h, g.w);
    int ho, wo;
    tnr_avgpool2_pad_dims(H, W, shave, &ho, &wo);
    hipLaunchKernelGGL(pool_bwd_kernel, dim3(pool_grid((int64_t)N * C * g.h * g.w)), dim3(256), 0, (hipStream_t)stream, gcoarse, g, ho, wo, gfine);
    return tnr_check_launch("avgpool2_pad_bwd");
}

extern "C" int tnr_msssim_combine(const double *sums, int32_t levels, int32_t N, const int64_t *counts, const float *weights,
                                  int32_t mode, float *value, float *coef, void *stream) {
    TNR_REQUIRE(sums && counts && value && coef && N > 0, "msssim_combine: bad arguments");
    TNR_REQUIRE(mode == 0 || mode == 1, "msssim_combine: mode must be 0 (SSIM) or 1 (MS-SSIM, relu, option 1)");
    TNR_REQUIRE(levels >= 1 && levels <= SS_MAXLEV && (mode == 1 || levels == 1), "msssim_combine: bad level count %d", levels);
    TNR_REQUIRE(mode == 0 || weights, "msssim_combine: MS-SSIM needs the level weights");
    SsLevels lv;
    lv.levels = levels;
    for (int l = 0; l < SS_MAXLEV; ++l) {
        lv.count[l] = l < levels ? (double)counts[l] : 1.0;
        TNR_REQUIRE(lv.count[l] > 0, "msssim_combine: empty level %d", l);
        // ssim.py:399: (cs[:-1] ** w[:-1]) * (ssim_last ** w[-1]) broadcasts the last factor over the levels-1 rows before the
        // product, so its exponent is (levels - 1) * w[-1]
        lv.expo[l] = mode == 1 && l < levels ? (l == levels - 1 ? (double)(levels - 1) * (double)weights[l] : (double)weights[l]) : 1.0;
    }
    hipLaunchKernelGGL(combine_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sums, (int)N, lv, (int)mode, value, coef);
    return tnr_check_launch("msssim_combine");
}
