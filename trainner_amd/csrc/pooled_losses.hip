// Image-space training losses of the form  box average -> (RGB -> UV) -> criterion -> sum  (codes/models/modules/loss.py: ColorLoss
// :587-597, AverageLoss :601-609, MultiscalePixelLoss :431-454, L1CosineSim :364-384) for fp32 image batches, value and d/dX
// (DESIGN.md section 22).  No pooled image reaches memory.
//
//   pool_fwd_kernel    one thread = one k x k cell of one image, all channels: the box means of x and of y in registers, the UV map
//                      when flagged, the criterion over the cell's channel vector (all in fp64: the launch is bound by its loads),
//                      the block's fp64 partials
//   pool_bwd_kernel    the same cells recomputed; the cell's derivative (through the transposed UV map) times scale / k^2 goes to
//                      each of its k x k pixels.  The cells cut off by the floor (trailing H % k rows, W % k columns) get zeros
//   ms_fwd_kernel      one workgroup = one 64 x 16 band of four 16 x 16-aligned tiles at a time, all channels: x - y (or, for l1cosinesim, x and y)
//                      staged in LDS, the four coarser levels built on chip by 2 x 2 means, every level's criterion times
//                      weight / count into one fp64 partial.  A cell outside floor(H / 2^i) x floor(W / 2^i) counts at no level i
//   ms_bwd_kernel      the pyramid rebuilt, every cell replaced by its derivative times weight / (count 4^i), then every pixel adds
//                      the five cells above it
// Both forwards are ONE launch: a block leaves its partials in its own fp64 slots and takes a ticket; the last block to arrive sums
// the slots in their fixed order and writes the scalar (no float atomics: two runs are bit-identical), then hands the ticket word
// back at zero.
#include "image_tile.h"

namespace {

enum { CRIT_L1COS = TNR_CRIT_L1COS };

constexpr float WR = 0.299f, WB = 0.114f, WG = 0.587f, UC = 0.493f, VC = 0.877f;     // BT.601 (dataops/colors.py:66-157, consts 'uv')
constexpr float COS_EPS = 1e-20f, COS_LAMBDA = 5.f;      // L1CosineSim: nn.CosineSimilarity(dim=1, eps=1e-20), loss_lambda = 5
constexpr int MAXK = 8;                                  // largest pool
// Blocks of the two forwards at most.  Every block ends with a ticket on ONE word.  Measured against the block count at
// 16 x 3 x 512 x 512 (tools/bench_pooled_losses.py --sweep-blocks, profiles/r31a_bench_pooled_losses.txt) the pool forward is fastest
// with one block per CU and the multi-scale forward, which also needs bands in flight, with about 1024; the supposed reason is that
// the tickets serialise.  tnr_pooled_forward_blocks overrides both for such measurements and for tests of the multi-band paths.
constexpr int PB = 256, MSB = 1024;
constexpr int MAX_SLOTS = 4096;                          // fp64 slots of the workspace: the upper end of any override
int g_pool_blocks = PB, g_ms_blocks = MSB;
constexpr int MTW = 64, MTH = 16, LV = 5;                // multi-scale band and levels
constexpr int PYR = 1364;                                // 64 x 16 + 32 x 8 + 16 x 4 + 8 x 2 + 4 x 1 cells per channel

__device__ __forceinline__ int lv_off(int l) { return l == 0 ? 0 : (l == 1 ? 1024 : (l == 2 ? 1280 : (l == 3 ? 1344 : 1360))); }

// The criterion over the K components of one cell: *v0 = sum rho(a - b) (l1cosinesim: sum |a - b|), *v1 = 1 - cos(a, b) (else 0).
// The cosine is a / max(|a|, eps) . b / max(|b|, eps), as the installed torch forms it.
// 1 - cos cancels where the vectors are nearly parallel (every well-trained pixel), so the value's cosine is formed in fp64: in fp32
// each cell would carry an absolute error of an ulp of 1 into a term of size 1e-3.  T = float (cells held in LDS) or double (the
// pooled loss, whose box means are fp64 sums: a value is a mean over few cells, and the fp32 rounding of a k x k sum shows in it).
__device__ __forceinline__ double rho64(double e, int crit) {
    const double a = fabs(e);
    switch (crit) {
    case CRIT_L1: return a;
    case CRIT_L2: return e * e;
    case CRIT_CB: return sqrt(e * e + 1e-12);
    case CRIT_ELASTIC: return (double)0.2f * (e * e) + (double)0.8f * a;          // ElasticLoss keeps its factors in fp32
    default: return fmin(a, 10.0);
    }
}

__device__ __forceinline__ double rho_of(double e, int crit) { return rho64(e, crit); }
__device__ __forceinline__ float rho_of(float e, int crit) { return rho(e, crit); }          // image_tile.h's, in fp32

template <int K, class T>
__device__ __forceinline__ void cell_value(const T (&a)[K], const T (&b)[K], int crit, double *v0, double *v1) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < K; ++c) s += (double)rho_of(a[c] - b[c], crit == CRIT_L1COS ? (int)CRIT_L1 : crit);
    *v0 = s;
    *v1 = 0.0;
    if (crit == CRIT_L1COS) {
        double aa = 0.0, bb = 0.0;
#pragma unroll
        for (int c = 0; c < K; ++c) { aa += (double)a[c] * a[c]; bb += (double)b[c] * b[c]; }
        const double na = fmax(sqrt(aa), (double)COS_EPS), nb = fmax(sqrt(bb), (double)COS_EPS);
        double cs = 0.0;
#pragma unroll
        for (int c = 0; c < K; ++c) cs += (a[c] / na) * (b[c] / nb);
        *v1 = 1.0 - cs;
    }
}

// g = m0 * d v0 / d a + m1 * d v1 / d a.  The clamp of a zero-norm a passes no gradient to its norm.
template <int K>
__device__ __forceinline__ void cell_grad(const float (&a)[K], const float (&b)[K], int crit, float m0, float m1, float (&g)[K]) {
#pragma unroll
    for (int c = 0; c < K; ++c) g[c] = m0 * drho(a[c] - b[c], crit == CRIT_L1COS ? (int)CRIT_L1 : crit);
    if (crit == CRIT_L1COS) {
        float aa = 0.f, bb = 0.f;
#pragma unroll
        for (int c = 0; c < K; ++c) { aa += a[c] * a[c]; bb += b[c] * b[c]; }
        const float ra = sqrtf(aa), na = fmaxf(ra, COS_EPS), nb = fmaxf(sqrtf(bb), COS_EPS);
        float cs = 0.f;
#pragma unroll
        for (int c = 0; c < K; ++c) cs += (a[c] / na) * (b[c] / nb);
        const float through_norm = ra > COS_EPS ? cs : 0.f;
#pragma unroll
        for (int c = 0; c < K; ++c) g[c] -= m1 * ((b[c] / nb - through_norm * (a[c] / na)) / na);
    }
}

__device__ __forceinline__ void to_uv(const float (&p)[3], float (&o)[2]) {
    const float yv = WR * p[0] + WG * p[1] + WB * p[2];
    o[0] = (p[2] - yv) * UC + 0.5f;
    o[1] = (p[0] - yv) * VC + 0.5f;
}

__device__ __forceinline__ void to_uv(const double (&p)[3], double (&o)[2]) {
    const double yv = 0.299 * p[0] + (1 - 0.299 - 0.114) * p[1] + 0.114 * p[2];
    o[0] = (p[2] - yv) * 0.493 + 0.5;
    o[1] = (p[0] - yv) * 0.877 + 0.5;
}

// The block's NS sums into its fp64 slots; the last block to take a ticket adds all slots in a fixed order.  Returns true in that
// block, with out[0 .. NS) valid in thread 0.  256 threads.
template <int NS>
__device__ __forceinline__ bool last_block_sums(const double (&acc)[NS], double *partial, unsigned *ticket, double *sh, double (&out)[NS]) {
    __shared__ int last;
    double r[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) r[j] = tnr_block_sum256(acc[j], sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NS; ++j) __hip_atomic_store(partial + NS * (int64_t)blockIdx.x + j, r[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();                                 // the slots are visible before the ticket is
        last = atomicAdd(ticket, 1u) == gridDim.x - 1u;
    }
    __syncthreads();
    if (!last) return false;
    __threadfence();
    double s[NS] = {};
    for (unsigned i = threadIdx.x; i < gridDim.x; i += 256)
#pragma unroll
        for (int j = 0; j < NS; ++j) s[j] += __hip_atomic_load(partial + NS * (int64_t)i + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int j = 0; j < NS; ++j) out[j] = tnr_block_sum256(s[j], sh);
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // zero for the next launch
    return true;
}

// ---------------------------------------------------------------------------------------------- pooled loss
// the k x k box means of x and y over the cell whose first pixel is at `base`, summed in fp64 (exact for fp32 pixels, so both kernels
// see the same cells whatever the order); vec: k % 4 == 0 and aligned NCHW rows
template <int C>
__device__ __forceinline__ void cell_means(const float *__restrict__ x, const float *__restrict__ y, const ImView &g, int64_t base, int k,
                                           int vec, double (&a)[C], double (&b)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) a[c] = b[c] = 0.0;
    for (int r = 0; r < k; ++r) {
        const int64_t row = base + (int64_t)r * g.sH;
        if (vec) {
            for (int j = 0; j < k; j += 4)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const f32x4 u = *(const f32x4 *)(x + row + j + c * g.sC), v = *(const f32x4 *)(y + row + j + c * g.sC);
                    a[c] += ((double)u.x + (double)u.y) + ((double)u.z + (double)u.w);
                    b[c] += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
                }
        } else {
            for (int j = 0; j < k; ++j)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    a[c] += x[row + (int64_t)j * g.sW + c * g.sC];
                    b[c] += y[row + (int64_t)j * g.sW + c * g.sC];
                }
        }
    }
    const double area = (double)(k * k);
#pragma unroll
    for (int c = 0; c < C; ++c) { a[c] /= area; b[c] /= area; }
}

struct PoolGeo {
    int k, hk, wk, hc, wc;                               // pool; whole cells; cells with the cut ones (ceil)
};

__device__ __forceinline__ void cell_of(int64_t i, int rows, int cols, int *n, int *cy, int *cx) {
    *cx = (int)(i % cols); i /= cols;
    *cy = (int)(i % rows); *n = (int)(i / rows);
}

// loss = s0 * sum v0 + s1 * sum v1 over the N x hk x wk cells
template <int C>
__global__ __launch_bounds__(256) void pool_fwd_kernel(const float *__restrict__ x, const float *__restrict__ y, ImView g, PoolGeo p, int uv,
                                                       int crit, int vec, double s0, double s1, double *partial, unsigned *ticket,
                                                       float *__restrict__ loss) {
    __shared__ double sh[256];
    const int64_t cells = (int64_t)g.N * p.hk * p.wk;
    double acc[2] = {0, 0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
        int n, cy, cx;
        cell_of(i, p.hk, p.wk, &n, &cy, &cx);
        double a[C], b[C], v0 = 0.0, v1 = 0.0;
        cell_means<C>(x, y, g, (int64_t)n * g.sN + (int64_t)cy * p.k * g.sH + (int64_t)cx * p.k * g.sW, p.k, vec, a, b);
        if constexpr (C == 3) {
            if (uv) {
                double ua[2], ub[2];
                to_uv(a, ua); to_uv(b, ub);
                cell_value<2>(ua, ub, crit, &v0, &v1);
            } else {
                cell_value<C>(a, b, crit, &v0, &v1);
            }
        } else {
            cell_value<C>(a, b, crit, &v0, &v1);
        }
        acc[0] += v0; acc[1] += v1;
    }
    double out[2];
    if (last_block_sums<2>(acc, partial, ticket, sh, out) && threadIdx.x == 0) *loss = (float)(out[0] * s0 + out[1] * s1);
}

// gx = or += gscale * (m0 * d sum v0 + m1 * d sum v1) / dx over the N x hc x wc cells, the cut ones included (zeros)
template <int C>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const float *__restrict__ x, const float *__restrict__ y, ImView g, PoolGeo p, int uv,
                                                       int crit, int vec, float m0, float m1, const float *__restrict__ gscale,
                                                       float *__restrict__ gx, int accumulate) {
    const float gs = gscale ? *gscale : 1.f;
    m0 *= gs; m1 *= gs;
    const int64_t cells = (int64_t)g.N * p.hc * p.wc;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
        int n, cy, cx;
        cell_of(i, p.hc, p.wc, &n, &cy, &cx);
        const int i0 = cy * p.k, j0 = cx * p.k;
        const int64_t base = (int64_t)n * g.sN + (int64_t)i0 * g.sH + (int64_t)j0 * g.sW;
        if (cy >= p.hk || cx >= p.wk) {                  // cut off by the floor: no pooled value, no gradient
            if (accumulate) continue;
            for (int r = 0; r < p.k && i0 + r < g.h; ++r)
                for (int j = 0; j < p.k && j0 + j < g.w; ++j)
#pragma unroll
                    for (int c = 0; c < C; ++c) gx[base + (int64_t)r * g.sH + (int64_t)j * g.sW + c * g.sC] = 0.f;
            continue;
        }
        double a64[C], b64[C];
        cell_means<C>(x, y, g, base, p.k, vec, a64, b64);
        float a[C], b[C], G[C];                          // the gradient in fp32, in autograd's order of operations
#pragma unroll
        for (int c = 0; c < C; ++c) { a[c] = (float)a64[c]; b[c] = (float)b64[c]; }
        if constexpr (C == 3) {
            if (uv) {
                float ua[2], ub[2], U[2];
                to_uv(a, ua); to_uv(b, ub);
                cell_grad<2>(ua, ub, crit, m0, m1, U);
                const float gy = -(UC * U[0]) - VC * U[1];                  // the transposed rgb -> uv matrix
                G[0] = WR * gy + VC * U[1];
                G[1] = WG * gy;
                G[2] = WB * gy + UC * U[0];
            } else {
                cell_grad<C>(a, b, crit, m0, m1, G);
            }
        } else {
            cell_grad<C>(a, b, crit, m0, m1, G);
        }
        const float area = (float)(p.k * p.k);           // the pool's adjoint divides last, as autograd's does
#pragma unroll
        for (int c = 0; c < C; ++c) G[c] /= area;
        for (int r = 0; r < p.k; ++r) {
            const int64_t row = base + (int64_t)r * g.sH;
            if (vec) {
                for (int j = 0; j < p.k; j += 4)
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        f32x4 v;
                        v.x = v.y = v.z = v.w = G[c];
                        f32x4 *o = (f32x4 *)(gx + row + j + c * g.sC);
                        if (accumulate) v += *o;
                        *o = v;
                    }
            } else {
                for (int j = 0; j < p.k; ++j)
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const int64_t at = row + (int64_t)j * g.sW + c * g.sC;
                        gx[at] = accumulate ? gx[at] + G[c] : G[c];
                    }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- multi-scale loss
struct MsScale {                                         // per level: weight / count of the difference term and of the cosine term
    double d[LV], c[LV];
};
struct MsMul {                                           // the same divided by 4^level, in fp32, for the gradient
    float d[LV], c[LV];
};

// what stage_tile stores: every channel of x - y, or (BOTH) of x and then of y
template <int C, bool BOTH>
struct MsPixel {
    const float *x, *y;
    int64_t sC;
    template <class V>
    __device__ __forceinline__ void operator()(int64_t a, V (&v)[BOTH ? 2 * C : C]) const {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if constexpr (BOTH) {
                v[c] = *(const V *)(x + a + c * sC);
                v[C + c] = *(const V *)(y + a + c * sC);
            } else {
                v[c] = *(const V *)(x + a + c * sC) - *(const V *)(y + a + c * sC);
            }
        }
    }
};

__device__ __forceinline__ void ms_decode(int b, int tilesX, int tilesY, int *n, int *y0, int *x0) {
    *x0 = (b % tilesX) * MTW; b /= tilesX;
    *y0 = (b % tilesY) * MTH; *n = b / tilesY;
}

// stages the band at level 0 of every plane and builds levels 1 .. 4 by successive 2 x 2 means; ends synchronised
template <int C, bool BOTH>
__device__ __forceinline__ void ms_pyramid(const float *__restrict__ x, const float *__restrict__ y, const ImView &g, int n, int y0, int x0,
                                           int vec, float (*pyr)[PYR]) {
    constexpr int NT = BOTH ? 2 * C : C;
    float *dst[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) dst[t] = pyr[t];
    float *const(&tiles)[NT] = dst;
    stage_tile<MTH, MTW, 0, MTW, 0, MTW>(g, (int64_t)n * g.sN, y0, x0, vec, tiles, MsPixel<C, BOTH>{x, y, g.sC});
    __syncthreads();
    for (int l = 1; l < LV; ++l) {
        const int cols = MTW >> l, cnt = (MTH >> l) * cols, pc = 2 * cols;
        for (int e = threadIdx.x; e < NT * cnt; e += 256) {
            const int t = e / cnt, rem = e - t * cnt, r = rem / cols, q = rem - r * cols;
            const float *s = pyr[t] + lv_off(l - 1) + 2 * r * pc + 2 * q;
            pyr[t][lv_off(l) + rem] = ((s[0] + s[1]) + (s[pc] + s[pc + 1])) * 0.25f;
        }
        __syncthreads();
    }
}

// sum over the levels and the thread's cells of the staged band of weight / count * criterion
template <int C, bool BOTH>
__device__ __forceinline__ double ms_band_value(const float (*pyr)[PYR], const ImView &g, int y0, int x0, int crit, const MsScale &sc) {
    double acc = 0;
    for (int l = 0; l < LV; ++l) {
        const int cols = MTW >> l, cnt = (MTH >> l) * cols;
        for (int e = threadIdx.x; e < cnt; e += 256) {
            const int r = e / cols, q = e - r * cols;
            if ((y0 >> l) + r >= (g.h >> l) || (x0 >> l) + q >= (g.w >> l)) continue;
            const int at = lv_off(l) + e;
            if constexpr (BOTH) {
                float a[C], b[C];
                double v0, v1;
#pragma unroll
                for (int c = 0; c < C; ++c) { a[c] = pyr[c][at]; b[c] = pyr[C + c][at]; }
                cell_value<C>(a, b, crit, &v0, &v1);
                acc += sc.d[l] * v0 + sc.c[l] * v1;
            } else {
                float v = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) v += rho(pyr[c][at], crit);
                acc += sc.d[l] * (double)v;
            }
        }
    }
    return acc;
}

template <int C, bool BOTH>
__global__ __launch_bounds__(256) void ms_fwd_kernel(const float *__restrict__ x, const float *__restrict__ y, ImView g, int crit, int tilesX,
                                                     int tilesY, int vec, MsScale sc, double *partial, unsigned *ticket,
                                                     float *__restrict__ loss) {
    __shared__ __attribute__((aligned(16))) float pyr[BOTH ? 2 * C : C][PYR];
    __shared__ double sh[256];
    double acc[1] = {0};
    for (int band = blockIdx.x; band < g.N * tilesY * tilesX; band += gridDim.x) {          // a few bands per block: fewer tickets
        int n, y0, x0;
        ms_decode(band, tilesX, tilesY, &n, &y0, &x0);
        __syncthreads();                                 // the previous band's cells have been read
        ms_pyramid<C, BOTH>(x, y, g, n, y0, x0, vec, pyr);
        acc[0] += ms_band_value<C, BOTH>(pyr, g, y0, x0, crit, sc);
    }
    double out[1];
    if (last_block_sums<1>(acc, partial, ticket, sh, out) && threadIdx.x == 0) *loss = (float)out[0];
}

template <int C, bool BOTH>
__global__ __launch_bounds__(256) void ms_bwd_kernel(const float *__restrict__ x, const float *__restrict__ y, ImView g, int crit, int tilesX,
                                                     int tilesY, int vec, MsMul mm, const float *__restrict__ gscale, float *__restrict__ gx,
                                                     int accumulate) {
    __shared__ __attribute__((aligned(16))) float pyr[BOTH ? 2 * C : C][PYR];
    const int tid = threadIdx.x;
    int n, y0, x0;
    ms_decode((int)blockIdx.x, tilesX, tilesY, &n, &y0, &x0);
    ms_pyramid<C, BOTH>(x, y, g, n, y0, x0, vec, pyr);
    const float gs = gscale ? *gscale : 1.f;
    for (int l = 0; l < LV; ++l) {                       // every cell -> its derivative (planes 0 .. C - 1), 0 where the floor cut it off
        const int cols = MTW >> l, cnt = (MTH >> l) * cols;
        const float m0 = mm.d[l] * gs, m1 = mm.c[l] * gs;
        for (int e = tid; e < cnt; e += 256) {
            const int r = e / cols, q = e - r * cols;
            const bool in = (y0 >> l) + r < (g.h >> l) && (x0 >> l) + q < (g.w >> l);
            const int at = lv_off(l) + e;
            float G[C];
            if constexpr (BOTH) {
                float a[C], b[C];
#pragma unroll
                for (int c = 0; c < C; ++c) { a[c] = pyr[c][at]; b[c] = pyr[C + c][at]; }
                cell_grad<C>(a, b, crit, m0, m1, G);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) G[c] = m0 * drho(pyr[c][at], crit);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) pyr[c][at] = in ? G[c] : 0.f;
        }
    }
    __syncthreads();
    const int r = tid >> 4, q0 = (tid & 15) * 4, i = y0 + r;
    if (i >= g.h) return;
    const int64_t base = (int64_t)n * g.sN + (int64_t)i * g.sH;
    float out[C][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = q0 + k;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float *p = pyr[c];
            // from the coarsest level down, the order in which autograd hands the levels' gradients on
            out[c][k] = p[r * MTW + q] + (p[1024 + (r >> 1) * 32 + (q >> 1)] + (p[1280 + (r >> 2) * 16 + (q >> 2)] +
                                                                              (p[1344 + (r >> 3) * 8 + (q >> 3)] + p[1360 + (q >> 4)])));
        }
    }
    if (vec && x0 + q0 < g.w) {                          // the thread's four columns are one aligned group inside the image
#pragma unroll
        for (int c = 0; c < C; ++c) {
            f32x4 *o = (f32x4 *)(gx + base + c * g.sC + x0 + q0);
            f32x4 v;
            v.x = out[c][0]; v.y = out[c][1]; v.z = out[c][2]; v.w = out[c][3];
            if (accumulate) v += *o;
            *o = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = x0 + q0 + k;
            if (j >= g.w) continue;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int64_t at = base + c * g.sC + (int64_t)j * g.sW;
                gx[at] = accumulate ? gx[at] + out[c][k] : out[c][k];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- host
int check_pooled_crit(const char *what, int crit) {
    TNR_REQUIRE(crit >= CRIT_L1 && crit <= CRIT_L1COS, "%s: unknown criterion %d", what, crit);
    return TNR_OK;
}

int pool_geometry(const char *what, int N, int C, int H, int W, int layout, int k, int uv, int crit, PoolGeo *p) {
    if (int rc = check_dense(what, N, C, H, W, layout)) return rc;
    if (int rc = check_pooled_crit(what, crit)) return rc;
    TNR_REQUIRE(C <= 4, "%s: at most 4 channels (got %d)", what, C);
    TNR_REQUIRE(k >= 1 && k <= MAXK, "%s: the pool k must be 1 .. %d (got %d)", what, MAXK, k);
    TNR_REQUIRE(!uv || C == 3, "%s: the UV map needs 3 channels (got %d)", what, C);
    TNR_REQUIRE(H >= k && W >= k, "%s: a %d x %d image has no %d x %d cell", what, H, W, k, k);
    p->k = k; p->hk = H / k; p->wk = W / k; p->hc = tnr_cdiv(H, k); p->wc = tnr_cdiv(W, k);
    return TNR_OK;
}

int ms_geometry(const char *what, int N, int C, int H, int W, int layout, int crit, int64_t *blocks, int *tilesX, int *tilesY) {
    if (int rc = check_batch(what, N, 1, H, W, layout, MTW, MTH, blocks, tilesX, tilesY)) return rc;
    if (int rc = check_pooled_crit(what, crit)) return rc;
    TNR_REQUIRE(C <= 4, "%s: at most 4 channels (got %d)", what, C);
    TNR_REQUIRE(H >= 16 && W >= 16, "%s: five levels need min(H, W) >= 16 (got %d x %d)", what, H, W);
    return TNR_OK;
}

constexpr int64_t WS_BYTES = 16 + MAX_SLOTS * (int64_t)sizeof(double);          // the ticket, then the slots

constexpr double MS_W[LV] = {1.0, 0.5, 0.25, 0.125, 0.125};

template <int C, class... A>
void launch_ms_fwd(bool both, int64_t blocks, hipStream_t s, A... a) {
    if (both) hipLaunchKernelGGL((ms_fwd_kernel<C, true>), dim3((unsigned)blocks), dim3(256), 0, s, a...);
    else hipLaunchKernelGGL((ms_fwd_kernel<C, false>), dim3((unsigned)blocks), dim3(256), 0, s, a...);
}

template <int C, class... A>
void launch_ms_bwd(bool both, int64_t blocks, hipStream_t s, A... a) {
    if (both) hipLaunchKernelGGL((ms_bwd_kernel<C, true>), dim3((unsigned)blocks), dim3(256), 0, s, a...);
    else hipLaunchKernelGGL((ms_bwd_kernel<C, false>), dim3((unsigned)blocks), dim3(256), 0, s, a...);
}

}  // namespace

extern "C" int64_t tnr_pooled_workspace_bytes(void) { return WS_BYTES; }

extern "C" int tnr_pooled_forward_blocks(int32_t pool_blocks, int32_t ms_blocks) {
    TNR_REQUIRE(pool_blocks <= MAX_SLOTS / 2 && ms_blocks <= MAX_SLOTS, "pooled_forward_blocks: at most %d (pool) and %d (multi-scale) blocks",
                MAX_SLOTS / 2, MAX_SLOTS);
    g_pool_blocks = pool_blocks > 0 ? pool_blocks : PB;
    g_ms_blocks = ms_blocks > 0 ? ms_blocks : MSB;
    return TNR_OK;
}

extern "C" int tnr_pool_loss_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t k,
                                 int32_t uv, int32_t crit, float *loss, void *ws, int64_t ws_bytes, void *stream) {
    PoolGeo p;
    if (int rc = pool_geometry("pool_loss_fwd", N, C, H, W, layout, k, uv, crit, &p)) return rc;
    TNR_REQUIRE(x && y && loss, "pool_loss_fwd: null pointer");
    TNR_REQUIRE(ws && ws_bytes >= WS_BYTES, "pool_loss_fwd: workspace missing or too small");
    const ImView g = make_view(N, C, H, W, layout);
    const int vec = (k & 3) == 0 && vec_rows(layout, W, x, y, nullptr);
    const int64_t cells = (int64_t)N * p.hk * p.wk;
    int64_t nb = tnr_cdiv64(cells, 256);
    if (nb > g_pool_blocks) nb = g_pool_blocks;
    const int K = uv ? 2 : C;
    const double s0 = 1.0 / ((double)cells * K), s1 = crit == CRIT_L1COS ? (double)COS_LAMBDA / (double)cells : 0.0;
    unsigned *ticket = (unsigned *)ws;
    double *partial = (double *)((char *)ws + 16);
    hipStream_t s = (hipStream_t)stream;
#define TNR_POOL_FWD(CC) \
    hipLaunchKernelGGL(pool_fwd_kernel<CC>, dim3((unsigned)nb), dim3(256), 0, s, x, y, g, p, (int)(uv != 0), (int)crit, vec, s0, s1, partial, ticket, loss)
    switch (C) {
    case 1: TNR_POOL_FWD(1); break;
    case 2: TNR_POOL_FWD(2); break;
    case 3: TNR_POOL_FWD(3); break;
    default: TNR_POOL_FWD(4); break;
    }
#undef TNR_POOL_FWD
    return tnr_check_launch("pool_loss_fwd");
}

extern "C" int tnr_pool_loss_bwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, int32_t k,
                                 int32_t uv, int32_t crit, const float *gscale, float *gx, int32_t accumulate, void *stream) {
    PoolGeo p;
    if (int rc = pool_geometry("pool_loss_bwd", N, C, H, W, layout, k, uv, crit, &p)) return rc;
    TNR_REQUIRE(x && y && gx && gx != x && gx != y, "pool_loss_bwd: null or aliased pointer");
    const ImView g = make_view(N, C, H, W, layout);
    const int vec = (k & 3) == 0 && vec_rows(layout, W, x, y, gx);
    const double cells = (double)N * p.hk * p.wk;
    const int K = uv ? 2 : C;
    const float m0 = (float)(1.0 / (cells * K)), m1 = crit == CRIT_L1COS ? COS_LAMBDA * (float)(1.0 / cells) : 0.f;
    int64_t nb = tnr_cdiv64((int64_t)N * p.hc * p.wc, 256);
    if (nb > 4096) nb = 4096;
    hipStream_t s = (hipStream_t)stream;
#define TNR_POOL_BWD(CC) \
    hipLaunchKernelGGL(pool_bwd_kernel<CC>, dim3((unsigned)nb), dim3(256), 0, s, x, y, g, p, (int)(uv != 0), (int)crit, vec, m0, m1, gscale, gx, (int)(accumulate != 0))
    switch (C) {
    case 1: TNR_POOL_BWD(1); break;
    case 2: TNR_POOL_BWD(2); break;
    case 3: TNR_POOL_BWD(3); break;
    default: TNR_POOL_BWD(4); break;
    }
#undef TNR_POOL_BWD
    return tnr_check_launch("pool_loss_bwd");
}

extern "C" int tnr_multiscale_loss_fwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout,
                                       int32_t crit, float *loss, void *ws, int64_t ws_bytes, void *stream) {
    int64_t blocks;
    int tilesX, tilesY;
    if (int rc = ms_geometry("multiscale_loss_fwd", N, C, H, W, layout, crit, &blocks, &tilesX, &tilesY)) return rc;
    TNR_REQUIRE(x && y && loss, "multiscale_loss_fwd: null pointer");
    TNR_REQUIRE(ws && ws_bytes >= WS_BYTES, "multiscale_loss_fwd: workspace missing or too small");
    const ImView g = make_view(N, C, H, W, layout);
    const int vec = vec_rows(layout, W, x, y, nullptr);
    MsScale sc;
    for (int l = 0; l < LV; ++l) {
        const double cells = (double)N * (H >> l) * (W >> l);
        sc.d[l] = MS_W[l] / (cells * C);
        sc.c[l] = crit == CRIT_L1COS ? MS_W[l] * (double)COS_LAMBDA / cells : 0.0;
    }
    unsigned *ticket = (unsigned *)ws;
    double *partial = (double *)((char *)ws + 16);
    hipStream_t s = (hipStream_t)stream;
    const bool both = crit == CRIT_L1COS;
    if (blocks > g_ms_blocks) blocks = g_ms_blocks;      // a block takes every g_ms_blocks-th band
    switch (C) {
    case 1: launch_ms_fwd<1>(both, blocks, s, x, y, g, (int)crit, tilesX, tilesY, vec, sc, partial, ticket, loss); break;
    case 2: launch_ms_fwd<2>(both, blocks, s, x, y, g, (int)crit, tilesX, tilesY, vec, sc, partial, ticket, loss); break;
    case 3: launch_ms_fwd<3>(both, blocks, s, x, y, g, (int)crit, tilesX, tilesY, vec, sc, partial, ticket, loss); break;
    default: launch_ms_fwd<4>(both, blocks, s, x, y, g, (int)crit, tilesX, tilesY, vec, sc, partial, ticket, loss); break;
    }
    return tnr_check_launch("multiscale_loss_fwd");
}

extern "C" int tnr_multiscale_loss_bwd(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout,
                                       int32_t crit, const float *gscale, float *gx, int32_t accumulate, void *stream) {
    int64_t blocks;
    int tilesX, tilesY;
    if (int rc = ms_geometry("multiscale_loss_bwd", N, C, H, W, layout, crit, &blocks, &tilesX, &tilesY)) return rc;
    TNR_REQUIRE(x && y && gx && gx != x && gx != y, "multiscale_loss_bwd: null or aliased pointer");
    const ImView g = make_view(N, C, H, W, layout);
    const int vec = vec_rows(layout, W, x, y, gx);
    MsMul mm;
    for (int l = 0; l < LV; ++l) {
        const double cells = (double)N * (H >> l) * (W >> l), area = (double)(1 << (2 * l));
        mm.d[l] = (float)(MS_W[l] / (cells * C * area));
        mm.c[l] = crit == CRIT_L1COS ? COS_LAMBDA * (float)(1.0 / cells) * (float)(MS_W[l] / area) : 0.f;          // w / 4^l is exact
    }
    hipStream_t s = (hipStream_t)stream;
    const bool both = crit == CRIT_L1COS;
    const int acc = accumulate != 0;
    switch (C) {
    case 1: launch_ms_bwd<1>(both, blocks, s, x, y, g, (int)crit, tilesX, tilesY, vec, mm, gscale, gx, acc); break;
    case 2: launch_ms_bwd<2>(both, blocks, s, x, y, g, (int)crit, tilesX, tilesY, vec, mm, gscale, gx, acc); break;
    case 3: launch_ms_bwd<3>(both, blocks, s, x, y, g, (int)crit, tilesX, tilesY, vec, mm, gscale, gx, acc); break;
    default: launch_ms_bwd<4>(both, blocks, s, x, y, g, (int)crit, tilesX, tilesY, vec, mm, gscale, gx, acc); break;
    }
    return tnr_check_launch("multiscale_loss_bwd");
}
