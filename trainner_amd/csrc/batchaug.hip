// Batch augmentations on the (target, input) pair of a training step (codes/dataops/batchaug.py: blend, rgb, mixup, cutmix, cutmixup,
// cutblur, cutout).  No op moves a pixel: every output element is a copy of the element at the SAME position of
// one of two sources, or fl(a * x) + fl(b * y) of two of them.  Two kernels:
//
//   batchaug_mix    out = region(x, x2[r[n]], col[n]): the image splits into the inside and the outside of one box (the same box
//                   in every image of the batch), and each region has one of four codes
//                       SELF          x[n, perm[c]]                        bitwise copy
//                       PARTNER       x2[r[n], c]                          bitwise copy
//                       LERP_PARTNER  fl(a x[n, c]) + fl(b x2[r[n], c])
//                       LERP_COLOUR   fl(a x[n, c]) + fl(b col[n, c])      (C = 3)
//                   A region's source is only loaded by the vectors that hold one of its elements, and the lanes of a vector that
//                   straddles a box edge select: a NaN of the partner reaches exactly the elements that read it.
//   batchaug_mask   out = x * (float)mask[n, y / s, x / s], mask uint8 N x (H / s) x (W / s): a real product (-1 * 0 = -0, NaN * 0 =
//                   NaN).  Cutout on the input (s = 1), apply_mask on generated and target, and its own adjoint.
//
// One thread = V consecutive floats of a row (NCHW: W floats of one channel plane; channels-last: W * C floats of one image row) and
// RPT rows; V = 4 with 16-byte accesses when the row length is a multiple of 4 and every pointer is 16-byte aligned, else V = 1.
// blockIdx.z names the plane, so no index is divided by a run-time size.  No atomics, no workspace: two runs are bit-identical.
// The file is compiled with -ffp-contract=off; the pragma below says so where it matters.
#include "image_tile.h"

namespace {

enum { R_SELF = 0, R_PARTNER = 1, R_LERP_PARTNER = 2, R_LERP_COLOUR = 3 };
constexpr int RPT = 4;                                   // rows per thread

struct BaGeo {
    int N, C, H, W;
    int rowlen;                                          // floats of a row: W (NCHW) or W * C (channels-last)
    int tw_log2;                                         // the 256 threads form (1 << tw_log2) columns x (256 >> tw_log2) rows
};

struct BaMix {
    int in_code, out_code;
    int y0, y1, x0, x1;                                  // the box: rows [y0, y1), columns [x0, x1)
    int p0, p1, p2, p3;                                  // out[:, c] reads x[:, p_c]
    float a, b;
};

__device__ __forceinline__ int perm_of(const BaMix &q, int c) { return c == 0 ? q.p0 : (c == 1 ? q.p1 : (c == 2 ? q.p2 : q.p3)); }

template <int V> struct Vec;
template <> struct Vec<1> { typedef float T; };
template <> struct Vec<4> { typedef f32x4 T; };
template <int V> __device__ __forceinline__ float lane(const typename Vec<V>::T &v, int k);
template <> __device__ __forceinline__ float lane<1>(const float &v, int) { return v; }
template <> __device__ __forceinline__ float lane<4>(const f32x4 &v, int k) { return v[k]; }
template <int V> __device__ __forceinline__ void set_lane(typename Vec<V>::T &v, int k, float f);
template <> __device__ __forceinline__ void set_lane<1>(float &v, int, float f) { v = f; }
template <> __device__ __forceinline__ void set_lane<4>(f32x4 &v, int k, float f) { v[k] = f; }

// the thread's first float j of the row and its first image row y; false when the thread has nothing to do
__device__ __forceinline__ bool thread_span(const BaGeo &g, int V, int *j, int *y, int *th) {
    const int tw = 1 << g.tw_log2;
    *th = 256 >> g.tw_log2;
    *j = ((int)blockIdx.x * tw + ((int)threadIdx.x & (tw - 1))) * V;
    *y = (int)blockIdx.y * (*th * RPT) + ((int)threadIdx.x >> g.tw_log2);
    return *j < g.rowlen;
}

// CC = 0: NCHW (blockIdx.z = n * C + c); CC = 1 .. 4: channels-last with CC channels (blockIdx.z = n)
template <int CC, int V>
__global__ __launch_bounds__(256) void batchaug_mix(const float *__restrict__ x, const float *__restrict__ x2, const int *__restrict__ r,
                                                    const float *__restrict__ col, BaGeo g, BaMix q, float *__restrict__ out) {
    typedef typename Vec<V>::T VT;
    int j, y, th;
    if (!thread_span(g, V, &j, &y, &th)) return;
    const int n = CC ? (int)blockIdx.z : (int)blockIdx.z / g.C;
    const int c0 = CC ? 0 : (int)blockIdx.z - n * g.C;
    int rn = r ? r[n] : n;
    rn = rn < 0 ? 0 : (rn >= g.N ? g.N - 1 : rn);        // (the host module checks the permutation; this only keeps the read inside)
    const int64_t plane = (int64_t)g.H * g.rowlen;       // floats of one blockIdx.z plane
    const int64_t ob = (int64_t)blockIdx.z * plane;
    const int64_t xb = CC ? ob : ((int64_t)n * g.C + perm_of(q, c0)) * plane;
    const int64_t pb = CC ? (int64_t)rn * plane : ((int64_t)rn * g.C + c0) * plane;
    // per lane: column, channel, inside the box's columns
    int ck[V];
    bool inx[V];
    bool any_in = false, all_in = true;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int xk = CC ? (j + k) / CC : j + k;
        ck[k] = CC ? (j + k) - xk * CC : c0;
        inx[k] = xk >= q.x0 && xk < q.x1;
        any_in |= inx[k];
        all_in &= inx[k];
    }
    for (int rr = 0; rr < RPT; ++rr, y += th) {
        if (y >= g.H) break;
        const bool iny = y >= q.y0 && y < q.y1;
        const bool has_in = iny && any_in, has_out = !(iny && all_in);
        const bool needx = (has_in && q.in_code != R_PARTNER) || (has_out && q.out_code != R_PARTNER);
        const bool needp = (has_in && (q.in_code == R_PARTNER || q.in_code == R_LERP_PARTNER)) ||
                           (has_out && (q.out_code == R_PARTNER || q.out_code == R_LERP_PARTNER));
        const int64_t off = (int64_t)y * g.rowlen + j;
        VT vx = {}, vp = {};
        if (needx) {
            if (CC && V == 1) vx = *(const VT *)(x + xb + off + (perm_of(q, ck[0]) - ck[0]));      // channels-last permutation: scalar path only
            else vx = *(const VT *)(x + xb + off);
        }
        if (needp) vp = *(const VT *)(x2 + pb + off);
        VT o;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int code = (iny && inx[k]) ? q.in_code : q.out_code;
            const float xv = lane<V>(vx, k), pv = lane<V>(vp, k);
            float v;
            if (code == R_SELF) v = xv;
            else if (code == R_PARTNER) v = pv;
            else {
#pragma clang fp contract(off)
                const float y2 = code == R_LERP_PARTNER ? pv : col[n * 3 + ck[k]];
                const float t0 = q.a * xv, t1 = q.b * y2;          // both products rounded to fp32, then one add
                v = t0 + t1;
            }
            set_lane<V>(o, k, v);
        }
        *(VT *)(out + ob + off) = o;
    }
}

template <int CC, int V>
__global__ __launch_bounds__(256) void batchaug_mask(const float *__restrict__ x, const unsigned char *__restrict__ mask, BaGeo g, int s,
                                                     int shift, float *__restrict__ out) {
    typedef typename Vec<V>::T VT;
    int j, y, th;
    if (!thread_span(g, V, &j, &y, &th)) return;
    const int n = CC ? (int)blockIdx.z : (int)blockIdx.z / g.C;
    const int h = g.H / s, w = g.W / s;
    const unsigned char *mb = mask + (int64_t)n * h * w;
    const int64_t ob = (int64_t)blockIdx.z * g.H * g.rowlen;
    int xs[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int xk = CC ? (j + k) / CC : j + k;
        xs[k] = shift >= 0 ? xk >> shift : xk / s;
    }
    for (int rr = 0; rr < RPT; ++rr, y += th) {
        if (y >= g.H) break;
        const int ys = shift >= 0 ? y >> shift : y / s;
        const unsigned char *mrow = mb + (int64_t)ys * w;
        const int64_t off = (int64_t)y * g.rowlen + j;
        const VT vx = *(const VT *)(x + ob + off);
        VT o;
#pragma unroll
        for (int k = 0; k < V; ++k) set_lane<V>(o, k, lane<V>(vx, k) * (float)mrow[xs[k]]);
        *(VT *)(out + ob + off) = o;
    }
}

// the launch geometry both entries share; vec: 16-byte accesses are possible
int make_geo(const char *what, int N, int C, int H, int W, int layout, bool vec, BaGeo *g, dim3 *grid) {
    if (int rc = check_dense(what, N, C, H, W, layout)) return rc;
    TNR_REQUIRE(C <= 4, "%s: at most 4 channels, got %d", what, C);
    TNR_REQUIRE((int64_t)W * C < (1ll << 30), "%s: rows too long", what);
    g->N = N; g->C = C; g->H = H; g->W = W;
    g->rowlen = layout ? W * C : W;
    const int spans = vec ? g->rowlen / 4 : g->rowlen;
    g->tw_log2 = spans > 32 ? 6 : (spans > 16 ? 5 : 4);
    const int64_t planes = layout ? (int64_t)N : (int64_t)N * C;
    const int gy = tnr_cdiv(H, (256 >> g->tw_log2) * RPT);
    TNR_REQUIRE(planes <= 65535 && gy <= 65535, "%s: batch too large (%lld planes, %d row tiles)", what, (long long)planes, gy);
    *grid = dim3((unsigned)tnr_cdiv(spans, 1 << g->tw_log2), (unsigned)gy, (unsigned)planes);
    return TNR_OK;
}

#define BA_DISPATCH(layout, C, vec, ...)                                                         \
    do {                                                                                         \
        if (vec) {                                                                               \
            constexpr int VV = 4;                                                                \
            switch ((layout) ? (C) : 0) {                                                        \
                case 0: { constexpr int CC = 0; __VA_ARGS__; } break;                            \
                case 1: { constexpr int CC = 1; __VA_ARGS__; } break;                            \
                case 2: { constexpr int CC = 2; __VA_ARGS__; } break;                            \
                case 3: { constexpr int CC = 3; __VA_ARGS__; } break;                            \
                default: { constexpr int CC = 4; __VA_ARGS__; } break;                           \
            }                                                                                    \
        } else {                                                                                 \
            constexpr int VV = 1;                                                                \
            switch ((layout) ? (C) : 0) {                                                        \
                case 0: { constexpr int CC = 0; __VA_ARGS__; } break;                            \
                case 1: { constexpr int CC = 1; __VA_ARGS__; } break;                            \
                case 2: { constexpr int CC = 2; __VA_ARGS__; } break;                            \
                case 3: { constexpr int CC = 3; __VA_ARGS__; } break;                            \
                default: { constexpr int CC = 4; __VA_ARGS__; } break;                           \
            }                                                                                    \
        }                                                                                        \
    } while (0)

bool needs_partner(int code) { return code == R_PARTNER || code == R_LERP_PARTNER; }

}  // namespace

extern "C" int tnr_batchaug_mix(const float *x, const float *x2, const int32_t *r, const float *col, int32_t N, int32_t C, int32_t H,
                                int32_t W, int32_t layout, const int32_t *prm, float a, float b, float *out, void *stream) {
    const char *what = "batchaug_mix";
    TNR_REQUIRE(prm, "%s: null parameter block", what);
    if (int rc = check_dense(what, N, C, H, W, layout)) return rc;
    TNR_REQUIRE(C <= 4, "%s: at most 4 channels, got %d", what, C);
    BaMix q;
    q.in_code = prm[0]; q.out_code = prm[1];
    const int y0 = prm[2], x0 = prm[3], bh = prm[4], bw = prm[5];
    TNR_REQUIRE(q.in_code >= R_SELF && q.in_code <= R_LERP_COLOUR && q.out_code >= R_SELF && q.out_code <= R_LERP_COLOUR,
                "%s: unknown region code (%d, %d)", what, q.in_code, q.out_code);
    TNR_REQUIRE(bh >= 0 && bw >= 0 && y0 >= 0 && x0 >= 0 && (int64_t)y0 + bh <= H && (int64_t)x0 + bw <= W,
                "%s: box %d x %d at (%d, %d) leaves the %d x %d image", what, bh, bw, y0, x0, H, W);
    q.y0 = y0; q.y1 = y0 + bh; q.x0 = x0; q.x1 = bw && bh ? x0 + bw : x0;
    if (!(bw && bh)) q.y1 = q.y0;                        // an empty box: everything is outside
    int p[4] = {0, 1, 2, 3};
    bool ident = true;
    for (int c = 0; c < C; ++c) {
        p[c] = prm[6 + c];
        TNR_REQUIRE(p[c] >= 0 && p[c] < C, "%s: channel permutation entry %d outside [0, %d)", what, p[c], C);
        ident = ident && p[c] == c;
    }
    q.p0 = p[0]; q.p1 = p[1]; q.p2 = p[2]; q.p3 = p[3];
    TNR_REQUIRE(ident || (q.in_code == R_SELF && q.out_code == R_SELF), "%s: a channel permutation goes with SELF regions only", what);
    const bool partner = needs_partner(q.in_code) || needs_partner(q.out_code);
    const bool colour = q.in_code == R_LERP_COLOUR || q.out_code == R_LERP_COLOUR;
    TNR_REQUIRE(!colour || C == 3, "%s: LERP_COLOUR (blend) needs 3 channels, got %d", what, C);
    TNR_REQUIRE(x && out && x != out && (!partner || (x2 && x2 != out)) && (!colour || col), "%s: null or aliased pointer", what);
    q.a = a; q.b = b;
    const int rowlen = layout ? W * C : W;
    const bool vec = (rowlen & 3) == 0 && aligned16(x) && aligned16(out) && (!partner || aligned16(x2)) && !(layout && !ident);
    BaGeo g;
    dim3 grid;
    if (int rc = make_geo(what, N, C, H, W, layout, vec, &g, &grid)) return rc;
    BA_DISPATCH(layout, C, vec, hipLaunchKernelGGL((batchaug_mix<CC, VV>), grid, dim3(256), 0, (hipStream_t)stream, x,
                                                    partner ? x2 : nullptr, (const int *)r, col, g, q, out));
    return tnr_check_launch(what);
}

extern "C" int tnr_batchaug_mask(const float *x, const uint8_t *mask, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout,
                                 int32_t s, float *out, void *stream) {
    const char *what = "batchaug_mask";
    if (int rc = check_dense(what, N, C, H, W, layout)) return rc;
    TNR_REQUIRE(s >= 1 && H % s == 0 && W % s == 0, "%s: scale %d does not divide the %d x %d image", what, s, H, W);
    TNR_REQUIRE(x && mask && out, "%s: null pointer", what);
    const int rowlen = layout ? W * C : W;
    const bool vec = (rowlen & 3) == 0 && aligned16(x) && aligned16(out);
    BaGeo g;
    dim3 grid;
    if (int rc = make_geo(what, N, C, H, W, layout, vec, &g, &grid)) return rc;
    int shift = -1;
    for (int k = 0; k < 31; ++k)
        if (s == (1 << k)) shift = k;
    BA_DISPATCH(layout, C, vec, hipLaunchKernelGGL((batchaug_mask<CC, VV>), grid, dim3(256), 0, (hipStream_t)stream, x,
                                                    (const unsigned char *)mask, g, s, shift, out));
    return tnr_check_launch(what);
}
