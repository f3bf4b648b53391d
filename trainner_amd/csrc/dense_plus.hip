// ESRGAN+ residual paths of a ResidualDenseBlock_5C (network_G `plus: true`, RRDBNet_arch.py:127, 153-158) in WEIGHT space.
//
// With u2 = act(conv2(..)), u4 = act(conv4(..)) and the bias-free 1x1 convolution P (nf -> gc) the block computes
//     x2 = u2 + P x,   x4 = u4 + x2 = u4 + u2 + P x.
// Everything the block adds is linear, P 0 = 0 commutes with the zero padding, so with [x | x1 | u2 | x3 | u4] in the 192-channel
// buffer the block IS a plain dense block with effective weights, per 3x3 tap:
//     W3e[:, x] = W3[:, x] + W3[:, x2] P          W5e[:, x ] = W5[:, x] + (W5[:, x2] + W5[:, x4]) P
//     W4e[:, x] = W4[:, x] + W4[:, x2] P          W5e[:, x2] = W5[:, x2] + W5[:, x4]
// and the convolution kernels never learn of it.  Two launches live here:
//
//   tnr_dense_plus_fold     real conv3..conv5 + P  ->  effective conv3..conv5, every block of a network in one launch
//   tnr_dense_plus_unfold   the adjoint: gradient w.r.t. the effective weights  ->  += the real gradients and dP
//
// Work split (both): one workgroup per (block, layer, tap).  A tap of an OIHW weight is a [cout x cin] matrix with element stride 9;
// the workgroup stages P and the layer's [cout x gc] (fold) or [cout x nf] (unfold) slice of that tap in LDS once, each lane owns
// output elements of the small product and runs ONE fp32 FMA chain per element in ascending reduction order.  The slices no product
// touches move as whole rows with 16-byte accesses, the rows dealt round-robin over the nine tap workgroups of the layer.  The
// products are 32x32x64 / 64x32x64 per tap (~2.3 MFLOP per block): launch latency and the stride-9 gathers decide the time, not the
// arithmetic, so this is vector-ALU code.
#include "common.h"

namespace {
constexpr int DP_THREADS = 256;
constexpr int DP_GC = 32;             // growth channels of the engine's dense blocks
constexpr int DP_NF_MAX = 64;
constexpr int DP_TAPS = 9;

struct PlusGeom {
    int L, tap, cout, cin, x2, x4;
};

__device__ __forceinline__ PlusGeom plus_geom(int job, int nf) {
    PlusGeom q;
    q.L = job / DP_TAPS;              // 0, 1, 2 -> conv3, conv4, conv5
    q.tap = job - q.L * DP_TAPS;
    q.cout = q.L == 2 ? nf : DP_GC;
    q.cin = nf + (2 + q.L) * DP_GC;
    q.x2 = nf + DP_GC;                // first input channel of the x2 group
    q.x4 = nf + 3 * DP_GC;
    return q;
}

// grid (27, blocks)
__global__ __launch_bounds__(DP_THREADS) void dense_plus_fold_kernel(const tnr_dense_plus_item *items, int nf) {
    __shared__ float sP[DP_GC * DP_NF_MAX];            // P[k][ci]
    __shared__ float sA[DP_NF_MAX * (DP_GC + 1)];      // A[co][k]: the tap's W[:, x2] (conv5: W[:, x2] + W[:, x4]), rows padded by one
    const tnr_dense_plus_item &it = items[blockIdx.y];      // (a reference: the per-layer pointers are indexed at run time)
    const PlusGeom q = plus_geom(blockIdx.x, nf);
    const float *w = it.w[q.L];
    float *e = it.eff[q.L];
    const int tid = threadIdx.x;
    for (int i = tid; i < DP_GC * nf; i += DP_THREADS) sP[i] = it.p[i];
    for (int i = tid; i < q.cout * DP_GC; i += DP_THREADS) {
        const int co = i / DP_GC, k = i - co * DP_GC;
        const size_t row = (size_t)co * q.cin;
        float a = w[(row + q.x2 + k) * DP_TAPS + q.tap];
        if (q.L == 2) {
            a = a + w[(row + q.x4 + k) * DP_TAPS + q.tap];
            e[(row + q.x2 + k) * DP_TAPS + q.tap] = a;                  // W5e[:, x2]
        }
        sA[co * (DP_GC + 1) + k] = a;
    }
    __syncthreads();
    for (int i = tid; i < q.cout * nf; i += DP_THREADS) {
        const int co = i / nf, ci = i - co * nf;
        const size_t at = ((size_t)co * q.cin + ci) * DP_TAPS + q.tap;
        const float *a = sA + co * (DP_GC + 1);
        float acc = w[at];                                               // the original x slice is the chain's initial value
#pragma unroll 8
        for (int k = 0; k < DP_GC; ++k) acc = fmaf(a[k], sP[k * nf + ci], acc);
        e[at] = acc;
    }
    // the untouched slices of rows tap, tap + 9, ...: [x1 .. end) of conv3 / conv4; x1, x3 and x4 of conv5
    const int a0 = nf * DP_TAPS / 4, a1 = (q.L == 2 ? q.x2 : q.cin) * DP_TAPS / 4;
    const int b0 = (q.x2 + DP_GC) * DP_TAPS / 4, b1 = q.L == 2 ? q.cin * DP_TAPS / 4 : 0;
    for (int co = q.tap; co < q.cout; co += DP_TAPS) {
        const float4 *src = reinterpret_cast<const float4 *>(w + (size_t)co * q.cin * DP_TAPS);
        float4 *dst = reinterpret_cast<float4 *>(e + (size_t)co * q.cin * DP_TAPS);
        for (int i = a0 + tid; i < a1; i += DP_THREADS) dst[i] = src[i];
        for (int i = b0 + tid; i < b1; i += DP_THREADS) dst[i] = src[i];
    }
}

// dP of one block in ONE workgroup: dP[k][ci] = sum over layer, cout chunk, tap, cout of A[co][k] G[co][ci].  The four waves split
// every 32-row chunk of couts (8 rows each, always the same rows), a lane owns gc nf / 64 outputs in registers, and the four partial
// sums meet in LDS as (w0 + w1) + (w2 + w3): no atomics, one order.  The next chunk's operands are fetched into registers while the
// current one is multiplied.
template <int NF>
__device__ __forceinline__ void dense_plus_dp(const tnr_dense_plus_item &it, float *lds) {
    constexpr int NJ = DP_GC * NF / 64, NA = 32 * DP_GC / DP_THREADS, NG = 32 * NF / DP_THREADS;
    constexpr int CH5 = NF / 32, NCHUNK = (2 + CH5) * DP_TAPS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float *sA = lds, *sG = lds + 32 * DP_GC;           // [32][gc], [32][NF]
    float acc[NJ], ra[NA], rg[NG];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = 0.f;

    auto fetch = [&](int c) {
        // chunk order: layer, 32-row cout chunk, tap (consecutive chunks gather from the same cache lines)
        const int part = c / DP_TAPS, tap = c - part * DP_TAPS;
        const int L = part < 2 ? part : 2, c0 = part < 2 ? 0 : (part - 2) * 32;
        const int cin = NF + (2 + L) * DP_GC, x2 = NF + DP_GC, x4 = NF + 3 * DP_GC;
        const float *w = it.w[L], *g = it.g[L];
#pragma unroll
        for (int n = 0; n < NA; ++n) {
            const int i = tid + n * DP_THREADS, r = i / DP_GC, k = i - r * DP_GC;
            const size_t row = (size_t)(c0 + r) * cin;
            float a = w[(row + x2 + k) * DP_TAPS + tap];
            if (L == 2) a = a + w[(row + x4 + k) * DP_TAPS + tap];
            ra[n] = a;
        }
#pragma unroll
        for (int n = 0; n < NG; ++n) {
            const int i = tid + n * DP_THREADS, r = i / NF, ci = i - r * NF;
            rg[n] = g[((size_t)(c0 + r) * cin + ci) * DP_TAPS + tap];
        }
    };

    fetch(0);
    for (int c = 0; c < NCHUNK; ++c) {
        __syncthreads();                                // the previous chunk is consumed
#pragma unroll
        for (int n = 0; n < NA; ++n) sA[tid + n * DP_THREADS] = ra[n];
#pragma unroll
        for (int n = 0; n < NG; ++n) sG[tid + n * DP_THREADS] = rg[n];
        __syncthreads();
        if (c + 1 < NCHUNK) fetch(c + 1);
        for (int r = wave * 8; r < wave * 8 + 8; ++r) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int o = lane + 64 * j, k = o / NF, ci = o - k * NF;
                acc[j] = fmaf(sA[r * DP_GC + k], sG[r * NF + ci], acc[j]);
            }
        }
    }
    __syncthreads();
    constexpr int NOUT = DP_GC * NF;
#pragma unroll
    for (int j = 0; j < NJ; ++j) lds[wave * NOUT + lane + 64 * j] = acc[j];
    __syncthreads();
    for (int o = tid; o < NOUT; o += DP_THREADS) {
        const float s = (lds[o] + lds[NOUT + o]) + (lds[2 * NOUT + o] + lds[3 * NOUT + o]);
        it.dp[o] = it.dp[o] + s;
    }
}

// grid (28, blocks): x < 27 a (layer, tap) job, x == 27 the block's dP
template <int NF>
__global__ __launch_bounds__(DP_THREADS) void dense_plus_unfold_kernel(const tnr_dense_plus_item *items) {
    __shared__ float lds[4 * DP_GC * DP_NF_MAX];       // 32 KB: the dP partials; the staging areas live in its front
    const tnr_dense_plus_item &it = items[blockIdx.y];      // (a reference: the per-layer pointers are indexed at run time)
    if (blockIdx.x == 3 * DP_TAPS) {
        dense_plus_dp<NF>(it, lds);
        return;
    }
    const PlusGeom q = plus_geom(blockIdx.x, NF);
    const float *g = it.g[q.L];
    float *dw = it.dw[q.L];
    const int tid = threadIdx.x;
    constexpr int ST = NF + 1;                          // padded rows: lanes walk k (sP) and co (sG) at a fixed ci
    float *sP = lds, *sG = lds + DP_GC * ST;            // P[k][ci], G[:, x] of this tap [co][ci]
    for (int i = tid; i < DP_GC * NF; i += DP_THREADS) {
        const int k = i / NF, ci = i - k * NF;
        sP[k * ST + ci] = it.p[i];
    }
    for (int i = tid; i < q.cout * NF; i += DP_THREADS) {
        const int co = i / NF, ci = i - co * NF;
        sG[co * ST + ci] = g[((size_t)co * q.cin + ci) * DP_TAPS + q.tap];
    }
    __syncthreads();
    // dW[:, x2] += G[:, x2] + G[:, x] P^T   (conv5 also: dW[:, x4] += G[:, x4] + G[:, x2] + G[:, x] P^T)
    for (int i = tid; i < q.cout * DP_GC; i += DP_THREADS) {
        const int co = i / DP_GC, k = i - co * DP_GC;
        const float *gr = sG + co * ST, *pr = sP + k * ST;
        float acc = 0.f;
#pragma unroll 8
        for (int ci = 0; ci < NF; ++ci) acc = fmaf(gr[ci], pr[ci], acc);
        const size_t row = (size_t)co * q.cin;
        const size_t at2 = (row + q.x2 + k) * DP_TAPS + q.tap;
        const float g2 = g[at2];
        dw[at2] = dw[at2] + (g2 + acc);
        if (q.L == 2) {
            const size_t at4 = (row + q.x4 + k) * DP_TAPS + q.tap;
            dw[at4] = dw[at4] + ((g[at4] + g2) + acc);
        }
    }
    // dW += G on the slices no product reaches, rows tap, tap + 9, ...: [x | x1], and x3 where the layer reads it
    const int a1 = q.x2 * DP_TAPS / 4, b0 = (q.x2 + DP_GC) * DP_TAPS / 4, b1 = q.cin >= q.x4 ? q.x4 * DP_TAPS / 4 : 0;
    for (int co = q.tap; co < q.cout; co += DP_TAPS) {
        const float4 *src = reinterpret_cast<const float4 *>(g + (size_t)co * q.cin * DP_TAPS);
        float4 *dst = reinterpret_cast<float4 *>(dw + (size_t)co * q.cin * DP_TAPS);
        for (int i = tid; i < a1; i += DP_THREADS) {
            const float4 s = src[i];
            float4 d = dst[i];
            d.x = d.x + s.x; d.y = d.y + s.y; d.z = d.z + s.z; d.w = d.w + s.w;
            dst[i] = d;
        }
        for (int i = b0 + tid; i < b1; i += DP_THREADS) {
            const float4 s = src[i];
            float4 d = dst[i];
            d.x = d.x + s.x; d.y = d.y + s.y; d.z = d.z + s.z; d.w = d.w + s.w;
            dst[i] = d;
        }
    }
}

int plus_args_ok(const tnr_dense_plus_item *items_dev, int32_t n, int32_t nf, int32_t gc, const char *who) {
    TNR_REQUIRE(items_dev != nullptr && n > 0 && n <= 65535, "%s: bad block table", who);
    TNR_REQUIRE(gc == DP_GC && (nf == 32 || nf == 64), "%s: nf %d / gc %d outside the shapes it is built for (gc 32, nf 32 or 64)", who, nf, gc);
    return TNR_OK;
}
}  // namespace

extern "C" int tnr_dense_plus_fold(const tnr_dense_plus_item *items_dev, int32_t n, int32_t nf, int32_t gc, void *stream) {
    if (int rc = plus_args_ok(items_dev, n, nf, gc, "dense_plus_fold")) return rc;
    hipLaunchKernelGGL(dense_plus_fold_kernel, dim3(3 * DP_TAPS, (unsigned)n), dim3(DP_THREADS), 0, (hipStream_t)stream, items_dev, nf);
    return tnr_check_launch("dense_plus_fold");
}

extern "C" int tnr_dense_plus_unfold(const tnr_dense_plus_item *items_dev, int32_t n, int32_t nf, int32_t gc, void *stream) {
    if (int rc = plus_args_ok(items_dev, n, nf, gc, "dense_plus_unfold")) return rc;
    const dim3 grid(3 * DP_TAPS + 1, (unsigned)n);
    if (nf == 64)
        hipLaunchKernelGGL(dense_plus_unfold_kernel<64>, grid, dim3(DP_THREADS), 0, (hipStream_t)stream, items_dev);
    else
        hipLaunchKernelGGL(dense_plus_unfold_kernel<32>, grid, dim3(DP_THREADS), 0, (hipStream_t)stream, items_dev);
    return tnr_check_launch("dense_plus_unfold");
}
