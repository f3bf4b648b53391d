// Gram matrix of an NHWC activation and its gradient, on the matrix core (the style term of PerceptualLoss: GramMatrix(out_norm='ci'),
// modules/loss.py:479-506, under nn.L1Loss).  DESIGN.md section 14.
//
//   tnr_gram_fwd:  G[n][i][j] = scale * sum_p X[n][p][i] X[n][p][j]                 (C x C, K = H W pixels: long K, small M / N)
//   tnr_gram_bwd:  dX[n][p][c] = scale * sum_j X[n][p][j] (S[n][j][c] + S[n][c][j])  (M = pixels, N = K = C)
//
// Arithmetic is the library's: TNR_MMA_BF16X3 splits every operand exactly into three bf16 values ONCE, in the stager, and keeps the six
// largest partial products in conv_body.h's order (v_mfma_f32_32x32x16_bf16); TNR_MMA_F32 runs v_mfma_f32_32x32x2_f32.
//
// Forward.  One workgroup (4 waves) owns one 64 x 64 tile (bi <= bj: the block upper triangle) of one image's G over one K split.  Per
// LDS fill it stages 64 pixels x 64 channels of X per panel -- ONE panel on the diagonal, where the same tile is both operands -- and
// wave (wr, wc) accumulates the 32 x 32 block (wr, wc); the block below the diagonal of a diagonal tile is not computed.  Both operands
// want "row = channel, k = pixel": bf16x3 keeps the panel channel-major (a row = 16 pixels of one channel as three 32-byte planes, the
// 96-byte swizzled rows of conv_body.h), transposed by the stager; f32 keeps it pixel-major and reads one dword per lane.  The partial
// tiles go to a workspace [n][split][tile][64][64]; a second launch adds the splits in their fixed order, applies `scale` and writes
// G[i][j] AND G[j][i] from the one sum of i <= j: bit-exactly symmetric, no floating-point atomics, run-to-run bit-identical.
//
// Backward.  One workgroup owns 128 pixels x 64 output channels and walks K = C in chunks of 32 channels: X tile pixel-major (the
// convolution's input layout), T = S + S^T formed by the stager (row c of the tile = T[c][j0 ..], one float4 of S[c][.] plus four
// strided reads of S[.][c]; S is small and L2-resident) and split there.  Wave w owns pixels 32 w .. 32 w + 31 and both 32-channel
// halves.  The store covers 128 contiguous bytes per half wave; `accumulate` adds into what is there.
#include "conv_body.h"

namespace {

constexpr int GR_KT = 64;          // pixels per LDS fill (forward)
constexpr int GR_PANEL = 6144;     // floats per 64-channel panel: 4 k-steps x 64 rows x 24 (bf16x3) = 64 pixels x 96 (f32)
constexpr int GR_F32_ST = 96;      // f32 pixel stride: 64 channels + 32, so that the two lane halves (pixels k, k + 1) use disjoint banks
constexpr int GR_MIN_CPS = 4;      // a K split is at least 4 fills (256 pixels)
constexpr int GR_WG_TARGET = 1024; // workgroups wanted per launch (256 CUs x 4)

struct GramF {
    const float *x;
    int ct, co, nb, T, nsplit, cps, chunks;
    int64_t P;
    float *ws;
};

template <bool X3>
__global__ void __launch_bounds__(256) gram_fwd_kernel(const GramF a) {
    __shared__ __attribute__((aligned(16))) float smem[2 * GR_PANEL];
    int bid = blockIdx.x;
    const int t = bid % a.T;
    bid /= a.T;
    const int sp = bid % a.nsplit;
    const int n = bid / a.nsplit;
    int bi = 0, rem = t;
    while (rem >= a.nb - bi) {
        rem -= a.nb - bi;
        ++bi;
    }
    const int bj = bi + rem;
    const int npan = bi == bj ? 1 : 2;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, half = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const bool active = !(bi == bj && wr > wc);          // wave-uniform: the block below the diagonal is the mirror of (0, 1)
    const float *xn = a.x + (size_t)n * a.P * a.ct + a.co;
    const int c_begin = sp * a.cps, c_end = min(a.chunks, c_begin + a.cps);

    // staging item of a thread: pixels 4 pq .. 4 pq + 3 of the fill x channels 4 q .. 4 q + 3 of each panel
    const int q = tid & 15, pq = tid >> 4;
    f32x4 rx[2][4];
    auto load_chunk = [&](int chunk) {
        const int64_t p0 = (int64_t)chunk * GR_KT + 4 * pq;
#pragma unroll
        for (int pan = 0; pan < 2; ++pan) {
            if (pan < npan) {
                const int cbase = (pan == 0 ? bi : bj) * 64 + 4 * q;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};               // ragged K: pixels past the image are zeros
                    if (p0 + i < a.P) v = *reinterpret_cast<const f32x4 *>(xn + (size_t)(p0 + i) * a.ct + cbase);
                    rx[pan][i] = v;
                }
            }
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int pan = 0; pan < 2; ++pan) {
            if (pan < npan) {
                float *base = smem + pan * GR_PANEL;
                if constexpr (X3) {
                    unsigned u[4][3][2];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        tnr_f32x2 pc[3];
                        tnr_split4_bf16x3(rx[pan][i], pc);
#pragma unroll
                        for (int s = 0; s < 3; ++s) {
                            const float c01 = pc[s][0], c23 = pc[s][1];      // (by value: a bit cast of a vector ELEMENT expression reads element 0)
                            u[i][s][0] = __builtin_bit_cast(unsigned, c01);
                            u[i][s][1] = __builtin_bit_cast(unsigned, c23);
                        }
                    }
                    const int ks = pq >> 2, pa = pq & 3;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int row = ks * 64 + 4 * q + e;
                        float *dst = base + row * TNR_X3_ROW + 4 * ((pa >> 1) ^ ((row >> TNR_X3_SWZ) & 1)) + 2 * (pa & 1);
#pragma unroll
                        for (int s = 0; s < 3; ++s) {
                            unsigned h[4];
#pragma unroll
                            for (int i = 0; i < 4; ++i) h[i] = (e & 1) ? (u[i][s][e >> 1] >> 16) : (u[i][s][e >> 1] & 0xffffu);
                            const tnr_f32x2 w = {__builtin_bit_cast(float, h[0] | (h[1] << 16)), __builtin_bit_cast(float, h[2] | (h[3] << 16))};
                            *reinterpret_cast<tnr_f32x2 *>(dst + 8 * s) = w;
                        }
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4 *>(base + (4 * pq + i) * GR_F32_ST + 4 * q) = rx[pan][i];
                }
            }
        }
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float *sA = smem, *sB = smem + (npan - 1) * GR_PANEL;

    load_chunk(c_begin);
    for (int chunk = c_begin; chunk < c_end; ++chunk) {
        __syncthreads();          // the previous fill's fragments are consumed
        store_chunk();
        __syncthreads();
        if (chunk + 1 < c_end) load_chunk(chunk + 1);      // in flight during the MFMA phase
        if (active) {
            if constexpr (X3) {
                constexpr int TA[6] = {0, 2, 1, 0, 1, 0}, TB[6] = {2, 0, 1, 1, 0, 0};      // the six kept partial products, smallest first
#pragma unroll
                for (int ks = 0; ks < GR_KT / 16; ++ks) {
                    const int ra = ks * 64 + wr * 32 + li, rb = ks * 64 + wc * 32 + li;
                    const float *pa = sA + ra * TNR_X3_ROW + 4 * (half ^ ((ra >> TNR_X3_SWZ) & 1));
                    const float *pb = sB + rb * TNR_X3_ROW + 4 * (half ^ ((rb >> TNR_X3_SWZ) & 1));
                    tnr_bf16x8 ca[3], cb[3];
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        ca[s] = *reinterpret_cast<const tnr_bf16x8 *>(pa + 8 * s);
                        cb[s] = *reinterpret_cast<const tnr_bf16x8 *>(pb + 8 * s);
                    }
#pragma unroll
                    for (int p = 0; p < 6; ++p) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ca[TA[p]], cb[TB[p]], acc, 0, 0, 0);
                }
            } else {
#pragma unroll 8
                for (int k = 0; k < GR_KT; k += 2) {
                    const float av = sA[(k + half) * GR_F32_ST + wr * 32 + li];
                    const float bv = sB[(k + half) * GR_F32_ST + wc * 32 + li];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
                }
            }
        }
    }
    if (active) {
        float *w = a.ws + (((size_t)n * a.nsplit + sp) * a.T + t) * 4096;
#pragma unroll
        for (int r = 0; r < 16; ++r) w[(wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * 64 + wc * 32 + li] = acc[r];
    }
}

// G[n][i][j] = G[n][j][i] = scale * (split 0 + split 1 + ...) for i <= j: one thread per element of a 64 x 64 tile
__global__ void __launch_bounds__(256) gram_reduce_kernel(const float *ws, float *G, int N, int C, int nb, int T, int nsplit, float scale) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)N * T * 4096) return;
    const int e = (int)(idx & 4095);
    const int t = (int)((idx >> 12) % T), n = (int)((idx >> 12) / T);
    int bi = 0, rem = t;
    while (rem >= nb - bi) {
        rem -= nb - bi;
        ++bi;
    }
    const int gi = bi * 64 + (e >> 6), gj = (bi + rem) * 64 + (e & 63);
    if (gi > gj) return;
    float s = 0.f;
    for (int sp = 0; sp < nsplit; ++sp) s += ws[(((size_t)n * nsplit + sp) * T + t) * 4096 + e];
    s *= scale;
    float *g = G + (size_t)n * C * C;
    g[(size_t)gi * C + gj] = s;
    g[(size_t)gj * C + gi] = s;
}

struct GramB {
    const float *x, *S;
    float *dx;
    int x_ct, x_co, d_ct, d_co, C, ptiles, ncb, accumulate;
    int64_t P;
    float scale;
};

constexpr int GB_PT = 128, GB_KC = 32, GB_F32_ST = GB_KC + 4;      // 36-dword rows: 9 p mod 16 is a permutation of the 16-byte slots

template <bool X3>
__global__ void __launch_bounds__(256) gram_bwd_kernel(const GramB a) {
    constexpr int XF = X3 ? (GB_KC / 16) * GB_PT * TNR_X3_ROW : GB_PT * GB_F32_ST;
    constexpr int TF = X3 ? (GB_KC / 16) * 64 * TNR_X3_ROW : 64 * GB_F32_ST;
    __shared__ __attribute__((aligned(16))) float smem[XF + TF];
    float *sX = smem, *sT = smem + XF;
    int bid = blockIdx.x;
    const int cb = bid % a.ncb;
    bid /= a.ncb;
    const int pt = bid % a.ptiles;
    const int n = bid / a.ptiles;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, half = lane >> 5;
    const float *xn = a.x + (size_t)n * a.P * a.x_ct + a.x_co;
    const float *sn = a.S + (size_t)n * a.C * a.C;
    const int64_t p_base = (int64_t)pt * GB_PT;

    // staging items: X i = tid + 256 it -> pixel row i / 8, channel quad i % 8; T likewise over the 64 output channels
    f32x4 rxv[4], rtv[2];
    auto load_chunk = [&](int chunk) {
        const int j0 = chunk * GB_KC;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int i = tid + it * 256, row = i >> 3, qq = i & 7;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (p_base + row < a.P) v = *reinterpret_cast<const f32x4 *>(xn + (size_t)(p_base + row) * a.x_ct + j0 + 4 * qq);
            rxv[it] = v;
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int i = tid + it * 256, c = cb * 64 + (i >> 3), j = j0 + 4 * (i & 7);
            f32x4 v = *reinterpret_cast<const f32x4 *>(sn + (size_t)c * a.C + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += sn[(size_t)(j + e) * a.C + c];       // S + S^T: S itself need not be symmetric
            rtv[it] = v;
        }
    };
    auto store_item = [&](float *base, int rows, int i, const f32x4 v) {
        const int row = i >> 3, qq = i & 7;
        if constexpr (X3) {
            tnr_f32x2 pc[3];
            tnr_split4_bf16x3(v, pc);
            const int R = (qq >> 2) * rows + row, q4 = qq & 3;
            float *dst = base + R * TNR_X3_ROW + 4 * ((q4 >> 1) ^ ((R >> TNR_X3_SWZ) & 1)) + 2 * (q4 & 1);
            *reinterpret_cast<tnr_f32x2 *>(dst) = pc[0];
            *reinterpret_cast<tnr_f32x2 *>(dst + 8) = pc[1];
            *reinterpret_cast<tnr_f32x2 *>(dst + 16) = pc[2];
        } else {
            *reinterpret_cast<f32x4 *>(base + row * GB_F32_ST + 4 * qq) = v;
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int it = 0; it < 4; ++it) store_item(sX, GB_PT, tid + it * 256, rxv[it]);
#pragma unroll
        for (int it = 0; it < 2; ++it) store_item(sT, 64, tid + it * 256, rtv[it]);
    };

    f32x16 acc[2];
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nn][r] = 0.f;

    const int nchunks = a.C / GB_KC;
    load_chunk(0);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        __syncthreads();
        store_chunk();
        __syncthreads();
        if (chunk + 1 < nchunks) load_chunk(chunk + 1);
        if constexpr (X3) {
            constexpr int TA[6] = {0, 2, 1, 0, 1, 0}, TB[6] = {2, 0, 1, 1, 0, 0};
#pragma unroll
            for (int ks = 0; ks < GB_KC / 16; ++ks) {
                const int ra = ks * GB_PT + wave * 32 + li;
                const float *pa = sX + ra * TNR_X3_ROW + 4 * (half ^ ((ra >> TNR_X3_SWZ) & 1));
                tnr_bf16x8 ca[3], cbf[2][3];
#pragma unroll
                for (int s = 0; s < 3; ++s) ca[s] = *reinterpret_cast<const tnr_bf16x8 *>(pa + 8 * s);
#pragma unroll
                for (int nn = 0; nn < 2; ++nn) {
                    const int rb = ks * 64 + nn * 32 + li;
                    const float *pb = sT + rb * TNR_X3_ROW + 4 * (half ^ ((rb >> TNR_X3_SWZ) & 1));
#pragma unroll
                    for (int s = 0; s < 3; ++s) cbf[nn][s] = *reinterpret_cast<const tnr_bf16x8 *>(pb + 8 * s);
                }
#pragma unroll
                for (int p = 0; p < 6; ++p)
#pragma unroll
                    for (int nn = 0; nn < 2; ++nn) acc[nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ca[TA[p]], cbf[nn][TB[p]], acc[nn], 0, 0, 0);
            }
        } else {
            // lane half h supplies channels 8 g + 4 h .. + 3 of both operands (one ds_read_b128 each): MFMA e of group g reduces the
            // channel pair (8 g + e, 8 g + 4 + e)
#pragma unroll
            for (int g = 0; g < GB_KC / 8; ++g) {
                const f32x4 va = *reinterpret_cast<const f32x4 *>(sX + (wave * 32 + li) * GB_F32_ST + 8 * g + 4 * half);
                f32x4 vb[2];
#pragma unroll
                for (int nn = 0; nn < 2; ++nn) vb[nn] = *reinterpret_cast<const f32x4 *>(sT + (nn * 32 + li) * GB_F32_ST + 8 * g + 4 * half);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int nn = 0; nn < 2; ++nn) acc[nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[e], vb[nn][e], acc[nn], 0, 0, 0);
            }
        }
    }
    float *dn = a.dx + (size_t)n * a.P * a.d_ct + a.d_co + cb * 64;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t p = p_base + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (p < a.P) {
#pragma unroll
            for (int nn = 0; nn < 2; ++nn) {
                float *d = dn + (size_t)p * a.d_ct + nn * 32 + li;
                float v = acc[nn][r] * a.scale;
                if (a.accumulate) v += *d;
                *d = v;
            }
        }
    }
}

struct GramPlan {
    int nb, T, chunks, cps, nsplit;
};

inline GramPlan gram_plan(int N, int64_t P, int C) {
    GramPlan g;
    g.nb = C / 64;
    g.T = g.nb * (g.nb + 1) / 2;
    g.chunks = (int)tnr_cdiv64(P, GR_KT);
    const int want = tnr_cdiv(GR_WG_TARGET, N * g.T);
    int ns = tnr_cdiv(g.chunks, GR_MIN_CPS);
    if (ns > want) ns = want;
    if (ns < 1) ns = 1;
    g.cps = tnr_cdiv(g.chunks, ns);
    g.nsplit = tnr_cdiv(g.chunks, g.cps);
    return g;
}

inline int gram_check(const char *who, tnr_view x, int N, int H, int W, int C, int mma) {
    TNR_REQUIRE(x.ptr != nullptr && N > 0 && H > 0 && W > 0, "%s: bad shape %d x %d x %d", who, N, H, W);
    TNR_REQUIRE(C >= 64 && C <= 512 && (C % 64) == 0, "%s: C = %d is not a multiple of 64 in 64 .. 512", who, C);
    TNR_REQUIRE((x.ctot % 4) == 0 && (x.coff % 4) == 0 && x.coff >= 0 && x.coff + C <= x.ctot, "%s: bad view (ctot %d, coff %d, C %d)", who,
                x.ctot, x.coff, C);
    TNR_REQUIRE(mma == TNR_MMA_F32 || mma == TNR_MMA_BF16X3, "%s: mma %d (TNR_MMA_F32 or TNR_MMA_BF16X3)", who, mma);
    TNR_REQUIRE((int64_t)N * H * W < ((int64_t)1 << 31), "%s: too many pixels", who);
    return TNR_OK;
}

}  // namespace

extern "C" int64_t tnr_gram_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C) {
    if (N <= 0 || H <= 0 || W <= 0 || C < 64 || C > 512 || (C % 64) != 0) return 0;
    const GramPlan g = gram_plan(N, (int64_t)H * W, C);
    return (int64_t)N * g.nsplit * g.T * 4096 * (int64_t)sizeof(float);
}

extern "C" int tnr_gram_fwd(tnr_view x, int32_t N, int32_t H, int32_t W, int32_t C, float scale, int32_t mma, float *G, float *ws,
                            int64_t ws_bytes, void *stream) {
    if (int rc = gram_check("gram_fwd", x, N, H, W, C, mma)) return rc;
    TNR_REQUIRE(G != nullptr && ws != nullptr && ws_bytes >= tnr_gram_workspace_bytes(N, H, W, C), "gram_fwd: workspace of %lld bytes needed",
                (long long)tnr_gram_workspace_bytes(N, H, W, C));
    const GramPlan g = gram_plan(N, (int64_t)H * W, C);
    GramF a;
    a.x = x.ptr;
    a.ct = x.ctot;
    a.co = x.coff;
    a.nb = g.nb;
    a.T = g.T;
    a.nsplit = g.nsplit;
    a.cps = g.cps;
    a.chunks = g.chunks;
    a.P = (int64_t)H * W;
    a.ws = ws;
    const int64_t wgs = (int64_t)N * g.nsplit * g.T;
    TNR_REQUIRE(wgs < ((int64_t)1 << 31), "gram_fwd: grid too large");
    hipStream_t s = (hipStream_t)stream;
    if (mma == TNR_MMA_BF16X3)
        hipLaunchKernelGGL(gram_fwd_kernel<true>, dim3((unsigned)wgs), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(gram_fwd_kernel<false>, dim3((unsigned)wgs), dim3(256), 0, s, a);
    if (int rc = tnr_check_launch("gram_fwd")) return rc;
    const int64_t elems = (int64_t)N * g.T * 4096;
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)tnr_cdiv64(elems, 256)), dim3(256), 0, s, ws, G, N, C, g.nb, g.T, g.nsplit, scale);
    return tnr_check_launch("gram_reduce");
}

extern "C" int tnr_gram_bwd(tnr_view x, const float *S, int32_t N, int32_t H, int32_t W, int32_t C, float scale, int32_t mma, tnr_view dx,
                            int32_t accumulate, void *stream) {
    if (int rc = gram_check("gram_bwd", x, N, H, W, C, mma)) return rc;
    TNR_REQUIRE(S != nullptr && dx.ptr != nullptr && (dx.ctot % 4) == 0 && (dx.coff % 4) == 0 && dx.coff >= 0 && dx.coff + C <= dx.ctot,
                "gram_bwd: bad gradient view (ctot %d, coff %d, C %d)", dx.ctot, dx.coff, C);
    GramB a;
    a.x = x.ptr;
    a.S = S;
    a.dx = dx.ptr;
    a.x_ct = x.ctot;
    a.x_co = x.coff;
    a.d_ct = dx.ctot;
    a.d_co = dx.coff;
    a.C = C;
    a.P = (int64_t)H * W;
    a.ptiles = (int)tnr_cdiv64(a.P, GB_PT);
    a.ncb = C / 64;
    a.accumulate = accumulate != 0;
    a.scale = scale;
    const int64_t wgs = (int64_t)N * a.ptiles * a.ncb;
    TNR_REQUIRE(wgs < ((int64_t)1 << 31), "gram_bwd: grid too large");
    hipStream_t s = (hipStream_t)stream;
    if (mma == TNR_MMA_BF16X3)
        hipLaunchKernelGGL(gram_bwd_kernel<true>, dim3((unsigned)wgs), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(gram_bwd_kernel<false>, dim3((unsigned)wgs), dim3(256), 0, s, a);
    return tnr_check_launch("gram_bwd");
}
