// Contextual loss over a pair of NHWC feature taps (Contextual_Loss, distance 'cosine', calc 'regular': modules/loss.py:769-1092) and
// its gradient with respect to the first operand.  DESIGN.md section 15.
//
//   X = the SR tap, Y = the HR tap, P positions each (all H W of them, or the `idx` list of a random pooling), C channels.
//   mu = mean of Y over batch and positions;  Xh, Yh = (X - mu), (Y - mu) normalised over C (F.normalize, eps 1e-12)
//   d[n][i][j] = max((1 - <Xh[n][i], Yh[n][j]>) / 2, 0);  m_i = min_j d_ij;  w_ij = exp((b - d_ij / (m_i + 1e-5)) / h)
//   cx_ij = w_ij / sum_j w_ij;  CS_n = mean_j max_i cx_ij;  loss = mean_n -log CS_n
//
// ONE fp32 matrix [N][P][LD] (LD = P rounded up to 4, so that a row starts on 16 bytes) lives in the caller's workspace and is
// transformed in place, d -> cx -> d loss / d cos:
//
//   tnr_cx_sums       per-channel sums of Y: fixed chunks of positions, then the chunks in their order (fp64; no atomics)
//   tnr_cx_prepare    one wave per position: gather, subtract mu, normalise -> Xh / Yh [N][P][C] and the clamped norms
//   tnr_cx_distance   d = the epilogue of Xh Yh^T (M = N = P, K = C): both operands pixel-major with K contiguous, the X tile of
//                     gram_bwd_kernel; TNR_MMA_BF16X3 splits in the stager, TNR_MMA_F32 runs v_mfma_f32_32x32x2_f32
//   tnr_cx_rows       a row (<= 4096 floats) sits in the registers of one workgroup: min / argmin, exp, the row sum, the normalisation
//                     and E_i = sum_j cx_ij d_ij are one read and one in-place write.  A workgroup walks CX_RB rows and keeps the column
//                     maxima of its rows as (value, row) in registers; they meet in a 64-bit integer max over (value bits, ~row):
//                     order-independent, ties to the smaller row.  cx is stored NEGATED where d == 0 (cx > 0 always), which keeps the
//                     clamp pattern for the gradient at no cost in bytes
//   tnr_cx_finalize   column max / argmax, CS_n, g_n = -1 / (N P CS_n) and the loss, in a fixed order
//   tnr_cx_grad_rows  d_win[j] = d at (argmax_j, j), recomputed from Xh, Yh (C products per column; d itself was overwritten), then per
//                     row: A_i, sum_k q_ik d_ik = g (sum_{J_i} cx d_win - A_i E_i), q, the argmin term and d loss / d cos, in place
//   tnr_cx_grad_gemm  dXh = G Yh (M = P, N = C, K = P): A as above, B "row = channel, k = position" through the transposing stager of
//                     gram_fwd_kernel (bf16x3) or position-major with one dword per lane (f32)
//   tnr_cx_norm_bwd   one wave per position of the FULL map: the normalisation's backward and the scatter; unsampled positions get 0
//
// Offsets into the matrix are 64-bit (N = 16, P = 4096: 1 GiB).  No floating-point atomics: two runs are bit-identical.
#include "conv_body.h"

namespace {

constexpr int CX_MAXP = 4096;      // a row in registers: 16 floats per thread of a 256-thread workgroup
constexpr int CX_RPT = CX_MAXP / 256;
constexpr int CX_RB = 32;          // rows per workgroup of the row passes
constexpr int CX_SUM_CHUNK = 64;   // positions per workgroup of the channel sums
constexpr int CX_PT = 128, CX_KC = 32, CX_F32_ST = CX_KC + 4;      // gram_bwd_kernel's tile: 128 rows x 64 columns, K chunks of 32

__host__ __device__ inline int cx_ld(int P) { return (P + 3) & ~3; }

// ------------------------------------------------------------------------------------------------ channel sums, prepare
__global__ void __launch_bounds__(256) cx_sums_partial_kernel(const float *y, int ct, int co, int C, int HW, int P, const int32_t *idx,
                                                              int64_t total, double *part) {
    const int64_t p0 = (int64_t)blockIdx.x * CX_SUM_CHUNK;
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0;
        for (int e = 0; e < CX_SUM_CHUNK; ++e) {
            const int64_t g = p0 + e;
            if (g >= total) break;
            const int64_t n = g / P;
            const int p = (int)(g - n * P);
            const int64_t src = n * HW + (idx ? idx[p] : p);
            s += (double)y[src * ct + co + c];
        }
        part[(int64_t)blockIdx.x * C + c] = s;
    }
}

__global__ void __launch_bounds__(256) cx_sums_reduce_kernel(const double *part, int nblk, int C, double count, float *sums) {
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * C + c];
        sums[c] = (float)s;
    }
    if (threadIdx.x == 0) sums[C] = (float)count;
}

__device__ __forceinline__ float cx_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(256) cx_prepare_kernel(const float *x, int ct, int co, int C, int HW, int P, const int32_t *idx,
                                                         int64_t total, const float *sums, float *xh, float *nrm) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= total) return;
    const int64_t n = g / P;
    const int p = (int)(g - n * P);
    const float *src = x + (n * HW + (idx ? idx[p] : p)) * ct + co;
    const float count = sums[C];
    float v[8], ss = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = lane + 64 * k;
        v[k] = 0.f;
        if (c < C) v[k] = src[c] - sums[c] / count;
        ss += v[k] * v[k];
    }
    ss = cx_wave_sum(ss);
    const float den = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = lane + 64 * k;
        if (c < C) xh[g * C + c] = v[k] / den;
    }
    if (lane == 0) nrm[g] = den;
}

// ------------------------------------------------------------------------------------------------ the two products
struct CxGemm {
    const float *A, *B;
    float *out;
    int M, K, lda, NB, ldb, ldo, mtiles, ntiles;
    int64_t a_img, b_img, o_img;
};

// GRAD = false: out[i][j] = max((1 - sum_k A[i][k] B[j][k]) / 2, 0)  (B rows j < NB, K contiguous in both)
// GRAD = true:  out[i][c] = sum_k A[i][k] B[k][c]                    (B position-major, 64 channels per workgroup)
template <bool X3, bool GRAD>
__global__ void __launch_bounds__(256) cx_gemm_kernel(const CxGemm a) {
    constexpr int AF = X3 ? (CX_KC / 16) * CX_PT * TNR_X3_ROW : CX_PT * CX_F32_ST;
    constexpr int BF = X3 ? (CX_KC / 16) * 64 * TNR_X3_ROW : (GRAD ? CX_KC * 64 : 64 * CX_F32_ST);
    __shared__ __attribute__((aligned(16))) float smem[AF + BF];
    float *sA = smem, *sB = smem + AF;
    int bid = blockIdx.x;
    const int nt = bid % a.ntiles;
    bid /= a.ntiles;
    const int mt = bid % a.mtiles;
    const int n = bid / a.mtiles;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, half = lane >> 5;
    const float *An = a.A + (int64_t)n * a.a_img;
    const float *Bn = a.B + (int64_t)n * a.b_img;
    const int m_base = mt * CX_PT;

    f32x4 ra[4], rb[4];
    auto load_chunk = [&](int chunk) {
        const int k0 = chunk * CX_KC;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int i = tid + it * 256, row = i >> 3, k = k0 + 4 * (i & 7);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (m_base + row < a.M && k < a.K) {
                const float *p = An + (int64_t)(m_base + row) * a.lda + k;
                v = *reinterpret_cast<const f32x4 *>(p);          // lda is a multiple of 4: the quad lies inside the row's storage
                if (k + 3 >= a.K) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (k + e >= a.K) v[e] = 0.f;             // ragged K: the padding of a row is not part of the sum
                }
            }
            ra[it] = v;
        }
        if constexpr (!GRAD) {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int i = tid + it * 256, j = nt * 64 + (i >> 3), k = k0 + 4 * (i & 7);
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (j < a.NB && k < a.K) v = *reinterpret_cast<const f32x4 *>(Bn + (int64_t)j * a.ldb + k);
                rb[it] = v;
            }
        } else if constexpr (X3) {
            // item of threads 0 .. 127: positions 4 pq .. 4 pq + 3 of the chunk x channels 4 q .. 4 q + 3 (gram_fwd_kernel's item)
            if (tid < 128) {
                const int q = tid & 15, pq = tid >> 4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = k0 + 4 * pq + i;
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if (k < a.K) v = *reinterpret_cast<const f32x4 *>(Bn + (int64_t)k * a.ldb + nt * 64 + 4 * q);
                    rb[i] = v;
                }
            }
        } else {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int i = tid + it * 256, k = k0 + (i >> 4);
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (k < a.K) v = *reinterpret_cast<const f32x4 *>(Bn + (int64_t)k * a.ldb + nt * 64 + 4 * (i & 15));
                rb[it] = v;
            }
        }
    };
    auto store_item = [&](float *base, int rows, int i, const f32x4 v) {      // gram_bwd_kernel's: row i / 8, K quad i % 8
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
            *reinterpret_cast<f32x4 *>(base + row * CX_F32_ST + 4 * qq) = v;
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int it = 0; it < 4; ++it) store_item(sA, CX_PT, tid + it * 256, ra[it]);
        if constexpr (!GRAD) {
#pragma unroll
            for (int it = 0; it < 2; ++it) store_item(sB, 64, tid + it * 256, rb[it]);
        } else if constexpr (X3) {
            if (tid < 128) {      // the transposing store of gram_fwd_kernel: a row = 16 positions of one channel, three planes
                const int q = tid & 15, pq = tid >> 4;
                unsigned u[4][3][2];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    tnr_f32x2 pc[3];
                    tnr_split4_bf16x3(rb[i], pc);
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        const float c01 = pc[s][0], c23 = pc[s][1];
                        u[i][s][0] = __builtin_bit_cast(unsigned, c01);
                        u[i][s][1] = __builtin_bit_cast(unsigned, c23);
                    }
                }
                const int ks = pq >> 2, pa = pq & 3;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = ks * 64 + 4 * q + e;
                    float *dst = sB + row * TNR_X3_ROW + 4 * ((pa >> 1) ^ ((row >> TNR_X3_SWZ) & 1)) + 2 * (pa & 1);
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        unsigned h[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) h[i] = (e & 1) ? (u[i][s][e >> 1] >> 16) : (u[i][s][e >> 1] & 0xffffu);
                        const tnr_f32x2 w = {__builtin_bit_cast(float, h[0] | (h[1] << 16)), __builtin_bit_cast(float, h[2] | (h[3] << 16))};
                        *reinterpret_cast<tnr_f32x2 *>(dst + 8 * s) = w;
                    }
                }
            }
        } else {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int i = tid + it * 256;
                *reinterpret_cast<f32x4 *>(sB + (i >> 4) * 64 + 4 * (i & 15)) = rb[it];
            }
        }
    };

    f32x16 acc[2];
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nn][r] = 0.f;

    const int nchunks = (a.K + CX_KC - 1) / CX_KC;
    load_chunk(0);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        __syncthreads();
        store_chunk();
        __syncthreads();
        if (chunk + 1 < nchunks) load_chunk(chunk + 1);
        if constexpr (X3) {
            constexpr int TA[6] = {0, 2, 1, 0, 1, 0}, TB[6] = {2, 0, 1, 1, 0, 0};      // the six kept partial products, smallest first
#pragma unroll
            for (int ks = 0; ks < CX_KC / 16; ++ks) {
                const int rw = ks * CX_PT + wave * 32 + li;
                const float *pa = sA + rw * TNR_X3_ROW + 4 * (half ^ ((rw >> TNR_X3_SWZ) & 1));
                tnr_bf16x8 ca[3], cbf[2][3];
#pragma unroll
                for (int s = 0; s < 3; ++s) ca[s] = *reinterpret_cast<const tnr_bf16x8 *>(pa + 8 * s);
#pragma unroll
                for (int nn = 0; nn < 2; ++nn) {
                    const int rbw = ks * 64 + nn * 32 + li;
                    const float *pb = sB + rbw * TNR_X3_ROW + 4 * (half ^ ((rbw >> TNR_X3_SWZ) & 1));
#pragma unroll
                    for (int s = 0; s < 3; ++s) cbf[nn][s] = *reinterpret_cast<const tnr_bf16x8 *>(pb + 8 * s);
                }
#pragma unroll
                for (int p = 0; p < 6; ++p)
#pragma unroll
                    for (int nn = 0; nn < 2; ++nn) acc[nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ca[TA[p]], cbf[nn][TB[p]], acc[nn], 0, 0, 0);
            }
        } else {
            // lane half h supplies k = 8 g + 4 h .. + 3 of both operands: MFMA e of group g reduces the pair (8 g + e, 8 g + 4 + e)
#pragma unroll
            for (int g = 0; g < CX_KC / 8; ++g) {
                const f32x4 va = *reinterpret_cast<const f32x4 *>(sA + (wave * 32 + li) * CX_F32_ST + 8 * g + 4 * half);
                f32x4 vb[2];
#pragma unroll
                for (int nn = 0; nn < 2; ++nn) {
                    if constexpr (GRAD) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) vb[nn][e] = sB[(8 * g + 4 * half + e) * 64 + nn * 32 + li];
                    } else {
                        vb[nn] = *reinterpret_cast<const f32x4 *>(sB + (nn * 32 + li) * CX_F32_ST + 8 * g + 4 * half);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int nn = 0; nn < 2; ++nn) acc[nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[e], vb[nn][e], acc[nn], 0, 0, 0);
            }
        }
    }
    float *on = a.out + (int64_t)n * a.o_img;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = m_base + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (i < a.M) {
#pragma unroll
            for (int nn = 0; nn < 2; ++nn) {
                const int j = nt * 64 + nn * 32 + li;
                if constexpr (GRAD) {
                    on[(int64_t)i * a.ldo + j] = acc[nn][r];
                } else {
                    if (j < a.NB) on[(int64_t)i * a.ldo + j] = fmaxf((1.f - acc[nn][r]) * 0.5f, 0.f);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ row passes
// (min, index) of a workgroup, ties to the smaller index: shuffles inside a wave, then the four waves through `sh`
__device__ __forceinline__ void cx_block_argmin(float &v, int &ix, float *shv, int *shi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(ix, o, 64);
        if (ov < v || (ov == v && oi < ix)) {
            v = ov;
            ix = oi;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        shv[threadIdx.x >> 6] = v;
        shi[threadIdx.x >> 6] = ix;
    }
    __syncthreads();
    v = shv[0];
    ix = shi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (shv[w] < v || (shv[w] == v && shi[w] < ix)) {
            v = shv[w];
            ix = shi[w];
        }
}

// the sums of two doubles over a workgroup in a fixed order
__device__ __forceinline__ void cx_block_sum2(double &s0, double &s1, double *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o, 64);
        s1 += __shfl_xor(s1, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[2 * (threadIdx.x >> 6)] = s0;
        sh[2 * (threadIdx.x >> 6) + 1] = s1;
    }
    __syncthreads();
    s0 = ((sh[0] + sh[2]) + sh[4]) + sh[6];
    s1 = ((sh[1] + sh[3]) + sh[5]) + sh[7];
}

__global__ void __launch_bounds__(256) cx_rows_kernel(float *D, int P, int ld, int rblocks, float b, float h, float *rowmin, int32_t *argmin,
                                                      float *rowE, unsigned long long *colpack) {
    __shared__ float shv[2][4];
    __shared__ int shi[2][4];
    __shared__ double shd[2][8];
    const int n = blockIdx.x / rblocks, rb = blockIdx.x % rblocks, tid = threadIdx.x;
    float *Dn = D + (int64_t)n * P * ld;
    float cmax[CX_RPT];
    int crow[CX_RPT];
#pragma unroll
    for (int k = 0; k < CX_RPT; ++k) {
        cmax[k] = -1.f;
        crow[k] = 0;
    }
    const int i_end = min(P, (rb + 1) * CX_RB);
    for (int i = rb * CX_RB; i < i_end; ++i) {
        const int par = i & 1;
        float *row = Dn + (int64_t)i * ld;
        float d[CX_RPT];
        float m = INFINITY;
        int mi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < CX_RPT; ++k) {
            const int j = tid + 256 * k;
            d[k] = j < P ? row[j] : INFINITY;
            if (d[k] < m) {          // j grows with k: the first of equal values stays
                m = d[k];
                mi = j;
            }
        }
        cx_block_argmin(m, mi, shv[par], shi[par]);
        const float den = m + 1e-5f;
        float w[CX_RPT];
        double s = 0.0, e = 0.0;
#pragma unroll
        for (int k = 0; k < CX_RPT; ++k) {
            const int j = tid + 256 * k;
            w[k] = 0.f;
            if (j < P) {
                w[k] = expf((b - d[k] / den) / h);
                s += (double)w[k];
                e += (double)w[k] * (double)d[k];
            }
        }
        cx_block_sum2(s, e, shd[par]);
        const float sf = (float)s;
#pragma unroll
        for (int k = 0; k < CX_RPT; ++k) {
            const int j = tid + 256 * k;
            if (j < P) {
                const float cx = w[k] / sf;
                row[j] = d[k] > 0.f ? cx : -cx;      // the sign carries the clamp pattern; cx itself is >= 0
                if (cx > cmax[k]) {                  // rows ascend: the first of equal values stays
                    cmax[k] = cx;
                    crow[k] = i;
                }
            }
        }
        if (tid == 0) {
            rowmin[(int64_t)n * P + i] = m;
            argmin[(int64_t)n * P + i] = mi;
            rowE[(int64_t)n * P + i] = (float)(e / s);
        }
    }
#pragma unroll
    for (int k = 0; k < CX_RPT; ++k) {
        const int j = tid + 256 * k;
        if (j < P) {
            const unsigned long long pk = ((unsigned long long)__builtin_bit_cast(unsigned, cmax[k]) << 32) | (unsigned long long)(0xffffffffu - (unsigned)crow[k]);
            atomicMax(colpack + (int64_t)n * P + j, pk);      // integer max: the order of arrival does not matter
        }
    }
}

__global__ void __launch_bounds__(256) cx_finalize_kernel(const unsigned long long *colpack, int N, int P, float *colmax, int32_t *argmax, float *CS,
                                                          float *gcoef) {
    __shared__ double sh[256];
    const int n = blockIdx.x;
    double s = 0.0;
    for (int j = threadIdx.x; j < P; j += 256) {
        const unsigned long long pk = colpack[(int64_t)n * P + j];
        const float v = __builtin_bit_cast(float, (unsigned)(pk >> 32));
        colmax[(int64_t)n * P + j] = v;
        argmax[(int64_t)n * P + j] = (int32_t)(0xffffffffu - (unsigned)(pk & 0xffffffffull));
        s += (double)v;
    }
    s = tnr_block_sum256(s, sh);
    if (threadIdx.x == 0) {
        const float cs = (float)(s / (double)P);
        CS[n] = cs;
        gcoef[n] = (float)(-1.0 / ((double)N * (double)P * (double)cs));
    }
}

__global__ void cx_loss_kernel(const float *CS, int N, float *loss) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0.0;
        for (int n = 0; n < N; ++n) s += -log((double)CS[n]);
        loss[0] = (float)(s / (double)N);
    }
}

// d at (argmax_j, j): one wave per column
__global__ void __launch_bounds__(256) cx_dwin_kernel(const float *xh, const float *yh, const int32_t *argmax, int P, int C, int64_t total, float *dwin) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= total) return;
    const int64_t n = g / P;
    const float *xr = xh + (n * P + argmax[g]) * C, *yr = yh + g * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += xr[c] * yr[c];
    s = cx_wave_sum(s);
    if (lane == 0) dwin[g] = fmaxf((1.f - s) * 0.5f, 0.f);
}

__global__ void __launch_bounds__(256) cx_grad_rows_kernel(float *D, int P, int ld, int rblocks, float h, const float *rowmin, const int32_t *argmin,
                                                           const float *rowE, const int32_t *argmax, const float *gcoef, const float *dwin) {
    __shared__ double shd[2][8];
    const int n = blockIdx.x / rblocks, rb = blockIdx.x % rblocks, tid = threadIdx.x;
    float *Dn = D + (int64_t)n * P * ld;
    int am[CX_RPT];
    float dw[CX_RPT];
#pragma unroll
    for (int k = 0; k < CX_RPT; ++k) {
        const int j = tid + 256 * k;
        am[k] = j < P ? argmax[(int64_t)n * P + j] : -1;
        dw[k] = j < P ? dwin[(int64_t)n * P + j] : 0.f;
    }
    const float g = gcoef[n];
    const int i_end = min(P, (rb + 1) * CX_RB);
    for (int i = rb * CX_RB; i < i_end; ++i) {
        float *row = Dn + (int64_t)i * ld;
        float v[CX_RPT];
        double A = 0.0, B = 0.0;
#pragma unroll
        for (int k = 0; k < CX_RPT; ++k) {
            const int j = tid + 256 * k;
            v[k] = j < P ? row[j] : 0.f;
            if (am[k] == i) {
                A += (double)fabsf(v[k]);
                B += (double)fabsf(v[k]) * (double)dw[k];
            }
        }
        cx_block_sum2(A, B, shd[i & 1]);
        const float Af = (float)A;
        const float den = rowmin[(int64_t)n * P + i] + 1e-5f;
        const int kstar = argmin[(int64_t)n * P + i];
        const float T = g * (float)(B - A * (double)rowE[(int64_t)n * P + i]);      // sum_k q_ik d_ik
#pragma unroll
        for (int k = 0; k < CX_RPT; ++k) {
            const int j = tid + 256 * k;
            if (j < P) {
                const float q = g * ((am[k] == i ? 1.f : 0.f) - Af) * fabsf(v[k]);
                float dd = -q / (h * den);
                if (j == kstar) dd += T / (h * den * den);
                row[j] = v[k] > 0.f ? -0.5f * dd : 0.f;       // a negative (or zero) entry marks d == 0: the clamp passes no gradient
            }
        }
    }
}

__global__ void __launch_bounds__(256) cx_norm_bwd_kernel(const float *dxh, const float *xh, const float *nrm, int HW, int P, int C, const int32_t *inv,
                                                          int64_t total, float *dx, int ct, int co) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= total) return;
    const int64_t n = g / HW;
    const int s = (int)(g - n * HW);
    const int slot = inv ? inv[s] : s;
    float *dst = dx + g * ct + co;
    if (slot < 0) {
        for (int c = lane; c < C; c += 64) dst[c] = 0.f;
        return;
    }
    const int64_t r = n * P + slot;
    float gv[8], xv[8], dot = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = lane + 64 * k;
        gv[k] = c < C ? dxh[r * C + c] : 0.f;
        xv[k] = c < C ? xh[r * C + c] : 0.f;
        dot += gv[k] * xv[k];
    }
    dot = cx_wave_sum(dot);
    const float den = nrm[r];
    if (!(den > 1e-12f)) dot = 0.f;          // below the eps of F.normalize the division is by a constant
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = lane + 64 * k;
        if (c < C) dst[c] = (gv[k] - xv[k] * dot) / den;
    }
}

inline int cx_check_view(const char *who, tnr_view x, int N, int H, int W, int C, int P) {
    TNR_REQUIRE(x.ptr != nullptr && N > 0 && H > 0 && W > 0, "%s: bad shape %d x %d x %d", who, N, H, W);
    TNR_REQUIRE(C >= 64 && C <= 512 && (C % 64) == 0, "%s: C = %d is not a multiple of 64 in 64 .. 512", who, C);
    TNR_REQUIRE((x.ctot % 4) == 0 && (x.coff % 4) == 0 && x.coff >= 0 && x.coff + C <= x.ctot, "%s: bad view (ctot %d, coff %d, C %d)", who,
                x.ctot, x.coff, C);
    TNR_REQUIRE((int64_t)N * H * W < ((int64_t)1 << 31), "%s: too many pixels", who);
    TNR_REQUIRE(P > 0 && P <= CX_MAXP && P <= H * W, "%s: P = %d positions (1 .. min(%d, H W))", who, P, CX_MAXP);
    return TNR_OK;
}

inline int cx_check_np(const char *who, int N, int P, int C) {
    TNR_REQUIRE(N > 0 && N <= 65535 && P > 0 && P <= CX_MAXP, "%s: bad shape N %d, P %d (P <= %d)", who, N, P, CX_MAXP);
    TNR_REQUIRE(C >= 64 && C <= 512 && (C % 64) == 0, "%s: C = %d is not a multiple of 64 in 64 .. 512", who, C);
    return TNR_OK;
}

template <bool GRAD>
int cx_launch_gemm(const char *who, const CxGemm &a, int N, int mma, hipStream_t s) {
    TNR_REQUIRE(mma == TNR_MMA_F32 || mma == TNR_MMA_BF16X3, "%s: mma %d (TNR_MMA_F32 or TNR_MMA_BF16X3)", who, mma);
    const int64_t wgs = (int64_t)N * a.mtiles * a.ntiles;
    if (mma == TNR_MMA_BF16X3)
        hipLaunchKernelGGL((cx_gemm_kernel<true, GRAD>), dim3((unsigned)wgs), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((cx_gemm_kernel<false, GRAD>), dim3((unsigned)wgs), dim3(256), 0, s, a);
    return tnr_check_launch(who);
}

}  // namespace

extern "C" int64_t tnr_cx_sums_workspace_bytes(int32_t N, int32_t P, int32_t C) {
    if (N <= 0 || P <= 0 || C <= 0) return 0;
    return tnr_cdiv64((int64_t)N * P, CX_SUM_CHUNK) * C * (int64_t)sizeof(double);
}

extern "C" int tnr_cx_sums(tnr_view y, int32_t N, int32_t H, int32_t W, int32_t C, const int32_t *idx, int32_t P, float *sums, void *ws,
                           int64_t ws_bytes, void *stream) {
    if (int rc = cx_check_view("cx_sums", y, N, H, W, C, P)) return rc;
    TNR_REQUIRE(idx != nullptr || P == H * W, "cx_sums: P = %d without an index list (H W = %d)", P, H * W);
    TNR_REQUIRE(sums != nullptr && ws != nullptr && ws_bytes >= tnr_cx_sums_workspace_bytes(N, P, C), "cx_sums: workspace of %lld bytes needed",
                (long long)tnr_cx_sums_workspace_bytes(N, P, C));
    const int64_t total = (int64_t)N * P;
    const int nblk = (int)tnr_cdiv64(total, CX_SUM_CHUNK);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cx_sums_partial_kernel, dim3(nblk), dim3(256), 0, s, y.ptr, y.ctot, y.coff, C, H * W, P, idx, total, (double *)ws);
    if (int rc = tnr_check_launch("cx_sums_partial")) return rc;
    hipLaunchKernelGGL(cx_sums_reduce_kernel, dim3(1), dim3(256), 0, s, (const double *)ws, nblk, C, (double)total, sums);
    return tnr_check_launch("cx_sums_reduce");
}

extern "C" int tnr_cx_prepare(tnr_view x, int32_t N, int32_t H, int32_t W, int32_t C, const int32_t *idx, int32_t P, const float *sums, float *xh,
                              float *nrm, void *stream) {
    if (int rc = cx_check_view("cx_prepare", x, N, H, W, C, P)) return rc;
    TNR_REQUIRE(idx != nullptr || P == H * W, "cx_prepare: P = %d without an index list (H W = %d)", P, H * W);
    TNR_REQUIRE(sums != nullptr && xh != nullptr && nrm != nullptr, "cx_prepare: null pointer");
    const int64_t total = (int64_t)N * P;
    hipLaunchKernelGGL(cx_prepare_kernel, dim3((unsigned)tnr_cdiv64(total, 4)), dim3(256), 0, (hipStream_t)stream, x.ptr, x.ctot, x.coff, C, H * W, P,
                       idx, total, sums, xh, nrm);
    return tnr_check_launch("cx_prepare");
}

extern "C" int64_t tnr_cx_matrix_bytes(int32_t N, int32_t P) {
    if (N <= 0 || P <= 0) return 0;
    return (int64_t)N * P * cx_ld(P) * (int64_t)sizeof(float);
}

extern "C" int tnr_cx_distance(const float *xh, const float *yh, int32_t N, int32_t P, int32_t C, int32_t mma, float *D, void *stream) {
    if (int rc = cx_check_np("cx_distance", N, P, C)) return rc;
    TNR_REQUIRE(xh != nullptr && yh != nullptr && D != nullptr, "cx_distance: null pointer");
    CxGemm a;
    a.A = xh;
    a.B = yh;
    a.out = D;
    a.M = P;
    a.K = C;
    a.lda = C;
    a.NB = P;
    a.ldb = C;
    a.ldo = cx_ld(P);
    a.mtiles = tnr_cdiv(P, CX_PT);
    a.ntiles = tnr_cdiv(P, 64);
    a.a_img = a.b_img = (int64_t)P * C;
    a.o_img = (int64_t)P * cx_ld(P);
    return cx_launch_gemm<false>("cx_distance", a, N, mma, (hipStream_t)stream);
}

extern "C" int tnr_cx_rows(float *D, int32_t N, int32_t P, float b, float h, float *rowmin, int32_t *argmin, float *rowE, void *colpack,
                           void *stream) {
    if (int rc = cx_check_np("cx_rows", N, P, 64)) return rc;
    TNR_REQUIRE(D != nullptr && rowmin != nullptr && argmin != nullptr && rowE != nullptr && colpack != nullptr, "cx_rows: null pointer");
    TNR_REQUIRE(h > 0.f, "cx_rows: band width %g", (double)h);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(colpack, 0, (size_t)N * P * sizeof(unsigned long long), s) != hipSuccess) {
        tnr_set_error("cx_rows: hipMemsetAsync failed");
        return TNR_EINVAL;
    }
    const int rblocks = tnr_cdiv(P, CX_RB);
    hipLaunchKernelGGL(cx_rows_kernel, dim3((unsigned)(N * rblocks)), dim3(256), 0, s, D, P, cx_ld(P), rblocks, b, h, rowmin, argmin, rowE,
                       (unsigned long long *)colpack);
    return tnr_check_launch("cx_rows");
}

extern "C" int tnr_cx_finalize(const void *colpack, int32_t N, int32_t P, float *colmax, int32_t *argmax, float *CS, float *gcoef, float *loss,
                               void *stream) {
    if (int rc = cx_check_np("cx_finalize", N, P, 64)) return rc;
    TNR_REQUIRE(colpack != nullptr && colmax != nullptr && argmax != nullptr && CS != nullptr && gcoef != nullptr && loss != nullptr,
                "cx_finalize: null pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cx_finalize_kernel, dim3(N), dim3(256), 0, s, (const unsigned long long *)colpack, N, P, colmax, argmax, CS, gcoef);
    if (int rc = tnr_check_launch("cx_finalize")) return rc;
    hipLaunchKernelGGL(cx_loss_kernel, dim3(1), dim3(64), 0, s, CS, N, loss);
    return tnr_check_launch("cx_loss");
}

extern "C" int tnr_cx_grad_rows(float *D, const float *xh, const float *yh, int32_t N, int32_t P, int32_t C, float h, const float *rowmin,
                                const int32_t *argmin, const float *rowE, const int32_t *argmax, const float *gcoef, float *dwin, void *stream) {
    if (int rc = cx_check_np("cx_grad_rows", N, P, C)) return rc;
    TNR_REQUIRE(D != nullptr && xh != nullptr && yh != nullptr && rowmin != nullptr && argmin != nullptr && rowE != nullptr && argmax != nullptr &&
                    gcoef != nullptr && dwin != nullptr, "cx_grad_rows: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (int64_t)N * P;
    hipLaunchKernelGGL(cx_dwin_kernel, dim3((unsigned)tnr_cdiv64(total, 4)), dim3(256), 0, s, xh, yh, argmax, P, C, total, dwin);
    if (int rc = tnr_check_launch("cx_dwin")) return rc;
    const int rblocks = tnr_cdiv(P, CX_RB);
    hipLaunchKernelGGL(cx_grad_rows_kernel, dim3((unsigned)(N * rblocks)), dim3(256), 0, s, D, P, cx_ld(P), rblocks, h, rowmin, argmin, rowE, argmax,
                       gcoef, dwin);
    return tnr_check_launch("cx_grad_rows");
}

extern "C" int tnr_cx_grad_gemm(const float *G, const float *yh, int32_t N, int32_t P, int32_t C, int32_t mma, float *dxh, void *stream) {
    if (int rc = cx_check_np("cx_grad_gemm", N, P, C)) return rc;
    TNR_REQUIRE(G != nullptr && yh != nullptr && dxh != nullptr, "cx_grad_gemm: null pointer");
    CxGemm a;
    a.A = G;
    a.B = yh;
    a.out = dxh;
    a.M = P;
    a.K = P;
    a.lda = cx_ld(P);
    a.NB = C;
    a.ldb = C;
    a.ldo = C;
    a.mtiles = tnr_cdiv(P, CX_PT);
    a.ntiles = C / 64;
    a.a_img = (int64_t)P * cx_ld(P);
    a.b_img = a.o_img = (int64_t)P * C;
    return cx_launch_gemm<true>("cx_grad_gemm", a, N, mma, (hipStream_t)stream);
}

extern "C" int tnr_cx_norm_bwd(const float *dxh, const float *xh, const float *nrm, int32_t N, int32_t H, int32_t W, int32_t C, int32_t P,
                               const int32_t *inv, tnr_view dx, void *stream) {
    if (int rc = cx_check_view("cx_norm_bwd", dx, N, H, W, C, P)) return rc;
    TNR_REQUIRE(inv != nullptr || P == H * W, "cx_norm_bwd: P = %d without an inverse index list (H W = %d)", P, H * W);
    TNR_REQUIRE(dxh != nullptr && xh != nullptr && nrm != nullptr, "cx_norm_bwd: null pointer");
    const int64_t total = (int64_t)N * H * W;
    hipLaunchKernelGGL(cx_norm_bwd_kernel, dim3((unsigned)tnr_cdiv64(total, 4)), dim3(256), 0, (hipStream_t)stream, dxh, xh, nrm, H * W, P, C, inv,
                       total, dx.ptr, dx.ctot, dx.coff);
    return tnr_check_launch("cx_norm_bwd");
}
