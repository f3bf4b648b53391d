// The optimisers beside Adam (reference codes/models/optimizers.py:100-129): SGD, RMSprop, MADGRAD, AdamP, SGDP and Ranger over a
// network's flat fp32 parameter / gradient buffers.  All of them are HBM-bound.
//
// A flat buffer is described by three device tables the host builds once per layout (trainner_amd/flat.py SegTable):
//   segs   [nseg][6] int64   one row per parameter tensor: offset, numel, rows (size(0) when dim() > 1, else 0), row length, dim(),
//                            index of the tensor's first row in the buffer-wide row numbering (-1 without rows)
//   chunks [nchunk][3] int64 the tensors cut into pieces of at most 1024 elements: offset, count, segment.  Every elementwise launch
//                            walks THIS table, one block per chunk and four elements per thread, so the alignment gaps between the
//                            tensors are never read or written and every access of a full chunk is 16 bytes wide (tensors start
//                            256-B aligned, chunks 4096 B apart)
//   rowseg [nrows] int32     the segment of every row (tensors with dim() > 1 only)
// Row-wise sums (AdamP / SGDP projection, Ranger's gradient centralisation) take one wave per row and add in fp64 in a fixed order:
// no atomics, bit-reproducible run to run.  An optimiser step is a fixed number of launches per flat buffer (1, 2 or 4), makes no
// device->host copy, and every launch that writes parameters or state first reads the fault latch as adam_kernel does.
#include "common.h"

namespace {

struct Seg { int64_t off, numel, rows, rowlen, dim, rowbase; };
struct Chunk { int64_t off, cnt, seg; };

constexpr int MAX_GRID = 2048;   // a chunk holds at most 1024 elements (256 threads x 4; trainner_amd/flat.py CHUNK)

__device__ __forceinline__ void ld4(const float *a, int64_t e, int nv, float *o) {
    if (nv == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(a + e);
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = k < nv ? a[e + k] : 0.f;
    }
}

__device__ __forceinline__ void st4(float *a, int64_t e, int nv, const float *o) {
    if (nv == 4) {
        f32x4 v = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4 *>(a + e) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nv) a[e + k] = o[k];
    }
}

// The thread's slice of chunk c: element index e and the number of valid elements nv (0: nothing to do).
__device__ __forceinline__ int chunk_slice(const Chunk &ck, int64_t &e) {
    const int64_t l0 = 4 * (int64_t)threadIdx.x;
    e = ck.off + l0;
    const int64_t left = ck.cnt - l0;
    return left >= 4 ? 4 : (left > 0 ? (int)left : 0);
}

// The buffer-wide row of a thread's first element; the rows of its next elements follow by counting (a chunk never crosses a tensor),
// so ONE 64-bit division per thread serves its four elements.
struct RowWalk {
    int64_t r, rem, len;
    __device__ __forceinline__ RowWalk(const Seg &sg, int64_t e, bool needed) : r(0), rem(0), len(sg.rowlen) {
        if (needed) {
            const int64_t l = e - sg.off, q = l / sg.rowlen;
            r = sg.rowbase + q;
            rem = l - q * sg.rowlen;
        }
    }
    __device__ __forceinline__ void next() {
        if (++rem == len) {
            rem = 0;
            ++r;
        }
    }
};

#define TNR_LATCH(fault) if ((fault) != nullptr && *(fault) != 0u) return     /* uniform: every thread reads the same word */

// ---------------------------------------------------------------------------------- elementwise rules
// torch.optim.SGD: g += wd p; buf = momentum buf + g (from a zero buffer the first step gives buf = g); p -= lr buf
__global__ void sgd_kernel(float *p, const float *g, float *buf, const Chunk *chunks, int nchunks, float neg_lr, float momentum, float wd,
                           const unsigned *fault) {
    TNR_LATCH(fault);
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        int64_t e;
        const int nv = chunk_slice(chunks[c], e);
        if (nv == 0) continue;
        float pv[4], gv[4], bv[4] = {0.f, 0.f, 0.f, 0.f};
        ld4(p, e, nv, pv);
        ld4(g, e, nv, gv);
        if (buf) ld4(buf, e, nv, bv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float gr = gv[k];
            if (wd != 0.f) gr += wd * pv[k];
            if (buf) {
                bv[k] = bv[k] * momentum + gr;
                gr = bv[k];
            }
            pv[k] = pv[k] + neg_lr * gr;
        }
        if (buf) st4(buf, e, nv, bv);
        st4(p, e, nv, pv);
    }
}

// torch.optim.RMSprop (not centered, no momentum): sq = alpha sq + (1 - alpha) g g; p += (-lr g) / (sqrt(sq) + eps)
__global__ void rmsprop_kernel(float *p, const float *g, float *sq, const Chunk *chunks, int nchunks, float neg_lr, float alpha, float oma,
                               float eps, float wd, const unsigned *fault) {
    TNR_LATCH(fault);
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        int64_t e;
        const int nv = chunk_slice(chunks[c], e);
        if (nv == 0) continue;
        float pv[4], gv[4], sv[4];
        ld4(p, e, nv, pv);
        ld4(g, e, nv, gv);
        ld4(sq, e, nv, sv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float gr = gv[k];
            if (wd != 0.f) gr += wd * pv[k];
            sv[k] = sv[k] * alpha + (oma * gr) * gr;
            const float avg = sqrtf(sv[k]) + eps;
            pv[k] = pv[k] + (neg_lr * gr) / avg;
        }
        st4(sq, e, nv, sv);
        st4(p, e, nv, pv);
    }
}

// MADGRAD (madgrad.py:85-179).  lamb = (lr + eps) sqrt(k + 1) and decay_mul = 1 - (lr + eps) decay come from the host; x0 == nullptr
// is the momentum-0 form, where x0 is recomputed from p, s and the OLD rms.
__global__ void madgrad_kernel(float *p, const float *g, float *gss, float *s, const float *x0, const Chunk *chunks, int nchunks, float lamb,
                               float eps, float decay, float decay_mul, int adamw, float ck, float omck, const unsigned *fault) {
    TNR_LATCH(fault);
    const float third = (float)(1.0 / 3.0);
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        int64_t e;
        const int nv = chunk_slice(chunks[c], e);
        if (nv == 0) continue;
        float pv[4], gv[4], qv[4], sv[4], xv[4] = {0.f, 0.f, 0.f, 0.f};
        ld4(p, e, nv, pv);
        ld4(g, e, nv, gv);
        ld4(gss, e, nv, qv);
        ld4(s, e, nv, sv);
        if (x0) ld4(x0, e, nv, xv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float gr = gv[k];
            if (decay != 0.f) {
                if (adamw) pv[k] *= decay_mul;
                else gr += decay * pv[k];
            }
            if (!x0) xv[k] = pv[k] + sv[k] / (powf(qv[k], third) + eps);
            qv[k] = qv[k] + (lamb * gr) * gr;
            const float rms = powf(qv[k], third) + eps;
            sv[k] = sv[k] + lamb * gr;
            const float z = xv[k] + (-sv[k]) / rms;
            pv[k] = x0 ? pv[k] * omck + ck * z : z;
        }
        st4(gss, e, nv, qv);
        st4(s, e, nv, sv);
        st4(p, e, nv, pv);
    }
}

// ---------------------------------------------------------------------------------- AdamP / SGDP
enum { RULE_ADAMP = 0, RULE_SGDP = 1 };
struct ProjP {
    float b1, omb1, b2, omb2, bc2_sqrt, eps;       // AdamP moments; SGDP: b1 = momentum, omb1 = 1 - dampening
    float step, wd, decay_1, decay_r;              // p = p decay - step perturb; decay_1 / decay_r: weight-decay ratio 1 / wd_ratio
    int nesterov;
};

// The perturbation of one element from its own NEW moments and gradient (pass 1 wrote them; passes 2 and 4 evaluate the very same
// fp32 expression, so both see the same bits).
template <int RULE>
__device__ __forceinline__ float perturb_of(float g, float m, float v, const ProjP &P) {
    if (RULE == RULE_ADAMP) {
        const float denom = sqrtf(v) / P.bc2_sqrt + P.eps;
        return P.nesterov ? (P.b1 * m + P.omb1 * g) / denom : m / denom;
    }
    return P.nesterov ? g + P.b1 * m : m;
}

template <int RULE>
__global__ void proj_moments_kernel(const float *g, float *m, float *v, const Chunk *chunks, int nchunks, ProjP P, const unsigned *fault) {
    TNR_LATCH(fault);
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        int64_t e;
        const int nv = chunk_slice(chunks[c], e);
        if (nv == 0) continue;
        float gv[4], mv[4], vv[4];
        ld4(g, e, nv, gv);
        ld4(m, e, nv, mv);
        if (RULE == RULE_ADAMP) ld4(v, e, nv, vv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mv[k] = mv[k] * P.b1 + P.omb1 * gv[k];
            if (RULE == RULE_ADAMP) vv[k] = vv[k] * P.b2 + (P.omb2 * gv[k]) * gv[k];
        }
        st4(m, e, nv, mv);
        if (RULE == RULE_ADAMP) st4(v, e, nv, vv);
    }
}

// Fixed-order sum of NS values per wave of a 256-thread block (sh: [NS][256] doubles); valid in lane 0 of each wave.
template <int NS>
__device__ __forceinline__ void wave_sums(double (*sh)[256], const double *a, double *out) {
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < NS; ++k) sh[k][tid] = a[k];
    __syncthreads();
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        if (lane < s)
#pragma unroll
            for (int k = 0; k < NS; ++k) sh[k][tid] += sh[k][tid + s];
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) out[k] = sh[k][tid];
    __syncthreads();
}

// rowsums[r] = {g.p, g.g, p.p, p.perturb} of row r, one wave per row
template <int RULE>
__global__ void proj_rowsums_kernel(const float *p, const float *g, const float *m, const float *v, const Seg *segs, const int *rowseg,
                                    int64_t nrows, ProjP P, double *rowsums) {
    __shared__ double sh[4][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t r0 = (int64_t)blockIdx.x * 4; r0 < nrows; r0 += (int64_t)gridDim.x * 4) {
        const int64_t r = r0 + wave;
        double a[4] = {0, 0, 0, 0};
        if (r < nrows) {
            const Seg sg = segs[rowseg[r]];
            const int64_t base = sg.off + (r - sg.rowbase) * sg.rowlen;
            for (int64_t i = lane; i < sg.rowlen; i += 64) {
                const float gv = g[base + i], pv = p[base + i];
                const float q = perturb_of<RULE>(gv, m[base + i], RULE == RULE_ADAMP ? v[base + i] : 0.f, P);
                a[0] += (double)gv * (double)pv;
                a[1] += (double)gv * (double)gv;
                a[2] += (double)pv * (double)pv;
                a[3] += (double)pv * (double)q;
            }
        }
        double t[4];
        wave_sums<4>(sh, a, t);
        if (lane == 0 && r < nrows) {
#pragma unroll
            for (int k = 0; k < 4; ++k) rowsums[r * 4 + k] = t[k];
        }
    }
}

// |cosine(g, p)| with F.cosine_similarity's clamp: each norm is clamped from below by eps
__device__ __forceinline__ double abs_cos(double gp, double gg, double pp, double eps) {
    double ng = sqrt(gg), np = sqrt(pp);
    if (ng < eps) ng = eps;
    if (np < eps) np = eps;
    return fabs(gp) / (ng * np);
}

// One block per tensor: the decision the reference takes on the host with `.max() < delta / sqrt(row length)` (adamp.py:57-71).
// segdec[s] = {mode (0 none, 1 per row, 2 whole tensor), whole-tensor norm + eps, whole-tensor sum(p_n perturb), -};
// rowcoef[r] = {row norm + eps, sum_row(p_n perturb)} with p_n = p / (norm + eps).
__global__ void proj_decide_kernel(const Seg *segs, const double *rowsums, double delta, double eps, float *rowcoef, float *segdec) {
    __shared__ double sh[256];
    const Seg sg = segs[blockIdx.x];
    const int tid = threadIdx.x;
    if (sg.rows == 0) {          // 1-D tensors are never projected
        if (tid == 0) segdec[4 * (int64_t)blockIdx.x] = 0.f;
        return;
    }
    double mx = 0, t[4] = {0, 0, 0, 0};
    for (int64_t r = tid; r < sg.rows; r += 256) {
        const double *S = rowsums + (sg.rowbase + r) * 4;
        const double c = abs_cos(S[0], S[1], S[2], eps);
        if (c > mx || c != c) mx = c;
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] += S[k];
        const float den = (float)sqrt(S[2]) + (float)eps;
        rowcoef[(sg.rowbase + r) * 2 + 0] = den;
        rowcoef[(sg.rowbase + r) * 2 + 1] = (float)(S[3] / (double)den);
    }
    sh[tid] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const double o = sh[tid + s];
            if (o > sh[tid] || o != o) sh[tid] = o;
        }
        __syncthreads();
    }
    mx = sh[0];
    __syncthreads();
    double T[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) T[k] = tnr_block_sum256(t[k], sh);
    if (tid == 0) {
        float mode = 0.f, den = 1.f, dotn = 0.f;
        if (mx < delta / sqrt((double)sg.rowlen)) {
            mode = 1.f;
        } else if (abs_cos(T[0], T[1], T[2], eps) < delta / sqrt((double)sg.numel)) {
            mode = 2.f;
            den = (float)sqrt(T[2]) + (float)eps;
            dotn = (float)(T[3] / (double)den);
        }
        float *o = segdec + 4 * (int64_t)blockIdx.x;
        o[0] = mode; o[1] = den; o[2] = dotn; o[3] = 0.f;
    }
}

// SGDP without Nesterov: the reference's perturbation IS its momentum buffer (d_p = buf, then `perturb -= ...` in place), so the
// projected perturbation is what the buffer holds afterwards: kept, the state resumes in either engine.
template <int RULE>
__global__ void proj_apply_kernel(float *p, const float *g, float *m, const float *v, const Chunk *chunks, int nchunks, const Seg *segs,
                                  const float *rowcoef, const float *segdec, ProjP P, const unsigned *fault) {
    TNR_LATCH(fault);
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Chunk ck = chunks[c];
        int64_t e;
        const int nv = chunk_slice(ck, e);
        if (nv == 0) continue;
        const Seg sg = segs[ck.seg];
        const float *dec = segdec + 4 * ck.seg;
        const int mode = (int)dec[0];
        float pv[4], gv[4], mv[4], vv[4] = {0.f, 0.f, 0.f, 0.f};
        ld4(p, e, nv, pv);
        ld4(g, e, nv, gv);
        ld4(m, e, nv, mv);
        if (RULE == RULE_ADAMP) ld4(v, e, nv, vv);
        const float decay = mode ? P.decay_r : P.decay_1;
        RowWalk row(sg, e, mode == 1);
#pragma unroll
        for (int k = 0; k < 4; ++k, row.next()) {
            if (k >= nv) break;
            float q = perturb_of<RULE>(gv[k], mv[k], vv[k], P);
            if (mode == 1) {
                q -= (pv[k] / rowcoef[2 * row.r]) * rowcoef[2 * row.r + 1];
            } else if (mode == 2) {
                q -= (pv[k] / dec[1]) * dec[2];
            }
            float x = pv[k];
            if (P.wd > 0.f) x *= decay;
            pv[k] = x - P.step * q;
            mv[k] = q;
        }
        if (RULE == RULE_SGDP && !P.nesterov && mode != 0) st4(m, e, nv, mv);
        st4(p, e, nv, pv);
    }
}

// ---------------------------------------------------------------------------------- Ranger
// rowmean[r] = mean of the gradient's row r (gradient centralisation, ranger.py:6-15), one wave per row
__global__ void row_mean_kernel(const float *g, const Seg *segs, const int *rowseg, int64_t nrows, float *rowmean) {
    __shared__ double sh[1][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t r0 = (int64_t)blockIdx.x * 4; r0 < nrows; r0 += (int64_t)gridDim.x * 4) {
        const int64_t r = r0 + wave;
        double a[1] = {0};
        int64_t len = 1;
        if (r < nrows) {
            const Seg sg = segs[rowseg[r]];
            const int64_t base = sg.off + (r - sg.rowbase) * sg.rowlen;
            len = sg.rowlen;
            for (int64_t i = lane; i < len; i += 64) a[0] += (double)g[base + i];
        }
        double t[1];
        wave_sums<1>(sh, a, t);
        if (lane == 0 && r < nrows) rowmean[r] = (float)(t[0] / (double)len);
    }
}

// Ranger (ranger.py:96-208): centralised gradient -> Adam moments -> (rectified) step -> lookahead, in one launch.
// gc_min_dim: tensors with dim() > gc_min_dim are centralised (1; 3 with gc_conv_only; a huge value switches it off).
// The reference's unrectified branch aliases G to exp_avg, so its `G += wd p` lands in exp_avg too: kept.
__global__ void ranger_kernel(float *p, const float *g, float *m, float *v, float *slow, const Chunk *chunks, int nchunks, const Seg *segs,
                              const float *rowmean, int gc_min_dim, float b1, float omb1, float b2, float omb2, float eps, float wd,
                              float step, int rectified, int look, float alpha, const unsigned *fault) {
    TNR_LATCH(fault);
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Chunk ck = chunks[c];
        int64_t e;
        const int nv = chunk_slice(ck, e);
        if (nv == 0) continue;
        const Seg sg = segs[ck.seg];
        const bool gc = sg.rows > 0 && sg.dim > gc_min_dim;
        float pv[4], gv[4], mv[4], vv[4], sv[4] = {0.f, 0.f, 0.f, 0.f};
        ld4(p, e, nv, pv);
        ld4(g, e, nv, gv);
        ld4(m, e, nv, mv);
        ld4(v, e, nv, vv);
        if (look) ld4(slow, e, nv, sv);
        RowWalk row(sg, e, gc);
#pragma unroll
        for (int k = 0; k < 4; ++k, row.next()) {
            if (k >= nv) break;
            float gr = gv[k];
            if (gc) gr = gr - rowmean[row.r];
            mv[k] = mv[k] * b1 + omb1 * gr;
            vv[k] = vv[k] * b2 + (omb2 * gr) * gr;
            float G = rectified ? mv[k] / (sqrtf(vv[k]) + eps) : mv[k];
            if (wd != 0.f) {
                G = G + wd * pv[k];
                if (!rectified) mv[k] = G;
            }
            pv[k] = pv[k] - step * G;
            if (look) {
                sv[k] = sv[k] + alpha * (pv[k] - sv[k]);
                pv[k] = sv[k];
            }
        }
        st4(m, e, nv, mv);
        st4(v, e, nv, vv);
        if (look) st4(slow, e, nv, sv);
        st4(p, e, nv, pv);
    }
}

// ---------------------------------------------------------------------------------- stochastic weight averaging
// torch.optim.swa_utils.AveragedModel's running mean, avg.lerp_(p, w) with w = fp32(1 / (n_averaged + 1)), in ATen's lerp form:
// w = 1 copies p exactly, p == avg leaves avg's bits alone.  A pure stream over the WHOLE flat buffer (alignment gaps included: they
// are zero in both buffers and stay zero), 12 bytes per element: 256 threads x 16 bytes per block, at most MAX_GRID blocks, the rest
// by grid-stride.  VEC needs both pointers 16-byte aligned (flat buffers are); the n % 4 tail elements go to the first block.
__device__ __forceinline__ float swa_lerp(float a, float p, float w) {
    const float d = p - a;
    return w < 0.5f ? a + w * d : p - d * (1.f - w);
}

template <bool VEC>
__global__ void swa_update_kernel(float *avg, const float *p, int64_t n, float w, const unsigned *fault) {
    TNR_LATCH(fault);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (VEC) {
        const int64_t n4 = n >> 2;
        for (int64_t i = tid; i < n4; i += stride) {
            const f32x4 pv = reinterpret_cast<const f32x4 *>(p)[i];
            f32x4 av = reinterpret_cast<f32x4 *>(avg)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) av[k] = swa_lerp(av[k], pv[k], w);
            reinterpret_cast<f32x4 *>(avg)[i] = av;
        }
        const int64_t e = (n4 << 2) + tid;
        if (tid < 4 && e < n) avg[e] = swa_lerp(avg[e], p[e], w);
    } else {
        for (int64_t e = tid; e < n; e += stride) avg[e] = swa_lerp(avg[e], p[e], w);
    }
}

inline unsigned grid_chunks(int64_t n) { return (unsigned)(n > MAX_GRID ? MAX_GRID : (n < 1 ? 1 : n)); }
inline unsigned grid_rows(int64_t nrows) { return grid_chunks(tnr_cdiv64(nrows, 4)); }

template <int RULE>
int proj_step(float *p, const float *g, float *m, float *v, const Chunk *chunks, int nchunks, const Seg *segs, int nseg, const int *rowseg,
              int64_t nrows, void *ws, const ProjP &P, double delta, const unsigned *fault, hipStream_t s) {
    hipLaunchKernelGGL(proj_moments_kernel<RULE>, dim3(grid_chunks(nchunks)), dim3(256), 0, s, g, m, v, chunks, nchunks, P, fault);
    double *rowsums = (double *)ws;
    float *rowcoef = (float *)(rowsums + 4 * (nrows > 0 ? nrows : 1));
    float *segdec = rowcoef + 2 * (nrows > 0 ? nrows : 1);
    if (nrows > 0)
        hipLaunchKernelGGL(proj_rowsums_kernel<RULE>, dim3(grid_rows(nrows)), dim3(256), 0, s, (const float *)p, g, (const float *)m,
                           (const float *)v, segs, rowseg, nrows, P, rowsums);
    hipLaunchKernelGGL(proj_decide_kernel, dim3(nseg), dim3(256), 0, s, segs, (const double *)rowsums, delta, (double)P.eps, rowcoef, segdec);
    hipLaunchKernelGGL(proj_apply_kernel<RULE>, dim3(grid_chunks(nchunks)), dim3(256), 0, s, p, g, m, (const float *)v, chunks,
                       nchunks, segs, (const float *)rowcoef, (const float *)segdec, P, fault);
    return tnr_check_launch(RULE == RULE_ADAMP ? "adamp" : "sgdp");
}

}  // namespace

// ================================================================================== C ABI
extern "C" int64_t tnr_optim_workspace_bytes(int32_t nseg, int64_t nrows) {
    if (nrows < 1) nrows = 1;
    if (nseg < 1) nseg = 1;
    return nrows * 4 * (int64_t)sizeof(double) + nrows * 2 * (int64_t)sizeof(float) + (int64_t)nseg * 4 * (int64_t)sizeof(float);
}

extern "C" int tnr_sgd_step_guarded(float *p, const float *g, float *buf, const int64_t *chunks, int32_t nchunks, float lr, float momentum,
                                    float weight_decay, const uint32_t *fault, void *stream) {
    TNR_REQUIRE(p && g && chunks && nchunks > 0, "sgd: bad arguments");
    TNR_REQUIRE((buf != nullptr) == (momentum != 0.f), "sgd: a momentum buffer goes with momentum != 0 and only with it");
    hipLaunchKernelGGL(sgd_kernel, dim3(grid_chunks(nchunks)), dim3(256), 0, (hipStream_t)stream, p, g, buf, (const Chunk *)chunks, nchunks,
                       -lr, momentum, weight_decay, (const unsigned *)fault);
    return tnr_check_launch("sgd");
}

extern "C" int tnr_rmsprop_step_guarded(float *p, const float *g, float *square_avg, const int64_t *chunks, int32_t nchunks, float lr,
                                        double alpha, float eps, float weight_decay, const uint32_t *fault, void *stream) {
    TNR_REQUIRE(p && g && square_avg && chunks && nchunks > 0, "rmsprop: bad arguments");
    hipLaunchKernelGGL(rmsprop_kernel, dim3(grid_chunks(nchunks)), dim3(256), 0, (hipStream_t)stream, p, g, square_avg, (const Chunk *)chunks,
                       nchunks, -lr, (float)alpha, (float)(1.0 - alpha), eps, weight_decay, (const unsigned *)fault);
    return tnr_check_launch("rmsprop");
}

extern "C" int tnr_madgrad_step_guarded(float *p, const float *g, float *grad_sum_sq, float *s, const float *x0, const int64_t *chunks,
                                        int32_t nchunks, float lamb, float eps, float decay, float decay_mul, int32_t adamw, double momentum,
                                        const uint32_t *fault, void *stream) {
    TNR_REQUIRE(p && g && grad_sum_sq && s && chunks && nchunks > 0, "madgrad: bad arguments");
    TNR_REQUIRE((x0 != nullptr) == (momentum != 0.0), "madgrad: x0 goes with momentum != 0 and only with it");
    const double ck = 1.0 - momentum;
    hipLaunchKernelGGL(madgrad_kernel, dim3(grid_chunks(nchunks)), dim3(256), 0, (hipStream_t)stream, p, g, grad_sum_sq, s, x0,
                       (const Chunk *)chunks, nchunks, lamb, eps, decay, decay_mul, adamw, (float)ck, (float)(1.0 - ck), (const unsigned *)fault);
    return tnr_check_launch("madgrad");
}

extern "C" int tnr_adamp_step_guarded(float *p, const float *g, float *m, float *v, const int64_t *chunks, int32_t nchunks, const int64_t *segs,
                                      int32_t nseg, const int32_t *rowseg, int64_t nrows, void *ws, int64_t ws_bytes, float step_size, double b1,
                                      double b2, float bc2_sqrt, float eps, int32_t nesterov, double delta, float weight_decay, float decay_1,
                                      float decay_r, const uint32_t *fault, void *stream) {
    TNR_REQUIRE(p && g && m && v && chunks && segs && ws && nchunks > 0 && nseg > 0 && nrows >= 0, "adamp: bad arguments");
    TNR_REQUIRE(nrows == 0 || rowseg, "adamp: no row table");
    TNR_REQUIRE(ws_bytes >= tnr_optim_workspace_bytes(nseg, nrows), "adamp: workspace too small");
    ProjP P{(float)b1, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), bc2_sqrt, eps, step_size, weight_decay, decay_1, decay_r, nesterov};
    return proj_step<RULE_ADAMP>(p, g, m, v, (const Chunk *)chunks, nchunks, (const Seg *)segs, nseg, rowseg, nrows, ws, P, delta,
                                 (const unsigned *)fault, (hipStream_t)stream);
}

extern "C" int tnr_sgdp_step_guarded(float *p, const float *g, float *buf, const int64_t *chunks, int32_t nchunks, const int64_t *segs,
                                     int32_t nseg, const int32_t *rowseg, int64_t nrows, void *ws, int64_t ws_bytes, float lr, float momentum,
                                     double dampening, float eps, int32_t nesterov, double delta, float weight_decay, float decay_1,
                                     float decay_r, const uint32_t *fault, void *stream) {
    TNR_REQUIRE(p && g && buf && chunks && segs && ws && nchunks > 0 && nseg > 0 && nrows >= 0, "sgdp: bad arguments");
    TNR_REQUIRE(nrows == 0 || rowseg, "sgdp: no row table");
    TNR_REQUIRE(ws_bytes >= tnr_optim_workspace_bytes(nseg, nrows), "sgdp: workspace too small");
    ProjP P{momentum, (float)(1.0 - dampening), 0.f, 0.f, 1.f, eps, lr, weight_decay, decay_1, decay_r, nesterov};
    return proj_step<RULE_SGDP>(p, g, buf, nullptr, (const Chunk *)chunks, nchunks, (const Seg *)segs, nseg, rowseg, nrows, ws, P, delta,
                                (const unsigned *)fault, (hipStream_t)stream);
}

extern "C" int tnr_ranger_step_guarded(float *p, const float *g, float *m, float *v, float *slow, const int64_t *chunks, int32_t nchunks,
                                       const int64_t *segs, int32_t nseg, const int32_t *rowseg, int64_t nrows, void *ws, int64_t ws_bytes,
                                       int32_t gc_min_dim, double b1, double b2, float eps, float weight_decay, float step, int32_t rectified,
                                       int32_t lookahead, float alpha, const uint32_t *fault, void *stream) {
    TNR_REQUIRE(p && g && m && v && slow && chunks && segs && ws && nchunks > 0 && nseg > 0 && nrows >= 0, "ranger: bad arguments");
    TNR_REQUIRE(nrows == 0 || rowseg, "ranger: no row table");
    TNR_REQUIRE(ws_bytes >= tnr_optim_workspace_bytes(nseg, nrows), "ranger: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float *rowmean = (float *)ws;
    if (nrows > 0)          // a launch that writes only the workspace: always made, so the step is 2 launches whatever gc_min_dim is
        hipLaunchKernelGGL(row_mean_kernel, dim3(grid_rows(nrows)), dim3(256), 0, s, g, (const Seg *)segs, rowseg, nrows, rowmean);
    hipLaunchKernelGGL(ranger_kernel, dim3(grid_chunks(nchunks)), dim3(256), 0, s, p, g, m, v, slow, (const Chunk *)chunks, nchunks,
                       (const Seg *)segs, (const float *)rowmean, gc_min_dim, (float)b1, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), eps,
                       weight_decay, step, rectified, lookahead, alpha, (const unsigned *)fault);
    return tnr_check_launch("ranger");
}

extern "C" int tnr_swa_update_guarded(float *avg, const float *p, int64_t n, float weight, const uint32_t *fault, void *stream) {
    TNR_REQUIRE(avg && p && n > 0, "swa_update: bad arguments");
    TNR_REQUIRE(weight > 0.f && weight <= 1.f, "swa_update: weight %g is not 1 / (n_averaged + 1)", (double)weight);
    const unsigned grid = grid_chunks(tnr_cdiv64(n, 1024));
    if ((((uintptr_t)avg | (uintptr_t)p) & 15) == 0)
        hipLaunchKernelGGL(swa_update_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, avg, p, n, weight, (const unsigned *)fault);
    else
        hipLaunchKernelGGL(swa_update_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, avg, p, n, weight, (const unsigned *)fault);
    return tnr_check_launch("swa_update");
}
