// Spectral normalisation of convolution weights (torch.nn.utils.spectral_norm, hook form, one power iteration, dim 0) for every
// wrapped layer of a network at once.  A weight W is the matrix [rows = Cout][K = Cin kh kw] in OIHW row order.
//
// One device table of jobs (one per wrapped layer) and four tile tables drive every launch; the number of launches does not depend on
// the number of layers.  Phase boundaries are launch boundaries:
//   forward, training (4 launches)                                        forward, eval (2 launches: the last two, iterate = 0)
//     1 wt_partial  tpart[rb][k] = sum over the 16 rows of block rb of W[r][k] u[r]
//     2 t_finish    t = sum over rb of tpart (256 columns per workgroup), and the workgroup's share of |t|^2
//     3 row_dot     v = t / max(|t|, eps) (in place, and into the record); s[r] = W[r] . v          (one wave per row)
//     4 scale       u = s / max(|s|, eps) (in place); sigma = u . s; Wn = W / sigma     (eval: sigma = u_stored . s, u and v untouched)
//   backward (2 launches)
//     1 gdot        gpart[c] = sum over chunk c of G Wn
//     2 apply       dW += (G - <G, Wn> u v^T) / sigma         with the u, v, sigma, Wn of the forward's record
// Sums run in fp64 in a fixed order (sequential per thread, then the shuffle / LDS tree), no atomics: the same inputs give the same
// bits on every run.  Values are fp32 and are rounded where torch rounds them (t, s, the norms, sigma).  Rows are read 16 bytes wide
// when K % 4 == 0 and the tensors are 16-byte aligned, else element by element; nothing is read or written past a row or a tensor.
#include "common.h"

namespace {

// One wrapped layer.  `ru`, `rv`, `sig` are the forward's record (copies of u and v as used by sigma, and sigma itself).
struct Job {
    const float *w;      // [rows][K] the parameter weight_orig
    float *wn;           // [rows][K] the derived weight W / sigma
    float *u, *v;        // [rows], [K] the buffers weight_u / weight_v
    float *ru, *rv, *sig;
    const float *g;      // [rows][K] dL/dWn (backward)
    float *dw;           // [rows][K] weight_orig.grad (backward, accumulated)
    int64_t rows, K;
    double *tpart;       // [ceil(rows / 16)][K]; after t_finish its first row holds t (rounded to fp32)
    float *s;            // [rows]
    double *gpart;       // [ngpart]
    int64_t ngpart;      // chunks of this job
    double *sspart;      // [ceil(K / 256)] shares of |t|^2
};
static_assert(sizeof(Job) == 16 * 8, "Job is 16 int64 words (trainner_amd/ops.py SpectralNormTable)");

struct Tile { int32_t job, a, b, c; };

constexpr int RB = 16;        // rows per wt_partial tile
constexpr int KB = 1024;      // columns per wt_partial tile (256 threads x 4)
constexpr int CHUNK = 4096;   // elements per elementwise block (256 threads x 4 x 4)
constexpr int MAX_GRID = 4096;

__device__ __forceinline__ bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ void ld4(const float *a, int64_t e, int nv, bool vec, float *o) {
    if (vec && nv == 4) {
        const f32x4 x = *reinterpret_cast<const f32x4 *>(a + e);
        o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; o[3] = x[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = k < nv ? a[e + k] : 0.f;
    }
}

__device__ __forceinline__ void st4(float *a, int64_t e, int nv, bool vec, const float *o) {
    if (vec && nv == 4) {
        f32x4 x = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4 *>(a + e) = x;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nv) a[e + k] = o[k];
    }
}

__device__ __forceinline__ int left4(int64_t left) { return left >= 4 ? 4 : (left > 0 ? (int)left : 0); }

// ---------------------------------------------------------------------------------- forward
__global__ void wt_partial_kernel(const Job *jobs, const Tile *tiles, int ntiles) {
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const Tile tl = tiles[t];
        const Job &jb = jobs[tl.job];
        const int64_t K = jb.K, k = (int64_t)tl.b + 4 * (int64_t)threadIdx.x;
        const int nv = left4(K - k);
        if (nv == 0) continue;
        const bool vec = (K & 3) == 0 && al16(jb.w);
        const int64_t r1 = min((int64_t)tl.a + RB, jb.rows);
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int64_t r = tl.a; r < r1; ++r) {
            float wv[4];
            ld4(jb.w, r * K + k, nv, vec, wv);
            const double ur = (double)jb.u[r];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += (double)wv[j] * ur;
        }
        double *out = jb.tpart + (int64_t)tl.c * K + k;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) out[j] = acc[j];
    }
}

// t[k] = the sum of the row blocks' partials, one column per thread; rounded to fp32 where torch holds it in fp32.
__global__ void t_finish_kernel(const Job *jobs, const Tile *tiles, int ntiles) {
    __shared__ double sh[256];
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const Tile tl = tiles[t];
        const Job &jb = jobs[tl.job];
        const int64_t K = jb.K, nrb = (jb.rows + RB - 1) / RB, k = (int64_t)tl.a + threadIdx.x;
        double ss = 0.0;
        if (k < K) {
            double acc = 0.0;
#pragma unroll 4
            for (int64_t b = 0; b < nrb; ++b) acc += jb.tpart[b * K + k];
            const float tf = (float)acc;
            jb.tpart[k] = (double)tf;                          // (this thread alone reads and writes column k)
            ss = (double)tf * (double)tf;
        }
        const double tot = tnr_block_sum256(ss, sh);
        if (threadIdx.x == 0) jb.sspart[tl.c] = tot;
    }
}

// s[r] = W[r] . v: four rows per workgroup, one wave each.  Training: v = t / max(|t|, eps) is formed on the fly from t and the
// shares of |t|^2 (every workgroup adds them in the same order: the same norm everywhere), and the workgroup of a job's first rows
// writes v and its record.  Eval: the stored v.
__global__ void row_dot_kernel(const Job *jobs, const Tile *tiles, int ntiles, int iterate, float eps) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const Tile tl = tiles[t];
        const Job &jb = jobs[tl.job];
        const int64_t r = (int64_t)tl.a + wave, K = jb.K;
        float nrm = 1.f;
        if (iterate) {
            double ss = 0.0;
            for (int64_t i = 0; i < (K + 255) / 256; ++i) ss += jb.sspart[i];
            nrm = fmaxf((float)sqrt(ss), eps);
            if (tl.a == 0)
                for (int64_t k = threadIdx.x; k < K; k += 256) {
                    const float vk = (float)jb.tpart[k] / nrm;
                    jb.v[k] = vk;
                    jb.rv[k] = vk;
                }
        }
        if (r >= jb.rows) continue;                            // (wave-uniform)
        const bool vec = (K & 3) == 0 && al16(jb.w) && al16(jb.v);
        double acc = 0.0;
        for (int64_t k = 4 * (int64_t)lane; k < K; k += 256) {
            const int nv = left4(K - k);
            float wv[4], vv[4];
            ld4(jb.w, r * K + k, nv, vec, wv);
            if (iterate) {
#pragma unroll
                for (int j = 0; j < 4; ++j) vv[j] = j < nv ? (float)jb.tpart[k + j] / nrm : 0.f;
            } else {
                ld4(jb.v, k, nv, vec, vv);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += (double)wv[j] * (double)vv[j];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if (lane == 0) jb.s[r] = (float)acc;
    }
}

// Every workgroup derives sigma of its job from s (the same fixed-order sums everywhere: the same bits), then scales its chunk.
// The workgroup of a job's first chunk also writes u (training) and the record.
__global__ void scale_kernel(const Job *jobs, const Tile *chunks, int nchunks, int iterate, float eps) {
    __shared__ double sh[256];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Tile ck = chunks[c];
        const Job &jb = jobs[ck.job];
        const int64_t rows = jb.rows, n = rows * jb.K;
        float nrm = 1.f;
        if (iterate) {
            double ss = 0.0;
            for (int64_t r = threadIdx.x; r < rows; r += 256) ss += (double)jb.s[r] * (double)jb.s[r];
            nrm = fmaxf((float)sqrt(tnr_block_sum256(ss, sh)), eps);
        }
        double us = 0.0;
        for (int64_t r = threadIdx.x; r < rows; r += 256) {
            const float ur = iterate ? jb.s[r] / nrm : jb.u[r];
            us += (double)ur * (double)jb.s[r];
        }
        const float sigma = (float)tnr_block_sum256(us, sh);
        if (ck.c == 0) {
            for (int64_t r = threadIdx.x; r < rows; r += 256) {
                const float ur = iterate ? jb.s[r] / nrm : jb.u[r];
                if (iterate) jb.u[r] = ur;
                jb.ru[r] = ur;
            }
            if (!iterate)
                for (int64_t k = threadIdx.x; k < jb.K; k += 256) jb.rv[k] = jb.v[k];
            if (threadIdx.x == 0) jb.sig[0] = sigma;
        }
        const bool vec = al16(jb.w) && al16(jb.wn);
#pragma unroll
        for (int i = 0; i < CHUNK / 1024; ++i) {
            const int64_t e = (int64_t)ck.a + i * 1024 + 4 * (int64_t)threadIdx.x;
            const int nv = left4(n - e);
            if (nv == 0) continue;
            float wv[4];
            ld4(jb.w, e, nv, vec, wv);
#pragma unroll
            for (int j = 0; j < 4; ++j) wv[j] = wv[j] / sigma;
            st4(jb.wn, e, nv, vec, wv);
        }
    }
}

// ---------------------------------------------------------------------------------- backward
__global__ void gdot_kernel(const Job *jobs, const Tile *chunks, int nchunks) {
    __shared__ double sh[256];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Tile ck = chunks[c];
        const Job &jb = jobs[ck.job];
        const int64_t n = jb.rows * jb.K;
        const bool vec = al16(jb.g) && al16(jb.wn);
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < CHUNK / 1024; ++i) {
            const int64_t e = (int64_t)ck.a + i * 1024 + 4 * (int64_t)threadIdx.x;
            const int nv = left4(n - e);
            if (nv == 0) continue;
            float gv[4], wv[4];
            ld4(jb.g, e, nv, vec, gv);
            ld4(jb.wn, e, nv, vec, wv);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += (double)gv[j] * (double)wv[j];
        }
        const double tot = tnr_block_sum256(acc, sh);
        if (threadIdx.x == 0) jb.gpart[ck.c] = tot;
    }
}

__global__ void apply_kernel(const Job *jobs, const Tile *chunks, int nchunks) {
    __shared__ double sh[256];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Tile ck = chunks[c];
        const Job &jb = jobs[ck.job];
        const int64_t K = jb.K, n = jb.rows * K;
        double part = 0.0;
        for (int64_t i = threadIdx.x; i < jb.ngpart; i += 256) part += jb.gpart[i];
        const float dot = (float)tnr_block_sum256(part, sh);
        const float sigma = jb.sig[0];
        const bool vec = al16(jb.g) && al16(jb.dw);
#pragma unroll
        for (int i = 0; i < CHUNK / 1024; ++i) {
            const int64_t e = (int64_t)ck.a + i * 1024 + 4 * (int64_t)threadIdx.x;
            const int nv = left4(n - e);
            if (nv == 0) continue;
            float gv[4], dv[4];
            ld4(jb.g, e, nv, vec, gv);
            ld4(jb.dw, e, nv, vec, dv);
            int64_t r = e / K, k = e - r * K;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < nv) {
                    const float uv = jb.ru[r] * jb.rv[k];
                    dv[j] = dv[j] + (gv[j] - dot * uv) / sigma;
                    if (++k == K) {
                        k = 0;
                        ++r;
                    }
                }
            }
            st4(jb.dw, e, nv, vec, dv);
        }
    }
}

inline unsigned grid_of(int n) { return (unsigned)(n > MAX_GRID ? MAX_GRID : (n < 1 ? 1 : n)); }

}  // namespace

// ================================================================================== C ABI
extern "C" int32_t tnr_sn_job_words(void) { return (int32_t)(sizeof(Job) / 8); }

extern "C" int tnr_sn_forward(const int64_t *jobs, int32_t njobs, const int32_t *wt_tiles, int32_t n_wt, const int32_t *col_tiles, int32_t n_col,
                              const int32_t *row_tiles, int32_t n_row, const int32_t *chunks, int32_t nchunks, int32_t iterate, float eps,
                              void *stream) {
    TNR_REQUIRE(jobs && wt_tiles && col_tiles && row_tiles && chunks && njobs > 0 && n_wt > 0 && n_col > 0 && n_row > 0 && nchunks > 0,
                "sn_forward: bad arguments");
    TNR_REQUIRE(eps > 0.f, "sn_forward: eps must be positive");
    hipStream_t s = (hipStream_t)stream;
    const Job *jb = (const Job *)jobs;
    if (iterate) {
        hipLaunchKernelGGL(wt_partial_kernel, dim3(grid_of(n_wt)), dim3(256), 0, s, jb, (const Tile *)wt_tiles, n_wt);
        hipLaunchKernelGGL(t_finish_kernel, dim3(grid_of(n_col)), dim3(256), 0, s, jb, (const Tile *)col_tiles, n_col);
    }
    hipLaunchKernelGGL(row_dot_kernel, dim3(grid_of(n_row)), dim3(256), 0, s, jb, (const Tile *)row_tiles, n_row, iterate ? 1 : 0, eps);
    hipLaunchKernelGGL(scale_kernel, dim3(grid_of(nchunks)), dim3(256), 0, s, jb, (const Tile *)chunks, nchunks, iterate ? 1 : 0, eps);
    return tnr_check_launch("sn_forward");
}

extern "C" int tnr_sn_backward(const int64_t *jobs, int32_t njobs, const int32_t *chunks, int32_t nchunks, void *stream) {
    TNR_REQUIRE(jobs && chunks && njobs > 0 && nchunks > 0, "sn_backward: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const Job *jb = (const Job *)jobs;
    hipLaunchKernelGGL(gdot_kernel, dim3(grid_of(nchunks)), dim3(256), 0, s, jb, (const Tile *)chunks, nchunks);
    hipLaunchKernelGGL(apply_kernel, dim3(grid_of(nchunks)), dim3(256), 0, s, jb, (const Tile *)chunks, nchunks);
    return tnr_check_launch("sn_backward");
}
