// Frequency separation (codes/dataops/filters.py FilterLow :643-671, FilterHigh :674-717): the zero-padded
// 9 x 9 low-pass L of a fp32 image batch (AvgPool2d(9, 1, 4, count_include_pad=True), or the depthwise Gaussian, sigma 1.5) and the
// "separator" high-pass  clamp((x - L x + 1) / 2, 0, 1),  value and adjoint, one launch per filter application.
//
//   freqsep_kernel<LOW>     out (+)= mul * (L s)                      forward (mul = 1) and backward of FilterLow: L is its own adjoint
//                                                                      (symmetric taps, zero padding)
//   freqsep_kernel<HIGH>    out = clamp((s - L s + 1) / 2, 0, 1)      FilterHigh forward, fused in the same pass
//   freqsep_kernel<HIGH_B>  out (+)= mul * (g' - L g')                FilterHigh backward; g' = 0.5 g where the SAVED OUTPUT o of the
//                                                                      forward lies strictly inside (0, 1) and 0 elsewhere, formed
//                                                                      while the tile is staged
//
// One workgroup = one 64 x 16 tile of one (n, c) plane.  The tile with a 4-pixel zero halo (72 x 24) is staged in LDS once; L is
// evaluated separably from the 9-tap vector of the kernel arguments (the 2-D taps are its outer product): a horizontal pass over the
// 24 staged rows into a second LDS tile, then a vertical pass in which every thread forms four neighbouring outputs of one row.  Every
// pass reads the tensor once and writes it once; fp32 throughout, explicit fmaf in a fixed order: two runs are bit-identical.
//
// The clamp mask comes from the saved output, not from the input: the backward then reads g and o (no second stencil).  torch's clamp
// passes the gradient on the closed interval; an output of exactly 0 or 1 cannot tell "on the edge" from "beyond it", so it passes
// nothing here.  The two differ only where x - L x is exactly -1 or +1.
#include "image_tile.h"

namespace {

constexpr int K = 9, R = K / 2;                          // taps per side, halo
constexpr int TW = 64, TH = 16;                          // tile; thread = 4 neighbouring columns of one row
constexpr int IW = TW + 2 * R, IH = TH + 2 * R;          // 72 x 24 staged pixels
// LDS row strides.  Both tiles are read 16 bytes per lane (ds_read_b128: banks (a / 4) mod 64, served in 16-lane groups that take
// lanes 0-3 and 12-15 of one row of the thread grid together with lanes 4-11 of the NEXT row).  With a row stride that is a multiple
// of 64 dwords the two rows of a group fall on the same bank row and its 16 lanes read the 16 different 16-byte slots 0-3, 12-15
// (first row) and 4-11 (second row): conflict-free.  Any other multiple of 4 shifts the second row's slots onto the first row's.
constexpr int SST = 128;                                 // staged tile: 72 columns used
constexpr int TST = 64;                                  // horizontally filtered tile: 64 columns

enum { LOW = 0, HIGH = 1, HIGH_B = 2 };

struct Taps {
    float w[K];
};

// torch.clamp(v, 0, 1): a NaN stays a NaN (fminf / fmaxf would turn it into a bound)
__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

__device__ __forceinline__ float masked_half(float g, float o) { return (o > 0.f && o < 1.f) ? 0.5f * g : 0.f; }
__device__ __forceinline__ f32x4 masked_half(f32x4 g, f32x4 o) {
    return f32x4{masked_half(g.x, o.x), masked_half(g.y, o.y), masked_half(g.z, o.z), masked_half(g.w, o.w)};
}

// what stage_tile stores: the source, or (HIGH_B) the gradient g' formed from it and the saved output
template <int MODE>
struct StagedPixel {
    const float *src, *saved;
    template <class V>
    __device__ __forceinline__ void operator()(int64_t a, V (&v)[1]) const {
        v[0] = *(const V *)(src + a);
        if (MODE == HIGH_B) v[0] = masked_half(v[0], *(const V *)(saved + a));
    }
};

// src: x (LOW, HIGH) or the incoming gradient g (LOW as a backward, HIGH_B); saved: the forward's output o (HIGH_B only)
template <int MODE>
__global__ __launch_bounds__(256) void freqsep_kernel(const float *__restrict__ src, const float *__restrict__ saved, ImView g, Taps taps,
                                                      int tilesX, int tilesY, float *__restrict__ out, const float *__restrict__ gscale,
                                                      int accumulate, int vec) {
    __shared__ __attribute__((aligned(16))) float sS[IH * SST];
    __shared__ __attribute__((aligned(16))) float sT[IH * TST];
    const int tid = threadIdx.x;
    int n, c, y0, x0;
    tile_of_block<TW, TH>(g, tilesX, tilesY, &n, &c, &y0, &x0);
    const int64_t base = (int64_t)n * g.sN + (int64_t)c * g.sC;
    // with 16-byte loads: the 18 aligned groups of four columns x0 - 4 .. x0 + 67 of every staged row; group gq is LDS columns
    // 4 gq .. 4 gq + 3, one aligned 16-byte store
    float *const tile[1] = {sS};
    stage_tile<IH, IW, R, SST, R, IW>(g, base, y0, x0, vec, tile, StagedPixel<MODE>{src, saved});
    __syncthreads();
    // horizontal pass: 24 rows x 16 groups of four columns; output column j of the tile is centred on staged column j + 4
    for (int i = tid; i < IH * (TW / 4); i += 256) {
        const int r = i >> 4, q = (i & 15) * 4;
        const f32x4 a0 = *(const f32x4 *)(sS + r * SST + q), a1 = *(const f32x4 *)(sS + r * SST + q + 4),
                    a2 = *(const f32x4 *)(sS + r * SST + q + 8);
        const float v[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
        float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float w = taps.w[k];
            t0 = fmaf(w, v[k], t0);
            t1 = fmaf(w, v[k + 1], t1);
            t2 = fmaf(w, v[k + 2], t2);
            t3 = fmaf(w, v[k + 3], t3);
        }
        f32x4 t = {t0, t1, t2, t3};
        *(f32x4 *)(sT + r * TST + q) = t;
    }
    __syncthreads();
    // vertical pass: output row `row` of the tile is centred on filtered row row + 4
    const int row = tid >> 4, col = (tid & 15) * 4;
    float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const f32x4 t = *(const f32x4 *)(sT + (row + k) * TST + col);
        const float w = taps.w[k];
        e0 = fmaf(w, t.x, e0);
        e1 = fmaf(w, t.y, e1);
        e2 = fmaf(w, t.z, e2);
        e3 = fmaf(w, t.w, e3);
    }
    float e[4] = {e0, e1, e2, e3};
    if (MODE != LOW) {
        const f32x4 ctr = *(const f32x4 *)(sS + (row + R) * SST + col + R);
        const float s[4] = {ctr.x, ctr.y, ctr.z, ctr.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = s[j] - e[j];
            e[j] = MODE == HIGH ? clamp01((d + 1.f) * 0.5f) : d;
        }
    }
    if (MODE != HIGH) {
        const float mul = gscale ? *gscale : 1.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = mul * e[j];
    }
    const int yy = y0 + row;
    if (yy >= g.h) return;
    if (vec) {
        if (x0 + col >= g.w) return;                     // the thread's four columns are one aligned group inside the image
        f32x4 *o = (f32x4 *)(out + base + (int64_t)yy * g.sH + x0 + col);
        f32x4 r = {e[0], e[1], e[2], e[3]};
        if (MODE != HIGH && accumulate) r = *o + r;
        *o = r;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = x0 + col + j;
            if (xx >= g.w) continue;
            const int64_t a = base + (int64_t)yy * g.sH + (int64_t)xx * g.sW;
            out[a] = (MODE != HIGH && accumulate) ? out[a] + e[j] : e[j];
        }
    }
}

template <int MODE>
int launch(const char *what, const float *src, const float *saved, int N, int C, int H, int W, int layout, const float *taps9, float *out,
           const float *gscale, int accumulate, void *stream) {
    int64_t blocks;
    int tilesX, tilesY;
    if (int rc = check_batch(what, N, C, H, W, layout, TW, TH, &blocks, &tilesX, &tilesY)) return rc;
    TNR_REQUIRE(src && out && taps9 && src != out, "%s: null or aliased pointer", what);
    TNR_REQUIRE(MODE != HIGH_B || (saved && saved != out), "%s: the saved forward output is missing or aliases the result", what);
    Taps t;
    for (int k = 0; k < K; ++k) t.w[k] = taps9[k];
    hipLaunchKernelGGL(freqsep_kernel<MODE>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, saved,
                       make_view(N, C, H, W, layout), t, tilesX, tilesY, out, gscale, accumulate, vec_rows(layout, W, src, out, saved));
    return tnr_check_launch(what);
}

}  // namespace

extern "C" int tnr_freqsep_low(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const float *taps9,
                               const float *gscale, float *out, int32_t accumulate, void *stream) {
    return launch<LOW>("freqsep_low", x, nullptr, N, C, H, W, layout, taps9, out, gscale, accumulate, stream);
}

extern "C" int tnr_freqsep_high_fwd(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout, const float *taps9,
                                    float *out, void *stream) {
    return launch<HIGH>("freqsep_high_fwd", x, nullptr, N, C, H, W, layout, taps9, out, nullptr, 0, stream);
}

extern "C" int tnr_freqsep_high_bwd(const float *g, const float *o, int32_t N, int32_t C, int32_t H, int32_t W, int32_t layout,
                                    const float *taps9, const float *gscale, float *gx, int32_t accumulate, void *stream) {
    return launch<HIGH_B>("freqsep_high_bwd", g, o, N, C, H, W, layout, taps9, gx, gscale, accumulate, stream);
}
