// LPIPS validation metric (reference: codes/utils/metrics.py:37,232-280 -> models/modules/LPIPS/networks_basic.py:32-120 with
// net = 'squeeze', model = 'net-lin', version = '0.1', spatial = False).  The SqueezeNet 1.1 backbone's Fire convolutions run
// through tnr_conv_forward; this file holds what is specific to the metric:
//   tnr_lpips_stem          : image -> ScalingLayer -> features[0] (conv 3x3 s2 p0, 3 -> 64) + bias + ReLU = relu1, NHWC[64] fp32.
//                             Vector ALU, lanes = output channels (27 MAC per output: store-bound).
//   tnr_maxpool3s2_ceil_fwd : nn.MaxPool2d(3, 2, ceil_mode=True) on NHWC views (exact: bit-identical to torch).
//   tnr_lpips_head          : one layer's normalise -> squared difference -> lin_l (1x1, no bias) -> spatial mean, as fixed-order
//                             fp64 partial sums per image; tnr_lpips_finalize divides by the layer's pixel count and sums the layers.
#include <algorithm>

#include "common.h"

namespace {

constexpr int HEAD_BLOCK = 256;
constexpr int HEAD_LANES = 16;                         // lanes per pixel (channel quads strided by 16)
constexpr int HEAD_PIX = HEAD_BLOCK / HEAD_LANES;      // pixels per block iteration
constexpr int HEAD_MAX_BLOCKS = 256;                   // partial sums per (layer, image)
constexpr int STEM_PIX = 4;                            // pixels per 256-thread block iteration (one wave64 per pixel)

inline bool view_ok(const tnr_view &v) { return v.ptr != nullptr && (v.ctot % 4) == 0 && (v.coff % 4) == 0; }

// src_kind 0: uint8 NHWC [N, H, W, 3] (tensor2np images), x = float32(u8 / 127.5 - 1) with the division in fp64 (im2tensor,
// perceptual_loss.py:148-151); src_kind 1: fp32 NCHW [N, 3, H, W] in [-1, 1] (PerceptualLoss.forward; normalize: 2 x - 1 first).
// Images 0..N-1 come from a, N..2N-1 from b.  Output (n, oy, ox) reads the cropped image at rows / cols 2 oy + crop .. + 2.
template <int KIND>
__global__ void __launch_bounds__(256) lpips_stem_kernel(const void *a, const void *b, int N, int H, int W, int crop, int normalize,
                                                          const float *shift, const float *scale, const float *w, const float *bias,
                                                          float *y, int y_ct, int y_co, int Ho, int Wo) {
    const int c = threadIdx.x & 63;
    float wr[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) wr[k] = w[c * 27 + k];          // OIHW: [c][ci][ky][kx]
    const float bc = bias[c];
    float sh[3], sc[3];
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
        sh[ci] = shift[ci];
        sc[ci] = scale[ci];
    }
    const int64_t hw = (int64_t)Ho * Wo, total = 2 * (int64_t)N * hw;
    for (int64_t p = (int64_t)blockIdx.x * STEM_PIX + (threadIdx.x >> 6); p < total; p += (int64_t)gridDim.x * STEM_PIX) {
        const int64_t n2 = p / hw, r = p - n2 * hw;
        const int oy = (int)(r / Wo), ox = (int)(r - (int64_t)oy * Wo);
        const int64_t n = n2 < N ? n2 : n2 - N;
        const int iy0 = 2 * oy + crop, ix0 = 2 * ox + crop;
        float acc = 0.f;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    float x;
                    if (KIND == 0) {
                        const uint8_t *src = (const uint8_t *)(n2 < N ? a : b);
                        const uint8_t v = src[((n * H + iy0 + ky) * W + ix0 + kx) * 3 + ci];
                        x = (float)((double)v / 127.5 - 1.0);
                    } else {
                        const float *src = (const float *)(n2 < N ? a : b);
                        x = src[((n * 3 + ci) * H + iy0 + ky) * W + ix0 + kx];
                        if (normalize) x = 2.0f * x - 1.0f;
                    }
                    const float s = (x - sh[ci]) / sc[ci];             // ScalingLayer (networks_basic.py:103-110), fp32
                    acc = fmaf(wr[(ci * 3 + ky) * 3 + kx], s, acc);
                }
        acc += bc;
        y[p * y_ct + y_co + c] = acc > 0.f ? acc : 0.f;              // features[1]: ReLU
    }
}

// PyTorch's pooling_output_shape for k 3, s 2, p 0, dilation 1, ceil_mode: the last window may hang over the border (clipped here)
// but must start inside the input.
__host__ __device__ inline int pool_out(int H) {
    int o = (H - 3 + 1) / 2 + 1;           // ceil((H - 3) / 2) + 1
    if ((o - 1) * 2 >= H) --o;
    return o;
}

__global__ void maxpool3s2_ceil_kernel(const float *x, int x_ct, int x_co, float *y, int y_ct, int y_co, int N, int H, int W, int C,
                                       int Ho, int Wo) {
    const int c4n = C / 4;
    const int64_t total = (int64_t)N * Ho * Wo * c4n;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(e % c4n);
        const int64_t pix = e / c4n;
        const int ox = (int)(pix % Wo);
        const int64_t q = pix / Wo;
        const int oy = (int)(q % Ho);
        const int64_t n = q / Ho;
        const int y0 = 2 * oy, x0 = 2 * ox;
        const int y1 = min(y0 + 3, H), x1 = min(x0 + 3, W);
        f32x4 best = *reinterpret_cast<const f32x4 *>(x + ((n * H + y0) * W + x0) * x_ct + x_co + c4 * 4);
        for (int iy = y0; iy < y1; ++iy)
            for (int ix = x0; ix < x1; ++ix) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(x + ((n * H + iy) * W + ix) * x_ct + x_co + c4 * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) best[j] = (v[j] > best[j] || isnan(v[j])) ? v[j] : best[j];     // NaN propagates (aten)
            }
        *reinterpret_cast<f32x4 *>(y + pix * y_ct + y_co + c4 * 4) = best;
    }
}

__device__ __forceinline__ double group_sum(double v) {           // over the 16 lanes of a pixel group, fixed butterfly order
#pragma unroll
    for (int m = HEAD_LANES / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, HEAD_LANES);
    return v;
}

inline int head_blocks(int64_t hw) { return (int)std::min<int64_t>(HEAD_MAX_BLOCKS, tnr_cdiv64(hw, HEAD_PIX)); }

// ws layout: partial[(layer * N + n) * HEAD_MAX_BLOCKS + block] for L layers, then meta[2 * layer] = H * W and
// meta[2 * layer + 1] = blocks used (written by block (0, 0) of the layer's launch).
// Per pixel, in fp64: a = ||f0|| + 1e-10, b = ||f1|| + 1e-10 (normalize_tensor, perceptual_loss.py:36-38), then
// sum_c w[c] (f0[c] / a - f1[c] / b)^2 -- the direct form, which is exactly 0 where f0 == f1.
__global__ void __launch_bounds__(HEAD_BLOCK) lpips_head_kernel(const float *f0, int f0_ct, int f0_co, const float *f1, int f1_ct,
                                                                int f1_co, int N, int HW, int C, const float *w, int layer, int L, double *ws) {
    __shared__ double red[HEAD_BLOCK];
    const int lane = threadIdx.x % HEAD_LANES, g = threadIdx.x / HEAD_LANES;
    const int n = blockIdx.y, c4n = C / 4;
    double acc = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * HEAD_PIX + g; p < HW; p += (int64_t)gridDim.x * HEAD_PIX) {
        const float *p0 = f0 + ((int64_t)n * HW + p) * f0_ct + f0_co;
        const float *p1 = f1 + ((int64_t)n * HW + p) * f1_ct + f1_co;
        double s0 = 0.0, s1 = 0.0;
        for (int c4 = lane; c4 < c4n; c4 += HEAD_LANES) {
            const f32x4 u = *reinterpret_cast<const f32x4 *>(p0 + 4 * c4), v = *reinterpret_cast<const f32x4 *>(p1 + 4 * c4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s0 += (double)u[j] * (double)u[j];
                s1 += (double)v[j] * (double)v[j];
            }
        }
        const double ia = 1.0 / (sqrt(group_sum(s0)) + 1e-10), ib = 1.0 / (sqrt(group_sum(s1)) + 1e-10);
        double d = 0.0;
        for (int c4 = lane; c4 < c4n; c4 += HEAD_LANES) {       // second pass: the pixel's channels are still in L1 / L2
            const f32x4 u = *reinterpret_cast<const f32x4 *>(p0 + 4 * c4), v = *reinterpret_cast<const f32x4 *>(p1 + 4 * c4);
            const f32x4 wv = *reinterpret_cast<const f32x4 *>(w + 4 * c4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double t = (double)u[j] * ia - (double)v[j] * ib;
                d += (double)wv[j] * (t * t);
            }
        }
        acc += group_sum(d);                                   // every lane of the group holds the pixel's value
    }
    static_assert(HEAD_BLOCK == 256, "tnr_block_sum256 adds 256 slots");
    acc = tnr_block_sum256(lane == 0 ? acc : 0.0, red);
    if (threadIdx.x == 0) {
        ws[((int64_t)layer * N + n) * HEAD_MAX_BLOCKS + blockIdx.x] = acc;
        if (blockIdx.x == 0 && n == 0) {
            double *meta = ws + (int64_t)L * N * HEAD_MAX_BLOCKS;
            meta[2 * layer] = (double)HW;
            meta[2 * layer + 1] = (double)gridDim.x;
        }
    }
}

// out[n] = sum_l (sum_b partial[l][n][b]) / HW_l;  per_layer[n * L + l] (optional) = the layer's term.  Fixed order throughout.
__global__ void lpips_finalize_kernel(int N, int L, const double *ws, const double *meta, double *out, double *per_layer) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double total = 0.0;
    for (int l = 0; l < L; ++l) {
        const int nb = (int)meta[2 * l + 1];
        const double *part = ws + ((int64_t)l * N + n) * HEAD_MAX_BLOCKS;
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += part[b];
        const double v = s / meta[2 * l];
        if (per_layer) per_layer[(int64_t)n * L + l] = v;
        total += v;
    }
    out[n] = total;
}

}  // namespace

extern "C" int64_t tnr_lpips_workspace_bytes(int32_t N, int32_t L) {
    if (N < 1 || L < 1) return 0;
    return ((int64_t)L * N * HEAD_MAX_BLOCKS + 2 * (int64_t)L) * (int64_t)sizeof(double);
}

extern "C" int tnr_lpips_stem_dims(int32_t H, int32_t W, int32_t crop, int32_t *Ho, int32_t *Wo) {
    TNR_REQUIRE(Ho && Wo && crop >= 0 && H - 2 * crop >= 3 && W - 2 * crop >= 3, "lpips_stem_dims: image smaller than the 3x3 stem");
    *Ho = (H - 2 * crop - 3) / 2 + 1;
    *Wo = (W - 2 * crop - 3) / 2 + 1;
    return TNR_OK;
}

extern "C" int tnr_lpips_stem(const void *a, const void *b, int32_t src_kind, int32_t N, int32_t H, int32_t W, int32_t C, int32_t crop,
                              int32_t normalize, const float *shift, const float *scale, const float *w, const float *bias, tnr_view y,
                              void *stream) {
    TNR_REQUIRE(a && b && shift && scale && w && bias && view_ok(y) && N >= 1 && C == 3 && (src_kind == 0 || src_kind == 1),
                "lpips_stem: bad arguments");
    TNR_REQUIRE(src_kind == 1 || normalize == 0, "lpips_stem: normalize applies to fp32 inputs only");
    int Ho = 0, Wo = 0;
    const int rc = tnr_lpips_stem_dims(H, W, crop, &Ho, &Wo);
    if (rc != TNR_OK) return rc;
    TNR_REQUIRE(y.coff + 64 <= y.ctot, "lpips_stem: the output view needs 64 channels");
    const int64_t total = 2 * (int64_t)N * Ho * Wo;
    const int64_t blocks = std::min<int64_t>(tnr_cdiv64(total, STEM_PIX), 1 << 16);
    hipStream_t s = (hipStream_t)stream;
    if (src_kind == 0)
        hipLaunchKernelGGL(lpips_stem_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, s, a, b, N, H, W, crop, 0, shift, scale, w, bias,
                           y.ptr, y.ctot, y.coff, Ho, Wo);
    else
        hipLaunchKernelGGL(lpips_stem_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, a, b, N, H, W, crop, normalize, shift, scale, w,
                           bias, y.ptr, y.ctot, y.coff, Ho, Wo);
    return tnr_check_launch("lpips_stem");
}

extern "C" int tnr_maxpool3s2_ceil_dims(int32_t H, int32_t W, int32_t *Ho, int32_t *Wo) {
    TNR_REQUIRE(Ho && Wo && H >= 3 && W >= 3, "maxpool3s2_ceil_dims: input smaller than the 3x3 window");
    *Ho = pool_out(H);
    *Wo = pool_out(W);
    return TNR_OK;
}

extern "C" int tnr_maxpool3s2_ceil_fwd(tnr_view x, tnr_view y, int32_t N, int32_t H, int32_t W, int32_t C, void *stream) {
    TNR_REQUIRE(view_ok(x) && view_ok(y) && N >= 1 && C >= 4 && (C % 4) == 0 && H >= 3 && W >= 3, "maxpool3s2_ceil_fwd: bad arguments");
    TNR_REQUIRE(x.coff + C <= x.ctot && y.coff + C <= y.ctot, "maxpool3s2_ceil_fwd: views narrower than C");
    const int Ho = pool_out(H), Wo = pool_out(W);
    const int64_t total = (int64_t)N * Ho * Wo * (C / 4);
    const int64_t blocks = std::min<int64_t>(tnr_cdiv64(total, 256), 1 << 16);
    hipLaunchKernelGGL(maxpool3s2_ceil_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x.ptr, x.ctot, x.coff, y.ptr,
                       y.ctot, y.coff, N, H, W, C, Ho, Wo);
    return tnr_check_launch("maxpool3s2_ceil_fwd");
}

extern "C" int tnr_lpips_head(tnr_view f0, tnr_view f1, int32_t N, int32_t H, int32_t W, int32_t C, const float *w, int32_t layer,
                              int32_t L, double *ws, int64_t ws_bytes, void *stream) {
    TNR_REQUIRE(view_ok(f0) && view_ok(f1) && w && ws && N >= 1 && H >= 1 && W >= 1 && C >= 4 && (C % 4) == 0 && layer >= 0 && layer < L,
                "lpips_head: bad arguments");
    TNR_REQUIRE(f0.coff + C <= f0.ctot && f1.coff + C <= f1.ctot, "lpips_head: views narrower than C");
    TNR_REQUIRE((int64_t)H * W < (1LL << 31), "lpips_head: layer too large");
    TNR_REQUIRE(ws_bytes >= tnr_lpips_workspace_bytes(N, L), "lpips_head: workspace too small");
    const int64_t hw = (int64_t)H * W;
    const int nb = head_blocks(hw);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lpips_head_kernel, dim3(nb, N), dim3(HEAD_BLOCK), 0, s, f0.ptr, f0.ctot, f0.coff, f1.ptr, f1.ctot, f1.coff, N,
                       (int)hw, C, w, layer, L, ws);
    return tnr_check_launch("lpips_head");
}

extern "C" int tnr_lpips_finalize(int32_t N, int32_t L, const double *ws, int64_t ws_bytes, double *out, double *per_layer,
                                  void *stream) {
    TNR_REQUIRE(ws && out && N >= 1 && L >= 1, "lpips_finalize: bad arguments");
    TNR_REQUIRE(ws_bytes >= tnr_lpips_workspace_bytes(N, L), "lpips_finalize: workspace too small");
    hipLaunchKernelGGL(lpips_finalize_kernel, dim3((unsigned)tnr_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, N, L, ws,
                       ws + (int64_t)L * N * HEAD_MAX_BLOCKS, out, per_layer);
    return tnr_check_launch("lpips_finalize");
}
