// The pixel-major matrix-core kernels' common ground (conv_up3.hip, conv_upconv_i2i.hip, conv_unshuffle.hip).  THE TILE CONVENTION: a
// workgroup of four waves owns an 8 x 16 pixel tile; wave w owns tile rows 2w and 2w + 1 = one 32-pixel block of the matrix core's B
// operand, lane (li, half) the pixel (2w + (li >> 4), li & 15).  The weights are the A operand, so a lane ends up holding 4 consecutive
// channels (8 q + 4 half .. + 3 of every 32-row block, q = 0..3) of ITS pixel and stores them as one float4.  One step = 16 reduced values of
// the lane's pixel against NT 32-row blocks of weights, in fp32 (8 x v_mfma_f32_32x32x2_f32 per block), bf16 (one v_mfma_f32_32x32x16_bf16)
// or the exact three-plane bf16 split (six of them, smallest product first).
// The kernels write the decode of this convention (thread -> wave, li, half, ly, lx; block -> n, y0, x0) and the float4 store loop out, each
// in its own body: a struct-returning helper or a store functor changes the code hipcc generates for them.
#pragma once
#include "conv_epilogue.h"

namespace {

constexpr int MP_TH = 8, MP_TW = 16, MP_TPIX = MP_TH * MP_TW;      // pixels per workgroup; 256 threads

template <int NT> __device__ __forceinline__ void mp_zero(f32x16 (&v)[NT]) {
#pragma unroll
    for (int nn = 0; nn < NT; ++nn)
#pragma unroll
        for (int r = 0; r < 16; ++r) v[nn][r] = 0.f;
}
template <int NT> __device__ __forceinline__ void mp_add(f32x16 (&acc)[NT], const f32x16 (&part)[NT]) {
#pragma unroll
    for (int nn = 0; nn < NT; ++nn) acc[nn] += part[nn];
}

constexpr int mp_planes(int mma) { return mma == TNR_MMA_BF16X3 ? 3 : 1; }

// four channels of a staged pixel into LDS in the operand format: fp32, or the bf16 planes (exact split; one plane = the rounding)
template <int MMA>
__device__ __forceinline__ void mp_stage4(f32x4 v, float *sf, __bf16 *sb, const int plane_stride) {
    if constexpr (MMA == TNR_MMA_F32) {
        *reinterpret_cast<f32x4 *>(sf) = v;
    } else {
#pragma unroll
        for (int p = 0; p < mp_planes(MMA); ++p) {
            tnr_bf16x4 pk;
            f32x4 res;
            tnr_pk_level(v, pk, res);
            *reinterpret_cast<tnr_bf16x4 *>(sb + p * plane_stride) = pk;
            v = res;
        }
    }
}

// one step's fragments of a lane.  fp32: [8-value group][block]; bf16: [plane][block].  NT = 1 with the pixel's 16 values: the B operand.
template <int NT, int MMA> struct MpFrag {
    f32x4 f[MMA == TNR_MMA_F32 ? 2 : 1][NT];
    tnr_bf16x8 b[mp_planes(MMA)][NT];
};

// 16 values of the lane's pixel from LDS at `pf` (fp32) | `pb` + plane * plane_stride (bf16)
template <int MMA>
__device__ __forceinline__ MpFrag<1, MMA> mp_pixel16(const float *pf, const __bf16 *pb, const int plane_stride, const int half) {
    MpFrag<1, MMA> x;
    if constexpr (MMA == TNR_MMA_F32) {
#pragma unroll
        for (int g = 0; g < 2; ++g) x.f[g][0] = *reinterpret_cast<const f32x4 *>(pf + g * 8 + half * 4);
    } else {
#pragma unroll
        for (int p = 0; p < mp_planes(MMA); ++p) x.b[p][0] = *reinterpret_cast<const tnr_bf16x8 *>(pb + p * plane_stride + half * 8);
    }
    return x;
}

// the six kept partial products of the three-plane split, smallest first: pixel plane MP_X3_PIX[q] x weight plane MP_X3_W[q]
constexpr int MP_X3_PIX[6] = {0, 2, 1, 0, 1, 0}, MP_X3_W[6] = {2, 0, 1, 1, 0, 0};

// one 8-value group of the fp32 step; the block index innermost, so dependent MFMAs stay apart
template <int NT>
__device__ __forceinline__ void mp_step8_f32(f32x16 (&acc)[NT], const f32x4 (&w)[NT], const f32x4 x) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nn = 0; nn < NT; ++nn) acc[nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[nn][m], x[m], acc[nn], 0, 0, 0);
}

// acc += A (the step's weights `w`) x B (the pixel's 16 values `x`)
template <int NT, int MMA>
__device__ __forceinline__ void mp_step(f32x16 (&acc)[NT], const MpFrag<NT, MMA> &w, const MpFrag<1, MMA> &x) {
    if constexpr (MMA == TNR_MMA_F32) {
#pragma unroll
        for (int g = 0; g < 2; ++g) mp_step8_f32<NT>(acc, w.f[g], x.f[g][0]);
    } else if constexpr (MMA == TNR_MMA_BF16X3) {
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int nn = 0; nn < NT; ++nn)
                acc[nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.b[MP_X3_W[q]][nn], x.b[MP_X3_PIX[q]][0], acc[nn], 0, 0, 0);
    } else {
#pragma unroll
        for (int nn = 0; nn < NT; ++nn) acc[nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.b[0][nn], x.b[0][0], acc[nn], 0, 0, 0);
    }
}

// the same with B read from LDS as mp_pixel16 does; in fp32 each 8-value group is read in front of ITS products, not both in front of the first
template <int NT, int MMA>
__device__ __forceinline__ void mp_step(f32x16 (&acc)[NT], const MpFrag<NT, MMA> &w, const float *pf, const __bf16 *pb, const int plane_stride,
                                        const int half) {
    if constexpr (MMA == TNR_MMA_F32) {
#pragma unroll
        for (int g = 0; g < 2; ++g) mp_step8_f32<NT>(acc, w.f[g], *reinterpret_cast<const f32x4 *>(pf + g * 8 + half * 4));
    } else {
        mp_step<NT, MMA>(acc, w, mp_pixel16<MMA>(pf, pb, plane_stride, half));
    }
}

// ------------------------------------------------------------------------------------------------ host side
inline bool mp_mma_ok(int mma) { return mma == TNR_MMA_F32 || mma == TNR_MMA_BF16 || mma == TNR_MMA_BF16X3; }
inline bool mp_view_ok(const tnr_view &v, int C) { return v.ptr != nullptr && view_aligned(v) && v.coff >= 0 && v.coff + C <= v.ctot; }
inline int64_t mp_tiles(int N, int H, int W) { return (int64_t)tnr_cdiv(W, MP_TW) * tnr_cdiv(H, MP_TH) * N; }

// the tile grid of an N x H x W extent whose layer reaches `scale` times as far
inline int mp_geometry(const char *who, int N, int H, int W, int scale, int *tiles_x, int *tiles_y, int64_t *tiles) {
    TNR_REQUIRE(N > 0 && H > 0 && W > 0, "%s: bad arguments", who);
    TNR_REQUIRE((int64_t)scale * H < (1 << 30) && (int64_t)scale * W < (1 << 30), "%s: image too large", who);
    *tiles_x = tnr_cdiv(W, MP_TW);
    *tiles_y = tnr_cdiv(H, MP_TH);
    *tiles = mp_tiles(N, H, W);
    TNR_REQUIRE(*tiles < (1LL << 31), "%s: grid too large", who);
    return TNR_OK;
}

// a table row: one entry per arithmetic, in the order of the codes (TNR_MMA_F32, _BF16, _BF16X3 = 0, 1, 2)
#define MP_MODES(ENTRY, ...) ENTRY(__VA_ARGS__, TNR_MMA_F32), ENTRY(__VA_ARGS__, TNR_MMA_BF16), ENTRY(__VA_ARGS__, TNR_MMA_BF16X3)

// launches table[index] over `grid` with the one argument struct `k`
inline int mp_launch_entry(const char *who, std::initializer_list<tnr_kernel_lds> table, int index, dim3 grid, void *k, void *stream) {
    const tnr_kernel_lds &kl = table.begin()[index];
    void *args[] = {k};
    (void)hipLaunchKernel(kl.fn, grid, dim3(256), args, kl.lds, (hipStream_t)stream);
    return tnr_check_launch(who);
}
// the same after the launch site's once-per-process tnr_kernel_setup of the table (a site whose index reads *cus calls the two itself)
inline int mp_launch(int *cus, const char *who, std::initializer_list<tnr_kernel_lds> table, int index, dim3 grid, void *k, void *stream) {
    const int rc = tnr_kernel_setup(cus, who, table);
    return rc != TNR_OK ? rc : mp_launch_entry(who, table, index, grid, k, stream);
}

}  // namespace
