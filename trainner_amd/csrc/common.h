// Shared device/host helpers for libtrainner_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <initializer_list>
#include "../../include/trainner_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// K-chunk (input channels staged per LDS fill) and the padded LDS pixel stride in dwords.
// 20 dwords: ds_read_b128 of consecutive pixels lands on distinct 16-B slots (5*p mod 16 is a
// permutation), see DESIGN.md "LDS layout".
constexpr int TNR_CK = 16;
constexpr int TNR_PST = TNR_CK + 4;

void tnr_set_error(const char *fmt, ...);
int tnr_check_launch(const char *what);
unsigned *tnr_fault_word_or(unsigned *fallback);      // the registered fault latch (tnr_set_fault_word), else `fallback`

#define TNR_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            tnr_set_error(__VA_ARGS__);   \
            return TNR_EINVAL;            \
        }                                 \
    } while (0)

// One kernel and the dynamic LDS its launches ask for (tnr_kernel_setup).
struct tnr_kernel_lds {
    const void *fn;
    size_t lds;
    template <class F> tnr_kernel_lds(F *f, size_t bytes) : fn(reinterpret_cast<const void *>(f)), lds(bytes) {}
};

// The once-per-process setup of a launch site: raises the dynamic-LDS limit of every listed kernel and leaves the device's CU count
// in *cus.  `cus` points at the call site's own `static int cus = 0`: while it is positive the call does nothing and returns TNR_OK.
// On failure *cus stays 0, so the NEXT call of the site tries again (nothing is latched), the error text names `who`, and the result
// is TNR_ELAUNCH.
inline int tnr_kernel_setup(int *cus, const char *who, std::initializer_list<tnr_kernel_lds> kernels) {
    if (*cus > 0) return TNR_OK;
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) {
        tnr_set_error("%s: cannot query the device", who);
        return TNR_ELAUNCH;
    }
    for (const tnr_kernel_lds &k : kernels)
        if (hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds) != hipSuccess) {
            tnr_set_error("%s: cannot raise dynamic LDS to %zu bytes", who, k.lds);
            return TNR_ELAUNCH;
        }
    *cus = n;
    return TNR_OK;
}

static inline int tnr_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int64_t tnr_cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int tnr_round_up(int a, int b) { return tnr_cdiv(a, b) * b; }

// Nearest x2 in front of a 3x3 s1 p1 convolution is the data-gradient of a virtual 4x4 s2 p1 convolution S whose 16 taps fold the 9
// (DESIGN.md 3.12).  Per axis, folded tap k = 0..3 sums the 3x3 taps tnr_upfold_lo(k) .. tnr_upfold_hi(k): {2}, {1,2}, {0,1}, {0}.
__host__ __device__ inline int tnr_upfold_lo(int k) { return k == 0 ? 2 : (k == 1 ? 1 : 0); }
__host__ __device__ inline int tnr_upfold_hi(int k) { return k <= 1 ? 2 : (k == 2 ? 1 : 0); }
// F[ky][kx] of the 3x3 filter w9, in ONE fp32 order: inside a row of the 3x3 filter over ascending kx first, then the row sums over ascending ky.
__host__ __device__ inline float tnr_upfold_tap(const float *w9, int ky, int kx) {
    const int ylo = tnr_upfold_lo(ky), yhi = tnr_upfold_hi(ky), xlo = tnr_upfold_lo(kx), xhi = tnr_upfold_hi(kx);
    float r0 = w9[ylo * 3 + xlo];
    if (xhi != xlo) r0 = r0 + w9[ylo * 3 + xhi];
    if (yhi == ylo) return r0;
    float r1 = w9[yhi * 3 + xlo];
    if (xhi != xlo) r1 = r1 + w9[yhi * 3 + xhi];
    return r0 + r1;
}
// The transpose: gradient of 3x3 tap (ty, tx) from the 16 gradients dF of the folded taps -- folded taps 2 - t and 3 - t per axis -- in
// the same order: inside a row of dF over ascending kx first, then the two rows over ascending ky.
__host__ __device__ inline float tnr_upfold_grad(const float *dF16, int ty, int tx) {
    const int ky = 2 - ty, kx = 2 - tx;
    return (dF16[ky * 4 + kx] + dF16[ky * 4 + kx + 1]) + (dF16[(ky + 1) * 4 + kx] + dF16[(ky + 1) * 4 + kx + 1]);
}

// The fixed-order fp64 sum of a 256-thread block (`sh`: 256 doubles of LDS); the result is valid in thread 0.  Every reduction of
// the library ends in it: two runs add in the same order and are bit-identical.
__device__ __forceinline__ double tnr_block_sum256(double v, double *sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float tnr_act(float v, int act, float slope) {
    if (act == TNR_ACT_LRELU) return v > 0.f ? v : v * slope;
    if (act == TNR_ACT_RELU) return v > 0.f ? v : 0.f;
    return v;
}
