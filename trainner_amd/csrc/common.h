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
