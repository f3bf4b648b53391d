// Several dependent 3x3 convolutions over the same pixel grid in ONE launch ("chain"): the five growing-K
// convolutions of a residual dense block (RRDBNet_arch.py:150-163) and the five of its gradient mirror.
//
// Why: a trunk layer is a single residency round (512 tiles = 2 workgroups x 256 CUs at batch 16).  As a
// launch of its own, every workgroup runs its prologue (first-tile fetch: a 37 MB HBM read burst) and its
// epilogue (a 33 MB write burst) at the same time as all others, with the matrix pipes idle -- 17 % of the
// layer (tools/probes/conv_timeline.hip).  In a chain a workgroup keeps its pixel tile through all stages:
// the stores of stage s drain while stage s+1 already runs on the channels that existed before, and only
// the chunk that first touches stage-s output waits -- for the 8 neighbouring tiles (3x3 halo), through a
// per-tile progress counter.
//
// Hand-off protocol (tools/probes/flag_sync.hip): producer = system-coherent stores (sc0 sc1), s_waitcnt
// vmcnt(0), workgroup barrier, one relaxed agent-scope store of the counter; consumer = relaxed
// agent-scope loads of the 8 counters, workgroup barrier, system-coherent loads.  No cache write-back /
// invalidate fences (they cost 4x a whole tile on this part).
// Deadlock freedom: the grid never exceeds the co-resident capacity and every workgroup walks its tiles
// stage-major, so a waited-for tile always belongs to a running workgroup at an earlier program point.
#include <stddef.h>
#include "conv_body.h"
#include "conv_epilogue.h"
#include "conv_handoff.h"

namespace {

struct ChainK {
    int nstages;
    int tiles_x, tiles_y, tiles;       // 16 x 32 pixel tiles over (N, H, W)
    unsigned *progress;                // [tiles]: base + (stages of that tile whose output is visible)
    unsigned base;
    unsigned *err;                     // set to 1 when a dependency wait gives up (never in a healthy run)
    unsigned *cu_ctr;                  // [CH_CU_KEYS] arrivals per CU, never reset: parity = which of the CU's two slots
    unsigned *tile_ctr;                // [2 sets][2 populations] tile dispensers; set (epoch & 1) is live, the other gets zeroed
    int dyn;                           // 1: one tile per workgroup, dealt at run time by CU slot (phase-shifted populations)
    int set;
    int wait_chunk[TNR_CHAIN_MAX];
    ConvK st[TNR_CHAIN_MAX];
};

// Stage s of the kernel-argument table, fetched with scalar loads: indexing the by-value struct with a
// run-time s would make the compiler copy all of it to scratch and turn every field into a VGPR.
__device__ __forceinline__ ConvK chain_stage(int s, int *wait_chunk) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) ChainK karg_chain;
    karg_chain *ka = (karg_chain *)__builtin_amdgcn_kernarg_segment_ptr();   // constant address space: s_load
    *wait_chunk = ka->wait_chunk[s];
    return ka->st[s];
#else
    *wait_chunk = -1;
    return ConvK();
#endif
}

template <int BF>
__global__ void __launch_bounds__(256, 2) conv_chain_kernel(const ChainK c) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int pend_tile = -1;          // wave-uniform
    unsigned pend_value = 0;
    int calls = 0;               // (timeline probe only)
    (void)calls;
    // Phase-shifted populations (c.dyn: tiles == grid == 2 workgroups per CU, i.e. the benchmark's trunk layers): all
    // workgroups reaching a stage boundary together leave the matrix pipes idle while the tile stores drain.  The two
    // workgroups of a CU are therefore put into different halves of the batch (dependencies never cross images) and the
    // second half starts TNR_CHAIN_STAGGER cycles late, so that one workgroup's boundary overlaps the other's MFMA phases.
    // Which slot of its CU a workgroup got is the parity of a per-CU arrival counter; tiles are dealt by two dispensers
    // (a workgroup whose half is exhausted takes from the other one, so the mapping stays a bijection whatever the parity).
    int first_tile = blockIdx.x, tile_step = gridDim.x;
#ifndef TNR_CHAIN_STAGGER
#define TNR_CHAIN_STAGGER 0
#endif
    if (TNR_CHAIN_STAGGER > 0 && c.dyn) {
        __shared__ int s_tile, s_slot;
        if (threadIdx.x == 0) {
            const unsigned hw = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));     // HW_REG_HW_ID
            const unsigned xcc = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11)) & 15u;   // HW_REG_XCC_ID
            const unsigned key = (xcc << 7) | (((hw >> 13) & 7u) << 5) | (((hw >> 12) & 1u) << 4) | ((hw >> 8) & 15u);
            const unsigned slot = atomicAdd(c.cu_ctr + key, 1u) & 1u;
            const unsigned half = (unsigned)c.tiles >> 1;
            unsigned *disp = c.tile_ctr + 2 * c.set;
            unsigned pop = slot, idx = atomicAdd(disp + pop, 1u);
            if (idx >= half) {
                pop ^= 1u;
                idx = atomicAdd(disp + pop, 1u);
            }
            s_tile = (int)(pop * half + idx);
            s_slot = (int)pop;
            if (blockIdx.x == 0) {                    // the other set serves the next launch on this stream
                c.tile_ctr[2 * (c.set ^ 1)] = 0u;
                c.tile_ctr[2 * (c.set ^ 1) + 1] = 0u;
            }
        }
        __syncthreads();
        first_tile = s_tile;
        tile_step = c.tiles;
        if (s_slot) {
            const unsigned long long t0 = __builtin_amdgcn_s_memtime();
            while (__builtin_amdgcn_s_memtime() - t0 < (unsigned long long)(TNR_CHAIN_STAGGER)) __builtin_amdgcn_s_sleep(64);
        }
    }
    for (int s = 0; s < c.nstages; ++s) {
        int wait_chunk;
        const ConvK st = chain_stage(s, &wait_chunk);
        const int ncb = st.KoutP >> 5;
        for (int tile = first_tile; tile < c.tiles; tile += tile_step) {
            int q = tile;
            const int tx = q % c.tiles_x;
            q /= c.tiles_x;
            const int ty = q % c.tiles_y;
            const int n = q / c.tiles_y;
            const ChainWait w{c.progress, c.base + (unsigned)s, n, ty, tx, c.tiles_x, c.tiles_y, c.err, &pend_tile, pend_value};
            for (int cb = 0; cb < ncb; ++cb) {
                // opaque copies: keep the per-tile index arithmetic of the body INSIDE the loops (hoisted out of
                // them it stays live across the whole kernel and spills)
                int txo = tx, tyo = ty, no = n;
                asm volatile("" : "+s"(txo), "+s"(tyo), "+s"(no));
                TNR_STAMP_CALL(calls++);
                conv_tile_body<TNR_CONV_3x3, 32, 1, 4, true, BF>(st, cb, txo, tyo, no, 0, smem, cb == 0 ? wait_chunk : -1, w);
            }
            // this tile's stage-s output is on its way to memory: published from inside the next tile body
            // (every stage has >= 2 input chunks, so the previous pending tile has been published by now)
            pend_tile = tile;
            pend_value = c.base + (unsigned)s + 1u;
        }
    }
    // nothing in this launch waits for the last stage; publish it anyway so the counters stay consistent
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (pend_tile >= 0 && threadIdx.x == 0)
        __hip_atomic_store(c.progress + pend_tile, pend_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int CH_TH = 16, CH_TW = 32;
constexpr size_t chain_lds(int bf = 0) {
    // (the split-operand form keeps the input tile as three bf16 planes: 96-byte rows, conv_body.h)
    const size_t lds_main = (size_t)((CH_TH + 2) * (CH_TW + 2) * ((bf == 2 && TNR_X3_REFILL != 0) ? TNR_X3_ROW : TNR_PST) + 9 * 32 * TNR_PST) * sizeof(float);
    const size_t lds_epi = (size_t)4 * 4 * 32 * 32 * sizeof(float);
    return lds_main > lds_epi ? lds_main : lds_epi;
}
static_assert(chain_lds(2) <= 80 * 1024, "two chain workgroups per CU");

int chain_capacity(int *out) {
    static int cap = 0;
    if (cap == 0) {
        static int cus = 0;
        if (const int rc = tnr_kernel_setup(&cus, "conv_chain", {{conv_chain_kernel<0>, chain_lds()}, {conv_chain_kernel<1>, chain_lds()},
                                                                  {conv_chain_kernel<2>, chain_lds(2)}}))
            return rc;
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, conv_chain_kernel<0>, 256, chain_lds()) != hipSuccess) {
            tnr_set_error("conv_chain: cannot size the grid");
            return TNR_ELAUNCH;
        }
        // LDS allows two workgroups per CU; never trust a larger answer (the progress waits need every
        // workgroup of the grid to be resident at once)
        if (per_cu > 2) per_cu = 2;
        int per_cu_x3 = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_x3, conv_chain_kernel<2>, 256, chain_lds(2)) != hipSuccess || per_cu_x3 < per_cu) {
            tnr_set_error("conv_chain: the split-operand form does not reach %d workgroups per CU (%d)", per_cu, per_cu_x3);
            return TNR_ELAUNCH;
        }
        if (per_cu < 1) {
            tnr_set_error("conv_chain: kernel does not fit a CU");
            return TNR_ELAUNCH;
        }
        cap = per_cu * cus;
    }
    *out = cap;
    return TNR_OK;
}

}  // namespace

extern "C" int64_t tnr_conv_chain_workspace_bytes(const tnr_conv_desc *d) {
    if (d == nullptr) return 0;
    // progress counters (sized for the 8 x 32 tiles of tnr_conv_sweep, which shares the buffer: twice the 16 x 32 tiles of this
    // kernel), the sweep's tile dispensers (words of their own: conv_handoff.h), per-CU arrival counters, 2 x 2 tile dispensers, the
    // error word (ALWAYS the last word of the buffer)
    const int64_t tiles = (int64_t)tnr_cdiv(d->Wo, CH_TW) * tnr_cdiv(d->Ho, 8) * d->N;
    return (tiles + CH_SWEEP_WORDS + CH_CU_KEYS + 4 + 1) * (int64_t)sizeof(uint32_t);
}

extern "C" int tnr_conv_chain(const tnr_conv_desc *stages, const int32_t *fresh_from, int32_t n, uint32_t *ws, int64_t ws_bytes,
                              uint32_t epoch, void *stream) {
    TNR_REQUIRE(stages != nullptr && fresh_from != nullptr && ws != nullptr && n >= 1 && n <= TNR_CHAIN_MAX,
                "conv_chain: 1..%d stages", TNR_CHAIN_MAX);
    const tnr_conv_desc &d0 = stages[0];
    TNR_REQUIRE(tnr_conv_chain_workspace_bytes(&d0) <= ws_bytes, "conv_chain: workspace too small");
    ChainK c;
    c.nstages = n;
    c.tiles_x = tnr_cdiv(d0.Wo, CH_TW);
    c.tiles_y = tnr_cdiv(d0.Ho, CH_TH);
    c.tiles = c.tiles_x * c.tiles_y * d0.N;
    c.progress = ws;
    c.cu_ctr = ws + (ws_bytes / 4 - 1 - 4 - CH_CU_KEYS);      // (behind the progress counters of either tile grid)
    c.tile_ctr = c.cu_ctr + CH_CU_KEYS;
    c.err = tnr_fault_word_or(ws + ws_bytes / 4 - 1);
    c.set = (int)(epoch & 1u);
    c.base = epoch * (uint32_t)(TNR_CHAIN_MAX + 2);
    for (int i = 0; i < n; ++i) {
        const tnr_conv_desc *d = &stages[i];
        TNR_REQUIRE(d->x.ptr && d->y.ptr && d->wp, "conv_chain: null pointer in stage %d", i);
        TNR_REQUIRE(d->mode == TNR_CONV_3x3 && d->N == d0.N && d->H == d0.H && d->W == d0.W && d->Ho == d0.H && d->Wo == d0.W,
                    "conv_chain: stage %d is not a 3x3 convolution over the pixel grid of stage 0", i);
        TNR_REQUIRE(d->KinP >= 2 * TNR_CK, "conv_chain: stage %d needs at least 32 (padded) input channels", i);
        TNR_REQUIRE((d->Cout % 32) == 0 && d->KoutP == d->Cout && (d->Cin % 4) == 0 && (d->KinP % TNR_CK) == 0 && d->Cin <= d->KinP,
                    "conv_chain: stage %d: Cout must be a multiple of 32, Cin of 4", i);
        TNR_REQUIRE(views_aligned(*d), "conv_chain: stage %d: x / y / r1 (+ r1_ch) / r2 / mask (+ range) views must be 4-channel aligned", i);
        TNR_REQUIRE(d->noise_pos >= 0 && d->noise_pos <= 2, "conv_chain: stage %d: bad noise_pos %d", i, d->noise_pos);
        TNR_REQUIRE(buffers_addressable(*d), "conv_chain: stage %d: buffers above 4 GiB are not addressable through a buffer descriptor", i);
        TNR_REQUIRE(fresh_from[i] < d->Cin && (i > 0 || fresh_from[i] < 0), "conv_chain: stage %d: bad fresh_from %d", i, fresh_from[i]);
        ConvK &k = c.st[i];
        k = conv_k_from_desc(*d);
        k.tiles_x = c.tiles_x; k.tiles_y = c.tiles_y; k.ncb = d->KoutP / 32;
        TNR_REQUIRE(d->mma == d0.mma, "conv_chain: stage %d: all stages share one matrix-core precision", i);
        c.wait_chunk[i] = fresh_from[i] < 0 ? -1 : fresh_from[i] / TNR_CK;
    }
    for (int i = n; i < TNR_CHAIN_MAX; ++i) { c.st[i] = c.st[0]; c.wait_chunk[i] = -1; }
    int cap = 0;
    const int rc = chain_capacity(&cap);
    if (rc != TNR_OK) return rc;
    const int grid = c.tiles < cap ? c.tiles : cap;
    c.dyn = (c.tiles == cap && (c.tiles & 1) == 0 && d0.N >= 2 && (d0.N & 1) == 0) ? 1 : 0;   // whole images per population
    if (d0.mma == TNR_MMA_BF16X3)
        hipLaunchKernelGGL(conv_chain_kernel<2>, dim3(grid), dim3(256), chain_lds(2), (hipStream_t)stream, c);
    else if (d0.mma == TNR_MMA_BF16)
        hipLaunchKernelGGL(conv_chain_kernel<1>, dim3(grid), dim3(256), chain_lds(), (hipStream_t)stream, c);
    else
        hipLaunchKernelGGL(conv_chain_kernel<0>, dim3(grid), dim3(256), chain_lds(), (hipStream_t)stream, c);
    return tnr_check_launch("conv_chain");
}
