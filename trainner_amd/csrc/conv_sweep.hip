// A residual dense block's five growing-K 3x3 convolutions (RRDBNet_arch.py:150-163) -- or the five of its gradient mirror -- in ONE
// launch, with every input channel chunk feeding ALL the stages that consume it ("sweep").
//
// Why (profiles/r03a_chain_timeline.txt): on the bf16x3 path conv_chain_kernel is bound by its memory traffic, not by the matrix core.
// Stage k re-reads the 64 + 32 (k - 1) channels the stages before it already read (832 channel reads per pixel for 192 distinct
// channels).  Here a workgroup keeps the accumulators of all six 32-channel output groups of its tile (x1, x2, x3, x4 and the two
// halves of x5: 192 fp32 per pixel) in registers and sweeps the input channels once per phase:
//     phase 0 = channels of x      -> accumulate into x1 .. x5        phase 1 = channels of x1 -> x2 .. x5      ...
//     phase 4 = channels of x4 -> x5
// so an input element is read (and split into its three bf16 planes) at most twice instead of up to five times, an A fragment read
// from LDS feeds up to 2 x 6 x 6 MFMAs, and the weights arrive PRE-SPLIT from HBM (tnr_conv_sweep_pack builds the stream once per
// optimiser step): no vector-ALU work on the weight path.
//
// Each phase runs as two passes.  Pass a computes ONLY the stage that completes in this phase (one output group), so that its epilogue
// (bias / LeakyReLU / residuals / mask, system-coherent stores) is issued as early as possible; pass b sweeps the same channels again
// for the remaining groups while those stores drain and the neighbouring tiles catch up -- the next phase's first chunk (this tile's
// and its 8 neighbours' fresh output: 3x3 halo) is fetched during the last chunk of pass b.  Same hand-off protocol as conv_chain.hip
// (conv_handoff.h).
//
// Geometry: tile 8 x 32 pixels, one workgroup of four waves per CU, one wave per SIMD: wave w owns tile rows 2 w, 2 w + 1 (two 32-pixel
// M-tiles) x up to six N-tiles (192 accumulator registers); see the comment in front of sweep4_chunk.  Input chunk = 16 channels of the
// 10 x 34 halo tile as 96-byte rows of three bf16 planes in LDS (split once, by the stager, double-buffered: 2 x 36.9 KB with a row of
// its own per staging item).  The weights never pass through LDS: the stream is a sequence of units (unit = one tap x one N-tile x 16
// channels = 32 rows x 96 B = 3 KB) in exactly the order the MFMA loop consumes them, and every wave reads them straight from L2 into a
// register ring.
// Deadlock freedom: the grid is at most one workgroup per CU and covers WHOLE images per round (dependencies never cross images).
// Tiles are DISPENSED in order from an atomic counter -- a waited-for tile was taken by a workgroup that is running, or is the next to
// be dispensed.  Stage s of tile T reads stage s - 1 of tile T + tiles_x + 1, so T completes once tiles up to T + 4 (tiles_x + 1) are
// held: progress needs 4 (tiles_x + 1) + 1 RESIDENT workgroups (21 on a 128-wide image; never more than the tiles of one image, which
// the grid always covers), not the whole grid.  Waits are bounded (fault latch, tnr_set_fault_word).
// Arithmetic (split, kept partial products and their order, channel and tap order, epilogue) is that of conv_tile_body<.., BF = 2>:
// results are bit-identical to five tnr_conv_forward launches in TNR_MMA_BF16X3.
// Three kernels: five stages in TNR_MMA_BF16X3, five stages in TNR_MMA_BF16 (`use_amp`, amp4_chunk), and FOUR stages in TNR_MMA_BF16X3
// (n = 4; SwPlan4 below): the block's conv1 .. conv4 with the same hand-off, dispenser, waits and arithmetic -- bit-identical to four
// tnr_conv_forward launches; the caller runs the 64-wide last stage as a launch of its own (ops.dense_block: the Winograd kernel).
// Still one workgroup per CU; the progress argument above holds with 3 (tiles_x + 1) + 1.
#include <stddef.h>
#include <type_traits>
#include <utility>
#include "conv_body.h"
#include "conv_epilogue.h"
#include "conv_handoff.h"

namespace {

constexpr int SW_TH = 8, SW_TW = 32, SW_HT = SW_TH + 2, SW_WT = SW_TW + 2;
constexpr int SW_ROW = TNR_X3_ROW;                                  // floats per LDS row: three planes of 16 bf16
constexpr int SW_A_ROWS = SW_HT * SW_WT;                            // 340 halo pixels
constexpr int SW_A_ALLOC_ROWS = 384;                                // rows per LDS buffer: every staging item (256 x 6 float4) has a row of its own,
constexpr int SW_A_FLOATS = SW_A_ALLOC_ROWS * SW_ROW;               // so the stager stores without lane masks (rows >= 340 are never read)
constexpr int SW_UNIT_FLOATS = 32 * SW_ROW;                         // one tap x one N-tile x 16 channels
constexpr int SW_NPASS = 9, SW_NSTAGE = 5, SW_NTILE = 6;

// The plan.  N-tile j = output channels [32 j, 32 j + 32) of the block's 192 (x1, x2, x3, x4, x5 lo, x5 hi); phase f sweeps the input
// channels that stage f - 1 produced (phase 0: the block input) into the N-tiles of stages >= f.  Pass p = 2 f (pass a: the N-tile
// of the stage that completes in this phase first -- plus one more, so that a chunk carries enough MFMAs to cover the next chunk's
// fetch) or 2 f + 1 (pass b: the remaining N-tiles, while the stores of pass a's epilogue drain and the neighbours catch up).
//                                       pass:  0  1  2  3  4  5  6  7  8
constexpr int SW_J0[SW_NPASS] =               { 0, 3, 1, 3, 2, 4, 3, 5, 4 };      // first N-tile
constexpr int SW_NJ[SW_NPASS] =               { 3, 3, 2, 3, 2, 2, 2, 1, 2 };      // N-tiles
__host__ __device__ constexpr int sw_phase(int p) { return p >> 1; }
__host__ __device__ constexpr bool sw_apass(int p) { return (p & 1) == 0; }
// (run-time p: arithmetic instead of a table in memory)
__host__ __device__ constexpr int sw_nj_rt(int p) { return p == 7 ? 1 : ((p == 0 || p == 1 || p == 3) ? 3 : 2); }
__host__ __device__ constexpr int sw_j0_rt(int p) { return p == 0 ? 0 : (p == 2 ? 1 : (p == 4 ? 2 : (p == 5 || p == 8 ? 4 : (p == 7 ? 5 : 3)))); }
constexpr bool sw_plan_ok() {
    for (int p = 0; p < SW_NPASS; ++p) {
        if (sw_nj_rt(p) != SW_NJ[p] || sw_j0_rt(p) != SW_J0[p]) return false;
        if (sw_apass(p) && SW_J0[p] != (sw_phase(p) < 4 ? sw_phase(p) : 4)) return false;           // pass a starts at the completing stage's N-tile
        if (!sw_apass(p) && SW_J0[p] != SW_J0[p - 1] + SW_NJ[p - 1]) return false;                  // pass b continues where pass a stopped
        if ((!sw_apass(p) || p == 8) && SW_J0[p] + SW_NJ[p] != SW_NTILE) return false;              // ... up to the last N-tile
    }
    return true;
}

static_assert(sw_plan_ok(), "sweep plan");

// The FOUR-stage plan (conv_sweep4_kernel<false, SwPlan4>): a dense block's conv1 .. conv4 -- or stages 1 .. 4 of its gradient
// mirror -- with the 64-wide last stage left to a launch of its own (the Winograd kernel, conv_wino.hip).  N-tile j = x_{j+1}; the same
// a / b pass structure: pass 2 f computes the stage that completes in phase f first (its epilogue is issued right behind it), pass
// 2 f + 1 the remaining N-tiles of the phase while those stores drain and the neighbours catch up; the last phase has one pass.  A
// phase WITHOUT a pass b would have to load its successor's first chunk -- this tile's and its neighbours' fresh output -- before
// the epilogue that produces it has been issued, so phase 2 is two one-tile passes rather than one pass of two.  18 stagings per tile
// for 252 units (the five-stage plan: 22 for 468), 128 accumulator registers per lane instead of 192.
//                                       pass:  0  1  2  3  4  5  6
constexpr int SW4_NPASS = 7, SW4_NSTAGE = 4, SW4_NTILE = 4;
constexpr int SW4_J0[SW4_NPASS] =             { 0, 2, 1, 3, 2, 3, 3 };
constexpr int SW4_NJ[SW4_NPASS] =             { 2, 2, 2, 1, 1, 1, 1 };
__host__ __device__ constexpr int sw4_nj_rt(int p) { return p < 3 ? 2 : 1; }
__host__ __device__ constexpr int sw4_j0_rt(int p) { return p == 0 ? 0 : (p == 2 ? 1 : ((p == 1 || p == 4) ? 2 : 3)); }
constexpr bool sw4_plan_ok() {
    for (int p = 0; p < SW4_NPASS; ++p) {
        if (sw4_nj_rt(p) != SW4_NJ[p] || sw4_j0_rt(p) != SW4_J0[p]) return false;
        if (sw_apass(p) && SW4_J0[p] != sw_phase(p)) return false;                                   // pass a starts at the completing stage's N-tile
        if (!sw_apass(p) && SW4_J0[p] != SW4_J0[p - 1] + SW4_NJ[p - 1]) return false;               // pass b continues where pass a stopped
        if ((!sw_apass(p) || p == SW4_NPASS - 1) && SW4_J0[p] + SW4_NJ[p] != SW4_NTILE) return false;      // ... up to the last N-tile
    }
    return true;
}
static_assert(sw4_plan_ok(), "four-stage sweep plan");

// A plan as a compile-time parameter of conv_sweep4_kernel (phase = pass / 2 and pass a = even pass in both).
struct SwPlan5 {
    static constexpr int NPASS = SW_NPASS, NSTAGE = SW_NSTAGE, NTILE = SW_NTILE;
    static constexpr int j0(int p) { return SW_J0[p]; }
    static constexpr int nj(int p) { return SW_NJ[p]; }
};
struct SwPlan4 {
    static constexpr int NPASS = SW4_NPASS, NSTAGE = SW4_NSTAGE, NTILE = SW4_NTILE;
    static constexpr int j0(int p) { return SW4_J0[p]; }
    static constexpr int nj(int p) { return SW4_NJ[p]; }
};
// (run-time stage count ns = 5 / 4: the pack kernels and the host)
__host__ __device__ constexpr int sw_npass_rt(int ns) { return ns == 4 ? SW4_NPASS : SW_NPASS; }
__host__ __device__ constexpr int sw_nj_rt(int p, int ns) { return ns == 4 ? sw4_nj_rt(p) : sw_nj_rt(p); }
__host__ __device__ constexpr int sw_j0_rt(int p, int ns) { return ns == 4 ? sw4_j0_rt(p) : sw_j0_rt(p); }

struct SweepK {
    int nck0;                          // chunks of phase 0 (channels of the block input / 16); the other phases have 2
    int tiles_x, tiles_y, tpi, tiles;  // 8 x 32 pixel tiles; tpi = tiles per image
    unsigned *progress;                // [tiles]: base + (stages of that tile whose output is visible)
    unsigned base;
    unsigned *err;
    unsigned *disp;                    // [2] tile dispenser + finished-workgroup count; zero between launches
    const float *wq;                   // pre-split weight stream (tnr_conv_sweep_pack)
    int wq_bytes;
    ConvK st[SW_NSTAGE];
};

__host__ __device__ inline int sw_nchunks(int p, int nck0) { return sw_phase(p) == 0 ? nck0 : 2; }
__host__ __device__ inline int sw_ch_lo(int p, int nck0) { return sw_phase(p) == 0 ? 0 : 16 * nck0 + 32 * (sw_phase(p) - 1); }
__host__ __device__ inline int sw_total_units(int nck0, int ns = SW_NSTAGE) {
    int u = 0;
    for (int p = 0; p < sw_npass_rt(ns); ++p) u += sw_nchunks(p, nck0) * 9 * sw_nj_rt(p, ns);
    return u;
}

// ---- weight stream: for every pass, chunk, tap and N-tile of the pass (in that order) one unit of 32 rows (output channels) x 16 input
// channels as three bf16 planes (hi, mid, lo) of 1 KB each.  A plane is ONE block in the order the lanes hold it -- lane (half = channel
// octet h, li = row r) owns 16 bytes -- so a fragment load is a fully coalesced 1 KB read straight into the MFMA operand registers.
struct SweepPackK {
    int nck0, units;
    int ns;                            // stages: 5, or 4 (the four-stage plan)
    const float *wp[SW_NSTAGE];
    int KinP[SW_NSTAGE], KoutP[SW_NSTAGE];
    float *out;
};

__device__ __forceinline__ void sweep_pack_one(const SweepPackK &a, const int g) {
    const int unit = g >> 6, r = (g >> 1) & 31, sp = g & 1;
    if (unit >= a.units) return;
    int p = 0, u0 = 0;
    for (; p < sw_npass_rt(a.ns); ++p) {
        const int n = sw_nchunks(p, a.nck0) * 9 * sw_nj_rt(p, a.ns);
        if (unit < u0 + n) break;
        u0 += n;
    }
    const int lu = unit - u0, nj = sw_nj_rt(p, a.ns);
    const int jj = lu % nj, ct = lu / nj, tap = ct % 9, ck = ct / 9;
    const int j = sw_j0_rt(p, a.ns) + jj;
    const int s = j < 4 ? j : 4, cb = j == 5 ? 1 : 0;
    const int h = sp ^ ((r >> TNR_X3_SWZ) & 1);
    const int ch = sw_ch_lo(p, a.nck0) + 16 * ck + 8 * h;
    const float *src = a.wp[s] + ((size_t)tap * a.KoutP[s] + cb * 32 + r) * a.KinP[s] + ch;
    const f32x4 q0 = *reinterpret_cast<const f32x4 *>(src), q1 = *reinterpret_cast<const f32x4 *>(src + 4);
    tnr_bf16x8 pl[3];
    tnr_split_bf16x3(q0, q1, pl);
    float *dst = a.out + (size_t)unit * SW_UNIT_FLOATS + (h * 32 + r) * 4;
#pragma unroll
    for (int k = 0; k < 3; ++k) *reinterpret_cast<tnr_bf16x8 *>(dst + k * 256) = pl[k];
}

__global__ void __launch_bounds__(256) sweep_pack_kernel(const SweepPackK a) { sweep_pack_one(a, blockIdx.x * 256 + threadIdx.x); }

// Stage s of the kernel-argument table, fetched with scalar loads (indexing the by-value struct with a run-time s would make the
// compiler copy all of it to scratch)
__device__ __forceinline__ ConvK sweep_stage(int s) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) SweepK karg_sweep;
    karg_sweep *ka = (karg_sweep *)__builtin_amdgcn_kernarg_segment_ptr();   // constant address space: s_load
    return ka->st[s];
#else
    return ConvK();
#endif
}

#ifdef SW_TIMELINE   /* probe build (tools/build_variant.py sw_tl -DSW_TIMELINE): cycles wave 0 of every workgroup spends per part of the loop */
__device__ unsigned long long sw_tl[16];
__device__ unsigned long long sw_tl2[16];      // cycles / count per unit class (sweep4_chunk)
#define SW_T(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#define SW_ADD(i, d) do { tl[i] += (d); } while (0)
#else
#define SW_T(v) do { } while (0)
#define SW_ADD(i, d) do { } while (0)
#endif

// =====================================================================================================================================
// The work of a tile among the four waves:
//   * one wave per SIMD (256 threads, the whole 512-entry register file): a wave owns TWO tile rows (2 M-tiles x 6 N-tiles = 192
//     accumulator registers), so a weight fragment feeds 12 MFMAs;
//   * a chunk (9 taps x NJ N-tiles) is ONE straight-line block: tap offsets, LDS addresses and the places of the side work are
//     compile-time, and nothing but MFMAs and the side work below is issued between two chunk tops (one barrier per chunk);
//   * the input chunk's operand split + LDS store (6 items per thread) is handed out over the last units of the chunk's second and
//     last third, and the epilogue of a completed stage runs behind its pass's chunk loop.
constexpr int S4_A_IT = (SW_A_ROWS * 4 + 255) / 256;                // staging items (float4) per thread and chunk: 6
static_assert(S4_A_IT == 6, "the side-work plan: 6 items per chunk");

template <int B, class F, int... I>
__device__ __forceinline__ void sw_static_for_seq(F &f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, B + I>{}), ...);
}
template <int B, int E, class F>
__device__ __forceinline__ void sw_static_for(F &&f) {
    sw_static_for_seq<B>(f, std::make_integer_sequence<int, (E > B ? E - B : 0)>{});
}

// One input chunk: N-tiles [J0, J0 + NJ) x 9 taps x 16 channels.
// With one wave per SIMD an instruction costs nothing only while an MFMA the wave has already issued is still executing (32 cycles
// each), so everything else is handed out over the 12 MFMAs of a unit, a few instructions behind each:
//     MFMA 0 .. 2   the three planes of the weight fragment two units ahead (`b_fetch`)
//     MFMA 3 .. 8   the six reads of the next tap's input fragments (units in front of a new tap)
//     MFMA 4 .. 8   one step of an input-chunk item (hi plane, mid plane, lo plane + store, store, store: see the kernel)
// (profiles/r03t_sweep4_timeline.txt: issued in blocks between the units these cost 50 .. 100 cycles per plain unit and 520 per item
// against the unit's 384 cycles of matrix core.)
// The weight fragments do not pass through LDS.  The stream is consumed strictly in order, one 3 KB unit per 12 MFMAs, and in the
// stream's layout (sweep_pack_kernel) a plane of a unit is one coalesced 1 KB read in register order: every wave fetches the fragments
// of unit g + 2 straight from L2 / L1 into a three-deep register ring behind the first three MFMAs of unit g (the four waves of a CU
// ask for the same lines within a few hundred cycles: one L2 read, three L1 hits).
template <int J0, int NJ, int NT, class Item, class Tick, class BFetch>
__device__ __forceinline__ void sweep4_chunk(f32x16 (&acc)[2][NT], const float *sa, const int (&apix0)[2], const int half,
                                             Item &&item_step, Tick &&tick, tnr_bf16x8 (&fbr)[3][3], BFetch &&b_fetch) {
    static_assert((9 * NJ) % 3 == 0, "a chunk starts at ring position 0");
    static_assert(J0 >= 0 && J0 + NJ <= NT, "the chunk's N-tiles are accumulators of the kernel");
    constexpr int TA[6] = {0, 2, 1, 0, 1, 0}, TB[6] = {2, 0, 1, 1, 0, 0};      // the six kept partial products, smallest first
    constexpr int NU = 9 * NJ, SU = 3 * NJ;
    tnr_bf16x8 fa[2][2][3];
    const float *a_src[2][2];          // [tap parity][M-tile]: LDS address of the tap's fragment rows
    auto addr_a = [&](auto tc) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value, dy = t / 3, dx = t % 3;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int pp = apix0[m] + dy * SW_WT + dx;
            a_src[t & 1][m] = sa + pp * SW_ROW + 4 * (half ^ ((pp >> TNR_X3_SWZ) & 1));
        }
    };
    auto read_a = [&](auto tc, int m, int sp) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value;
        fa[t & 1][m][sp] = *reinterpret_cast<const tnr_bf16x8 *>(a_src[t & 1][m] + 8 * sp);
    };
    addr_a(std::integral_constant<int, 0>{});
#pragma unroll
    for (int k = 0; k < 6; ++k) read_a(std::integral_constant<int, 0>{}, k / 3, k % 3);
    sw_static_for<0, NU>([&](auto uc) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value, t = u / NJ, jj = u % NJ;
#ifdef SW_TIMELINE
        const unsigned long long tu0 = __builtin_amdgcn_s_memtime();
#endif
        constexpr bool NEXT_TAP = u + 1 < NU && (u + 1) % NJ == 0;
        // input-chunk item i: behind the last units of the chunk's second and last third (NJ = 1: one per unit from unit 3)
        constexpr int ITEM = NJ == 1 ? u - 3 : (u >= 2 * SU - 4 && u <= 2 * SU - 2 ? u - (2 * SU - 4) : (u >= 3 * SU - 3 ? u - (3 * SU - 3) + 3 : -1));
        if constexpr (NEXT_TAP) addr_a(std::integral_constant<int, (t + 1 < 9 ? t + 1 : 8)>{});
        __builtin_amdgcn_sched_barrier(0);
        sw_static_for<0, 12>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = decltype(ic)::value, p = i / 2, m = i % 2;
            acc[m][J0 + jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[t & 1][m][TA[p]], fbr[u % 3][TB[p]], acc[m][J0 + jj], 0, 0, 0);
            if constexpr (i < 3) b_fetch(std::integral_constant<int, (u + 2) % 3>{}, i);       // unit g + 2 into the slot unit g - 1 left
            if constexpr (NEXT_TAP && i >= 3 && i < 9) read_a(std::integral_constant<int, (t + 1 < 9 ? t + 1 : 8)>{}, (i - 3) / 3, (i - 3) % 3);
            if constexpr (ITEM >= 0 && ITEM < S4_A_IT && i >= 4 && i < 9) item_step(std::integral_constant<int, (ITEM >= 0 && ITEM < S4_A_IT ? ITEM : 0)>{}, std::integral_constant<int, (i >= 4 && i < 9 ? i - 4 : 0)>{});
            __builtin_amdgcn_sched_barrier(0);
        });
#ifdef SW_TIMELINE
        if constexpr (NJ == 3 || NJ == 2) {
            // class: 2 units with an input-chunk item, 3 plain (NJ = 2: classes 6, 7)
            constexpr int cls = ITEM >= 0 && ITEM < S4_A_IT ? 2 : 3;
            tick(cls + (NJ == 2 ? 4 : 0), __builtin_amdgcn_s_memtime() - tu0);
        }
#endif
    });
}

// The same chunk in TNR_MMA_BF16 (`use_amp`: operands ROUNDED to bf16, base_model.py:736-744): one product per (tap, N-tile, M-tile), so a
// unit is 2 MFMAs (64 cycles of matrix core) and only plane 0 of either operand is used -- the weight stream's hi plane IS the
// round-to-nearest bf16 weight, the input tile's hi plane the rounded activation (the stager skips the other two).  With units this
// short the fragment ring is nine deep (unit g + 8 is fetched behind the first MFMA of unit g: ~500 cycles of look-ahead, an L2 hit),
// one whole input-chunk item (convert + one 8-byte LDS store) rides behind the second MFMA of the chunk's last units.
template <int J0, int NJ, int NT, class Item, class BFetch>
__device__ __forceinline__ void amp4_chunk(f32x16 (&acc)[2][NT], const float *sa, const int (&apix0)[2], const int half,
                                           Item &&item, tnr_bf16x8 (&fbq)[9], BFetch &&b_fetch) {
    constexpr int NU = 9 * NJ;
    static_assert(NU % 9 == 0, "a chunk starts at ring position 0");
    tnr_bf16x8 fa[2][2];               // [tap parity][M-tile]
    const float *a_src[2][2];
    auto addr_a = [&](auto tc) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value, dy = t / 3, dx = t % 3;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int pp = apix0[m] + dy * SW_WT + dx;
            a_src[t & 1][m] = sa + pp * SW_ROW + 4 * (half ^ ((pp >> TNR_X3_SWZ) & 1));
        }
    };
    addr_a(std::integral_constant<int, 0>{});
    fa[0][0] = *reinterpret_cast<const tnr_bf16x8 *>(a_src[0][0]);
    fa[0][1] = *reinterpret_cast<const tnr_bf16x8 *>(a_src[0][1]);
    sw_static_for<0, NU>([&](auto uc) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value, t = u / NJ, jj = u % NJ;
        constexpr bool NEXT_TAP = u + 1 < NU && (u + 1) % NJ == 0;
        constexpr int ITEM = u - (NU - S4_A_IT);               // the chunk's last six units carry the next chunk's six items
        if constexpr (NEXT_TAP) addr_a(std::integral_constant<int, (t + 1 < 9 ? t + 1 : 8)>{});
        __builtin_amdgcn_sched_barrier(0);
        acc[0][J0 + jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[t & 1][0], fbq[u % 9], acc[0][J0 + jj], 0, 0, 0);
        b_fetch(std::integral_constant<int, (u + 8) % 9>{});
        if constexpr (NEXT_TAP) fa[(t + 1) & 1][0] = *reinterpret_cast<const tnr_bf16x8 *>(a_src[(t + 1) & 1][0]);
        __builtin_amdgcn_sched_barrier(0);
        acc[1][J0 + jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[t & 1][1], fbq[u % 9], acc[1][J0 + jj], 0, 0, 0);
        if constexpr (NEXT_TAP) fa[(t + 1) & 1][1] = *reinterpret_cast<const tnr_bf16x8 *>(a_src[(t + 1) & 1][1]);
        if constexpr (ITEM >= 0 && ITEM < S4_A_IT) item(std::integral_constant<int, (ITEM >= 0 && ITEM < S4_A_IT ? ITEM : 0)>{});
        __builtin_amdgcn_sched_barrier(0);
    });
}

template <bool AMP = false, class P = SwPlan5>
__global__ void __launch_bounds__(256, 1) conv_sweep4_kernel(const SweepK c) {
    static_assert(std::is_same<P, SwPlan5>::value || !AMP, "the four-stage plan exists in bf16x3 only");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *s_a = smem;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, half = lane >> 5;
    // Tiles are DISPENSED, not dealt: a workgroup takes the next tile from an atomic counter.  With a static deal (tile = b + grid * k)
    // the hand-off needs EVERY workgroup of the grid resident: with one CU held by another kernel (tools/probes/sweep_hog.py,
    // profiles/r03ad_sweep_hog*.txt) the tiles of the missing workgroup stall all their neighbours until a CU comes free (4.0x slower
    // there, against 1.10x dispensed).  Dispensed in order, a tile's neighbours are always taken by workgroups that ARE running; a
    // handful of resident workgroups is enough for progress, and a CU (or an XCD) that runs slower simply takes fewer tiles.
    const int g = gridDim.x;
    __shared__ int s_next_tile;
    auto next_tile = [&]() __attribute__((always_inline)) {
        if (tid == 0) s_next_tile = (int)atomicAdd(c.disp, 1u);
        __syncthreads();
        return __builtin_amdgcn_readfirstlane(s_next_tile);
    };
    const ConvK &x0 = c.st[0];
    const __amdgpu_buffer_rsrc_t x_rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x0.x), 0, (int)((unsigned)x0.N * x0.H * x0.W * x0.x_ct * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(c.wq), 0, c.wq_bytes, 0x00020000);
    const int apix0[2] = {(2 * wave) * SW_WT + li, (2 * wave + 1) * SW_WT + li};
    int pend_tile = -1;          // tile whose newest stage output still has to be published (wave-uniform)
    unsigned pend_value = 0;
    int pend_age = 0;
#ifdef SW_TIMELINE
    unsigned long long tl[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tl2[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long tl_begin = __builtin_amdgcn_s_memtime();
#endif

    for (int tile = next_tile(); tile < c.tiles; tile = next_tile()) {
        SW_T(t_tile0);
        const int n = tile / c.tpi, rem = tile - n * c.tpi;
        const int ty = rem / c.tiles_x, tx = rem - ty * c.tiles_x;
        const int ty0 = ty * SW_TH, tx0 = tx * SW_TW;
        // ---- staging plan of the input tile: item i = tid + 256 it -> halo pixel i / 4, channel quad i % 4
        int in_off[S4_A_IT], a_dst[S4_A_IT];
#pragma unroll
        for (int it = 0; it < S4_A_IT; ++it) {
            const int i = tid + it * 256, row = i >> 2, q = i & 3;
            const int hr = row / SW_WT, hc = row - hr * SW_WT;
            const int Y = ty0 + hr - 1, X = tx0 + hc - 1;
            const bool in = (row < SW_A_ROWS) & (Y >= 0) & (Y < x0.H) & (X >= 0) & (X < x0.W);
            in_off[it] = in ? (((n * x0.H + Y) * x0.W + X) * x0.x_ct + x0.x_co + q * 4) : -1;
            a_dst[it] = row * SW_ROW + 4 * ((q >> 1) ^ ((row >> TNR_X3_SWZ) & 1)) + 2 * (q & 1);        // (row < SW_A_ALLOC_ROWS: always a valid address)
        }
        static_assert(S4_A_IT * 256 <= SW_A_ALLOC_ROWS * 4, "a row per staging item");
        f32x4 rin[S4_A_IT];
        auto a_load = [&](int ch, bool valid = true) __attribute__((always_inline)) {          // system-coherent: the channels may have been written by another CU in this launch
#pragma unroll
            for (int it = 0; it < S4_A_IT; ++it) {
                const unsigned bo = (valid && in_off[it] >= 0) ? (unsigned)(in_off[it] + ch) * 4u : 0xfffffff0u;      // (past the end: the range check returns 0)
                rin[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, (int)bo, 0, TNR_COH_LOAD_AUX));
            }
        };
        // item `it` in five steps (see sweep4_chunk), each over the item's four channels at once so that no instruction waits for the one
        // in front of it: 0 hi plane and first residual, 1 mid plane and second residual, 2 lo plane + store hi, 3 store mid, 4 store lo
        // (tnr_split4_bf16x3's arithmetic with ONE packed conversion per channel pair and level -- tnr_split4_bf16x3_pk's form, conv_body.h:
        // 22 instead of 30 vector instructions per item, bit-identical)
        tnr_bf16x4 ih, im, il;
        f32x4 ir;
        auto item_step_buf = [&](auto ic, auto kc, int buf) __attribute__((always_inline)) {
            constexpr int it = decltype(ic)::value, k = decltype(kc)::value;
            if constexpr (k == 0) {
                tnr_pk_level(rin[it], ih, ir);
            } else if constexpr (k == 1) {
                const f32x4 r1 = ir;
                tnr_pk_level(r1, im, ir);
            } else {
                if constexpr (k == 2) {
                    const tnr_f32x2 a = {ir[0], ir[1]}, b = {ir[2], ir[3]};
                    il = __builtin_bit_cast(tnr_bf16x4, tnr_f32x2{__builtin_bit_cast(float, __builtin_convertvector(a, tnr_bf16x2)),
                                                                __builtin_bit_cast(float, __builtin_convertvector(b, tnr_bf16x2))});
                }
                float *dst = s_a + buf * SW_A_FLOATS + a_dst[it] + 8 * (k - 2);
                *reinterpret_cast<tnr_f32x2 *>(dst) = __builtin_bit_cast(tnr_f32x2, k == 2 ? ih : (k == 3 ? im : il));
            }
        };
        auto a_store_item = [&](auto ic, int buf) __attribute__((always_inline)) {
            sw_static_for<0, 5>([&](auto kc) __attribute__((always_inline)) { item_step_buf(ic, kc, buf); });
        };

        f32x16 acc[2][P::NTILE];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < P::NTILE; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.f;

        // ---- prologue: input chunk 0 into LDS, the first weight fragments on their way
        a_load(0);
        __syncthreads();                 // the previous tile's last fragments are consumed
        // register ring of weight fragments, unit `bq` is the next to fetch (wave-uniform); units 0 and 1 go out now
        tnr_bf16x8 fbr[3][3];
        int bq = 0;
        auto b_fetch = [&](auto rc, int sp) __attribute__((always_inline)) {
            constexpr int r = decltype(rc)::value;
            fbr[r][sp] = __builtin_bit_cast(tnr_bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rs, lane * 16, (bq * 3 + sp) * 1024, 0));      // (past the end of the stream: zeros)
            if (sp == 2) ++bq;
        };
        // bf16-operand form: nine single-plane fragments (plane 0 of unit `bq`), units 0 .. 7 go out now
        tnr_bf16x8 fbq[9];
        auto b_fetch1 = [&](auto rc) __attribute__((always_inline)) {
            constexpr int r = decltype(rc)::value;
            fbq[r] = __builtin_bit_cast(tnr_bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rs, lane * 16, bq * 3072, 0));
            ++bq;
        };
        auto a_item1 = [&](auto ic, int buf) __attribute__((always_inline)) {      // a whole item: round to bf16, store plane 0
            constexpr int it = decltype(ic)::value;
            const tnr_bf16x4 h = __builtin_convertvector(rin[it], tnr_bf16x4);
            *reinterpret_cast<tnr_f32x2 *>(s_a + buf * SW_A_FLOATS + a_dst[it]) = __builtin_bit_cast(tnr_f32x2, h);
        };
        if constexpr (AMP) {
            sw_static_for<0, 8>([&](auto rc) __attribute__((always_inline)) { b_fetch1(rc); });
            sw_static_for<0, S4_A_IT>([&](auto ic) __attribute__((always_inline)) { a_item1(ic, 0); });
        } else {
#pragma unroll
            for (int sp = 0; sp < 3; ++sp) b_fetch(std::integral_constant<int, 0>{}, sp);
#pragma unroll
            for (int sp = 0; sp < 3; ++sp) b_fetch(std::integral_constant<int, 1>{}, sp);
        }
        if constexpr (!AMP) sw_static_for<0, S4_A_IT>([&](auto ic) __attribute__((always_inline)) { a_store_item(ic, 0); });
        { SW_T(t_pro); SW_ADD(0, t_pro - t_tile0); }
        int e = 0;                       // input chunks consumed so far in this tile
        bool has_next = false;
        auto tick = [&](int cls, unsigned long long dt) __attribute__((always_inline)) {
#ifdef SW_TIMELINE
            tl2[cls] += dt;
            tl2[8 + cls] += 1;
#endif
        };
        // chunk top: only the input tile's double buffer is synchronised (LDS stores of every wave done, the other buffer consumed) --
        // the weight prefetch stays in flight across the barrier.  A pending stage output is published at the second chunk top after
        // its epilogue (a whole chunk later: its stores have drained, vmcnt(0) costs the two prefetched units).
        auto chunk_top = [&]() __attribute__((always_inline)) {
            const bool pub = pend_tile >= 0 && ++pend_age >= 2;
            SW_T(t_s0);
            if (pub) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            SW_T(t_s2);
            SW_ADD(4, t_s2 - t_s0);
            if (pub) {
                if (tid == 0) __hip_atomic_store(c.progress + pend_tile, pend_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                pend_tile = -1;
            }
        };
        // (the stage index is a compile-time constant at every accumulator access: a run-time switch or select over the array elements
        //  is rewritten into one load at a computed address and the whole accumulator array then lives in scratch memory)
        auto epilogue_of = [&](auto sc) __attribute__((always_inline)) {
            constexpr int S = decltype(sc)::value;
            SW_T(t_e0);
            const ConvK a = sweep_stage(S);
            const __amdgpu_buffer_rsrc_t y_rs =
                __builtin_amdgcn_make_buffer_rsrc(a.y, 0, (int)((unsigned)a.N * a.Ho * a.Wo * a.y_ct * 4u), 0x00020000);
            if constexpr (S < 4) {
                f32x16 t[2][1];
                t[0][0] = acc[0][S];
                t[1][0] = acc[1][S];
                conv_epilogue_dpp<TNR_CONV_3x3, SW_TW, 1, 2, true, 8, false>(a, t, 0, n, ty0, tx0, 0, wave, li, half, y_rs);
            } else {
                f32x16 t[2][2];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    t[m][0] = acc[m][4];
                    t[m][1] = acc[m][5];
                }
                conv_epilogue_dpp<TNR_CONV_3x3, SW_TW, 2, 2, true, 8>(a, t, 0, n, ty0, tx0, 0, wave, li, half, y_rs);
            }
            pend_tile = tile;
            pend_value = c.base + (unsigned)S + 1u;
            pend_age = 0;
            { SW_T(t_e1); SW_ADD(8, t_e1 - t_e0); }
        };
        auto item_step = [&](auto ic, auto kc) __attribute__((always_inline)) {
            if (has_next) item_step_buf(ic, kc, (e + 1) & 1);
        };

        // The nine passes are unrolled in the source: every accumulator access and every stage index is a compile-time constant, and
        // the control flow the register allocator sees is a plain sequence of chunk loops.
        sw_static_for<0, P::NPASS>([&](auto pc) __attribute__((always_inline)) {
            constexpr int p = decltype(pc)::value;
            const int nchunks = sw_nchunks(p, c.nck0), ch_lo = sw_ch_lo(p, c.nck0);
#pragma unroll 1
            for (int ck = 0; ck < nchunks; ++ck) {
                chunk_top();                 // the chunk's input tile is in LDS
                const bool last_ck = ck + 1 == nchunks;
                has_next = !(last_ck && p == P::NPASS - 1);
                int ch_keep = 0;
                if (has_next) {
                    int ch_next = ch_lo + 16 * (ck + 1);
                    if (last_ck) {
                        ch_next = sw_ch_lo(p + 1 < P::NPASS ? p + 1 : p, c.nck0);
                        if constexpr (p + 1 < P::NPASS && sw_apass(p + 1)) {
                            // the first chunk of the next phase is the output of the stage this tile and its 8 neighbours finished
                            // in pass a of the current phase
                            const ChainWait w{c.progress, c.base + (unsigned)sw_phase(p + 1), n, ty, tx, c.tiles_x, c.tiles_y, c.err,
                                              &pend_tile, pend_value};
                            SW_T(t_w0);
                            w();
                            { SW_T(t_w1); SW_ADD(1, t_w1 - t_w0); }
                        }
                    }
                    ch_keep = ch_next;
                }
                {
                    // the loads are issued on EVERY path (past-the-end addresses when there is no next chunk): with a branch around
                    // them the compiler has to assume the shorter queue in front of the first fragment use and waits for these loads too
                    SW_T(t_al0);
                    a_load(ch_keep, has_next);
                    { SW_T(t_al1); SW_ADD(2, t_al1 - t_al0); }
                }
                const float *sa = s_a + (e & 1) * SW_A_FLOATS;
                SW_T(t_c0);
                if constexpr (AMP) {
                    auto item1 = [&](auto ic) __attribute__((always_inline)) {
                        if (has_next) a_item1(ic, (e + 1) & 1);
                    };
                    amp4_chunk<P::j0(p), P::nj(p)>(acc, sa, apix0, half, item1, fbq, b_fetch1);
                } else {
                    sweep4_chunk<P::j0(p), P::nj(p)>(acc, sa, apix0, half, item_step, tick, fbr, b_fetch);
                }
                { SW_T(t_c1); SW_ADD(6, t_c1 - t_c0); SW_ADD(15, 1ull); SW_ADD(9 + (P::nj(p) == 3 ? 0 : (P::nj(p) == 2 ? 1 : 2)), t_c1 - t_c0); }
                ++e;
            }
            if constexpr (sw_apass(p) && p + 1 < P::NPASS) {
                // the epilogue of the stage this pass completed stands BEHIND the pass's chunk loop, on every path -- under
                // `if (ck == 0)` at the top of the next pass the compiler must assume, at the join, that the fragment ring is the
                // youngest thing in the memory queue and makes the first unit wait for the epilogue's stores.  Published two chunk tops
                // later (chunk_top): a whole chunk after the stores were issued.
                epilogue_of(std::integral_constant<int, sw_phase(p)>{});
            }
        });
        epilogue_of(std::integral_constant<int, P::NSTAGE - 1>{});      // the last stage (the last pass is a pass a)
    }
    // nothing in this launch waits for the last stage; publish it anyway so the counters stay consistent
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (pend_tile >= 0 && tid == 0) __hip_atomic_store(c.progress + pend_tile, pend_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0 && atomicAdd(c.disp + 1, 1u) == (unsigned)g - 1u) {      // the last workgroup out leaves both words at zero for the next launch
        __hip_atomic_store(c.disp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(c.disp + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#ifdef SW_TIMELINE
    if (tid == 0) {
        tl[14] = __builtin_amdgcn_s_memtime() - tl_begin;
        for (int i = 0; i < 16; ++i) atomicAdd(&sw_tl[i], tl[i]);
        for (int i = 0; i < 16; ++i) atomicAdd(&sw_tl2[i], tl2[i]);
    }
#endif
}

// =====================================================================================================================================
// A plain 3x3 convolution / data-gradient on the machinery of the sweep ("d4"; TNR_MMA_BF16X3, Cout % 64 == 0, Cin % 16 == 0).
// The 8-wave kernel of conv_x3w8.h splits and stages the 9 x 64 x 16 weight slab through LDS in every workgroup at every chunk, in a
// phase of its own between two barriers (the matrix core idles meanwhile: MFMA busy 0.62).  Here the weights come as a pre-split stream
// (tnr_conv_wq_pack: units of one tap x one 32-cout N-tile x 16 channels, 3 KB, plane by plane in register order) straight from L2 into a
// register ring, the input tile is double-buffered in LDS and its split + store is handed out behind the MFMAs -- sweep4_chunk<0, 2>,
// the chunk body of the dense-block sweep with two N-tiles: one barrier per chunk, nothing but MFMAs and side work between them.
// Tile 8 x 32 pixels x 64 output channels, four waves (wave w: tile rows 2 w, 2 w + 1), two workgroups per CU (73.7 KB of LDS each):
// one workgroup's epilogue / prologue / barrier runs under the other's MFMAs.  Arithmetic (split, kept products and their
// order, chunk and tap order, epilogue) is that of conv_tile_body<.., BF = 2> / conv3x3_x3w8_kernel: bit-identical results.
struct D4K {
    ConvK a;
    const float *wq;                   // [cb][chunk][tap][N-tile] units (the sweep's unit layout)
    int wq_bytes;
    int nck;                           // input chunks (Cin / 16)
    int tiles_x, tiles_y, ncb, tiles;
};

struct D4PackK {
    const float *wp;
    int KinP, KoutP, nck, ncb, units;
    int shuffle;                       // 2: the stream's cout r' = sub * (Cout / 4) + c holds conv channel 4 c + sub (tnr_conv_desc.shuffle)
    float *out;
};

__global__ void __launch_bounds__(256) d4_pack_kernel(const D4PackK a) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int unit = g >> 6, r = (g >> 1) & 31, h = g & 1;
    if (unit >= a.units) return;
    const int per_cb = a.nck * 18;
    const int cb = unit / per_cb, rem = unit - cb * per_cb;
    const int ck = rem / 18, tj = rem - ck * 18, tap = tj >> 1, j = tj & 1;
    int co = cb * 64 + j * 32 + r;
    if (a.shuffle == 2) {
        const int nfc = a.KoutP >> 2;
        co = (co % nfc) * 4 + co / nfc;
    }
    const float *src = a.wp + ((size_t)tap * a.KoutP + co) * a.KinP + 16 * ck + 8 * h;
    const f32x4 q0 = *reinterpret_cast<const f32x4 *>(src), q1 = *reinterpret_cast<const f32x4 *>(src + 4);
    tnr_bf16x8 pl[3];
    tnr_split_bf16x3(q0, q1, pl);
    float *dst = a.out + (size_t)unit * SW_UNIT_FLOATS + (h * 32 + r) * 4;
#pragma unroll
    for (int k = 0; k < 3; ++k) *reinterpret_cast<tnr_bf16x8 *>(dst + k * 256) = pl[k];
}

template <bool AMP = false, bool PS = false>
__global__ void __launch_bounds__(256, 2) conv3x3_d4_kernel(const D4K c) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *s_a = smem;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, half = lane >> 5;
    const ConvK &a = c.a;
    const __amdgpu_buffer_rsrc_t x_rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x), 0, (int)((unsigned)a.N * a.H * a.W * a.x_ct * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(c.wq), 0, c.wq_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t y_rs =
        __builtin_amdgcn_make_buffer_rsrc(a.y, 0, (int)((unsigned)a.N * a.Ho * a.Wo * a.y_ct * 4u), 0x00020000);
    const int apix0[2] = {(2 * wave) * SW_WT + li, (2 * wave + 1) * SW_WT + li};

    for (int tile = blockIdx.x; tile < c.tiles; tile += gridDim.x) {
        // (cb innermost: the ncb workgroups of a pixel tile run side by side and share its input in L2)
        const int cb = tile % c.ncb;
        int rest = tile / c.ncb;
        const int tx = rest % c.tiles_x;
        rest /= c.tiles_x;
        const int ty = rest % c.tiles_y, n = rest / c.tiles_y;
        const int ty0 = ty * SW_TH, tx0 = tx * SW_TW;
        int in_off[S4_A_IT], a_dst[S4_A_IT];
#pragma unroll
        for (int it = 0; it < S4_A_IT; ++it) {
            const int i = tid + it * 256, row = i >> 2, q = i & 3;
            const int hr = row / SW_WT, hc = row - hr * SW_WT;
            int Y = ty0 + hr - 1, X = tx0 + hc - 1;
            if (a.reflect) {         // nn.ReflectionPad2d(1) in front of the layer: row / column -1 is 1, H / W is H - 2 / W - 2
                Y = Y == -1 ? 1 : (Y == a.H ? a.H - 2 : Y);
                X = X == -1 ? 1 : (X == a.W ? a.W - 2 : X);
            }
            const bool in = (row < SW_A_ROWS) & (Y >= 0) & (Y < a.H) & (X >= 0) & (X < a.W);
            in_off[it] = in ? (((n * a.H + Y) * a.W + X) * a.x_ct + a.x_co + q * 4) : -1;
            a_dst[it] = row * SW_ROW + 4 * ((q >> 1) ^ ((row >> TNR_X3_SWZ) & 1)) + 2 * (q & 1);
        }
        f32x4 rin[S4_A_IT];
        auto a_load = [&](int ch, bool valid) __attribute__((always_inline)) {     // on every path (past-the-end addresses read zeros)
#pragma unroll
            for (int it = 0; it < S4_A_IT; ++it) {
                const unsigned bo = (valid && in_off[it] >= 0) ? (unsigned)(in_off[it] + ch) * 4u : 0xfffffff0u;
                rin[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, (int)bo, 0, 0));
            }
        };
        tnr_bf16x4 ih, im, il;
        f32x4 ir;
        auto item_step_buf = [&](auto ic, auto kc, int buf) __attribute__((always_inline)) {      // (conv_sweep4_kernel: five steps per item)
            constexpr int it = decltype(ic)::value, k = decltype(kc)::value;
            if constexpr (k == 0) {
                tnr_pk_level(rin[it], ih, ir);           // (the packed-conversion form of the split: conv_sweep4_kernel's stager, bit-identical)
            } else if constexpr (k == 1) {
                const f32x4 r1 = ir;
                tnr_pk_level(r1, im, ir);
            } else {
                if constexpr (k == 2) {
                    const tnr_f32x2 a2 = {ir[0], ir[1]}, b2 = {ir[2], ir[3]};
                    il = __builtin_bit_cast(tnr_bf16x4, tnr_f32x2{__builtin_bit_cast(float, __builtin_convertvector(a2, tnr_bf16x2)),
                                                                __builtin_bit_cast(float, __builtin_convertvector(b2, tnr_bf16x2))});
                }
                float *dst = s_a + buf * SW_A_FLOATS + a_dst[it] + 8 * (k - 2);
                *reinterpret_cast<tnr_f32x2 *>(dst) = __builtin_bit_cast(tnr_f32x2, k == 2 ? ih : (k == 3 ? im : il));
            }
        };
        f32x16 acc[2][SW_NTILE];         // (only N-tiles 0 and 1 are ever touched: the rest is never materialised)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.f;

        a_load(0, true);
        __syncthreads();                 // the previous tile's last fragments are consumed
        tnr_bf16x8 fbr[3][3];
        int bq = cb * c.nck * 18;        // this channel block's part of the stream
        auto b_fetch = [&](auto rc, int sp) __attribute__((always_inline)) {
            constexpr int r = decltype(rc)::value;
            fbr[r][sp] = __builtin_bit_cast(tnr_bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rs, lane * 16, (bq * 3 + sp) * 1024, 0));
            if (sp == 2) ++bq;
        };
        tnr_bf16x8 fbq[9];               // bf16-operand form (TNR_MMA_BF16): nine single-plane fragments, see amp4_chunk
        auto b_fetch1 = [&](auto rc) __attribute__((always_inline)) {
            constexpr int r = decltype(rc)::value;
            fbq[r] = __builtin_bit_cast(tnr_bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rs, lane * 16, bq * 3072, 0));
            ++bq;
        };
        auto a_item1 = [&](auto ic, int buf) __attribute__((always_inline)) {
            constexpr int it = decltype(ic)::value;
            const tnr_bf16x4 h = __builtin_convertvector(rin[it], tnr_bf16x4);
            *reinterpret_cast<tnr_f32x2 *>(s_a + buf * SW_A_FLOATS + a_dst[it]) = __builtin_bit_cast(tnr_f32x2, h);
        };
        if constexpr (AMP) {
            sw_static_for<0, 8>([&](auto rc) __attribute__((always_inline)) { b_fetch1(rc); });
            sw_static_for<0, S4_A_IT>([&](auto ic) __attribute__((always_inline)) { a_item1(ic, 0); });
        } else {
#pragma unroll
            for (int sp = 0; sp < 3; ++sp) b_fetch(std::integral_constant<int, 0>{}, sp);
#pragma unroll
            for (int sp = 0; sp < 3; ++sp) b_fetch(std::integral_constant<int, 1>{}, sp);
            sw_static_for<0, S4_A_IT>([&](auto ic) __attribute__((always_inline)) {
                sw_static_for<0, 5>([&](auto kc) __attribute__((always_inline)) { item_step_buf(ic, kc, 0); });
            });
        }
        bool has_next = false;
        int e = 0;
        auto item_step = [&](auto ic, auto kc) __attribute__((always_inline)) {
            if (has_next) item_step_buf(ic, kc, (e + 1) & 1);
        };
        auto tick = [&](int, unsigned long long) __attribute__((always_inline)) {};
#pragma unroll 1
        for (int ck = 0; ck < c.nck; ++ck) {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // the chunk's input tile is in LDS; the other buffer is consumed
            has_next = ck + 1 < c.nck;
            a_load(16 * (ck + 1), has_next);
            if constexpr (AMP) {
                auto item1 = [&](auto ic) __attribute__((always_inline)) {
                    if (has_next) a_item1(ic, (e + 1) & 1);
                };
                amp4_chunk<0, 2>(acc, s_a + (e & 1) * SW_A_FLOATS, apix0, half, item1, fbq, b_fetch1);
            } else {
                sweep4_chunk<0, 2>(acc, s_a + (e & 1) * SW_A_FLOATS, apix0, half, item_step, tick, fbr, b_fetch);
            }
            ++e;
        }
        f32x16 t[2][2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            t[m][0] = acc[m][0];
            t[m][1] = acc[m][1];
        }
        // (two workgroups per CU: the other one's MFMAs cover this epilogue's load latency -- one unit of look-ahead keeps it in 256 registers)
        if constexpr (PS) {
            // nn.PixelShuffle(2) folded into the store (tnr_conv_desc.shuffle): the stream's 64-cout block cb holds the channels
            // c of ONE sub-pixel (dy, dx) = cb / (blocks per sub-pixel): 256-byte rows of the shuffled tensor, written where they belong
            ConvK ap = a;
            const int nfb = c.ncb >> 2, sub = cb / nfb;
            ap.Cout = a.Cout >> 2;
            ap.Ho = 2 * a.Ho;
            ap.Wo = 2 * a.Wo;
            ap.bias = a.bias != nullptr ? a.bias + sub : nullptr;
            conv_epilogue_dpp<TNR_DGRAD_4x4_S2, SW_TW, 2, 2, false, 1, false, 4>(ap, t, cb - sub * nfb, n, ty0, tx0, sub, wave, li, half, y_rs);
        } else {
            conv_epilogue_dpp<TNR_CONV_3x3, SW_TW, 2, 2, false, 1>(a, t, cb, n, ty0, tx0, 0, wave, li, half, y_rs);
        }
    }
}

// =====================================================================================================================================
// The four-tap convolutions of the discriminators on the same machinery ("s2"; TNR_MMA_BF16X3 / TNR_MMA_BF16, Cout % 64 == 0, Cin % 16 == 0):
//   TNR_CONV_4x4_S2   k4 s2 p1 (discriminators.py:24-34) as 2 x 2 taps over the four parity planes of the input: chunk = (parity plane pp,
//                     16 channels), halo tile 9 x 33 positions of that plane;
//   TNR_DGRAD_4x4_S2  its data-gradient, one output parity class (py, px) per tile: 2 x 2 taps at positions (1 + py - ty, 1 + px - tx)
//                     of the 10 x 34 halo tile of the incoming gradient, stored to pixels (2 y + py, 2 x + px).
// conv_tile_kernel splits and stages a 4 x 64 x 16 weight slab through LDS per workgroup and chunk between two barriers; here the weights
// are a pre-split stream (tnr_conv_wq_pack: units of one tap x one 32-cout N-tile x 16 channels in register order) read straight from L2
// into a four-deep register ring, the input tile is double-buffered and its split + store rides behind the MFMAs: one barrier per chunk.
// Chunk, tap and product order are conv_tile_body's: bit-identical results.
constexpr int S2_TAPS = 4, S2_NU = S2_TAPS * 2, S2_RING = 4;
struct S2K {
    ConvK a;
    const float *wq;                   // forward: [cb][pp][chunk][tap][N-tile] units; gradient: [par][cb][chunk][tap][N-tile]
    int wq_bytes;
    int nck;                           // 16-channel chunks per parity plane (forward) / of the gradient's channels
    int tiles_x, tiles_y, ncb, tiles;
};
struct S2PackK {
    const float *wp;
    int KinP, KoutP, nck, ncb, units, dgrad;
    float *out;
};

__global__ void __launch_bounds__(256) s2_pack_kernel(const S2PackK a) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int unit = g >> 6, r = (g >> 1) & 31, h = g & 1;
    if (unit >= a.units) return;
    const int j = unit & 1, tap = (unit >> 1) & 3;
    int rest = unit >> 3;
    const float *src;
    if (a.dgrad) {       // [par][cb][ck]: packed slab [par][tap][KoutP][KinP]
        const int ck = rest % a.nck;
        rest /= a.nck;
        const int cb = rest % a.ncb, par = rest / a.ncb;
        src = a.wp + (((size_t)par * 4 + tap) * a.KoutP + cb * 64 + j * 32 + r) * a.KinP + 16 * ck + 8 * h;
    } else {             // [cb][pp][ck]: packed slab [tap][KoutP][4 KinP], parity plane pp = columns pp KinP ..
        const int ck = rest % a.nck;
        rest /= a.nck;
        const int pp = rest & 3, cb = rest >> 2;
        src = a.wp + ((size_t)tap * a.KoutP + cb * 64 + j * 32 + r) * (4 * a.KinP) + pp * a.KinP + 16 * ck + 8 * h;
    }
    const f32x4 q0 = *reinterpret_cast<const f32x4 *>(src), q1 = *reinterpret_cast<const f32x4 *>(src + 4);
    tnr_bf16x8 pl[3];
    tnr_split_bf16x3(q0, q1, pl);
    float *dst = a.out + (size_t)unit * SW_UNIT_FLOATS + (h * 32 + r) * 4;
#pragma unroll
    for (int k = 0; k < 3; ++k) *reinterpret_cast<tnr_bf16x8 *>(dst + k * 256) = pl[k];
}

// one input chunk: 4 taps x 2 N-tiles = 8 units of 12 MFMAs; tap t of M-tile m reads its fragment rows at LDS offset aaddr[m][t] (floats:
// row and slot swizzle of the SHIFTED row); everything else as in sweep4_chunk with a four-deep fragment ring
// (8 units = two turns of it)
template <bool AMP, class Item, class BFetch>
__device__ __forceinline__ void tap4_chunk(f32x16 (&acc)[2][2], const float *sa, const int (&aaddr)[2][4], Item &&item_step,
                                           tnr_bf16x8 (&fbr)[S2_RING][3], BFetch &&b_fetch) {
    constexpr int TA[6] = {0, 2, 1, 0, 1, 0}, TB[6] = {2, 0, 1, 1, 0, 0};      // the six kept partial products, smallest first
    tnr_bf16x8 fa[2][2][3];
    auto read_a = [&](auto tc, int m, int sp) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value;
        fa[t & 1][m][sp] = *reinterpret_cast<const tnr_bf16x8 *>(sa + aaddr[m][t] + 8 * sp);
    };
#pragma unroll
    for (int k = 0; k < (AMP ? 2 : 6); ++k) read_a(std::integral_constant<int, 0>{}, AMP ? k : k / 3, AMP ? 0 : k % 3);
    sw_static_for<0, S2_NU>([&](auto uc) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value, t = u >> 1, jj = u & 1;
        constexpr bool NEXT_TAP = jj == 1 && t + 1 < S2_TAPS;
        constexpr int ITEM = u - (S2_NU - 6);           // the chunk's last six units carry the next chunk's (up to) six items
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (AMP) {
            sw_static_for<0, 2>([&](auto mc) __attribute__((always_inline)) {
                constexpr int m = decltype(mc)::value;
                acc[m][jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[t & 1][m][0], fbr[u % S2_RING][0], acc[m][jj], 0, 0, 0);
                if constexpr (m == 0) b_fetch(std::integral_constant<int, (u + 3) % S2_RING>{}, 0);
                if constexpr (NEXT_TAP) read_a(std::integral_constant<int, (t + 1 < S2_TAPS ? t + 1 : t)>{}, m, 0);
                if constexpr (m == 1 && ITEM >= 0) item_step(std::integral_constant<int, (ITEM >= 0 ? ITEM : 0)>{}, std::integral_constant<int, -1>{});
                __builtin_amdgcn_sched_barrier(0);
            });
        } else {
            sw_static_for<0, 12>([&](auto ic) __attribute__((always_inline)) {
                constexpr int i = decltype(ic)::value, p = i / 2, m = i % 2;
                acc[m][jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[t & 1][m][TA[p]], fbr[u % S2_RING][TB[p]], acc[m][jj], 0, 0, 0);
                if constexpr (i < 3) b_fetch(std::integral_constant<int, (u + 3) % S2_RING>{}, i);       // unit g + 3 into the slot unit g - 1 left
                if constexpr (NEXT_TAP && i >= 3 && i < 9) read_a(std::integral_constant<int, (t + 1 < S2_TAPS ? t + 1 : t)>{}, (i - 3) / 3, (i - 3) % 3);
                if constexpr (ITEM >= 0 && i >= 4 && i < 9) item_step(std::integral_constant<int, (ITEM >= 0 ? ITEM : 0)>{}, std::integral_constant<int, (i >= 4 && i < 9 ? i - 4 : 0)>{});
                __builtin_amdgcn_sched_barrier(0);
            });
        }
    });
}

template <int MODE, bool AMP>
__global__ void __launch_bounds__(256, 2) conv_s2_d4_kernel(const S2K c) {
    constexpr bool DG = MODE == TNR_DGRAD_4x4_S2;
    constexpr int HT = DG ? SW_HT : SW_TH + 1, WT = DG ? SW_WT : SW_TW + 1, ROWS = HT * WT;      // halo tile of the gradient / of one parity plane
    constexpr int A_IT = (ROWS * 4 + 255) / 256;                                                 // 6 / 5 staging items per thread and chunk
    static_assert(A_IT <= 6 && A_IT * 256 <= SW_A_ALLOC_ROWS * 4, "staging plan");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *s_a = smem;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, half = lane >> 5;
    const ConvK &a = c.a;
    const __amdgpu_buffer_rsrc_t x_rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x), 0, (int)((unsigned)a.N * a.H * a.W * a.x_ct * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(c.wq), 0, c.wq_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t y_rs =
        __builtin_amdgcn_make_buffer_rsrc(a.y, 0, (int)((unsigned)a.N * a.Ho * a.Wo * a.y_ct * 4u), 0x00020000);
    const int nchunks = DG ? c.nck : 4 * c.nck;

    for (int tile = blockIdx.x; tile < c.tiles; tile += gridDim.x) {
        // (cb -- and the gradient's parity class -- innermost: the workgroups of a pixel tile run side by side and share its input in L2)
        int rest = tile;
        const int cb = rest % c.ncb;
        rest /= c.ncb;
        int par = 0;
        if constexpr (DG) {
            par = rest & 3;
            rest >>= 2;
        }
        const int tx = rest % c.tiles_x;
        rest /= c.tiles_x;
        const int ty = rest % c.tiles_y, n = rest / c.tiles_y;
        const int ty0 = ty * SW_TH, tx0 = tx * SW_TW;
        const int py = par >> 1, px = par & 1;
        // tap t = (t >> 1, t & 1) sits at position (pos_y, pos_x) of the halo tile; fragment rows of this wave's two M-tiles (tile rows
        // 2 w, 2 w + 1): row (2 w + m + pos_y) WT + li + pos_x, slot swizzle of THAT row
        int aaddr[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int pos_y = DG ? 1 + py - (t >> 1) : (t >> 1), pos_x = DG ? 1 + px - (t & 1) : (t & 1);
                const int pp = (2 * wave + m + pos_y) * WT + li + pos_x;
                aaddr[m][t] = pp * SW_ROW + 4 * (half ^ ((pp >> TNR_X3_SWZ) & 1));
            }
        int in_off[A_IT], a_dst[A_IT];
        auto plan = [&](int pp) __attribute__((always_inline)) {        // forward: the parity plane pp of the input; gradient: pp = 0
#pragma unroll
            for (int it = 0; it < A_IT; ++it) {
                const int i = tid + it * 256, row = i >> 2, q = i & 3;
                const int hr = row / WT, hc = row - hr * WT;
                const int Y = DG ? ty0 + hr - 1 : 2 * (ty0 + hr) - 1 + (pp >> 1), X = DG ? tx0 + hc - 1 : 2 * (tx0 + hc) - 1 + (pp & 1);
                const bool in = (row < ROWS) & (Y >= 0) & (Y < a.H) & (X >= 0) & (X < a.W);
                in_off[it] = in ? (((n * a.H + Y) * a.W + X) * a.x_ct + a.x_co + q * 4) : -1;
                a_dst[it] = row * SW_ROW + 4 * ((q >> 1) ^ ((row >> TNR_X3_SWZ) & 1)) + 2 * (q & 1);
            }
        };
        plan(0);
        f32x4 rin[A_IT];
        auto a_load = [&](int ch, bool valid) __attribute__((always_inline)) {     // on every path (past-the-end addresses read zeros)
#pragma unroll
            for (int it = 0; it < A_IT; ++it) {
                const unsigned bo = (valid && in_off[it] >= 0) ? (unsigned)(in_off[it] + ch) * 4u : 0xfffffff0u;
                rin[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, (int)bo, 0, 0));
            }
        };
        tnr_bf16x4 ih, im, il;
        f32x4 ir;
        auto item_step_buf = [&](auto ic, auto kc, int buf) __attribute__((always_inline)) {      // (conv_sweep4_kernel: five steps per item; k = -1: a whole bf16-operand item)
            constexpr int it = decltype(ic)::value, k = decltype(kc)::value;
            if constexpr (it < A_IT) {
                if constexpr (k < 0) {
                    const tnr_bf16x4 hh = __builtin_convertvector(rin[it], tnr_bf16x4);
                    *reinterpret_cast<tnr_f32x2 *>(s_a + buf * SW_A_FLOATS + a_dst[it]) = __builtin_bit_cast(tnr_f32x2, hh);
                } else if constexpr (k == 0) {
                    tnr_pk_level(rin[it], ih, ir);       // (the packed-conversion form of the split, bit-identical)
                } else if constexpr (k == 1) {
                    const f32x4 r1 = ir;
                    tnr_pk_level(r1, im, ir);
                } else {
                    if constexpr (k == 2) {
                        const tnr_f32x2 a2 = {ir[0], ir[1]}, b2 = {ir[2], ir[3]};
                        il = __builtin_bit_cast(tnr_bf16x4, tnr_f32x2{__builtin_bit_cast(float, __builtin_convertvector(a2, tnr_bf16x2)),
                                                                    __builtin_bit_cast(float, __builtin_convertvector(b2, tnr_bf16x2))});
                    }
                    float *dst = s_a + buf * SW_A_FLOATS + a_dst[it] + 8 * (k - 2);
                    *reinterpret_cast<tnr_f32x2 *>(dst) = __builtin_bit_cast(tnr_f32x2, k == 2 ? ih : (k == 3 ? im : il));
                }
            }
        };
        f32x16 acc[2][2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.f;

        a_load(0, true);
        __syncthreads();                 // the previous tile's last fragments are consumed
        tnr_bf16x8 fbr[S2_RING][3];
        int bq = (DG ? (par * c.ncb + cb) * c.nck : cb * 4 * c.nck) * S2_NU;        // this tile's part of the stream
        auto b_fetch = [&](auto rc, int sp) __attribute__((always_inline)) {
            constexpr int r = decltype(rc)::value;
            if constexpr (AMP) {
                fbr[r][0] = __builtin_bit_cast(tnr_bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rs, lane * 16, bq * 3072, 0));
                ++bq;
            } else {
                fbr[r][sp] = __builtin_bit_cast(tnr_bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rs, lane * 16, (bq * 3 + sp) * 1024, 0));
                if (sp == 2) ++bq;
            }
        };
        sw_static_for<0, 3>([&](auto rc) __attribute__((always_inline)) {
#pragma unroll
            for (int sp = 0; sp < (AMP ? 1 : 3); ++sp) b_fetch(rc, sp);
        });
        sw_static_for<0, 6>([&](auto ic) __attribute__((always_inline)) {
            if constexpr (AMP) item_step_buf(ic, std::integral_constant<int, -1>{}, 0);
            else sw_static_for<0, 5>([&](auto kc) __attribute__((always_inline)) { item_step_buf(ic, kc, 0); });
        });
        bool has_next = false;
        int e = 0;
        auto item_step = [&](auto ic, auto kc) __attribute__((always_inline)) {
            if (has_next) item_step_buf(ic, kc, (e + 1) & 1);
        };
#pragma unroll 1
        for (int ck = 0; ck < nchunks; ++ck) {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // the chunk's input tile is in LDS; the other buffer is consumed
            has_next = ck + 1 < nchunks;
            int ch_next = 16 * (ck + 1);
            if constexpr (!DG) {                     // forward: chunk = (parity plane, 16 channels); a new plane has its own addresses
                const int nx = ck + 1, ppn = nx / c.nck;
                ch_next = 16 * (nx - ppn * c.nck);
                if (has_next && ppn != ck / c.nck) plan(ppn);
            }
            a_load(ch_next, has_next);
            tap4_chunk<AMP>(acc, s_a + (e & 1) * SW_A_FLOATS, aaddr, item_step, fbr, b_fetch);
            ++e;
        }
        f32x16 t2[2][2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            t2[m][0] = acc[m][0];
            t2[m][1] = acc[m][1];
        }
        conv_epilogue_dpp<MODE, SW_TW, 2, 2, false, 1>(a, t2, cb, n, ty0, tx0, par, wave, li, half, y_rs);
    }
}

bool s2_ok(const tnr_conv_desc *d) {
    if (d->mode != TNR_CONV_4x4_S2 && d->mode != TNR_DGRAD_4x4_S2) return false;
    const bool dg = d->mode == TNR_DGRAD_4x4_S2;
    const int tw = dg ? d->W : d->Wo, th = dg ? d->H : d->Ho;            // the tile space
    return (d->mma == TNR_MMA_BF16X3 || d->mma == TNR_MMA_BF16) && d->pad_mode == 0 && d->shuffle == 0 && (d->Cout % 64) == 0 && d->KoutP == d->Cout &&
           d->Cin == d->KinP && (d->Cin % 16) == 0 && d->Cin >= 32 && tw >= 32 && th >= 8 &&
           (dg ? (d->Ho == 2 * d->H && d->Wo == 2 * d->W) : (d->H == 2 * d->Ho && d->W == 2 * d->Wo)) &&
           buffers_addressable(*d) &&
           (int64_t)(d->Cout / 64) * (d->Cin / 16) * 4 * S2_NU * SW_UNIT_FLOATS * (int64_t)sizeof(float) < (1LL << 31);
}

bool d4_ok(const tnr_conv_desc *d) {
    if (d->shuffle != 0 && !(d->shuffle == 2 && (d->Cout % 256) == 0 && d->r1.ptr == nullptr && d->r2.ptr == nullptr && d->m.ptr == nullptr &&
                             d->noise_pos == 0 && d->pad_mode == 0 && (d->y.ctot % 4) == 0 &&
                             (int64_t)d->N * d->H * d->W * 4 * d->y.ctot < (1LL << 30)))
        return false;
    return d->mode == TNR_CONV_3x3 && (d->mma == TNR_MMA_BF16X3 || d->mma == TNR_MMA_BF16) && (d->pad_mode == 0 || (d->pad_mode == 1 && d->H >= 2 && d->W >= 2)) &&
           (d->Cout % 64) == 0 && d->KoutP == d->Cout &&
           d->Cin == d->KinP && (d->Cin % 16) == 0 && d->Cin >= 32 && d->Ho == d->H && d->Wo == d->W && d->W >= 32 && d->H >= 8 &&
           buffers_addressable(*d) &&
           (int64_t)(d->Cout / 64) * (d->Cin / 16) * 18 * SW_UNIT_FLOATS * (int64_t)sizeof(float) < (1LL << 31);
}

// Do the stages form a dense block the sweep kernel covers?  (5 stages over ONE input buffer, stage k reading channels [0, nf + 32 k)
// and -- except the last -- writing the next 32 channels of that buffer; 32, 32, 32, 32, 64 output channels.  n = 4: the first four of
// them -- the four-stage plan, bf16x3 only.)
bool sweep_pattern(const tnr_conv_desc *st, int n, const char **why) {
    auto no = [&](const char *w) { if (why) *why = w; return false; };
    if (st == nullptr || (n != SW_NSTAGE && n != SW4_NSTAGE)) return no("not 5 (or 4) stages");
    if (n == SW4_NSTAGE && st[0].mma != TNR_MMA_BF16X3) return no("the four-stage form exists in bf16x3 only");
    const tnr_conv_desc &d0 = st[0];
    if (d0.Cin < 32 || (d0.Cin % 16) != 0) return no("block input channels must be a multiple of 16, >= 32");
    for (int i = 0; i < n; ++i) {
        const tnr_conv_desc &d = st[i];
        if (d.mode != TNR_CONV_3x3 || (d.mma != TNR_MMA_BF16X3 && d.mma != TNR_MMA_BF16) || d.mma != d0.mma || d.pad_mode != 0)
            return no("stage is not a zero-padded 3x3 in bf16x3 (or all stages with bf16 operands)");
        if (d.N != d0.N || d.H != d0.H || d.W != d0.W || d.Ho != d0.H || d.Wo != d0.W) return no("pixel grids differ");
        if (d.x.ptr != d0.x.ptr || d.x.ctot != d0.x.ctot || d.x.coff != d0.x.coff) return no("stages read different buffers");
        if (d.Cin != d0.Cin + 32 * i || d.KinP != d.Cin) return no("input channels do not grow by 32 per stage");
        if (d.Cout != (i < 4 ? 32 : 64) || d.KoutP != d.Cout) return no("output channels are not 32, 32, 32, 32, 64");
        if (i < 4 && (d.y.ptr != d0.x.ptr || d.y.ctot != d0.x.ctot || d.y.coff != d0.x.coff + d.Cin)) return no("stage output is not the next channel group");
        if (!views_aligned(d)) return no("x / y / r1 / r2 / mask views must be 4-channel aligned");
        if (d.noise_pos < 0 || d.noise_pos > 2 || (i < 4 && d.noise_pos != 0)) return no("the noise multiplier belongs to the last stage");
        if (!buffers_addressable(d)) return no("buffer above 4 GiB");
        if (!d.x.ptr || !d.y.ptr || !d.wp) return no("null pointer");
    }
    const tnr_conv_desc &dl = st[n - 1];
    if (n == SW_NSTAGE && dl.y.ptr == d0.x.ptr && dl.y.coff < d0.x.coff + dl.Cin && dl.y.coff + dl.Cout > d0.x.coff) return no("last stage overwrites its own input");
    return true;
}

constexpr size_t SW_LDS_BYTES = (size_t)(2 * SW_A_FLOATS) * sizeof(float);      // the input tile's double buffer

// CU count once the sweep kernels are set up, 0 when they cannot be (tnr_kernel_setup has the reason; tnr_conv_sweep_image_bytes
// answers 0 then: the sweep is unavailable)
int sweep_cus() {
    static int cus = 0;
    tnr_kernel_setup(&cus, "conv_sweep", {{conv_sweep4_kernel<>, SW_LDS_BYTES}, {conv_sweep4_kernel<true>, SW_LDS_BYTES},
                                          {conv_sweep4_kernel<false, SwPlan4>, SW_LDS_BYTES}});
    return cus;
}

// the pack kernel's arguments for a block that passed sweep_pattern; `who` prefixes the messages
int sweep_pack_args(const char *who, const tnr_conv_desc *stages, int n, void *image, int64_t image_bytes, SweepPackK &a) {
    a.nck0 = stages[0].Cin / 16;
    a.ns = n;
    a.units = sw_total_units(a.nck0, n);
    TNR_REQUIRE((int64_t)a.units * SW_UNIT_FLOATS * (int64_t)sizeof(float) <= image_bytes, "%s: image buffer too small", who);
    for (int i = 0; i < SW_NSTAGE; ++i) {
        const tnr_conv_desc &d = stages[i < n ? i : n - 1];          // (four stages: the fifth entry is never read)
        a.wp[i] = d.wp;
        a.KinP[i] = d.KinP;
        a.KoutP[i] = d.KoutP;
    }
    a.out = static_cast<float *>(image);
    return TNR_OK;
}

}  // namespace

#ifdef SW_TIMELINE
extern "C" int tnr_debug_sweep_units(unsigned long long *out16, int reset) {
    if (out16 != nullptr && hipMemcpyFromSymbol(out16, HIP_SYMBOL(sw_tl2), sizeof(sw_tl2)) != hipSuccess) return TNR_ELAUNCH;
    if (reset) {
        unsigned long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(sw_tl2), z, sizeof(z)) != hipSuccess) return TNR_ELAUNCH;
    }
    return TNR_OK;
}
extern "C" int tnr_debug_sweep_timeline(unsigned long long *out16, int reset) {
    if (out16 != nullptr && hipMemcpyFromSymbol(out16, HIP_SYMBOL(sw_tl), sizeof(sw_tl)) != hipSuccess) return TNR_ELAUNCH;
    if (reset) {
        unsigned long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(sw_tl), z, sizeof(z)) != hipSuccess) return TNR_ELAUNCH;
    }
    return TNR_OK;
}
#endif

extern "C" int64_t tnr_conv_sweep_image_bytes(const tnr_conv_desc *stages, int32_t n) {
    if (stages == nullptr || !sweep_pattern(stages, n, nullptr)) return 0;
    const int cus = sweep_cus();
    const int tpi = tnr_cdiv(stages[0].W, SW_TW) * tnr_cdiv(stages[0].H, SW_TH);
    if (cus < 1 || tpi > cus) return 0;          // an image's tiles must be co-resident (one workgroup per CU)
    return (int64_t)sw_total_units(stages[0].Cin / 16, n) * SW_UNIT_FLOATS * (int64_t)sizeof(float);
}

extern "C" int tnr_conv_sweep_pack(const tnr_conv_desc *stages, int32_t n, void *image, int64_t image_bytes, void *stream) {
    const char *why = "";
    TNR_REQUIRE(stages != nullptr && image != nullptr && sweep_pattern(stages, n, &why), "conv_sweep_pack: not a sweepable dense block (%s)", why);
    SweepPackK a;
    if (const int rc = sweep_pack_args("conv_sweep_pack", stages, n, image, image_bytes, a)) return rc;
    hipLaunchKernelGGL(sweep_pack_kernel, dim3((unsigned)tnr_cdiv(a.units * 64, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return tnr_check_launch("conv_sweep_pack");
}

extern "C" int tnr_conv_sweep(const tnr_conv_desc *stages, int32_t n, const void *image, uint32_t *ws, int64_t ws_bytes, uint32_t epoch,
                              void *stream) {
    const char *why = "";
    TNR_REQUIRE(stages != nullptr && image != nullptr && ws != nullptr && sweep_pattern(stages, n, &why),
                "conv_sweep: not a sweepable dense block (%s)", why);
    const tnr_conv_desc &d0 = stages[0];
    TNR_REQUIRE(tnr_conv_chain_workspace_bytes(&d0) <= ws_bytes, "conv_sweep: workspace too small");
    const int cus = sweep_cus();
    if (cus < 1) return TNR_ELAUNCH;
    SweepK c;
    c.nck0 = d0.Cin / 16;
    c.tiles_x = tnr_cdiv(d0.W, SW_TW);
    c.tiles_y = tnr_cdiv(d0.H, SW_TH);
    c.tpi = c.tiles_x * c.tiles_y;
    c.tiles = c.tpi * d0.N;
    TNR_REQUIRE(c.tpi <= cus, "conv_sweep: the %d tiles of an image exceed the %d co-resident workgroups", c.tpi, cus);
    c.progress = ws;
    c.err = tnr_fault_word_or(ws + ws_bytes / 4 - 1);
    c.disp = ws + (ws_bytes / 4 - 1 - 4 - CH_CU_KEYS - CH_SWEEP_WORDS);      // (words of their own, zero-initialised; every launch leaves them at zero)
    c.base = epoch * (uint32_t)(TNR_CHAIN_MAX + 2);
    c.wq = static_cast<const float *>(image);
    c.wq_bytes = sw_total_units(c.nck0, n) * SW_UNIT_FLOATS * (int)sizeof(float);
    for (int i = 0; i < SW_NSTAGE; ++i) {
        const tnr_conv_desc *d = &stages[i < n ? i : n - 1];         // (four stages: the fifth entry is never read)
        ConvK &k = c.st[i] = conv_k_from_desc(*d);
        k.tiles_x = c.tiles_x; k.tiles_y = c.tiles_y; k.ncb = d->KoutP / 32;
    }
    // whole images per round of the grid, one tile per workgroup and round
    const int per_round = (cus / c.tpi) * c.tpi;
    const int grid = c.tiles < per_round ? c.tiles : per_round;
    if (n == SW4_NSTAGE) hipLaunchKernelGGL((conv_sweep4_kernel<false, SwPlan4>), dim3((unsigned)grid), dim3(256), SW_LDS_BYTES, (hipStream_t)stream, c);
    else if (stages[0].mma == TNR_MMA_BF16) hipLaunchKernelGGL(conv_sweep4_kernel<true>, dim3((unsigned)grid), dim3(256), SW_LDS_BYTES, (hipStream_t)stream, c);
    else hipLaunchKernelGGL(conv_sweep4_kernel<>, dim3((unsigned)grid), dim3(256), SW_LDS_BYTES, (hipStream_t)stream, c);
    return tnr_check_launch("conv_sweep");
}

extern "C" int64_t tnr_conv_wq_bytes(const tnr_conv_desc *d) {
    if (d != nullptr && s2_ok(d)) return (int64_t)(d->Cout / 64) * (d->Cin / 16) * 4 * S2_NU * SW_UNIT_FLOATS * (int64_t)sizeof(float);
    if (d == nullptr || !d4_ok(d)) return 0;
    return (int64_t)(d->Cout / 64) * (d->Cin / 16) * 18 * SW_UNIT_FLOATS * (int64_t)sizeof(float);
}

extern "C" int tnr_conv_wq_pack(const tnr_conv_desc *d, void *image, int64_t image_bytes, void *stream) {
    if (d != nullptr && image != nullptr && d->wp != nullptr && s2_ok(d)) {      // the four-tap forms: 4 (parity planes | parity classes) x chunks x 4 taps x 2 N-tiles
        S2PackK a;
        a.wp = d->wp; a.KinP = d->KinP; a.KoutP = d->KoutP; a.nck = d->Cin / 16; a.ncb = d->Cout / 64;
        a.dgrad = d->mode == TNR_DGRAD_4x4_S2;
        a.units = a.ncb * 4 * a.nck * S2_NU;
        TNR_REQUIRE((int64_t)a.units * SW_UNIT_FLOATS * (int64_t)sizeof(float) <= image_bytes, "conv_wq_pack: image buffer too small");
        a.out = static_cast<float *>(image);
        hipLaunchKernelGGL(s2_pack_kernel, dim3((unsigned)tnr_cdiv(a.units * 64, 256)), dim3(256), 0, (hipStream_t)stream, a);
        return tnr_check_launch("conv_wq_pack (four-tap form)");
    }
    TNR_REQUIRE(d != nullptr && image != nullptr && d->wp != nullptr && d4_ok(d), "conv_wq_pack: the launch cannot use a pre-split weight stream");
    D4PackK a;
    a.wp = d->wp; a.KinP = d->KinP; a.KoutP = d->KoutP; a.nck = d->Cin / 16; a.ncb = d->Cout / 64;
    a.units = a.ncb * a.nck * 18;
    a.shuffle = d->shuffle;
    TNR_REQUIRE((int64_t)a.units * SW_UNIT_FLOATS * (int64_t)sizeof(float) <= image_bytes, "conv_wq_pack: image buffer too small");
    a.out = static_cast<float *>(image);
    hipLaunchKernelGGL(d4_pack_kernel, dim3((unsigned)tnr_cdiv(a.units * 64, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return tnr_check_launch("conv_wq_pack");
}

namespace {

constexpr int SW_GRID_CAP = 2;      // persistent grids of the weight-stream kernels: at most this many workgroups per CU

// Does the four-tap kernel take this launch?  Fills its arguments: the launcher's and the plan query's one answer.
bool s2_takes(const tnr_conv_desc *d, S2K &c) {
    if (!s2_ok(d) || d->wq == nullptr || d->wq_bytes < tnr_conv_wq_bytes(d) || d->noise_pos != 0) return false;
    return stream_k_from_desc(c, *d, tnr_conv_wq_bytes(d), SW_TW, SW_TH, d->mode == TNR_DGRAD_4x4_S2 ? 4 : 1);
}

// The same for the direct 3x3 kernel.
bool d4_takes(const tnr_conv_desc *d, D4K &c) {
    if (!d4_ok(d) || d->wq == nullptr || d->wq_bytes < tnr_conv_wq_bytes(d) || d->noise_pos < 0 || d->noise_pos > 2) return false;
    return stream_k_from_desc(c, *d, tnr_conv_wq_bytes(d), SW_TW, SW_TH, 1);
}

}  // namespace

// host only (no device, no launch): 0 and the plan where tnr_launch_conv_s2_d4 / tnr_launch_conv3x3_d4 would launch, 1 where they decline
int tnr_plan_conv_s2_d4(const tnr_conv_desc *d, ConvStreamPlan *p) {
    S2K c;
    if (!s2_takes(d, c)) return 1;
    stream_plan_of(c, SW_TW, SW_TH, 2, 2, SW_GRID_CAP, p);
    return 0;
}
int tnr_plan_conv3x3_d4(const tnr_conv_desc *d, ConvStreamPlan *p) {
    D4K c;
    if (!d4_takes(d, c)) return 1;
    stream_plan_of(c, SW_TW, SW_TH, 2, 2, SW_GRID_CAP, p);
    return 0;
}

// the four-tap forms (4x4 stride 2 forward, its data-gradient) with a pre-split weight stream; 1: not for this kernel
int tnr_launch_conv_s2_d4(const tnr_conv_desc *d, void *stream) {
    S2K c;
    if (!s2_takes(d, c)) return 1;
    static int cus = 0;
    if (const int rc = tnr_kernel_setup(&cus, "conv_s2_d4", {{conv_s2_d4_kernel<TNR_CONV_4x4_S2, false>, SW_LDS_BYTES}, {conv_s2_d4_kernel<TNR_CONV_4x4_S2, true>, SW_LDS_BYTES},
                                                             {conv_s2_d4_kernel<TNR_DGRAD_4x4_S2, false>, SW_LDS_BYTES}, {conv_s2_d4_kernel<TNR_DGRAD_4x4_S2, true>, SW_LDS_BYTES}}))
        return rc;
    const bool dg = d->mode == TNR_DGRAD_4x4_S2;
    const unsigned grid = (unsigned)(c.tiles < SW_GRID_CAP * cus ? c.tiles : SW_GRID_CAP * cus);
    const bool amp = d->mma == TNR_MMA_BF16;
    if (dg) {
        if (amp) hipLaunchKernelGGL((conv_s2_d4_kernel<TNR_DGRAD_4x4_S2, true>), dim3(grid), dim3(256), SW_LDS_BYTES, (hipStream_t)stream, c);
        else hipLaunchKernelGGL((conv_s2_d4_kernel<TNR_DGRAD_4x4_S2, false>), dim3(grid), dim3(256), SW_LDS_BYTES, (hipStream_t)stream, c);
    } else {
        if (amp) hipLaunchKernelGGL((conv_s2_d4_kernel<TNR_CONV_4x4_S2, true>), dim3(grid), dim3(256), SW_LDS_BYTES, (hipStream_t)stream, c);
        else hipLaunchKernelGGL((conv_s2_d4_kernel<TNR_CONV_4x4_S2, false>), dim3(grid), dim3(256), SW_LDS_BYTES, (hipStream_t)stream, c);
    }
    return tnr_check_launch("conv_s2_d4");
}

// called by tnr_conv_forward (conv_tile.hip) for a launch that carries a pre-split weight stream; 1: not for this kernel
int tnr_launch_conv3x3_d4(const tnr_conv_desc *d, void *stream) {
    D4K c;
    if (!d4_takes(d, c)) return 1;
    static int cus = 0;
    if (const int rc = tnr_kernel_setup(&cus, "conv3x3_d4", {{conv3x3_d4_kernel<>, SW_LDS_BYTES}, {conv3x3_d4_kernel<true>, SW_LDS_BYTES},
                                                             {conv3x3_d4_kernel<false, true>, SW_LDS_BYTES}, {conv3x3_d4_kernel<true, true>, SW_LDS_BYTES}}))
        return rc;
    const unsigned grid = (unsigned)(c.tiles < SW_GRID_CAP * cus ? c.tiles : SW_GRID_CAP * cus);
    if (d->shuffle == 2) {
        // the buffer the store addresses is the shuffled one: [N, 2 Ho, 2 Wo, Cout / 4] (same element count)
        if (d->mma == TNR_MMA_BF16) hipLaunchKernelGGL((conv3x3_d4_kernel<true, true>), dim3(grid), dim3(256), SW_LDS_BYTES, (hipStream_t)stream, c);
        else hipLaunchKernelGGL((conv3x3_d4_kernel<false, true>), dim3(grid), dim3(256), SW_LDS_BYTES, (hipStream_t)stream, c);
        return tnr_check_launch("conv3x3_d4 (pixel-shuffle store)");
    }
    if (d->mma == TNR_MMA_BF16) hipLaunchKernelGGL(conv3x3_d4_kernel<true>, dim3(grid), dim3(256), SW_LDS_BYTES, (hipStream_t)stream, c);
    else hipLaunchKernelGGL(conv3x3_d4_kernel<>, dim3(grid), dim3(256), SW_LDS_BYTES, (hipStream_t)stream, c);
    return tnr_check_launch("conv3x3_d4");
}
