// iris_shares_batch.hip — several DistanceEngine queries in one pass over a TILES share database.
//
// DistanceEngine::batch_process (src/lib.rs:42-52) for G queries at once: out[q][t][k] =
// sum_i rot_k(query_q)[i] e_t[i] mod 2^16, with the i8 byte-plane arithmetic of
// iris_engines_mfma.hip (S1 = q'_lo e'_lo, S2 = q'_lo e'_hi + q'_hi e'_lo, the row-31 byte sums and
// the qsum bias terms).  A single-query pass is bound by the 25 600 B it reads per share while the
// matrix cores idle: 3 x 400 v_mfma_i32_32x32x32_i8 per 32-share tile and query are ~4.9 ms of
// MFMA time per 10M shares next to ~37 ms of HBM time.  Here a wave loads a tile's lo / hi
// B-fragments once per K-chunk and issues the three MFMAs for each of G queries, so G queries cost
// one read of the database.
//
// The query side: every wave needs G x 2 KB of A-fragments per chunk, G/T times the HBM stream if
// each wave read them from L2 itself.  The workgroup's four waves (different tiles, the same
// queries) share them instead: per step of 2 chunks the 256 threads fetch the G queries' 4 KB
// each from L2 once, one uint4 per thread and query, and pass them through a two-slot LDS ring;
// each wave then reads its A-fragments with ds_read_b128 (2 per 3 T MFMAs).
#include <hip/hip_runtime.h>

#include "iris_engines_device.hpp"

namespace iris {

namespace {

constexpr int kStepChunks = 2;                                  // K-chunks per pipeline step
constexpr int kSteps = kShareChunks / kStepChunks;              // 200
constexpr int kStepUint4 = kStepChunks * 2 * 64;                // one query's fragments of a step (4 KB)

// The G queries of one launch: fragments (kShareFragUint4 uint4, then the 32 int2 row sums) and
// the query's output slab ([n][31] u16).  Slots valid .. G-1 repeat slot 0's fragments and are
// never stored.
template <int G>
struct BatchQueries {
    const uint4 *frag[G];
    uint16_t *out[G];
    int valid;
};

}  // namespace

// Large ranges.  Workgroup = 4 waves, wave w owns tiles (4 b + w) T .. + T - 1; three register stages
// of share fragments (a step's T x 2 chunks x lo / hi), loaded two steps ahead.  The query
// fragments of step s + 2 are fetched into registers at the start of step s -- before that step's
// share loads, so the wait that precedes their LDS write at the end of step s + 1 (vmcnt counts in
// order) leaves the two youngest share stages in flight -- and read from the ring in step s + 2.
// One barrier per step: ring slot (s + 1) % 2 was last read in step s - 1.
template <int G, int T>
__global__ void __launch_bounds__(256, 2)
    shares_batch_kernel(const uint4 *__restrict__ db, BatchQueries<G> qs, uint64_t tile0, uint64_t ntiles,
                        uint64_t first, uint64_t end) {
    static_assert(kSteps % 6 == 2, "pipeline geometry: the two tail steps");
    __shared__ uint4 ring[2][G][kStepUint4];
    __shared__ __attribute__((aligned(16))) uint16_t sh_out[kWaveSlots][1024];
    const int lane = threadIdx.x & 63;
    const int tid = threadIdx.x;
    // wave-uniform, so the tile addresses are scalar bases plus a per-lane index
    const uint64_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaveSlots + (threadIdx.x >> 6));
    const uint64_t tw = wave * T;  // may lie past the range: such a wave computes the last tile and stores nothing

    v16i s1[G][T], s2[G][T];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                s1[g][t][i] = 0;
                s2[g][t][i] = 0;
            }
    const uint4 *dp[T];  // the tile's first uint4 (scalar)
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const uint64_t rel = (tw + t < ntiles) ? tw + t : ntiles - 1;
        dp[t] = db + (tile0 + rel) * (uint64_t)kShareTileUint4;
    }
    struct Stage {
        uint4 lo[T][kStepChunks], hi[T][kStepChunks];
    };
    typedef uint4 QRegs[G];
    // Addresses are a scalar base plus one 32-bit per-lane byte offset per step; the empty asm keeps the
    // offset from being strength-reduced into a 64-bit per-lane pointer per stream (spilled at 256 VGPRs)
    auto load = [&](Stage &st, int s) {
        s = s < kSteps ? s : kSteps - 1;
        uint32_t off = ((uint32_t)s * kStepUint4 + (uint32_t)lane) * 16u;  // chunk c: lo at 2c KB, hi at (2c + 1) KB
        asm volatile("" : "+v"(off));
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const char *base = (const char *)dp[t] + off;
#pragma unroll
            for (int i = 0; i < kStepChunks; ++i) {
                st.lo[t][i] = nt_load16((const uint4 *)(base + (2 * i) * 1024));
                st.hi[t][i] = nt_load16((const uint4 *)(base + (2 * i + 1) * 1024));
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto qload = [&](QRegs &q, int s) {
        s = s < kSteps ? s : kSteps - 1;
        uint32_t off = ((uint32_t)s * kStepUint4 + (uint32_t)tid) * 16u;
        asm volatile("" : "+v"(off));
#pragma unroll
        for (int g = 0; g < G; ++g) q[g] = load16((const uint4 *)((const char *)qs.frag[g] + off));
        __builtin_amdgcn_sched_barrier(0);
    };
    auto qstore = [&](int slot, const QRegs &q) {
#pragma unroll
        for (int g = 0; g < G; ++g) store16(&ring[slot][g][tid], q[g]);
    };
    // the A-fragments of (chunk, query) pair j + 1 are read from the ring while pair j's 3 T MFMAs
    // run; the scheduling barriers keep the reads from being hoisted further (8 registers each)
    auto compute = [&](const Stage &st, int slot) {
        uint4 qlo[2], qhi[2];
        qlo[0] = load16(&ring[slot][0][lane]);
        qhi[0] = load16(&ring[slot][0][64 + lane]);
#pragma unroll
        for (int j = 0; j < kStepChunks * G; ++j) {
            const int i = j / G, g = j % G;
            if (j + 1 < kStepChunks * G) {
                const int i1 = (j + 1) / G, g1 = (j + 1) % G;
                qlo[(j + 1) % 2] = load16(&ring[slot][g1][(2 * i1) * 64 + lane]);
                qhi[(j + 1) % 2] = load16(&ring[slot][g1][(2 * i1 + 1) * 64 + lane]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < T; ++t) {
                s1[g][t] = mfma_i8(qlo[j % 2], st.lo[t][i], s1[g][t]);
                s2[g][t] = mfma_i8(qlo[j % 2], st.hi[t][i], s2[g][t]);
                s2[g][t] = mfma_i8(qhi[j % 2], st.lo[t][i], s2[g][t]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // named stages (arrays of them indexed by the unrolled step end up in scratch memory)
    Stage st0, st1, st2;
    QRegs q0, q1;
    // step s: `cur` holds its shares, `last` (consumed in step s - 1) takes those of step s + 2;
    // qfree (stored at the end of step s - 1) takes the queries of step s + 2, qnext holds step s + 1's
    auto step = [&](const Stage &cur, Stage &last, QRegs &qfree, const QRegs &qnext, int slot, int s) {
        qload(qfree, s + 2);
        load(last, s + 2);
        compute(cur, slot);
        qstore(slot ^ 1, qnext);
        __syncthreads();
    };
    qload(q0, 0);
    qload(q1, 1);
    load(st0, 0);
    load(st1, 1);
    qstore(0, q0);
    __syncthreads();
    // three share stages x two query sets: the pattern repeats every 6 steps (200 = 33 * 6 + 2)
    int s = 0;
#pragma unroll 1
    for (; s + 6 <= kSteps; s += 6) {
        step(st0, st2, q0, q1, 0, s);
        step(st1, st0, q1, q0, 1, s + 1);
        step(st2, st1, q0, q1, 0, s + 2);
        step(st0, st2, q1, q0, 1, s + 3);
        step(st1, st0, q0, q1, 0, s + 4);
        step(st2, st1, q1, q0, 1, s + 5);
    }
    step(st0, st2, q0, q1, 0, s);
    step(st1, st0, q1, q0, 1, s + 1);

    uint16_t *lds = sh_out[threadIdx.x >> 6];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g >= qs.valid) break;  // wave-uniform
        const int2 *qsum = (const int2 *)(qs.frag[g] + kShareFragUint4);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            store_query_tile(qs.out[g], lds, qsum, s1[g][t], s2[g][t], (tile0 + tw + t) * kTile, first, end,
                             tw + t < ntiles, lane);
            __builtin_amdgcn_wave_barrier();  // the LDS rows are read before the next query overwrites them
        }
    }
}

// Small ranges (the participant's 20 000-record chunks, src/main.rs:427-431, are 625 tiles): the form
// of shares_split_kernel with G accumulator pairs.  A workgroup of KS waves owns one tile and wave w
// sums K-slice w, so a 625-tile range still starts 625 KS waves; each wave reads its slice of the G
// queries' fragments from L2 itself (the slices of a workgroup's waves differ, so there is nothing
// to share), the slices' i32 sums meet in LDS and wave 0 writes the tile's rows for every query.
template <int G, int KS>
__global__ void __launch_bounds__(64 * KS, 2)
    shares_batch_split_kernel(const uint4 *__restrict__ db, BatchQueries<G> qs, uint64_t tile0, uint64_t first,
                              uint64_t end) {
    constexpr int kSliceSteps = kSteps / KS;
    static_assert(kSteps % KS == 0, "K-split geometry");
    const int lane = threadIdx.x & 63;
    const int slice = threadIdx.x >> 6;
    const uint64_t tile = tile0 + blockIdx.x;
    const int g0 = slice * kSliceSteps;
    v16i s1[G], s2[G];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            s1[g][i] = 0;
            s2[g][i] = 0;
        }
    const uint4 *dp = db + tile * (uint64_t)kShareTileUint4 + lane;
    struct Stage {
        uint4 lo[kStepChunks], hi[kStepChunks];
    };
    auto load = [&](Stage &st, int s) {
        s = g0 + (s < kSliceSteps ? s : kSliceSteps - 1);
#pragma unroll
        for (int i = 0; i < kStepChunks; ++i) {
            const int c = kStepChunks * s + i;
            st.lo[i] = nt_load16(dp + (2 * c) * 64);
            st.hi[i] = nt_load16(dp + (2 * c + 1) * 64);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto compute = [&](const Stage &st, int s) {
        s = g0 + s;
#pragma unroll
        for (int i = 0; i < kStepChunks; ++i) {
            const int c = kStepChunks * s + i;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const uint4 qlo = load16(&qs.frag[g][(2 * c) * 64 + lane]);
                const uint4 qhi = load16(&qs.frag[g][(2 * c + 1) * 64 + lane]);
                s1[g] = mfma_i8(qlo, st.lo[i], s1[g]);
                s2[g] = mfma_i8(qlo, st.hi[i], s2[g]);
                s2[g] = mfma_i8(qhi, st.lo[i], s2[g]);
            }
        }
    };
    // six share stages in flight (HBM); the query fragments come from L2 as they are used
    constexpr int kSt = 6;
    Stage st[kSt];
#pragma unroll
    for (int u = 0; u < kSt - 1; ++u) load(st[u], u);
    int s = 0;
#pragma unroll 1
    for (; s + kSt <= kSliceSteps; s += kSt) {
#pragma unroll
        for (int u = 0; u < kSt; ++u) {
            load(st[(u + kSt - 1) % kSt], s + u + kSt - 1);
            compute(st[u], s + u);
        }
    }
#pragma unroll
    for (int u = 0; u < kSt - 1; ++u)
        if (s + u < kSliceSteps) compute(st[u], s + u);

    __shared__ SliceSums<KS, G> red;
    __shared__ __attribute__((aligned(16))) uint16_t sh_out[1024];
    if (slice != 0) slice_put<KS, G>(red, slice, lane, s1, s2);
    __syncthreads();
    if (slice != 0) return;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g >= qs.valid) break;  // wave-uniform
        slice_add<KS, G>(red, g, lane, s1[g], s2[g]);
        store_query_tile(qs.out[g], sh_out, (const int2 *)(qs.frag[g] + kShareFragUint4), s1[g], s2[g], tile * kTile,
                         first, end, true, lane);
        __builtin_amdgcn_wave_barrier();  // the LDS rows are read before the next query overwrites them
    }
}

// Queries per pass and tiles per wave of the large form; slices of the small form.
constexpr int kBatchG = 4;
constexpr int kBatchT = 1;
constexpr int kBatchSplitKS = 2;
// Up to kSharesSplitTiles tiles (131 072 shares) a range runs in the K-split form, as a single query's
// does: the large form starts one workgroup per 4 T = 4 tiles, at most two
// rounds of its 2 workgroups per CU below it.  (T = 2 at one wave per SIMD, 256 accumulators in
// AGPRs: the register allocator spilled ~315 VGPRs with 150 unused, so T = 1.)
// IRIS_TILES_PER_WAVE (a test hook) pins the large form on ranges of any size, as it pins the
// single-query and masks kernels' variants: T is 1, so both of its values select the same kernel.

// nq queries (qfrags[q]: a DistanceEngine's fragments) over [r.first, r.first + r.n) of a TILES share
// database; query q's rows go to out + q * r.n * 31.  Large ranges: groups of kBatchG queries per
// pass, two or three left-over queries a pass with unused slots, a single one the single-query
// kernel.  Small ranges: only full groups run the K-split batch form (measured at 20 000 shares:
// 4 queries 0.30 ms against 4 x 0.103 ms of single-query passes, but 2 queries 0.295 against 0.206);
// left-over queries run single-query passes, so no nq is slower than the calls it replaces.
// sig (optional): the completion word of a blocking device-output call, handed to the last launch
// when that is a single-query launch that signals (launches of one stream run in order).
// forms (optional): the passes launched, by kernel form.
int launch_shares_batch(const Hooks &h, void *stream, const void *db, const void *const *qfrags, uint32_t nq,
                        LaunchRange r, uint16_t *out, DoneSignal *sig, SharesBatchForms *forms) {
    if (sig) sig->armed = false;
    if (forms) *forms = SharesBatchForms{};
    if (r.n == 0 || nq == 0) return 0;
    const uint64_t t0 = tile_span(r).tile0, ntiles = tile_span(r).ntiles;
    const uint64_t slab = r.n * (uint64_t)kRot;
    const bool split = ntiles <= kSharesSplitTiles && !h.tiles_per_wave;  // the hook pins the large form for tests
    for (uint32_t q0 = 0; q0 < nq;) {
        const uint32_t m = nq - q0 < (uint32_t)kBatchG ? nq - q0 : (uint32_t)kBatchG;
        if (m == 1 || (split && m < (uint32_t)kBatchG)) {
            const bool last = q0 + 1 == nq;
            if (launch_shares_mfma(h, stream, db, qfrags[q0], r, out + q0 * slab, last ? sig : nullptr) != 0) return -1;
            if (forms) forms->single += 1;
            q0 += 1;
            continue;
        }
        BatchQueries<kBatchG> qs;
        for (uint32_t g = 0; g < (uint32_t)kBatchG; ++g) {
            qs.frag[g] = (const uint4 *)qfrags[g < m ? q0 + g : q0];
            qs.out[g] = out + (g < m ? q0 + g : q0) * slab;
        }
        qs.valid = (int)m;
        if (split) {
            hipLaunchKernelGGL((shares_batch_split_kernel<kBatchG, kBatchSplitKS>), dim3((uint32_t)ntiles),
                               dim3(64 * kBatchSplitKS), 0, (hipStream_t)stream, (const uint4 *)db, qs, t0, r.first,
                               r.first + r.n);
        } else {
            const uint64_t per_block = (uint64_t)kWaveSlots * kBatchT;
            hipLaunchKernelGGL((shares_batch_kernel<kBatchG, kBatchT>),
                               dim3((uint32_t)((ntiles + per_block - 1) / per_block)), dim3(256), 0, (hipStream_t)stream,
                               (const uint4 *)db, qs, t0, ntiles, r.first, r.first + r.n);
        }
        if (check_launch() != 0) return -1;
        if (forms) {
            (split ? forms->split : forms->large) += 1;
            (split ? forms->split_queries : forms->large_queries) += m;
        }
        q0 += m;
    }
    return 0;
}

}  // namespace iris
