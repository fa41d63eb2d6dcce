// iris_masks_batch.hip — several MasksEngine queries in one pass over a TILES masks database.
//
// MasksEngine::batch_process (src/lib.rs:69-79) for G queries at once: out[q][t][k] =
// popcount(rot_k(qm_q) & m_t), with the fp4 arithmetic of masks_mfma_kernel (iris_engines_mfma.hip):
// one v_mfma_scale_f32_32x32x64_f8f6f4 per 64-bit chunk, 32 rotation rows x 32 masks, 200 chunks,
// every intermediate an exact integer <= 12 800 in f32.  A single-query pass is bound by the 1600 B
// it reads per record while the matrix cores idle; here a wave expands each 16-B load of a mask
// tile into the four B operands once and issues them against the A operands of G queries, so G
// queries cost one read of the database.  The resolve form decodes, per query, the participants'
// summed share rows of that query's slab against the denominators still in the accumulators
// (the resolver step of src/main.rs:510-519 + 597-621) and keeps one running best per query.
// The match form decodes the same way and, in place of the running best, appends every record
// below the threshold to the query's own MatchSink (iris_resolver_batch_matches_masks).
// The top-k form keeps, in place of the running best, each query's k best records of the wave as
// a wave-resident sorted list (topk_insert, iris_device.hpp) and stores one list per wave and
// query for launch_topk_merge to fold (iris_resolver_batch_topk_masks).
// The report form feeds two or three of those sinks -- the match list, the wave's top-k list, the
// LDS histogram -- from the one best rotation per (query, record) (iris_resolver_batch_report_masks).
//
// The query side: each wave reads the G queries' compact words (16 B per lane, step and query)
// from L2, as masks_mfma_kernel<MASKS_RESOLVE> does for its one query; a query's fragments are
// 51 KB, so G of them do not fit in LDS beside the output staging.  (Sharing each step's words among
// the workgroup's waves through a two-slot LDS ring, one barrier per step, measured slower: 6.31
// against 6.06 ms for 4 queries over 10M masks, profiles/r08_masks_batch.txt.)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "iris_engines_device.hpp"

namespace iris {

namespace {

constexpr uint32_t kSteps = kMaskChunks / 4;  // 50 steps of 4 chunks

enum { BATCH_OUT = 0, BATCH_RESOLVE = 1, BATCH_MATCH = 2, BATCH_TOPK = 3, BATCH_HIST = 4, BATCH_REPORT = 5 };

__device__ __forceinline__ uint32_t dword_of(const uint4 &v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// The G query slots of one launch.  Slots valid .. G-1 repeat slot 0's fragments and are never
// stored or resolved.
template <int G>
struct MaskBatchArgs {
    const uint4 *frag[G];
    int valid;
    // BATCH_OUT: the slot's [n][31] u16 slab
    uint16_t *out[G];
    // BATCH_RESOLVE, BATCH_MATCH, BATCH_TOPK: the participants' query-major arrays; slot g's slab starts slab[g]
    // elements in
    const uint16_t *shares[8];
    uint64_t slab[G];
    double *dist[G];        // BATCH_RESOLVE: the slot's n doubles, or all NULL
    Partial *partials[G];   // BATCH_RESOLVE: the slot's run of gridDim.x partials
    uint32_t parts;
    uint32_t aligned;       // bit g: slab g of every part starts 16-B aligned
    MatchSink match[G];     // BATCH_MATCH: the slot's own records, room, counter and threshold
                            // BATCH_TOPK: topk_sink -- buf = the slot's lists [gridDim.x * 4][k], cap = k
                            // BATCH_HIST: hist_sink -- the slot's counter copies; every slot the same nbins and copies
                            // BATCH_REPORT: report_sink -- the slot's ReportSinks of the device array; every slot
                            // the same parts, k, nbins and copies
};

}  // namespace

// Persistent, the shape of masks_mfma_kernel: each wave walks the tile groups wave, wave + nwaves, ...
// of T tiles as one flat stream of (group, step) K-steps through register stages, so the next
// group's loads are in flight while the current group's G x T tiles are written out.
// BATCH_MATCH: BATCH_RESOLVE's staging and decode; each tile's records below a.match[g].threshold
// are appended to a.match[g] (one atomic per wave, tile and slot with a hit) -- no running best,
// no partials, nothing after the loop.
// BATCH_TOPK: BATCH_RESOLVE's staging and decode; best[g] is this lane's entry of slot g's list of
// the wave (topk_insert; half 0 votes, as in masks_mfma_kernel<MASKS_TOPK>), resident while the wave
// walks its tile groups.  After the loop every wave of the grid -- one with no tile group stores
// an empty list, launch_topk_merge reads them all -- stores each valid slot's list at
// a.match[g].buf[wave]: no shuffle reduction, no sh_best, no partials.
// BATCH_HIST: BATCH_RESOLVE's staging and decode; each record of a valid slot is counted in the slot's
// LDS histogram (hist_lds<G>(), slot g at g * (kHistMaxBins + 1): 16.4 KB beside sh_out's 8 KB for
// four slots), resident while the wave walks its tile groups.  The histograms are zeroed ahead of a
// barrier before the walk and, behind a barrier after it, each valid slot's non-zero words are added
// once to the workgroup's copy of a.match[g]'s counters (hist_flush).
// BATCH_REPORT: BATCH_MATCH, BATCH_TOPK and BATCH_HIST from one walk.  a.match[g] points at slot g's
// ReportSinks; they are scalar-loaded (report_sinks_load: a wave-uniform address) where they are used
// -- per valid slot at the end of a tile group, and once more after the walk -- never held across the
// K loop.  Whether a part is present is read from slot 0's struct (every slot selects the same parts),
// so the test is the same for every wave of the grid: with a histogram part every wave of the
// workgroup reaches the zeroing barrier and the flush barrier, both outside `if (total)`; with a
// top-k part every wave of the grid stores each valid slot's list at BATCH_TOPK's unit numbers.
template <int G, int T, int MODE>
__global__ void __launch_bounds__(256, 2)
    masks_batch_kernel(const uint4 *__restrict__ db, MaskBatchArgs<G> a, uint64_t tile0, uint64_t ntiles, uint64_t first,
                       uint64_t end) {
    __shared__ __attribute__((aligned(16))) uint16_t sh_out[kWaveSlots][1024];
    const int lane = threadIdx.x & 63;
    const uint64_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaveSlots + (threadIdx.x >> 6));
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaveSlots;
    const uint64_t ngroups = (ntiles + T - 1) / T;
    // BATCH_RESOLVE and BATCH_TOPK: every wave of the grid writes after the walk; BATCH_HIST: every
    // wave of the workgroup reaches the two histogram barriers; BATCH_REPORT: both
    if (MODE != BATCH_RESOLVE && MODE != BATCH_TOPK && MODE != BATCH_HIST && MODE != BATCH_REPORT && wave >= ngroups) return;
    const uint32_t total = wave < ngroups ? (uint32_t)((ngroups - wave + nwaves - 1) / nwaves) * kSteps : 0;
    uint16_t *lds = sh_out[threadIdx.x >> 6];
    Partial best[G];
#pragma unroll
    for (int g = 0; g < G; ++g) best[g] = partial_none();

    uint32_t *hist = nullptr;
    if constexpr (MODE == BATCH_HIST) {
        hist = hist_lds<G>();
#pragma unroll
        for (int g = 0; g < G; ++g) hist_zero(hist + g * (kHistMaxBins + 1), hist_sink_bins(a.match[0]));
        __syncthreads();
    }
    if constexpr (MODE == BATCH_REPORT) {
        hist = hist_lds<G>();
        const ReportSinks up = report_sinks_load(a.match[0]);
        if (report_has_hist(up)) {  // workgroup-uniform
#pragma unroll
            for (int g = 0; g < G; ++g) hist_zero(hist + g * (kHistMaxBins + 1), hist_sink_bins(up.hist));
            __syncthreads();
        }
    }
    // BATCH_REPORT alone: a slot's sinks, loaded at the end of each tile group for the slot's tiles; every
    // other mode neither writes nor reads it (resolve_tile's report path is the one reader)
    ReportSinks group{};

    v16f acc[G][T];
    auto zero = [&] {
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[g][t][i] = 0.f;
    };
    if (total) {
        zero();
        // the mask tiles (HBM) are loaded two steps ahead through three register stages, the query
        // words (L2) one step ahead through two: 16 G registers fewer than three stages of both
        struct StageD {
            uint4 d[T];
        };
        struct StageW {
            uint4 w[G];
        };
        auto load_d = [&](StageD &st, uint32_t s) {
            s = s < total ? s : total - 1;
            const uint32_t j = s / kSteps, c = s - j * kSteps;
            const uint64_t tw = (wave + (uint64_t)j * nwaves) * T;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const uint64_t rel = (tw + t < ntiles) ? tw + t : ntiles - 1;
                st.d[t] = nt_load16(db + (tile0 + rel) * (uint64_t)kMaskTileUint4 + c * 64 + lane);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        auto load_w = [&](StageW &st, uint32_t s) {
            s = s < total ? s : total - 1;
            const uint32_t c = s % kSteps;
#pragma unroll
            for (int g = 0; g < G; ++g) st.w[g] = load16(a.frag[g] + c * 64 + lane);
            __builtin_amdgcn_sched_barrier(0);
        };
        auto compute = [&](const StageD &sd, const StageW &st, uint32_t s) {
            if (s >= total) return;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                // the tile dwords' B operands, expanded once for the G queries
                v8i b[T];
#pragma unroll
                for (int t = 0; t < T; ++t) b[t] = mask_b(dword_of(sd.d[t], c));
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const v8i av = mask_a(dword_of(st.w[g], c));
#pragma unroll
                    for (int t = 0; t < T; ++t) acc[g][t] = mfma_fp4(av, b[t], acc[g][t]);
                }
            }
            const uint32_t j = s / kSteps;
            if (s - j * kSteps == kSteps - 1) {  // group j done: write its rows / resolve it, per slot
                const uint64_t tw = (wave + (uint64_t)j * nwaves) * T;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (g < a.valid) {  // wave-uniform
                        if constexpr (MODE == BATCH_REPORT) group = report_sinks_load(a.match[g]);
#pragma unroll
                        for (int t = 0; t < T; ++t) {
                            if constexpr (MODE == BATCH_OUT) {
                                store_tile_rows(a.out[g], lds, (tile0 + tw + t) * kTile, first, end, tw + t < ntiles, lane,
                                                [&](int r) { return (uint16_t)(uint32_t)acc[g][t][r]; });
                                __builtin_amdgcn_wave_barrier();  // the LDS rows are read before the next tile's
                            } else {
                                // slot g's slab of every share array; alignment is the slab's own
                                const ResolveView view{a.shares, a.parts, a.slab[g], ((a.aligned >> g) & 1u) != 0, a.match[g],
                                                       MODE == BATCH_RESOLVE ? a.dist[g] : nullptr, best[g],
                                                       MODE == BATCH_HIST || MODE == BATCH_REPORT ? hist + g * (kHistMaxBins + 1) : nullptr,
                                                       MODE == BATCH_REPORT ? &group : nullptr};
                                resolve_tile<MODE == BATCH_MATCH, MODE == BATCH_TOPK, MODE == BATCH_HIST, MODE == BATCH_REPORT>(
                                    view, lds, lane, (tile0 + tw + t) * kTile, tw + t < ntiles, acc[g][t], first, end);
                            }
                        }
                    }
                }
                zero();
            }
        };
        // step s: the query words of step s + 1 are requested first, then the tiles of step s + 2, so
        // the wait for step s + 1's operands (vmcnt counts in order) leaves the tile loads in flight
        StageD d0, d1, d2;
        StageW w0, w1;
        auto step = [&](const StageD &dcur, StageD &dfree, const StageW &wcur, StageW &wfree, uint32_t s) {
            load_w(wfree, s + 1);
            load_d(dfree, s + 2);
            compute(dcur, wcur, s);
        };
        load_d(d0, 0);
        load_d(d1, 1);
        load_w(w0, 0);
#pragma unroll 1
        for (uint32_t s = 0; s < total; s += 6) {  // three tile stages x two query stages
            step(d0, d2, w0, w1, s);
            step(d1, d0, w1, w0, s + 1);
            step(d2, d1, w0, w1, s + 2);
            step(d0, d2, w1, w0, s + 3);
            step(d1, d0, w0, w1, s + 4);
            step(d2, d1, w1, w0, s + 5);
        }
    }
    if constexpr (MODE == BATCH_TOPK) {
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (g < a.valid) topk_store(a.match[g], wave, lane, best[g]);  // every wave of the grid: one list per slot
    }
    if constexpr (MODE == BATCH_HIST) {  // every wave of the workgroup: the counts are in before the flush reads them
        __syncthreads();
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (g < a.valid)
                hist_flush(hist + g * (kHistMaxBins + 1), hist_sink_bins(a.match[g]), hist_sink_copy(a.match[g]));
    }
    if constexpr (MODE == BATCH_REPORT) {  // each part as its own mode above, under the same grid-uniform tests
        const ReportSinks done = report_sinks_load(a.match[0]);
        if (report_has_topk(done)) {  // every wave of the grid: one list per slot
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (g < a.valid) topk_store(report_sinks_load(a.match[g]).topk, wave, lane, best[g]);
        }
        if (report_has_hist(done)) {  // every wave of the workgroup
            __syncthreads();
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (g < a.valid) {
                    const ReportSinks slot = report_sinks_load(a.match[g]);
                    hist_flush(hist + g * (kHistMaxBins + 1), hist_sink_bins(slot.hist), hist_sink_copy(slot.hist));
                }
        }
    }
    if constexpr (MODE == BATCH_RESOLVE) {
        __shared__ Partial sh_best[G][kWaveSlots];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            best[g] = wave_argmin(best[g]);
            if (lane == 0) sh_best[g][threadIdx.x >> 6] = best[g];
        }
        __syncthreads();
        if (threadIdx.x < G && (int)threadIdx.x < a.valid) {
            const int g = threadIdx.x;
            Partial b;
            fold_waves(b, sh_best[g], kWaveSlots);
            Partial *dst = a.partials[0];
#pragma unroll
            for (int i = 1; i < G; ++i)
                if (g == i) dst = a.partials[i];
            dst[blockIdx.x] = b;
        }
    }
}

namespace {

// Tiles per wave, G x T = 8 (128 accumulators): 2 for four queries, 4 for two, or 1 where that
// would leave fewer waves than the chip holds at two workgroups per CU (tiles_per_wave,
// iris_device.hpp); IRIS_TILES_PER_WAVE pins either for tests.  Measured on
// one box, interleaved, 10M masks: two queries 3.60 ms at 4 tiles against 3.83 at 2 (resolve
// form 4.17 against 4.42); the resolve form of four queries 7.40 ms at 2 tiles against 8.65 at 1.
// VGPRs (no scratch in any instantiation): rows form 98 / 242 for two queries at 1 / 4 tiles,
// 164 / 234 for four at 1 / 2; resolve form 122 / 256 and 192 / 256; match form 110 / 245 and
// 169 / 233 (it keeps no running best: profiles/r10_masks_batch_matches.txt); top-k form 120 / 254
// and 188 / 252 (the lists live in the running bests' registers, topk_insert's broadcasts in SGPRs:
// profiles/r14_masks_batch_topk.txt), so this mode takes the resolve form's choice unchanged;
// report form 122 / 256 and 193 / 256, BATCH_HIST's LDS (the sinks are scalar-loaded per tile group,
// not held across the walk: profiles/r28_resources.txt), the top-k form's choice too.
template <int G>
constexpr int batch_big_tiles() { return G == 2 ? 4 : 2; }

struct BatchTiles {
    uint64_t tile0, ntiles;
    int tpw;
    uint32_t grid;
};

// grid = min(ceil(ceil(ntiles / tpw) / 4), 2 workgroups per CU): past 2 x CUs x 4 x tpw tiles a wave
// walks more than one tile group
BatchTiles batch_tiles(const Hooks &h, LaunchRange r, int big) {
    BatchTiles t;
    t.tile0 = tile_span(r).tile0;
    t.ntiles = tile_span(r).ntiles;
    t.tpw = tiles_per_wave(h, t.ntiles, big);
    const uint64_t waves = (t.ntiles + t.tpw - 1) / t.tpw;
    t.grid = (uint32_t)std::min<uint64_t>((waves + kWaveSlots - 1) / kWaveSlots, resident_blocks(2));
    return t;
}

template <int G, int MODE>
int launch_group(void *stream, const void *db, const MaskBatchArgs<G> &a, const BatchTiles &t, LaunchRange r) {
    auto kern = t.tpw == 1 ? masks_batch_kernel<G, 1, MODE> : masks_batch_kernel<G, batch_big_tiles<G>(), MODE>;
    hipLaunchKernelGGL(kern, dim3(t.grid), dim3(256), 0, (hipStream_t)stream, (const uint4 *)db, a, t.tile0, t.ntiles,
                       r.first, r.first + r.n);
    return check_launch();
}

template <int G>  // mode = BATCH_*: BATCH_OUT writes `out`, the others read rs, BATCH_MATCH, BATCH_TOPK, BATCH_HIST and BATCH_REPORT fill sinks
int launch_slots(int mode, const Hooks &h, void *stream, const void *db, const void *const *qfrags, uint32_t m,
                 LaunchRange r, uint16_t *out, const MasksBatchResolve *rs, uint32_t *np, const MatchSink *sinks) {
    const BatchTiles t = batch_tiles(h, r, batch_big_tiles<G>());
    if (np) *np = t.grid;
    const uint64_t slab = r.n * (uint64_t)kRot;
    MaskBatchArgs<G> a{};
    a.valid = (int)m;
    for (uint32_t g = 0; g < (uint32_t)G; ++g) {
        const uint32_t s = g < m ? g : 0;
        a.frag[g] = (const uint4 *)qfrags[s];
        if (mode == BATCH_OUT) {
            a.out[g] = out + s * slab;
            continue;
        }
        a.slab[g] = (rs->q0 + s) * slab;
        if (mode != BATCH_RESOLVE) {
            a.match[g] = sinks[s];
        } else {
            a.dist[g] = rs->dist_out ? rs->dist_out + (rs->q0 + s) * r.n : nullptr;
            a.partials[g] = rs->partials + (uint64_t)s * rs->stride;
        }
        bool al = true;
        for (uint32_t p = 0; p < rs->parts; ++p) al &= ((uintptr_t)(rs->shares[p] + a.slab[g]) & 15) == 0;
        a.aligned |= (al ? 1u : 0u) << g;
    }
    if (mode == BATCH_OUT) return launch_group<G, BATCH_OUT>(stream, db, a, t, r);
    a.parts = rs->parts;
    for (uint32_t p = 0; p < rs->parts; ++p) a.shares[p] = rs->shares[p];
    if (mode == BATCH_TOPK) return launch_group<G, BATCH_TOPK>(stream, db, a, t, r);
    if (mode == BATCH_HIST) return launch_group<G, BATCH_HIST>(stream, db, a, t, r);
    if (mode == BATCH_REPORT) return launch_group<G, BATCH_REPORT>(stream, db, a, t, r);
    if (mode == BATCH_MATCH) return launch_group<G, BATCH_MATCH>(stream, db, a, t, r);
    return launch_group<G, BATCH_RESOLVE>(stream, db, a, t, r);
}

int launch_mode(int mode, const Hooks &h, void *stream, const void *db, const void *const *qfrags, uint32_t m, LaunchRange r,
                uint16_t *out, const MasksBatchResolve *rs, uint32_t *np, const MatchSink *sinks) {
    return (m == 2 ? launch_slots<2> : launch_slots<kMasksBatchG>)(mode, h, stream, db, qfrags, m, r, out, rs, np, sinks);  // m == 3: a slot unused
}

}  // namespace

// Ranges the batch kernel runs: those past the single-query kernels' K-split threshold (kMasksSplitTiles;
// the resolver's 20 000-record chunk is 625).  Below it a batch runs one single-query launch per
// query through the K-split and fused resolve kernels: no K-split batch form is shipped.
bool masks_batch_runs(const Hooks &h, LaunchRange r) {
    if (r.n == 0) return false;
    return tile_span(r).ntiles > kMasksSplitTiles || h.tiles_per_wave != 0;  // the hook pins the batch kernel for tests
}

// the most partials per query a pass over r writes (the grid at one tile per wave)
uint32_t masks_batch_partials(const Hooks &h, LaunchRange r) { return r.n ? batch_tiles(h, r, 1).grid : 0; }

// the lists each query of a top-k pass, or of a report pass with a top-k part, over r writes: one per
// wave of the grid (launch_slots')
uint64_t masks_batch_topk_units(const Hooks &h, LaunchRange r, uint32_t m) {
    if (r.n == 0) return 0;
    return (uint64_t)batch_tiles(h, r, m == 2 ? batch_big_tiles<2>() : batch_big_tiles<kMasksBatchG>()).grid * kWaveSlots;
}

// m = 2 .. kMasksBatchG queries (qfrags[s]: a MasksEngine's compact fragments) over [r.first, r.first +
// r.n) of a TILES masks database in one pass: the same slots, tiles per wave and grid in every mode
// (MasksBatchOut has the operands of each).
int launch_masks_batch(Pass p, const Hooks &h, void *stream, const void *db, const void *const *qfrags, uint32_t m,
                       LaunchRange r, const MasksBatchOut &o) {
    if (o.np) *o.np = 0;
    if (r.n == 0) return 0;
    if (m < 2 || m > (uint32_t)kMasksBatchG) return -1;
    const MasksBatchResolve *rs = o.resolve ? &o.rs : nullptr;
    if (rs && (rs->parts == 0 || rs->parts > 8)) return -1;
    MatchSink ts[kMasksBatchG];
    switch (p) {
    case Pass::Search:
        if (o.sinks || o.lists || o.hists || (!rs && !o.rows)) return -1;
        return launch_mode(rs ? BATCH_RESOLVE : BATCH_OUT, h, stream, db, qfrags, m, r, o.rows, rs, o.np, nullptr);
    case Pass::Match:
        if (!rs || !o.sinks || o.hists || o.reports) return -1;
        return launch_mode(BATCH_MATCH, h, stream, db, qfrags, m, r, nullptr, rs, nullptr, o.sinks);
    case Pass::Topk:
        if (!rs || !o.lists || o.hists || o.k == 0 || o.k > kTopkMax) return -1;
        for (uint32_t s = 0; s < m; ++s) ts[s] = topk_sink(o.lists + s * o.stride, o.k);
        return launch_mode(BATCH_TOPK, h, stream, db, qfrags, m, r, nullptr, rs, nullptr, ts);
    case Pass::Hist:  // one nbins and one number of copies for all slots: the kernel zeroes by slot 0's
        if (!rs || !o.hists || o.sinks || o.lists || o.rows) return -1;
        for (uint32_t s = 0; s < m; ++s)
            if (!hist_sink_ok(o.hists[s]) || o.hists[s].cap != o.hists[0].cap) return -1;
        return launch_mode(BATCH_HIST, h, stream, db, qfrags, m, r, nullptr, rs, nullptr, o.hists);
    case Pass::Report:  // two or three parts, and the same parts, k, nbins and copies for all slots: the kernel tests slot 0's
        if (!rs || !o.reports || !o.staged || o.sinks || o.lists || o.hists || o.rows) return -1;
        for (uint32_t s = 0; s < m; ++s) {
            const ReportSinks &x = o.staged[s], &x0 = o.staged[0];
            const bool has_match = x.match.count, has_topk = x.topk.cap != 0, has_hist = x.hist.count;
            if (has_match + has_topk + has_hist < 2) return -1;
            if (has_match != (x0.match.count != nullptr) || x.topk.cap != x0.topk.cap) return -1;
            if (has_topk && (x.topk.cap > kTopkMax || !x.topk.buf)) return -1;
            if (has_hist != (x0.hist.count != nullptr) || (has_hist && (!hist_sink_ok(x.hist) || x.hist.cap != x0.hist.cap))) return -1;
            ts[s] = report_sink(o.reports + s);
        }
        return launch_mode(BATCH_REPORT, h, stream, db, qfrags, m, r, nullptr, rs, nullptr, ts);
    default: return -1;
    }
}

}  // namespace iris
