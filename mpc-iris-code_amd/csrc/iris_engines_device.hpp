// iris_engines_device.hpp — the device pieces that the single-query and the batched MasksEngine /
// DistanceEngine kernels share (iris_engines_mfma.hip, iris_masks_batch.hip, iris_shares_batch.hip):
// the masks resolver epilogue, the shares K-loop, its recombining epilogue and the K-split's slice
// sum.  Everything is inlined into the kernel that calls it; the __shared__ arrays stay with the kernels.
#pragma once
#include "iris_device.hpp"

namespace iris {

// ------------------------------------------------------------------ masks: the resolver step of a tile

// One query's operands of the fused resolver: the participants' [n][31] u16 outputs, row i = record
// first + i (src/main.rs:597-607), from element `base` on (a batch slot's slab; 0 for a single query).
struct ResolveView {
    const uint16_t *const *shares;
    uint32_t parts;
    uint64_t base;
    bool aligned;           // every share array is 16-B aligned at `base`
    const MatchSink &sink;  // MATCH: the query's records, room, counter and threshold; TOPK: topk_sink; HIST: hist_sink;
                            // REPORT: report_sink of the device's ReportSinks
    double *dist;           // null, or the query's n distances
    Partial &best;          // the lane's running best; TOPK: this lane's entry of the wave's list
    uint32_t *hist = nullptr;  // HIST: the query's LDS histogram of the workgroup (hist_sink_bins(sink) + 1 words)
    const ReportSinks *report = nullptr;  // REPORT: the three sinks, loaded by the caller ahead of a tile group's tiles
};

// Resolver epilogue of one tile (records t0 .. t0+31 of the database), `den` its denominators in the
// MFMA C layout and lds the wave's 2 KB: the tile's summed shares are staged in LDS, each lane decodes
// its 16 (record, rotation) cells (decode_distance, src/lib.rs:97-107) and half 0 of the wave
// takes the record's best to the running best, or (MATCH) appends it to the sink if it lies below
// the threshold, or (TOPK) inserts it into the wave's list, or (HIST) counts it in v.hist
// (hist_count: no running best, no dist, no append; the caller zeroes and flushes v.hist around
// its walk, behind workgroup barriers).
// REPORT: the staging and the best rotation once, then every sink *v.report holds, each as its own
// mode above runs it.  The caller reads the sinks where they are used (report_sinks_load: wave-uniform
// scalar loads, once per tile group), so they live for this epilogue only, not across the K loop,
// and a part's presence is the same for every wave of the workgroup.
template <bool MATCH, bool TOPK, bool HIST = false, bool REPORT = false>
__device__ __forceinline__ void resolve_tile(const ResolveView &v, uint16_t *lds, int lane, uint64_t t0, bool tv,
                                             const v16f &den, uint64_t first, uint64_t end) {
    const bool full = tv && t0 >= first && t0 + 32 <= end && ((t0 - first) & 7) == 0 && v.aligned;
    const uint64_t e0 = v.base + (t0 - first) * kRot;  // first share element of the tile (when full)
    if (full) {  // wave-uniform: 124 16-B words per share array
        for (int i = lane; i < 32 * kRot / 8; i += 64) {
            // plain loads (nontemporal measured the same, 2.75-2.79 ms per 10M either way)
            u16x8 s = *(const u16x8 *)(v.shares[0] + e0 + 8 * i);
            for (uint32_t p = 1; p < v.parts; ++p) s += *(const u16x8 *)(v.shares[p] + e0 + 8 * i);
            *(u16x8 *)&lds[8 * i] = s;
        }
    } else {
        for (int i = lane; i < 32 * kRot; i += 64) {
            const uint64_t tg = t0 + (uint64_t)(i / kRot);
            uint16_t s = 0;
            if (tv && tg >= first && tg < end) {
                const uint64_t e = v.base + (tg - first) * kRot + (uint64_t)(i % kRot);
                for (uint32_t p = 0; p < v.parts; ++p) s = (uint16_t)(s + v.shares[p][e]);
            }
            lds[i] = s;
        }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes landed
    __builtin_amdgcn_wave_barrier();
    const int h = lane >> 5;
    uint32_t bn, bd;
    int br;
    best_rotation(lane, [&](int r, uint32_t &u, uint32_t &d) {
        const int k = (r & 3) + 8 * (r >> 2) + 4 * h;
        d = (uint32_t)den[r] & 0xFFFFu;  // the MasksEngine output value (u16)
        u = k < kRot ? (uint32_t)((uint16_t)(d - lds[(lane & 31) * kRot + k]) >> 1) : 0;  // src/lib.rs:104
    }, bn, bd, br);
    const uint64_t tg = t0 + (lane & 31);
    const bool valid = tv && tg >= first && tg < end;
    if constexpr (REPORT) {
        const ReportSinks &rs = *v.report;
        if (report_has_hist(rs)) hist_count(v.hist, hist_sink_bins(rs.hist), lane, valid && h == 0, bn, bd);
        if (report_has_match(rs)) {
            const bool hit[1] = {match_hit(rs.match, valid && h == 0, bn, bd)};
            const uint32_t hn[1] = {bn}, hd[1] = {bd};
            const int hr[1] = {br};
            const uint64_t hi[1] = {tg - first};
            append_matches<1>(rs.match, lane, hit, hn, hd, hr, hi);
        }
        if (report_has_topk(rs))
            topk_insert(v.best, (uint32_t)rs.topk.cap, lane, partial_of(bn, valid ? bd : 0, br, tg - first), h == 0);
        __builtin_amdgcn_wave_barrier();  // LDS reads done before the next tile overwrites
        return;
    }
    if constexpr (HIST) {  // half 0 counts: both halves hold the record's best
        hist_count(v.hist, hist_sink_bins(v.sink), lane, valid && h == 0, bn, bd);
        __builtin_amdgcn_wave_barrier();  // LDS reads done before the next tile overwrites
        return;
    }
    if constexpr (MATCH) {
        const bool hit[1] = {match_hit(v.sink, valid && h == 0, bn, bd)};
        const uint32_t hn[1] = {bn}, hd[1] = {bd};
        const int hr[1] = {br};
        const uint64_t hi[1] = {tg - first};
        append_matches<1>(v.sink, lane, hit, hn, hd, hr, hi);
        __builtin_amdgcn_wave_barrier();  // LDS reads done before the next tile overwrites
        return;
    }
    if (valid && v.dist && h == 0) v.dist[tg - first] = bd ? (double)bn / (double)bd : __builtin_inf();
    const Partial c = partial_of(bn, valid ? bd : 0, br, tg - first);
    if constexpr (TOPK) {
        topk_insert(v.best, (uint32_t)v.sink.cap, lane, c, h == 0);
        __builtin_amdgcn_wave_barrier();  // LDS reads done before the next tile overwrites
        return;
    }
    if (partial_better_dev(c, v.best)) v.best = c;
    __builtin_amdgcn_wave_barrier();  // LDS reads done before the next tile overwrites
}

// ------------------------------------------------------------------ shares: K-loop, epilogue, slice sum

// kSteps steps of 2 chunks from step g0 on, of the T tiles at dp[] (each the tile's first uint4 plus
// the lane) against the query fragments at qp (chunk c: lo [(2c) * 64], hi [(2c+1) * 64]), into
// S1 = sum q'_lo e'_lo and S2 = sum q'_lo e'_hi + q'_hi e'_lo.  Three register stages: the loads of
// step g + 2 are in flight while step g computes.
template <int kSteps, int T>
__device__ __forceinline__ void shares_accumulate(const uint4 *(&dp)[T], const uint4 *qp, int g0, v16i (&s1)[T],
                                                  v16i (&s2)[T]) {
    struct Stage {
        uint4 lo[T][2], hi[T][2];
        uint4 qlo[2], qhi[2];
    };
    auto load = [&](Stage &st, int g) {
        g = g0 + (g < kSteps ? g : kSteps - 1);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = 2 * g + i;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                st.lo[t][i] = nt_load16(dp[t] + (2 * c) * 64);
                st.hi[t][i] = nt_load16(dp[t] + (2 * c + 1) * 64);
            }
            st.qlo[i] = qp[(2 * c) * 64];
            st.qhi[i] = qp[(2 * c + 1) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto compute = [&](const Stage &st) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int t = 0; t < T; ++t) {
                s1[t] = mfma_i8(st.qlo[i], st.lo[t][i], s1[t]);
                s2[t] = mfma_i8(st.qlo[i], st.hi[t][i], s2[t]);
                s2[t] = mfma_i8(st.qhi[i], st.lo[t][i], s2[t]);
            }
    };
    Stage sa, sb, sc;
    load(sa, 0);
    load(sb, 1);
    int g = 0;
#pragma unroll 1
    for (; g + 3 <= kSteps; g += 3) {
        load(sc, g + 2);
        compute(sa);
        load(sa, g + 3);
        compute(sb);
        load(sb, g + 4);
        compute(sc);
    }
    // kSteps = 3q + {0, 1, 2} (200 = 66 * 3 + 2)
    if (g < kSteps) compute(sa);
    if (g + 1 < kSteps) compute(sb);
}

// One tile's rows of one query from its sums (every K-slice added): [32][31] u16 through
// store_tile_rows.  A caller that stores several tiles through one lds buffer puts a wave barrier
// between them.
__device__ __forceinline__ void store_query_tile(uint16_t *out, uint16_t *lds, const int2 *qsum, const v16i &s1,
                                                 const v16i &s2, uint64_t tile_t0, uint64_t first, uint64_t end,
                                                 bool tile_valid, int lane, bool wt = false) {
    // row 31 (lane t + 32, register 15) holds sum e'_lo in S1 and sum e'_hi + sum e'_lo in S2
    const int h = lane >> 5;
    const int src = (lane & 31) + 32;
    const int elo = __shfl(s1[15], src);
    const int ehi = __shfl(s2[15], src) - elo;
    store_tile_rows(out, lds, tile_t0, first, end, tile_valid, lane, [&](int r) {
        const int k = (r & 3) + 8 * (r >> 2) + 4 * h;
        const int2 qs = qsum[k < kRot ? k : 0];  // (sum q'_lo, sum q'_hi) of row k
        // the 16384 * K terms vanish mod 2^16 (K = 12800)
        const uint32_t lo = (uint32_t)s1[r] + 128u * (uint32_t)elo + 128u * (uint32_t)qs.x;
        const uint32_t cross = (uint32_t)s2[r] + 128u * (uint32_t)ehi + 128u * (uint32_t)qs.x +
                               128u * (uint32_t)elo + 128u * (uint32_t)qs.y;
        return (uint16_t)(lo + 256u * cross);
    }, wt);
}

// The K-split forms' slice sum through LDS: the waves of slices 1 .. KS - 1 put their N sum pairs
// (slice_put), the workgroup reaches a barrier, and slice 0's wave adds them pair by pair
// (slice_add) -- exact mod 2^16 like every partial here.
template <int KS, int N>
using SliceSums = int[KS - 1][N][2][16][64];

template <int KS, int N>
__device__ __forceinline__ void slice_put(SliceSums<KS, N> &red, int slice, int lane, const v16i (&s1)[N],
                                          const v16i (&s2)[N]) {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            red[slice - 1][n][0][i][lane] = s1[n][i];
            red[slice - 1][n][1][i][lane] = s2[n][i];
        }
}
template <int KS, int N>
__device__ __forceinline__ void slice_add(const SliceSums<KS, N> &red, int n, int lane, v16i &s1, v16i &s2) {
#pragma unroll
    for (int k = 0; k < KS - 1; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            s1[i] += red[k][n][0][i][lane];
            s2[i] += red[k][n][1][i][lane];
        }
}

}  // namespace iris
