// iris_mfma.hip — Template masked Hamming on the gfx950 matrix cores (fp4).
//
// Why MFMA for bit work: on gfx950 the integer VALU ops this path needs
// (v_bcnt, v_bitop3) issue at 16 lanes/clk, so the XOR+AND+popcount form is
// capped near 39 T lane-ops/s = ~11 ms per 10M templates (35 % of the HBM
// roofline; tools/ubench_ops.hip).  The same numbers are an
// exact integer matrix product:
//
//   den[k][t] = sum_b qm_k[b] * em_t[b]                       (jointly valid bits)
//   S  [k][t] = sum_b enc(q_k)[b] * enc(e_t)[b],  enc in {0,+1,-1}  (src/lib.rs:16-26)
//   num       = (den - S) / 2                                 (src/lib.rs:134-163 identity)
//
// with M = 32 rotation rows (k = 0..30 + a zero row), N = 32 templates per
// tile, K = 12800 bits: v_mfma_scale_f32_32x32x64_f8f6f4 with e2m1 operands.
// Every product is 0 or +-1 and every sum is an integer <= 12800 < 2^24, so the
// f32 accumulation is exact whatever the internal order.
//
// Operands: the 31 rotated query copies are precomputed once per engine as
// fp4 A-fragments (iris_host.cpp, 400 KB, L2-resident).  The template side
// is streamed from HBM once in the TILES layout (iris_internal.hpp), whose
// interleaved dwords turn into fp4 B-fragments with four v_and + two
// shift-and per dword pair — fast VOP2 ops, hidden under the MFMAs.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <type_traits>

#include "iris_device.hpp"

namespace iris {

constexpr int kTileUint4 = kPlaneGroups * 64;  // 6400 uint4 = 102400 B per tile
constexpr int kMfmaTiles = 4;    // tiles per wave (128 templates)
constexpr int kMfmaWgs = 2;      // workgroups per CU the register budget allows
constexpr int kSplitStages = 6;  // load ring depth of the K-split (small-range) form
// tiles per workgroup of the K-split form: every query-fragment load (2 per chunk pair and
// wave, from L2) feeds this many tiles -- at 1 the query stream is twice the template stream
constexpr int kSplitT = 2;

// Query-side den operand from the enc operand: |enc| as fp4 1.0, doubled to
// 2.0 in the dwords whose template-side value is 0.5 (fragment dwords 1, 3).
struct QFrag {
    v8i am, ae;
};
__device__ __forceinline__ QFrag qfrag_of(const uint4 &qe) {
    QFrag f;
    f.ae = v8i{(int)qe.x, (int)qe.y, (int)qe.z, (int)qe.w, 0, 0, 0, 0};
    f.am = v8i{(int)(qe.x & 0x22222222u), (int)((qe.y & 0x22222222u) << 1), (int)(qe.z & 0x22222222u),
               (int)((qe.w & 0x22222222u) << 1), 0, 0, 0, 0};
    return f;
}

// One 64-bit chunk of K for one tile.  x0/x1: the lane's interleaved dwords.
__device__ __forceinline__ void chunk_step(uint32_t x0, uint32_t x1, const QFrag &q, v16f &den, v16f &s) {
    const v8i bm = {(int)(x0 & 0x22222222u), (int)(x0 & 0x11111111u), (int)(x1 & 0x22222222u),
                    (int)(x1 & 0x11111111u), 0, 0, 0, 0};
    const v8i be = {(int)(x0 & 0xAAAAAAAAu), (int)((x0 << 1) & 0xAAAAAAAAu), (int)(x1 & 0xAAAAAAAAu),
                    (int)((x1 << 1) & 0xAAAAAAAAu), 0, 0, 0, 0};
    den = mfma_fp4(q.am, bm, den);
    s = mfma_fp4(q.ae, be, s);
}

// MF_MATCH: every record of the range whose best rotation's f64 distance is below ms.threshold
// is appended to ms (iris_template_matches); no partials, no reduce
// MF_TOPK: the wave's k best records (ms = topk_sink: k = ms.cap) go to its list ms.buf[wave]
// (iris_template_topk); the running best becomes the wave-resident list, no partials, no reduce
// MF_HIST: every record of the range is counted in the bin of its best rotation's distance (ms =
// hist_sink: iris_template_histogram) -- LDS atomics into the workgroup's histogram, whose non-zero
// words are added to the workgroup's copy of the counters once; no partials, no reduce
// MF_REPORT: MF_MATCH, MF_TOPK and MF_HIST from one read (iris_template_report): ms = report_sink
// points at the device's ReportSinks, read after the K loop, and each tile's best rotation, computed
// once, goes to every sink the struct holds -- a part's presence is workgroup-uniform
enum { MF_COUNTS = 0, MF_SEARCH = 1, MF_MATCH = 2, MF_TOPK = 3, MF_HIST = 4, MF_REPORT = 5 };

// KS > 1 (small ranges, T = kSplitT): the KS waves of a tile group split K -- wave w computes
// chunk groups [w' * 100 / KS, +100 / KS) of tiles T * (blockIdx.x * (4 / KS) + w / KS) + t (w' = w % KS)
// -- and the partial sums (exact integers in f32) meet in LDS before the epilogue, so a range of
// a few hundred tiles still puts several waves on every SIMD.
// FUSED (search, small grids): the last workgroup to finish folds every workgroup's
// partial and writes the winner to fin.dst itself (iris_device.hpp, fold_partials_last).
template <int MODE, int T = kMfmaTiles, int KS = 1, bool FUSED = false>
__global__ void __launch_bounds__(64 * kWaveSlots, kMfmaWgs)
    template_mfma_kernel(const uint4 *__restrict__ db, const uint4 *__restrict__ qfrag, uint64_t tile0,
                         uint64_t ntiles, uint64_t first, uint64_t end, uint16_t *__restrict__ num_out,
                         uint16_t *__restrict__ den_out, double *__restrict__ dist_out,
                         Partial *__restrict__ partials, FusedFinish fin, MatchSink ms) {
    constexpr int W = kWaveSlots;
    static_assert(KS == 1 || (W % KS == 0 && kPlaneGroups % KS == 0), "K-split geometry");
    const int lane = threadIdx.x & 63;
    const int wslot = threadIdx.x >> 6;
    const int slice = wslot % KS;
    const uint64_t wave = (uint64_t)blockIdx.x * (W / KS) + wslot / KS;
    const uint64_t tw = wave * T;  // first tile (relative to tile0) of this wave
    const bool active = tw < ntiles;  // wave-uniform
    constexpr int kG = kPlaneGroups / KS;  // chunk groups of this wave's K-slice
    const int g0 = slice * kG;

    v16f den[T], s[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            den[t][i] = 0.f;
            s[t][i] = 0.f;
        }
    }

    if (active) {
        // 3-stage register pipeline: the loads of step g+2 are in flight
        // while step g computes (one step = 2 chunks = 16 MFMAs per wave).
        const uint4 *dp[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint64_t rel = (tw + t < ntiles) ? tw + t : ntiles - 1;  // clamp: extra tiles re-read a valid one
            dp[t] = db + (tile0 + rel) * (uint64_t)kTileUint4 + lane;
        }
        const uint4 *qp = qfrag + lane;  // chunk c: qfrag[c * 64 + lane]
        struct Stage {
            uint4 d[T];
            uint4 q0, q1;
        };
        auto load = [&](Stage &st, int g) {
            g = (g < kG ? g : kG - 1) + g0;
#pragma unroll
            for (int t = 0; t < T; ++t) st.d[t] = nt_load16(dp[t] + g * 64);
            st.q0 = qp[(2 * g) * 64];
            st.q1 = qp[(2 * g + 1) * 64];
            // keep this stage's loads together and ahead of the compute that
            // follows: vmcnt retires in order, so a query load sunk next to
            // its use would also drain the HBM prefetches issued before it
            __builtin_amdgcn_sched_barrier(0);
        };
        auto compute = [&](const Stage &st) {
            const QFrag f0 = qfrag_of(st.q0);
#pragma unroll
            for (int t = 0; t < T; ++t) chunk_step(st.d[t].x, st.d[t].y, f0, den[t], s[t]);
            const QFrag f1 = qfrag_of(st.q1);
#pragma unroll
            for (int t = 0; t < T; ++t) chunk_step(st.d[t].z, st.d[t].w, f1, den[t], s[t]);
        };
        if constexpr (KS > 1) {
            // K-slice of kG = 25 steps, fully unrolled over a kSplitStages-deep ring: the wave
            // keeps (kSplitStages - 1) steps of loads in flight instead of 2, so a range of a
            // few hundred tiles -- one short slice per wave, nothing to overlap between
            // slices -- is not bound by one HBM round trip per two steps
            Stage st[kSplitStages];
#pragma unroll
            for (int i = 0; i < kSplitStages - 1; ++i) load(st[i], i);
#pragma unroll
            for (int g = 0; g < kG; ++g) {
                if (g + kSplitStages - 1 < kG) load(st[(g + kSplitStages - 1) % kSplitStages], g + kSplitStages - 1);
                compute(st[g % kSplitStages]);
            }
        } else {
            Stage sa, sb, sc;
            load(sa, 0);
            load(sb, 1);
            int g = 0;
#pragma unroll 1
            for (; g + 3 <= kG; g += 3) {
                load(sc, g + 2);
                compute(sa);
                load(sa, g + 3);
                compute(sb);
                load(sb, g + 4);
                compute(sc);
            }
            // kG = 3q + {1, 2} (100; 50): the remaining steps' data is in sa (, sb)
            if constexpr (kG % 3 >= 1) compute(sa);
            if constexpr (kG % 3 == 2) compute(sb);
        }
    }
    // MF_HIST: every wave zeroes its share of the workgroup's histogram -- inactive waves and
    // non-zero K-slices too -- ahead of a barrier all of them reach (K-split: the one below)
    if constexpr (MODE == MF_HIST) {
        hist_zero(hist_lds<1>(), hist_sink_bins(ms));
        if constexpr (KS == 1) __syncthreads();
    }
    // MF_REPORT: the three sinks; with a histogram part (workgroup-uniform) the same zeroing and barrier
    ReportSinks rs{};
    if constexpr (MODE == MF_REPORT) {
        rs = report_sinks_load(ms);
        if (report_has_hist(rs)) {
            hist_zero(hist_lds<1>(), hist_sink_bins(rs.hist));
            if constexpr (KS == 1) __syncthreads();
        }
    }
    if constexpr (KS > 1) {  // the K-slices' partial sums -> slice 0's accumulators (exact)
        __shared__ float red[W][T][32][64];
        if (slice != 0) {
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    red[wslot][t][i][lane] = den[t][i];
                    red[wslot][t][16 + i][lane] = s[t][i];
                }
        }
        __syncthreads();
        if (slice == 0) {
#pragma unroll
            for (int k = 1; k < KS; ++k)
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        den[t][i] += red[wslot + k][t][i][lane];
                        s[t][i] += red[wslot + k][t][16 + i][lane];
                    }
        }
    }

    // C layout: lane l holds template (l & 31) of the tile and rotation rows
    // k = (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 0..15.
    const int h = lane >> 5;
    Partial best = partial_none();
    // MF_MATCH: the tiles' candidates (half 0 of the wave votes: both halves hold the record's best)
    bool hit[T];
    uint32_t hn[T], hd[T];
    int hr[T];
    uint64_t hi[T];
    // MF_TOPK recomputes the wave's first tile here from an opaque copy of threadIdx.x: at T = 4 the
    // main loop has no register to spare, and the 64-bit tile numbers this epilogue needs would
    // otherwise be spilled across it (MF_REPORT: its top-k part's)
    uint64_t twe = tw, wave_e = wave;
    if constexpr (MODE == MF_TOPK || MODE == MF_REPORT) {
        uint32_t tx = threadIdx.x;
        asm volatile("" : "+v"(tx));
        wave_e = (uint64_t)blockIdx.x * (W / KS) + (tx >> 6) / KS;
        twe = wave_e * T;
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const uint64_t t0 = (tile0 + twe + t) * kTile;  // global index of the tile's first template
        const bool tv = active && (twe + t < ntiles) && slice == 0;
        if constexpr (MODE == MF_COUNTS) {
            __shared__ __attribute__((aligned(16))) uint16_t sh_out[W][1024];
            uint16_t *lds = sh_out[wslot];
            if (num_out)
                store_tile_rows(num_out, lds, t0, first, end, tv, lane,
                                [&](int r) { return (uint16_t)(((int)den[t][r] - (int)s[t][r]) >> 1); });
            if (den_out)
                store_tile_rows(den_out, lds, t0, first, end, tv, lane,
                                [&](int r) { return (uint16_t)(uint32_t)den[t][r]; });
        } else {
            const uint64_t tg = t0 + (lane & 31);
            const bool valid = tv && tg >= first && tg < end;
            const uint64_t o = tg - first;
            uint32_t bn, bd;
            int br;
            best_rotation(lane, [&](int r, uint32_t &nn, uint32_t &dd) {
                dd = (uint32_t)den[t][r];
                nn = (uint32_t)(((int)dd - (int)s[t][r]) >> 1);  // num = (den - S) / 2
            }, bn, bd, br);
            if constexpr (MODE == MF_MATCH) {
                hit[t] = match_hit(ms, valid && h == 0, bn, bd);
                hn[t] = bn;
                hd[t] = bd;
                hr[t] = br;
                hi[t] = o;
                continue;
            }
            if constexpr (MODE == MF_HIST) {  // half 0 counts: both halves hold the record's best
                hist_count(hist_lds<1>(), hist_sink_bins(ms), lane, valid && h == 0, bn, bd);
                continue;
            }
            if constexpr (MODE == MF_TOPK) {  // den = 0: no candidate (half 0 votes)
                hn[t] = bn;
                hd[t] = valid && h == 0 ? bd : 0;
                hr[t] = br;
                continue;
            }
            if constexpr (MODE == MF_REPORT) {
                // the histogram's count as MF_HIST; the candidate as MF_TOPK keeps it, which is also
                // MF_MATCH's record wherever it hits (a hit is a valid lane of half 0)
                if (report_has_hist(rs)) hist_count(hist_lds<1>(), hist_sink_bins(rs.hist), lane, valid && h == 0, bn, bd);
                hit[t] = report_has_match(rs) && match_hit(rs.match, valid && h == 0, bn, bd);
                hn[t] = bn;
                hd[t] = valid && h == 0 ? bd : 0;
                hr[t] = br;
                hi[t] = o;
                continue;
            }
            if (valid && dist_out && h == 0) dist_out[o] = bd ? (double)bn / (double)bd : __builtin_inf();
            const Partial c = partial_of(bn, valid ? bd : 0, br, o);
            if (partial_better_dev(c, best)) best = c;
        }
    }
    if constexpr (MODE == MF_MATCH) append_matches<T>(ms, lane, hit, hn, hd, hr, hi);
    // MF_HIST: the kernel has no early exit, so every wave reaches this barrier as it reached the first
    if constexpr (MODE == MF_HIST) {
        __syncthreads();
        hist_flush(hist_lds<1>(), hist_sink_bins(ms), hist_sink_copy(ms));
    }
    // MF_TOPK: the tiles' candidates go into the wave's list once the accumulators are dead (best:
    // this lane's entry).  One list per tile group: with a K-split only slice 0's wave holds sums.
    if constexpr (MODE == MF_TOPK) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            topk_insert(best, (uint32_t)ms.cap, lane,
                        partial_of(hn[t], hd[t], hr[t], (tile0 + twe + t) * kTile + (lane & 31) - first), true);
        }
        if (slice == 0) topk_store(ms, wave_e, lane, best);
    }
    // MF_REPORT: the parts the sinks hold, each as its own mode above -- the histogram's second
    // barrier under the same workgroup-uniform test as its first
    if constexpr (MODE == MF_REPORT) {
        if (report_has_hist(rs)) {
            __syncthreads();
            hist_flush(hist_lds<1>(), hist_sink_bins(rs.hist), hist_sink_copy(rs.hist));
        }
        if (report_has_match(rs)) append_matches<T>(rs.match, lane, hit, hn, hd, hr, hi);
        if (report_has_topk(rs)) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                topk_insert(best, (uint32_t)rs.topk.cap, lane,
                            partial_of(hn[t], hd[t], hr[t], (tile0 + twe + t) * kTile + (lane & 31) - first), true);
            }
            if (slice == 0) topk_store(rs.topk, wave_e, lane, best);
        }
    }
    if constexpr (MODE == MF_SEARCH) {
        __shared__ Partial sh[W];
        const bool folded = block_argmin(best, sh, W);  // thread 0: the workgroup's winner
        if constexpr (FUSED) fold_partials_last(partials, best, fin);
        else if (folded) partials[blockIdx.x] = best;
    }
}

// ------------------------------------------------------------------ a few queries per pass

// NQ queries against one streamed pass of the database: per 64-bit chunk and
// tile 2 NQ MFMAs share one expansion of the template bits, so up to NQ = 2 the
// pass stays near the HBM bound while one single-query pass per query would
// stream the database NQ times.  T = 4 / NQ tiles per wave keeps the NQ x T x 2
// accumulators at 128 VGPRs.  Partials: [NQ][gridDim.x].
struct QueryFrags {
    const uint4 *q[4];
};

template <int NQ>
__global__ void __launch_bounds__(256, 2)
    template_multi_kernel(const uint4 *__restrict__ db, QueryFrags qf, uint64_t tile0, uint64_t ntiles,
                          uint64_t first, uint64_t end, Partial *__restrict__ partials) {
    constexpr int T = 4 / NQ;
    const int lane = threadIdx.x & 63;
    const int wslot = threadIdx.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * kWaveSlots + wslot;
    const uint64_t tw = wave * T;
    const bool active = tw < ntiles;  // wave-uniform

    v16f den[NQ][T], s[NQ][T];
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                den[qi][t][i] = 0.f;
                s[qi][t][i] = 0.f;
            }

    if (active) {
        const uint4 *dp[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint64_t rel = (tw + t < ntiles) ? tw + t : ntiles - 1;
            dp[t] = db + (tile0 + rel) * (uint64_t)kTileUint4 + lane;
        }
        struct Stage {
            uint4 d[T];
            uint4 q[NQ][2];
        };
        auto load = [&](Stage &st, int g) {
            g = g < kPlaneGroups ? g : kPlaneGroups - 1;
#pragma unroll
            for (int t = 0; t < T; ++t) st.d[t] = nt_load16(dp[t] + g * 64);
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) {
                st.q[qi][0] = qf.q[qi][(2 * g) * 64 + lane];
                st.q[qi][1] = qf.q[qi][(2 * g + 1) * 64 + lane];
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        auto compute = [&](const Stage &st) {
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) {
                const QFrag f0 = qfrag_of(st.q[qi][0]);
#pragma unroll
                for (int t = 0; t < T; ++t) chunk_step(st.d[t].x, st.d[t].y, f0, den[qi][t], s[qi][t]);
                const QFrag f1 = qfrag_of(st.q[qi][1]);
#pragma unroll
                for (int t = 0; t < T; ++t) chunk_step(st.d[t].z, st.d[t].w, f1, den[qi][t], s[qi][t]);
            }
        };
        Stage sa, sb, sc;
        load(sa, 0);
        load(sb, 1);
        int g = 0;
#pragma unroll 1
        for (; g + 3 <= kPlaneGroups; g += 3) {
            load(sc, g + 2);
            compute(sa);
            load(sa, g + 3);
            compute(sb);
            load(sb, g + 4);
            compute(sc);
        }
        if (g < kPlaneGroups) compute(sa);
    }

    Partial best[NQ];
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) best[qi] = partial_none();
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const uint64_t tg = (tile0 + tw + t) * kTile + (lane & 31);
        const bool valid = active && (tw + t < ntiles) && tg >= first && tg < end;
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
            uint32_t bn, bd;
            int br;
            best_rotation(lane, [&](int r, uint32_t &nn, uint32_t &dd) {
                dd = (uint32_t)den[qi][t][r];
                nn = (uint32_t)(((int)dd - (int)s[qi][t][r]) >> 1);
            }, bn, bd, br);
            const Partial c = partial_of(bn, valid ? bd : 0, br, tg - first);
            if (partial_better_dev(c, best[qi])) best[qi] = c;
        }
    }
    __shared__ Partial sh[NQ][kWaveSlots];
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
        best[qi] = wave_argmin(best[qi]);
        if (lane == 0) sh[qi][wslot] = best[qi];
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        const int qi = threadIdx.x;
        Partial b;
        fold_waves(b, sh[qi], kWaveSlots);
        partials[(uint64_t)qi * gridDim.x + blockIdx.x] = b;
    }
}

// ------------------------------------------------------------------ shared passes

// One round of a sharing pass: NQ queries against the T tiles from tw (relative to tile0), the
// streaming loop of template_mfma_kernel (NQ = 1, T = 4) and of template_multi_kernel<2> (NQ = 2,
// T = 2); the round's sums go to epi(den, s): round_candidates (search) or round_matches (match).
// Query fragments as pointers into global memory by type: the guest's pointer comes out of LDS, and
// as a generic pointer its loads would be flat ones, behind which every wait drains the whole
// load queue -- the prefetch ring of both paths would collapse.
typedef const __attribute__((address_space(1))) u32x4 *GlobalFrag;
__device__ __forceinline__ uint4 frag_load(GlobalFrag p) {
    const u32x4 v = *p;
    return make_uint4(v.x, v.y, v.z, v.w);
}

// A round's epilogue: each query's best rotation per record of the T tiles from tw, folded into
// best[].  Tiles past the range (tw + t >= ntiles: the loop streamed a clamped one) give no candidate.
template <int NQ, int T>
__device__ __forceinline__ void round_candidates(const v16f (&den)[NQ][T], const v16f (&s)[NQ][T], uint64_t tile0,
                                                 uint64_t ntiles, uint64_t tw, uint64_t first, uint64_t end, int lane,
                                                 Partial (&best)[NQ]) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const uint64_t tg = (tile0 + tw + t) * kTile + (lane & 31);
        const bool valid = (tw + t < ntiles) && tg >= first && tg < end;
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
            uint32_t bn, bd;
            int br;
            best_rotation(lane, [&](int r, uint32_t &nn, uint32_t &dd) {
                dd = (uint32_t)den[qi][t][r];
                nn = (uint32_t)(((int)dd - (int)s[qi][t][r]) >> 1);  // num = (den - S) / 2
            }, bn, bd, br);
            const Partial c = partial_of(bn, valid ? bd : 0, br, tg - first);
            if (partial_better_dev(c, best[qi])) best[qi] = c;
        }
    }
}

// The match form's epilogue of a round: every record of the T tiles from tw whose best rotation
// lies below query qi's threshold is appended to sink[qi] (half 0 of the wave votes, as in
// template_mfma_kernel<MF_MATCH>).  The sinks' pointers are global by type, as the fragments: a
// flat store or atomic would make every wait of the next round's loop a full drain.
typedef __attribute__((address_space(1))) Partial *GlobalPartial;
struct GlobalSink {
    GlobalPartial buf;
    uint64_t cap;
    __attribute__((address_space(1))) uint64_t *count;
    double threshold;
};
template <int NQ, int T>
__device__ __forceinline__ void round_matches(const v16f (&den)[NQ][T], const v16f (&s)[NQ][T], uint64_t tile0,
                                              uint64_t ntiles, uint64_t tw, uint64_t first, uint64_t end, int lane,
                                              const GlobalSink (&sink)[NQ]) {
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
        bool hit[T];
        uint32_t hn[T], hd[T];
        int hr[T];
        uint64_t hi[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint64_t tg = (tile0 + tw + t) * kTile + (lane & 31);
            const bool valid = (tw + t < ntiles) && tg >= first && tg < end;
            best_rotation(lane, [&](int r, uint32_t &nn, uint32_t &dd) {
                dd = (uint32_t)den[qi][t][r];
                nn = (uint32_t)(((int)dd - (int)s[qi][t][r]) >> 1);  // num = (den - S) / 2
            }, hn[t], hd[t], hr[t]);
            hit[t] = match_hit(sink[qi], valid && (lane >> 5) == 0, hn[t], hd[t]);
            hi[t] = tg - first;
        }
        append_matches<T>(sink[qi], lane, hit, hn, hd, hr, hi);
    }
}

// The top-k form's epilogue of a round: each query's candidates of the T tiles from tw (half 0 of
// the wave votes, den = 0 otherwise, as in template_mfma_kernel<MF_TOPK>) go into that query's
// wave-resident list, list[qi] being this lane's entry.  A query's T candidates are formed first, so
// its accumulators are dead when the inserts run.
struct GlobalLists {
    GlobalPartial buf;  // lists[units][k]
    uint32_t k;
};
template <int NQ, int T>
__device__ __forceinline__ void round_topk(const v16f (&den)[NQ][T], const v16f (&s)[NQ][T], uint64_t tile0,
                                           uint64_t ntiles, uint64_t tw, uint64_t first, uint64_t end, int lane,
                                           const uint32_t (&k)[NQ], Partial (&list)[NQ]) {
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
        uint32_t hn[T], hd[T];
        int hr[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint64_t tg = (tile0 + tw + t) * kTile + (lane & 31);
            const bool valid = (tw + t < ntiles) && tg >= first && tg < end;
            best_rotation(lane, [&](int r, uint32_t &nn, uint32_t &dd) {
                dd = (uint32_t)den[qi][t][r];
                nn = (uint32_t)(((int)dd - (int)s[qi][t][r]) >> 1);  // num = (den - S) / 2
            }, hn[t], hd[t], hr[t]);
            if (!(valid && (lane >> 5) == 0)) hd[t] = 0;
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            topk_insert(list[qi], k[qi], lane,
                        partial_of(hn[t], hd[t], hr[t], (tile0 + tw + t) * kTile + (lane & 31) - first), true);
        }
    }
}

// The report form's epilogue of a round (iris_template_report_async): per query and tile the best
// rotation once, and from it every part that query's sinks hold, each as its own form above feeds
// it -- the histogram's count into the query's LDS histogram `hist` (hist_count), the hits appended
// to its match sink (round_matches), the candidates into its wave-resident list (round_topk; list:
// this lane's entry).  A part's presence is a scalar test, the same for every wave of the workgroup;
// the pointers are global by type, as every sink's of a sharing pass.
typedef __attribute__((address_space(1))) uint64_t *GlobalCounter;
struct GlobalReport {
    GlobalSink match;    // count null: no matches part
    GlobalLists topk;    // k 0: no top-k part
    GlobalCounter hist;  // counters[copy_mask + 1][nbins + 1]; null: no histogram part
    uint32_t nbins, copy_mask;
};
__device__ __forceinline__ bool report_has_match(const GlobalReport &r) { return (uint64_t)r.match.count != 0; }
__device__ __forceinline__ bool report_has_topk(const GlobalReport &r) { return r.topk.k != 0; }
__device__ __forceinline__ bool report_has_hist(const GlobalReport &r) { return (uint64_t)r.hist != 0; }
// the words a workgroup's thread 0 keeps of a query's ReportSinks in LDS (kReportWords u64 a query)
// and a wave's copy of them, made uniform: SGPRs, read where a round's epilogue uses them, so that
// nothing of them is carried across the streaming loop
constexpr int kReportWords = 8;
__device__ __forceinline__ uint64_t (*report_words_lds())[kReportWords] {  // of the kernel that calls it only
    __shared__ uint64_t w[2][kReportWords];
    return w;
}
__device__ __forceinline__ void report_words_store(uint64_t *w, const ReportSinks *sinks) {
    const __attribute__((address_space(1))) ReportSinks *const p = (const __attribute__((address_space(1))) ReportSinks *)sinks;
    w[0] = (uint64_t)p->match.buf;
    w[1] = p->match.cap;
    w[2] = (uint64_t)p->match.count;
    w[3] = (uint64_t)__double_as_longlong(p->match.threshold);
    w[4] = (uint64_t)p->topk.buf;
    w[5] = p->topk.cap;
    w[6] = p->hist.cap;
    w[7] = (uint64_t)p->hist.count;
}
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {  // as template_share_kernel's uniform64
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ GlobalReport report_words_load(const uint64_t *w) {
    GlobalReport r;
    r.match = GlobalSink{(GlobalPartial)uniform_u64(w[0]), uniform_u64(w[1]), (GlobalCounter)uniform_u64(w[2]),
                         __longlong_as_double((long long)uniform_u64(w[3]))};
    r.topk = GlobalLists{(GlobalPartial)uniform_u64(w[4]), (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w[5])};
    const uint64_t hc = uniform_u64(w[6]);
    r.hist = (GlobalCounter)uniform_u64(w[7]);
    r.nbins = (uint32_t)hc;
    r.copy_mask = (uint32_t)(hc >> 32);
    return r;
}
// One query's T tiles from tw.  Tiles past the range and records outside it are neither counted nor
// candidates (the histogram counts EVERY record of the range once, so a clamped duplicate would show
// in its sum); half 0 of the wave votes, as in every form above.
template <int T>
__device__ __forceinline__ void round_report(const GlobalReport &r, uint32_t *hist, const v16f (&den)[T],
                                             const v16f (&s)[T], uint64_t tile0, uint64_t ntiles, uint64_t tw,
                                             uint64_t first, uint64_t end, int lane, Partial &list) {
    bool hit[T];
    uint32_t hn[T], hd[T];
    int hr[T];
    uint64_t hi[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const uint64_t tg = (tile0 + tw + t) * kTile + (lane & 31);
        const bool counted = (tw + t < ntiles) && tg >= first && tg < end && (lane >> 5) == 0;
        best_rotation(lane, [&](int rr, uint32_t &nn, uint32_t &dd) {
            dd = (uint32_t)den[t][rr];
            nn = (uint32_t)(((int)dd - (int)s[t][rr]) >> 1);  // num = (den - S) / 2
        }, hn[t], hd[t], hr[t]);
        if (report_has_hist(r)) hist_count(hist, r.nbins, lane, counted, hn[t], hd[t]);
        hit[t] = report_has_match(r) && match_hit(r.match, counted, hn[t], hd[t]);
        if (!counted) hd[t] = 0;  // no candidate (a hit is a counted lane: its record keeps its den)
        hi[t] = tg - first;
    }
    if (report_has_match(r)) append_matches<T>(r.match, lane, hit, hn, hd, hr, hi);
    if (report_has_topk(r)) {
#pragma unroll
        for (int t = 0; t < T; ++t) topk_insert(list, r.topk.k, lane, partial_of(hn[t], hd[t], hr[t], hi[t]), true);
    }
}

template <int NQ, int T, class Epi>
__device__ __forceinline__ void share_round(const uint4 *__restrict__ db, const GlobalFrag (&qf)[NQ], uint64_t tile0,
                                            uint64_t ntiles, uint64_t tw, int lane, Epi &&epi) {
    const bool active = tw < ntiles;  // wave-uniform
    v16f den[NQ][T], s[NQ][T];
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                den[qi][t][i] = 0.f;
                s[qi][t][i] = 0.f;
            }

    if (active) {
        const uint4 *dp[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint64_t rel = (tw + t < ntiles) ? tw + t : ntiles - 1;  // clamp: extra tiles re-read a valid one
            dp[t] = db + (tile0 + rel) * (uint64_t)kTileUint4 + lane;
        }
        struct Stage {
            uint4 d[T];
            uint4 q[NQ][2];
        };
        auto load = [&](Stage &st, int g) {
            g = g < kPlaneGroups ? g : kPlaneGroups - 1;
#pragma unroll
            for (int t = 0; t < T; ++t) st.d[t] = nt_load16(dp[t] + g * 64);
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) {
                st.q[qi][0] = frag_load(qf[qi] + (2 * g) * 64 + lane);
                st.q[qi][1] = frag_load(qf[qi] + (2 * g + 1) * 64 + lane);
            }
            __builtin_amdgcn_sched_barrier(0);  // as in template_mfma_kernel: the stage's loads stay together
        };
        auto compute = [&](const Stage &st) {
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) {
                const QFrag f0 = qfrag_of(st.q[qi][0]);
#pragma unroll
                for (int t = 0; t < T; ++t) chunk_step(st.d[t].x, st.d[t].y, f0, den[qi][t], s[qi][t]);
                const QFrag f1 = qfrag_of(st.q[qi][1]);
#pragma unroll
                for (int t = 0; t < T; ++t) chunk_step(st.d[t].z, st.d[t].w, f1, den[qi][t], s[qi][t]);
            }
        };
        Stage sa, sb, sc;
        load(sa, 0);
        load(sb, 1);
        int g = 0;
#pragma unroll 1
        for (; g + 3 <= kPlaneGroups; g += 3) {
            load(sc, g + 2);
            compute(sa);
            load(sa, g + 3);
            compute(sb);
            load(sb, g + 4);
            compute(sc);
        }
        if constexpr (kPlaneGroups % 3 >= 1) compute(sa);
        if constexpr (kPlaneGroups % 3 == 2) compute(sb);
    }
    epi(den, s);
}

// The two-query round (2 queries x 2 tiles per wave) with the query operands staged once per
// workgroup.  Through registers every wave pulls the same 4 KB of fragments per step out of L2 --
// twice its 2 KB of templates -- and derives the den operand from each of them again.  Here the
// 256 threads fetch a step's 4 KB with one 16-B load each: wave w fetches fragment 2 g + (w & 1) of
// query w >> 1, applies qfrag_of once and writes both operands to a two-slot LDS ring
// [slot][query][chunk of the step][am, ae][lane] (lane-linear 1-KB rows: ds_read_b128 without
// conflicts); every wave reads the step's 8 operands from there.
//   The fetch rides in the register stage of its step, behind the stage's two template loads, so
// the stage is 12 VGPRs instead of 24 and the ring is DEPTH deep: loads retire in order, and the
// wait for step g + 1's fragment ahead of its LDS write leaves the template loads of steps
// g + 2 .. g + DEPTH - 1 in flight.  One barrier per step: slot (g + 1) & 1 was last read in step
// g - 1, before that step's barrier.
//   Every wave of the workgroup walks all 100 steps -- the barriers and the fetch duty do not
// depend on ntiles.  A wave whose tiles lie past the range streams the clamped last tile, as
// partial waves do, and `valid` drops its candidates.  Nothing in the walk branches on anything
// that is not workgroup-uniform.
constexpr int kStagedDepth = 4;  // 242 VGPRs; 5: 255, no faster; 6 spills
typedef uint4 FragRing[2][2][2][2][64];

template <int DEPTH, class Epi>
__device__ __forceinline__ void staged_round(const uint4 *__restrict__ db, const GlobalFrag (&qf)[2], uint64_t tile0,
                                             uint64_t ntiles, uint64_t tw, int lane, int wslot, FragRing &ring,
                                             Epi &&epi) {
    constexpr int T = 2;
    static_assert(kWaveSlots == 4 && DEPTH >= 3, "one fetch per wave: 2 queries x 2 chunks of a step");
    v16f den[2][T], s[2][T];
#pragma unroll
    for (int qi = 0; qi < 2; ++qi)
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                den[qi][t][i] = 0.f;
                s[qi][t][i] = 0.f;
            }

    const uint4 *dp[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const uint64_t rel = (tw + t < ntiles) ? tw + t : ntiles - 1;  // clamp: extra tiles re-read a valid one
        dp[t] = db + (tile0 + rel) * (uint64_t)kTileUint4 + lane;
    }
    const int fq = wslot >> 1, fc = wslot & 1;  // this wave's fetch duty (wave-uniform)
    const GlobalFrag fp = (fq ? qf[1] : qf[0]) + fc * 64 + lane;
    struct Stage {
        uint4 d[T];
        uint4 f;
    };
    auto load = [&](Stage &st, int g) {
        g = g < kPlaneGroups ? g : kPlaneGroups - 1;
#pragma unroll
        for (int t = 0; t < T; ++t) st.d[t] = nt_load16(dp[t] + g * 64);
        st.f = frag_load(fp + (2 * g) * 64);
        __builtin_amdgcn_sched_barrier(0);  // as in template_mfma_kernel: the stage's loads stay together
    };
    auto stage_frag = [&](const Stage &st, int slot) {
        const QFrag f = qfrag_of(st.f);
        ring[slot][fq][fc][0][lane] = make_uint4(f.am[0], f.am[1], f.am[2], f.am[3]);
        ring[slot][fq][fc][1][lane] = st.f;
    };
    auto operand = [&](int slot, int qi, int c, int e) {
        const uint4 v = ring[slot][qi][c][e][lane];
        return v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
    };
    auto compute = [&](const Stage &st, int slot) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int qi = 0; qi < 2; ++qi) {
                QFrag f;
                f.am = operand(slot, qi, c, 0);
                f.ae = operand(slot, qi, c, 1);
#pragma unroll
                for (int t = 0; t < T; ++t)
                    chunk_step(c ? st.d[t].z : st.d[t].x, c ? st.d[t].w : st.d[t].y, f, den[qi][t], s[qi][t]);
            }
    };
    // step g: the loads of step g + DEPTH - 1, the step's MFMAs from slot g & 1, then step g + 1's
    // operands into the other slot (past the last step: the clamped fragment, never read)
    auto step = [&](Stage &free_, const Stage &cur, const Stage &next, int g) {
        load(free_, g + DEPTH - 1);
        compute(cur, g & 1);
        stage_frag(next, (g + 1) & 1);
        __syncthreads();
    };
    Stage st[DEPTH];
#pragma unroll
    for (int i = 0; i < DEPTH - 1; ++i) load(st[i], i);
    stage_frag(st[0], 0);
    __syncthreads();
    int g = 0;
#pragma unroll 1
    for (; g + DEPTH <= kPlaneGroups; g += DEPTH) {
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) step(st[(i + DEPTH - 1) % DEPTH], st[i], st[(i + 1) % DEPTH], g + i);
    }
#pragma unroll
    for (int i = 0; i < kPlaneGroups % DEPTH; ++i) step(st[(i + DEPTH - 1) % DEPTH], st[i], st[(i + 1) % DEPTH], g + i);
    epi(den, s);
}

// A round's bests of NQ queries -> the wave's entries sh[qi * N + pos] (LDS: nothing of a round
// stays in registers across the next one).
template <int NQ, int N>
__device__ __forceinline__ void share_stash(Partial (&best)[NQ], int lane, int pos, Partial *sh) {
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
        best[qi] = wave_argmin(best[qi]);
        if (lane == 0) sh[qi * N + pos] = best[qi];
    }
}

// The N stashed entries of query threadIdx.x < NQ -> its Partial in out[qi][blockIdx.x] (global by
// type, as the fragments: no flat store either).
template <int NQ, int N>
__device__ __forceinline__ void share_finish(const Partial *sh, const GlobalPartial (&out)[NQ]) {
    __syncthreads();
    if (threadIdx.x < NQ) {
        const int qi = threadIdx.x;
        Partial b;
        fold_waves(b, sh + qi * N, N);
        const GlobalPartial o = out[qi] + blockIdx.x;
        o->num = b.num;
        o->den = b.den;
        o->rot = b.rot;
        o->pad = b.pad;
        o->idx = b.idx;
    }
}

// The pass of iris_template_search_async, iris_template_matches_async, iris_template_topk_async and
// iris_template_report_async over large TILES ranges (4 tiles per wave; the search with its separate reduce).  Each workgroup
// decides at its start, from words another stream may write while the pass runs: its tile group was
// computed for this query by the pass that hosted it (own_done) -> nothing to do; a guest has been
// published in the slot -> both queries for the workgroup's 16 tiles in the two-query shape (2
// tiles x 2 queries per wave, twice), both queries' results, then the guest's done word; else the
// single-query pass.
//   SH_SEARCH: `out` is the partials array, and a workgroup's results are one Partial per query
// (the guest's into slot->partials).  SH_MATCH: `out` is the query's MatchSink, and every round
// appends its hits to it and, in the two-query shape, the guest's hits to slot->sink; a tile group
// is appended for a query by exactly one workgroup -- the hosting pass's, which then sets the done
// word, or else the query's own -- so the counters stay exact.  SH_TOPK: `out` is the query's
// topk_sink, the guest's is slot->sink (k may differ); every wave keeps one sorted list per query
// over its 4 tiles (round_topk) and stores it, empty or not, at unit blockIdx.x * kWaveSlots +
// wslot of that query's lists -- the unit template_mfma_kernel<MF_TOPK> numbers -- so each unit of
// a query's lists is written exactly once, by the hosting pass or by the query's own launch.
// SH_REPORT: `out` is report_sink of the query's device ReportSinks and so is slot->sink for the
// guest's; thread 0 reads both structs into LDS (the guest's behind the acquire: it was complete
// before `ready` was published), and a round's epilogue feeds, per query, the parts that query's
// struct holds (round_report): hits as SH_MATCH, the wave's list as SH_TOPK -- parked in LDS between
// the rounds, stored at the same unit, empty lists included -- and every record's bin in the query's
// own LDS histogram, which covers both rounds and is flushed once, behind a barrier under a
// workgroup-uniform test, into copy blockIdx.x % copies of that query's counters.  A tile group feeds
// a query's sinks in exactly one workgroup, so the histogram's sum is the range.
//   Memory order: only the slot is written while the pass runs.  The done words and whatever a
// pass writes for its guest (partials; records, counter and histogram adds, the adds agent-scope relaxed; lists) are
// read by the guest's own launch and what follows it on the device stream, so the end of the
// kernel publishes them: they are plain stores, and own_done is read relaxed.  (An agent-scope
// release store per tile group wrote the XCD's L2 back 19 532 times a pass, 0.43 ms of a 7.8-ms
// two-query pass; an acquire load invalidates the CU's L1 under the other workgroup's query
// fragments.)  `ready` is read relaxed, and only a workgroup that finds it set pays the acquire,
// ahead of the slot's fields and the guest's fragments.
// even_only (test hook): the guest counts as not visible in odd tile groups.
// (ints, not an unnamed enum: MODE == SH_SEARCH is part of the kernel's mangled name, and host and
// device passes number unnamed types differently)
constexpr int SH_SEARCH = 0, SH_MATCH = 1, SH_TOPK = 2, SH_REPORT = 3;
template <int MODE>
__global__ void __launch_bounds__(64 * kWaveSlots, kMfmaWgs)
    template_share_kernel(const uint4 *__restrict__ db, const uint4 *__restrict__ qfrag, uint64_t tile0, uint64_t ntiles,
                          uint64_t first, uint64_t end,
                          std::conditional_t<MODE == SH_SEARCH, Partial *__restrict__, MatchSink> out,
                          const GuestSlot *slot, const uint32_t *own_done, unsigned long long *count,
                          uint32_t even_only) {
    // one thread reads the words (agent-scope atomics: a plain load could be served from the scalar
    // cache) and the slot's fields behind them; LDS makes the decision the same for every wave
    __shared__ uint32_t sh_flag[2];
    __shared__ uint64_t sh_guest[MODE == SH_MATCH ? 6 : MODE == SH_TOPK ? 4 : 3];
    // SH_REPORT: the words of both queries' sinks ([0] this pass's, [1] the guest's), and the two LDS
    // histograms zeroed by every wave ahead of the barrier below, which every wave reaches
    uint64_t (*sh_report)[kReportWords] = nullptr;
    if constexpr (MODE == SH_REPORT) {
        sh_report = report_words_lds();
        hist_zero(hist_lds<2>(), 2 * (kHistMaxBins + 1) - 1);
    }
    if (threadIdx.x == 0) {
        const uint32_t dn =
            own_done ? __hip_atomic_load(own_done + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        uint32_t rdy = 0;
        if (slot && !dn && !(even_only && (blockIdx.x & 1)))
            rdy = __hip_atomic_load(&slot->ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (rdy) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            sh_guest[0] = (uint64_t)slot->frag;
            sh_guest[2] = (uint64_t)slot->done;
            if constexpr (MODE == SH_TOPK) {
                sh_guest[1] = (uint64_t)slot->sink.buf;
                sh_guest[3] = slot->sink.cap;
            } else if constexpr (MODE == SH_MATCH) {
                sh_guest[1] = (uint64_t)slot->sink.buf;
                sh_guest[3] = slot->sink.cap;
                sh_guest[4] = (uint64_t)slot->sink.count;
                sh_guest[5] = (uint64_t)__double_as_longlong(slot->sink.threshold);
            } else if constexpr (MODE == SH_REPORT) {
                // the guest's struct was complete in device memory before `ready` was published
                sh_guest[1] = 0;
                report_words_store(sh_report[1], (const ReportSinks *)slot->sink.buf);
            } else {
                sh_guest[1] = (uint64_t)slot->partials;
            }
        }
        if constexpr (MODE == SH_REPORT) {  // this pass's own: complete before its launch
            if (!dn) report_words_store(sh_report[0], (const ReportSinks *)out.buf);
        }
        sh_flag[0] = dn;
        sh_flag[1] = rdy;
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(sh_flag[0])) return;
    const bool shared = __builtin_amdgcn_readfirstlane(sh_flag[1]) != 0;
    const int lane = threadIdx.x & 63;
    const int wslot = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: kept in SGPRs
    const uint64_t tw = ((uint64_t)blockIdx.x * kWaveSlots + wslot) * kMfmaTiles;
    auto uniform64 = [](uint64_t v) {  // the builtin returns int: each half goes through uint32_t, unextended
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
        return (uint64_t)hi << 32 | lo;
    };
    constexpr int kRounds = kMfmaTiles / 2;
    __shared__ FragRing sh_ring;  // the two-query rounds' operands (static: a solo workgroup holds it too)
    typedef __attribute__((address_space(1))) uint32_t *GlobalWord;
    if constexpr (MODE == SH_REPORT) {
        const uint64_t unit = (uint64_t)blockIdx.x * kWaveSlots + wslot;
        uint32_t *const hist = hist_lds<2>();  // query qi's: hist + qi * (kHistMaxBins + 1), over both rounds
        if (!shared) {
            const GlobalFrag qf[1] = {(GlobalFrag)qfrag};
            share_round<1, kMfmaTiles>(db, qf, tile0, ntiles, tw, lane, [&](const auto &den, const auto &s) {
                const GlobalReport r = report_words_load(sh_report[0]);
                Partial list = partial_none();
                round_report<kMfmaTiles>(r, hist, den[0], s[0], tile0, ntiles, tw, first, end, lane, list);
                if (report_has_topk(r)) topk_store_lists(r.topk, unit, lane, list);
            });
        } else {
            const GlobalFrag qf[2] = {(GlobalFrag)qfrag, (GlobalFrag)uniform64(sh_guest[0])};
            // a query's list waits in LDS while the next round streams, as SH_TOPK parks it; only one
            // of the two is in registers at a time, and each lane reads back the entry it wrote
            __shared__ Partial sh_list[kWaveSlots][2][64];
#pragma unroll
            for (int rd = 0; rd < kRounds; ++rd)
                staged_round<kStagedDepth>(db, qf, tile0, ntiles, tw + 2 * rd, lane, wslot, sh_ring,
                                           [&](const auto &den, const auto &s) {
#pragma unroll
                                               for (int qi = 0; qi < 2; ++qi) {
                                                   const GlobalReport r = report_words_load(sh_report[qi]);
                                                   Partial list = partial_none();
                                                   if (rd > 0 && report_has_topk(r)) list = sh_list[wslot][qi][lane];
                                                   round_report<2>(r, hist + qi * (kHistMaxBins + 1), den[qi], s[qi], tile0,
                                                                   ntiles, tw + 2 * rd, first, end, lane, list);
                                                   if (report_has_topk(r)) {
                                                       if (rd + 1 < kRounds) sh_list[wslot][qi][lane] = list;
                                                       else topk_store_lists(r.topk, unit, lane, list);
                                                   }
                                               }
                                           });
        }
        // the histograms, once, after the last round: behind a barrier under a workgroup-uniform test
        const GlobalReport own = report_words_load(sh_report[0]);
        GlobalReport guest = own;
        if (shared) guest = report_words_load(sh_report[1]);
        const bool own_hist = report_has_hist(own), guest_hist = shared && report_has_hist(guest);
        if (own_hist || guest_hist) {
            __syncthreads();
            if (own_hist) hist_flush(hist, own.nbins, own.hist + (uint64_t)(blockIdx.x & own.copy_mask) * (own.nbins + 1));
            if (guest_hist)
                hist_flush(hist + (kHistMaxBins + 1), guest.nbins,
                           guest.hist + (uint64_t)(blockIdx.x & guest.copy_mask) * (guest.nbins + 1));
        }
        if (shared) {
            const GlobalWord guest_done = (GlobalWord)uniform64(sh_guest[2]);
            __syncthreads();  // every wave has fed the guest's sinks: only then is its tile group done
            if (threadIdx.x == 1) {
                __hip_atomic_store(guest_done + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (count) atomicAdd(count, 1ull);
            }
        }
    } else if constexpr (MODE == SH_TOPK) {
        const uint64_t unit = (uint64_t)blockIdx.x * kWaveSlots + wslot;
        const GlobalLists own{(GlobalPartial)out.buf, (uint32_t)out.cap};
        if (!shared) {
            const GlobalFrag qf[1] = {(GlobalFrag)qfrag};
            const uint32_t k[1] = {own.k};
            Partial list[1] = {partial_none()};
            share_round<1, kMfmaTiles>(db, qf, tile0, ntiles, tw, lane, [&](const auto &den, const auto &s) {
                round_topk<1, kMfmaTiles>(den, s, tile0, ntiles, tw, first, end, lane, k, list);
            });
            topk_store_lists(own, unit, lane, list[0]);
            return;
        }
        const GlobalFrag qf[2] = {(GlobalFrag)qfrag, (GlobalFrag)uniform64(sh_guest[0])};
        const GlobalLists guest{(GlobalPartial)uniform64(sh_guest[1]),
                                (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)sh_guest[3])};
        const GlobalWord guest_done = (GlobalWord)uniform64(sh_guest[2]);
        const uint32_t k[2] = {own.k, guest.k};
        // the two lists wait in LDS while the next round streams (resident, their 10 VGPRs spill:
        // 256 VGPRs and 12 B of scratch); each lane reads back the entry it wrote, so no barrier
        __shared__ Partial sh_list[kWaveSlots][2][64];
        Partial list[2] = {partial_none(), partial_none()};
#pragma unroll
        for (int rd = 0; rd < kRounds; ++rd) {
            staged_round<kStagedDepth>(db, qf, tile0, ntiles, tw + 2 * rd, lane, wslot, sh_ring,
                                       [&](const auto &den, const auto &s) {
                                           if (rd > 0) {
                                               list[0] = sh_list[wslot][0][lane];
                                               list[1] = sh_list[wslot][1][lane];
                                           }
                                           round_topk<2, 2>(den, s, tile0, ntiles, tw + 2 * rd, first, end, lane, k, list);
                                       });
            if (rd + 1 < kRounds) {
                sh_list[wslot][0][lane] = list[0];
                sh_list[wslot][1][lane] = list[1];
            }
        }
        topk_store_lists(own, unit, lane, list[0]);
        topk_store_lists(guest, unit, lane, list[1]);
        __syncthreads();  // every wave has stored the guest's list: only then is its tile group done
        if (threadIdx.x == 1) {
            __hip_atomic_store(guest_done + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (count) atomicAdd(count, 1ull);
        }
    } else if constexpr (MODE == SH_MATCH) {
        typedef __attribute__((address_space(1))) uint64_t *GlobalCount;
        const GlobalSink own{(GlobalPartial)out.buf, out.cap, (GlobalCount)out.count, out.threshold};
        if (!shared) {
            const GlobalFrag qf[1] = {(GlobalFrag)qfrag};
            const GlobalSink sink[1] = {own};
            share_round<1, kMfmaTiles>(db, qf, tile0, ntiles, tw, lane, [&](const auto &den, const auto &s) {
                round_matches<1, kMfmaTiles>(den, s, tile0, ntiles, tw, first, end, lane, sink);
            });
            return;
        }
        const GlobalFrag qf[2] = {(GlobalFrag)qfrag, (GlobalFrag)uniform64(sh_guest[0])};
        const GlobalSink sink[2] = {own, GlobalSink{(GlobalPartial)uniform64(sh_guest[1]), uniform64(sh_guest[3]),
                                                    (GlobalCount)uniform64(sh_guest[4]),
                                                    __longlong_as_double((long long)uniform64(sh_guest[5]))}};
        const GlobalWord guest_done = (GlobalWord)uniform64(sh_guest[2]);
#pragma unroll
        for (int rd = 0; rd < kRounds; ++rd)
            staged_round<kStagedDepth>(db, qf, tile0, ntiles, tw + 2 * rd, lane, wslot, sh_ring,
                                       [&](const auto &den, const auto &s) {
                                           round_matches<2, 2>(den, s, tile0, ntiles, tw + 2 * rd, first, end, lane, sink);
                                       });
        __syncthreads();  // every wave has appended for the guest: only then is its tile group done
        if (threadIdx.x == 1) {
            __hip_atomic_store(guest_done + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (count) atomicAdd(count, 1ull);
        }
    } else {
        __shared__ Partial sh_best[2 * kRounds * kWaveSlots];
        if (!shared) {
            Partial best[1] = {partial_none()};
            const GlobalFrag qf[1] = {(GlobalFrag)qfrag};
            share_round<1, kMfmaTiles>(db, qf, tile0, ntiles, tw, lane, [&](const auto &den, const auto &s) {
                round_candidates<1, kMfmaTiles>(den, s, tile0, ntiles, tw, first, end, lane, best);
            });
            share_stash<1, kWaveSlots>(best, lane, wslot, sh_best);
            const GlobalPartial o[1] = {(GlobalPartial)out};
            share_finish<1, kWaveSlots>(sh_best, o);
            return;
        }
        const GlobalFrag qf[2] = {(GlobalFrag)qfrag, (GlobalFrag)uniform64(sh_guest[0])};
#pragma unroll  // two copies of the loop: kept as a loop, the round counter and tile numbers spill
        for (int rd = 0; rd < kRounds; ++rd) {
            Partial best[2] = {partial_none(), partial_none()};
            staged_round<kStagedDepth>(db, qf, tile0, ntiles, tw + 2 * rd, lane, wslot, sh_ring,
                                       [&](const auto &den, const auto &s) {
                                           round_candidates<2, 2>(den, s, tile0, ntiles, tw + 2 * rd, first, end, lane, best);
                                       });
            share_stash<2, kRounds * kWaveSlots>(best, lane, rd * kWaveSlots + wslot, sh_best);
        }
        const GlobalPartial o[2] = {(GlobalPartial)out, (GlobalPartial)uniform64(sh_guest[1])};
        const GlobalWord guest_done = (GlobalWord)uniform64(sh_guest[2]);
        share_finish<2, kRounds * kWaveSlots>(sh_best, o);
        if (threadIdx.x == 1) {  // the thread that stored the guest's partial
            __hip_atomic_store(guest_done + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (count) atomicAdd(count, 1ull);
        }
    }
}

__global__ void share_prepare_kernel(GuestSlot *slot, uint32_t *done, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *slot = GuestSlot{};
    if (done && i < n) done[i] = 0;
}

__global__ void share_publish_kernel(GuestSlot *slot, const void *frag, Partial *partials, uint32_t *done) {
    slot->frag = frag;
    slot->partials = partials;
    slot->done = done;
    __hip_atomic_store(&slot->ready, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// a match or top-k pass's registration: the guest's sink (a top-k pass: topk_sink(lists, k)) in place
// of its partials
__global__ void share_publish_match_kernel(GuestSlot *slot, const void *frag, MatchSink sink, uint32_t *done) {
    slot->frag = frag;
    slot->sink = sink;
    slot->done = done;
    __hip_atomic_store(&slot->ready, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// a report pass's own preparation: its ReportSinks stored in device memory (thread 0) and the
// `words` counters behind `zero` cleared -- the histogram's copies and the match counter
__global__ void __launch_bounds__(256) report_prepare_kernel(ReportSinks *dst, ReportSinks sinks, uint64_t *zero,
                                                             uint64_t words) {
    const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 == 0) *dst = sinks;
    for (uint64_t i = i0; i < words; i += (uint64_t)gridDim.x * blockDim.x) zero[i] = 0;
}

__global__ void share_delay_kernel(uint64_t ticks) {
    const uint64_t t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// ------------------------------------------------------------------ TILES layout plumbing
// (declared in iris_device.hpp; launch_*_tiles_kind, iris_engines_mfma.hip, launches these three on
// grid_stride_blocks(n * 2 * kPlaneGroups) workgroups of 256, the `total` of their loops)

// reference Template record (pattern dwords 0..399, mask dwords 400..799) ->
// TILES uint4 of (record t, chunk pair g, half h)
__global__ void __launch_bounds__(256) pack_tiles_kernel(const uint32_t *__restrict__ staging,
                                                         uint4 *__restrict__ db, uint64_t t_first, uint64_t n) {
    const uint64_t total = n * (uint64_t)(2 * kPlaneGroups);
    for (uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; tid < total;
         tid += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = tid % n, gh = tid / n;
        const int g = (int)(gh >> 1), h = (int)(gh & 1);
        const uint32_t *rec = staging + i * (2 * kPlaneDwords);
        const int w0 = 4 * g + h, w1 = 4 * g + 2 + h;
        const uint32_t em0 = rec[kPlaneDwords + w0], ep0 = rec[w0], em1 = rec[kPlaneDwords + w1], ep1 = rec[w1];
        const uint64_t t = t_first + i;
        uint4 v;
        v.x = xpack(em0 & 0xFFFFu, ep0 & 0xFFFFu);
        v.y = xpack(em0 >> 16, ep0 >> 16);
        v.z = xpack(em1 & 0xFFFFu, ep1 & 0xFFFFu);
        v.w = xpack(em1 >> 16, ep1 >> 16);
        db[(t / kTile) * (uint64_t)kTileUint4 + (uint64_t)g * 64 + (t % kTile) + 32 * h] = v;
    }
}

__global__ void __launch_bounds__(256) unpack_tiles_kernel(const uint4 *__restrict__ db, uint32_t *__restrict__ staging,
                                                           uint64_t t_first, uint64_t n) {
    const uint64_t total = n * (uint64_t)(2 * kPlaneGroups);
    for (uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; tid < total;
         tid += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = tid % n, gh = tid / n;
        const int g = (int)(gh >> 1), h = (int)(gh & 1);
        const uint64_t t = t_first + i;
        const uint4 v = db[(t / kTile) * (uint64_t)kTileUint4 + (uint64_t)g * 64 + (t % kTile) + 32 * h];
        uint32_t a, b, c, d;
        xunpack(v.x, a, b);
        xunpack(v.y, c, d);
        uint32_t *rec = staging + i * (2 * kPlaneDwords);
        const int w0 = 4 * g + h, w1 = 4 * g + 2 + h;
        rec[kPlaneDwords + w0] = a | (c << 16);
        rec[w0] = b | (d << 16);
        xunpack(v.z, a, b);
        xunpack(v.w, c, d);
        rec[kPlaneDwords + w1] = a | (c << 16);
        rec[w1] = b | (d << 16);
    }
}

__global__ void __launch_bounds__(256) generate_tiles_kernel(uint4 *__restrict__ db, uint64_t t_first, uint64_t n,
                                                             uint64_t key, uint64_t global_index0) {
    const uint64_t total = n * (uint64_t)(2 * kPlaneGroups);
    for (uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; tid < total;
         tid += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = tid % n, gh = tid / n;
        const int g = (int)(gh >> 1), h = (int)(gh & 1);
        const uint64_t gt = global_index0 + i;
        // dword 4g+h is half h of limb 2g, dword 4g+2+h half h of limb 2g+1
        const uint64_t m0 = gen_limb(key, gt * 400 + 200 + 2 * g), m1 = gen_limb(key, gt * 400 + 200 + 2 * g + 1);
        const uint64_t p0 = gen_limb(key, gt * 400 + 2 * g), p1 = gen_limb(key, gt * 400 + 2 * g + 1);
        const uint32_t em0 = (uint32_t)(m0 >> (32 * h)), ep0 = (uint32_t)(p0 >> (32 * h));
        const uint32_t em1 = (uint32_t)(m1 >> (32 * h)), ep1 = (uint32_t)(p1 >> (32 * h));
        const uint64_t t = t_first + i;
        uint4 v;
        v.x = xpack(em0 & 0xFFFFu, ep0 & 0xFFFFu);
        v.y = xpack(em0 >> 16, ep0 >> 16);
        v.z = xpack(em1 & 0xFFFFu, ep1 & 0xFFFFu);
        v.w = xpack(em1 >> 16, ep1 >> 16);
        db[(t / kTile) * (uint64_t)kTileUint4 + (uint64_t)g * 64 + (t % kTile) + 32 * h] = v;
    }
}

struct TileRange {
    uint64_t tile0, ntiles, grid;
    bool fusable;  // small enough for the search's in-kernel reduce
    int tiles_per_wave;
    int ksplit;  // 4: a tile's 4 waves split K (ranges of at most kSplitTiles tiles)
};

// Below this many tiles, 4 tiles per wave would leave CUs idle (fewer than 2
// workgroups per CU): small ranges run one tile per wave, 4x the workgroups.
constexpr uint64_t kSmallTiles = 4 * kWaveSlots * 256 * 2;
// Up to this many tiles (32k templates: configs[0]'s 10k, the reference's 20k-record chunks)
// even one tile per wave leaves most SIMDs without a wave: the 4 waves of a workgroup split
// one tile's K instead.
constexpr uint64_t kSplitTiles = 1024;

// The form and grid of every single-query pass: one workgroup per 16 tiles (a persistent grid
// measured slower), 4 tiles on small ranges, kSplitT under the K-split.
static TileRange tile_range(const Hooks &h, LaunchRange r) {
    TileRange t;
    t.tile0 = tile_span(r).tile0;
    t.ntiles = tile_span(r).ntiles;
    t.tiles_per_wave = t.ntiles < kSmallTiles ? 1 : kMfmaTiles;
    t.ksplit = t.ntiles <= kSplitTiles ? 4 : 1;
    // test hook: IRIS_TILES_PER_WAVE=1|4 pins the variant (tests run all three on small ranges:
    // unset = the K-split form there)
    if (h.tiles_per_wave) {
        t.tiles_per_wave = h.tiles_per_wave == 1 ? 1 : kMfmaTiles;
        t.ksplit = 1;
    }
    if (t.ksplit > 1) {
        t.tiles_per_wave = kSplitT;
        t.grid = (t.ntiles + kSplitT - 1) / kSplitT;  // kSplitT tiles per workgroup
    } else {
        const uint64_t waves = (t.ntiles + t.tiles_per_wave - 1) / t.tiles_per_wave;
        t.grid = (waves + kWaveSlots - 1) / kWaveSlots;
    }
    t.fusable = t.grid <= (uint64_t)kFusedReduceMax;
    return t;
}

// partial records a search writes
uint32_t mfma_search_partials(const Hooks &h, LaunchRange r) { return (uint32_t)tile_range(h, r).grid; }

// lists a top-k pass writes: one per wave that holds sums (a workgroup's one tile group under the K-split)
uint64_t mfma_topk_units(const Hooks &h, LaunchRange r) {
    const TileRange t = tile_range(h, r);
    return t.grid * (uint64_t)(t.ksplit > 1 ? 1 : kWaveSlots);
}

// test hook: IRIS_FUSED_REDUCE=0 runs small searches with the separate reduce kernel
bool fused_search_ok(const Hooks &h, LaunchRange r) { return h.fused_reduce && r.n != 0 && tile_range(h, r).fusable; }

bool share_search_ok(const Hooks &h, LaunchRange r) {
    if (r.n == 0 || fused_search_ok(h, r)) return false;
    const TileRange t = tile_range(h, r);
    return t.ksplit == 1 && t.tiles_per_wave == kMfmaTiles;
}

// The one dispatch of template_mfma_kernel: the K-split form on small ranges, else one or four
// tiles per wave; a search with a fused finish runs the FUSED instance of the same form.
template <int MODE>
static int mfma_pass(const Hooks &h, void *stream, const void *db, const void *qfrag, LaunchRange r, const PassOut &o,
                     uint32_t *n_partials, const FusedFinish *fin) {
    const TileRange t = tile_range(h, r);
    if (n_partials) *n_partials = (uint32_t)t.grid;  // an empty range's too
    if (r.n == 0) return 0;
    auto kern = t.ksplit > 1 ? template_mfma_kernel<MODE, kSplitT, 4>
                : t.tiles_per_wave == 1 ? template_mfma_kernel<MODE, 1> : template_mfma_kernel<MODE>;
    if (fin) {
        if (MODE != MF_SEARCH || !t.fusable) return -1;  // the caller asks fused_search_ok() first
        if constexpr (MODE == MF_SEARCH)
            kern = t.ksplit > 1 ? template_mfma_kernel<MODE, kSplitT, 4, true>
                   : t.tiles_per_wave == 1 ? template_mfma_kernel<MODE, 1, 1, true>
                                           : template_mfma_kernel<MODE, kMfmaTiles, 1, true>;
    }
    hipLaunchKernelGGL(kern, dim3((uint32_t)t.grid), dim3(64 * kWaveSlots), 0, (hipStream_t)stream,
                       (const uint4 *)db, (const uint4 *)qfrag, t.tile0, t.ntiles, r.first, r.first + r.n, o.num_out,
                       o.den_out, o.dist_out, o.partials, fin ? *fin : FusedFinish{}, o.sink);
    return check_launch();
}

int launch_template_mfma(Pass p, const Hooks &h, void *stream, const void *db, const void *qfrag, LaunchRange r,
                         const PassOut &o, uint32_t *n_partials, const FusedFinish *fin) {
    if (r.n != 0 && !o.fits(p)) return -1;
    switch (p) {
    case Pass::Counts: return mfma_pass<MF_COUNTS>(h, stream, db, qfrag, r, o, n_partials, fin);
    case Pass::Search: return mfma_pass<MF_SEARCH>(h, stream, db, qfrag, r, o, n_partials, fin);
    case Pass::Match: return mfma_pass<MF_MATCH>(h, stream, db, qfrag, r, o, n_partials, fin);
    case Pass::Topk: return mfma_pass<MF_TOPK>(h, stream, db, qfrag, r, o, n_partials, fin);
    case Pass::Hist: return mfma_pass<MF_HIST>(h, stream, db, qfrag, r, o, n_partials, fin);
    case Pass::Report: return mfma_pass<MF_REPORT>(h, stream, db, qfrag, r, o, n_partials, fin);
    }
    return -1;
}

// The one launch of template_share_kernel (tile_range's 4-tiles-per-wave grid; `out` is the
// partials array of a search and the sink of a match or a top-k pass).
template <int MODE>
static int share_pass(const Hooks &h, void *stream, const void *db, const void *qfrag, LaunchRange r, const PassOut &o,
                      uint32_t *n_partials, const GuestSlot *slot, const uint32_t *own_done, unsigned long long *count) {
    if (!share_search_ok(h, r)) return -1;  // the caller asks first
    const TileRange t = tile_range(h, r);
    if (n_partials) *n_partials = (uint32_t)t.grid;
    // test hook: a pass that is nobody's guest carries its guest in even tile groups only (the
    // guest's own launch then computes the odd ones, and carries its own guest there)
    const bool even_only = h.search_share_even && !own_done;
    std::conditional_t<MODE == SH_SEARCH, Partial *, MatchSink> out;
    if constexpr (MODE == SH_SEARCH) out = o.partials;
    else out = o.sink;
    hipLaunchKernelGGL(template_share_kernel<MODE>, dim3((uint32_t)t.grid), dim3(64 * kWaveSlots), 0,
                       (hipStream_t)stream, (const uint4 *)db, (const uint4 *)qfrag, t.tile0, t.ntiles, r.first,
                       r.first + r.n, out, slot, own_done, count, (uint32_t)even_only);
    return check_launch();
}

int launch_template_share(Pass p, const Hooks &h, void *stream, const void *db, const void *qfrag, LaunchRange r,
                          const PassOut &o, uint32_t *n_partials, const GuestSlot *slot, const uint32_t *own_done,
                          unsigned long long *count) {
    if (!o.fits(p)) return -1;
    switch (p) {
    case Pass::Search: return share_pass<SH_SEARCH>(h, stream, db, qfrag, r, o, n_partials, slot, own_done, count);
    case Pass::Match: return share_pass<SH_MATCH>(h, stream, db, qfrag, r, o, n_partials, slot, own_done, count);
    case Pass::Topk: return share_pass<SH_TOPK>(h, stream, db, qfrag, r, o, n_partials, slot, own_done, count);
    case Pass::Report: return share_pass<SH_REPORT>(h, stream, db, qfrag, r, o, n_partials, slot, own_done, count);
    default: return -1;  // counts have no sharing form; a histogram's is a report pass of that part alone
    }
}

int launch_share_prepare(void *stream, GuestSlot *slot, uint32_t *done, uint32_t n) {
    const uint32_t words = done ? (n ? n : 1) : 1;
    hipLaunchKernelGGL(share_prepare_kernel, dim3((words + 255) / 256), dim3(256), 0, (hipStream_t)stream, slot, done, n);
    return check_launch();
}

int launch_share_publish(void *stream, GuestSlot *slot, const void *frag, Partial *partials, uint32_t *done) {
    hipLaunchKernelGGL(share_publish_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, slot, frag, partials, done);
    return check_launch();
}

int launch_share_publish_match(void *stream, GuestSlot *slot, const void *frag, const MatchSink &sink, uint32_t *done) {
    hipLaunchKernelGGL(share_publish_match_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, slot, frag, sink, done);
    return check_launch();
}

int launch_report_prepare(void *stream, ReportSinks *dst, const ReportSinks &sinks, uint64_t *zero, uint64_t words) {
    hipLaunchKernelGGL(report_prepare_kernel, dim3((uint32_t)grid_stride_blocks(words ? words : 1)), dim3(256), 0,
                       (hipStream_t)stream, dst, sinks, zero, words);
    return check_launch();
}

int launch_share_delay(void *stream, uint64_t ticks) {
    hipLaunchKernelGGL(share_delay_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, ticks);
    return check_launch();
}

uint32_t multi_search_partials(LaunchRange r, int nq) {
    const uint64_t waves = (tile_span(r).ntiles + (4 / nq) - 1) / (4 / nq);
    return (uint32_t)((waves + kWaveSlots - 1) / kWaveSlots);
}

int launch_template_multi_search(void *stream, const void *db, const void *const *qfrags, int nq, LaunchRange r,
                                 Partial *partials, uint32_t *n_partials) {
    *n_partials = multi_search_partials(r, nq);
    if (r.n == 0) return 0;
    if (nq != 2) return -1;
    const TileSpan t = tile_span(r);
    QueryFrags qf{};
    for (int i = 0; i < nq; ++i) qf.q[i] = (const uint4 *)qfrags[i];
    hipLaunchKernelGGL(template_multi_kernel<2>, dim3(*n_partials), dim3(256), 0, (hipStream_t)stream,
                       (const uint4 *)db, qf, t.tile0, t.ntiles, r.first, r.first + r.n, partials);
    return check_launch();
}

}  // namespace iris
