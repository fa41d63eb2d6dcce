// iris_internal.hpp — device layouts, generator and launch declarations shared
// by the HIP kernels (iris_kernels.hip) and the C ABI (iris_api*.hip).
//
// Device layout: records are grouped in blocks of 64 — one
// record per lane of a wavefront — and each block stores, for every 16-byte
// group g of a record plane, the 64 lanes' 16 bytes contiguously (1 KiB).
// One `global_load_dwordx4` of a wave therefore reads 1 KiB fully coalesced,
// and every lane holds word 4g..4g+3 of its own record: the rotated query
// words are then wave-uniform and live in SGPRs (no LDS, no cross-lane
// reduction).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <sys/types.h>

#include "../../include/iris_hip.h"

#if defined(__HIPCC__)
#define IRIS_HD __host__ __device__
#else
#define IRIS_HD
#endif

namespace iris {

constexpr int kLanes = 64;            // records per block (= wavefront width)
constexpr int kRot = IRIS_ROTATIONS;  // 31
constexpr int kWaveSlots = 4;         // waves per workgroup (256 threads)

// dwords of one record plane (12800 bits) and its 16-byte groups
constexpr int kPlaneDwords = IRIS_BITS / 32;     // 400
constexpr int kPlaneGroups = kPlaneDwords / 4;   // 100
constexpr int kShareDwords = IRIS_BITS / 2;      // 6400 (two u16 per dword)
constexpr int kShareGroups = kShareDwords / 4;   // 1600

// Device layouts.
//  LANES (VALU kernels): blocks of 64 records, one per lane; for each 16-byte
//    group G of a record the 64 lanes' 16 B are contiguous (1 KiB):
//      TEMPLATES: G = 2*g + p, p = 0 mask plane, p = 1 pattern plane  (200 groups)
//      MASKS:     G = g                                               (100 groups)
//      SHARES:    G = g                                               (1600 groups)
//  TILES (MFMA kernels, TEMPLATES only): tiles of 32 records.  For chunk pair
//    g (template bits [128g, 128g+128) of both planes) lane L = t + 32h holds
//    one uint4 {X0(2g,h), X1(2g,h), X0(2g+1,h), X1(2g+1,h)}: the interleaved
//    mask/pattern bits of plane dword w = 2c + h (see xpack below), which is
//    exactly the fp4 B-operand fragment source of lane L for chunk c.
struct KindInfo {
    int kind;
    int layout;         // IRIS_LAYOUT_LANES or IRIS_LAYOUT_TILES
    int block;          // records per block (64 lanes or 32-record tiles)
    int groups;         // 16-byte groups per record (LANES) / per lane (TILES)
    int planes;         // planes interleaved per g (LANES)
    int rec_dwords;     // dwords per record in the reference layout
    int plane_src[2];   // dword offset of plane p inside the reference record
    size_t rec_bytes;   // bytes per reference record
};

inline KindInfo kind_info(int kind, int layout = IRIS_LAYOUT_LANES) {
    switch (kind) {
    case IRIS_KIND_TEMPLATES:
        if (layout == IRIS_LAYOUT_TILES) return {kind, layout, 32, kPlaneGroups, 2, 2 * kPlaneDwords, {kPlaneDwords, 0}, 3200};
        return {kind, IRIS_LAYOUT_LANES, 64, 2 * kPlaneGroups, 2, 2 * kPlaneDwords, {kPlaneDwords, 0}, 3200};
    case IRIS_KIND_MASKS:
        if (layout == IRIS_LAYOUT_TILES) return {kind, layout, 32, kPlaneGroups / 2, 1, kPlaneDwords, {0, 0}, 1600};
        return {kind, IRIS_LAYOUT_LANES, 64, kPlaneGroups, 1, kPlaneDwords, {0, 0}, 1600};
    case IRIS_KIND_SHARES:
        if (layout == IRIS_LAYOUT_TILES) return {kind, layout, 32, kShareDwords / 16, 2, kShareDwords, {0, 0}, 25600};
        return {kind, IRIS_LAYOUT_LANES, 64, kShareGroups, 1, kShareDwords, {0, 0}, 25600};
    default: return {0, 0, 0, 0, 0, 0, {0, 0}, 0};
    }
}

inline size_t block_bytes(const KindInfo &k) { return (size_t)k.block * k.rec_bytes; }

// TILES interleave of 16 mask bits and 16 pattern bits into one dword:
//   nibble p: bit0 = em[2p+1], bit1 = em[2p], bit2 = ep[2p+1], bit3 = ep[2p]
// so that (x & 0xAAAAAAAA) and ((x+x) & 0xAAAAAAAA) are fp4 e2m1 values
// {0, +1, -1} = encode() of K positions 2p and 2p+1, and (x & 0x22222222),
// (x & 0x11111111) are the mask bits as fp4 1.0 and 0.5.
IRIS_HD inline uint32_t xpack(uint32_t em16, uint32_t ep16) {
    uint32_t x = 0;
    for (int p = 0; p < 8; ++p) {
        x |= ((em16 >> (2 * p + 1)) & 1u) << (4 * p);
        x |= ((em16 >> (2 * p)) & 1u) << (4 * p + 1);
        x |= ((ep16 >> (2 * p + 1)) & 1u) << (4 * p + 2);
        x |= ((ep16 >> (2 * p)) & 1u) << (4 * p + 3);
    }
    return x;
}
IRIS_HD inline void xunpack(uint32_t x, uint32_t &em16, uint32_t &ep16) {
    em16 = 0;
    ep16 = 0;
    for (int p = 0; p < 8; ++p) {
        em16 |= ((x >> (4 * p)) & 1u) << (2 * p + 1);
        em16 |= ((x >> (4 * p + 1)) & 1u) << (2 * p);
        ep16 |= ((x >> (4 * p + 2)) & 1u) << (2 * p + 1);
        ep16 |= ((x >> (4 * p + 3)) & 1u) << (2 * p);
    }
}
// fp4 K index j (0..31) of a lane's fragment <-> bit of the lane's plane dword
IRIS_HD inline int frag_bit(int j) { return (j & 16) + 2 * (j & 7) + ((j >> 3) & 1); }

// MFMA query fragments: for chunk c (template bits [64c, 64c+64)) and lane
// L = k + 32h (k = rotation index 0..30, 31 = zero row), one uint4 at
// [c * 64 + L]: fp4 e2m1 of encode(q rotated by k - 15) at bit frag_bit(j) of
// plane dword 2c + h (+1.0 = 0x2, -1.0 = 0xA, 0).  The den operand is derived
// from it in-kernel (|enc|, doubled where the template side carries 0.5).
constexpr int kFragDwords = 4;

// TILES layouts of the other kinds (iris_mfma.hip):
//  MASKS  (fp4, den only): tile of 32 masks = 3200 uint4.  uint4 [g*64 + L]
//    (g = 0..49, L = t + 32h) = mask dwords {8g+h, 8g+2+h, 8g+4+h, 8g+6+h}, i.e.
//    the lane's dword of chunks 4g..4g+3.  Fragment dword d of a chunk is
//    x & (0x11111111 << d) for d < 3 and (x >> 1) & 0x44444444 for d = 3, so
//    K index j <-> mask bit 4 (j % 8) + j / 8 with template-side value
//    0.5 / 1 / 2 / 2 and query-side value 2 / 1 / 0.5 / 0.5.
//  SHARES (i8): tile of 32 shares = 51200 uint4.  For chunk c (elements
//    [32c, 32c+32)) and lane L = t + 32h: uint4 [(2c) * 64 + L] = low bytes,
//    [(2c+1) * 64 + L] = high bytes of elements 32c + 16h + j (j = 0..15), each
//    XOR 0x80 (the byte minus 128 as an i8), the B fragment of
//    v_mfma_i32_32x32x32_i8 (lane l holds K = 16 (l >> 5) + j).
constexpr int kMaskTileUint4 = (kPlaneGroups / 2) * 64;   // 3200
constexpr int kShareTileUint4 = (kShareDwords / 16) * 2 * 64;  // 51200
constexpr int kMaskChunks = kPlaneDwords / 2;   // 200 chunks of 64 bits
constexpr int kShareChunks = IRIS_BITS / 32;    // 400 chunks of 32 elements
// masks A-fragments, one bit per fp4 element: uint4 [step g = 50][lane 64], one
// dword per chunk 4g + i; element j of a lane's 32 is bit 4 (j & 7) + {2, 1, 0, 3}[j >> 3]
constexpr size_t kMaskFragUint4 = (size_t)(kMaskChunks / 4) * 64;
constexpr size_t kShareFragUint4 = (size_t)kShareChunks * 64 * 2;  // + 32 int2 row constants after it
IRIS_HD inline int mask_frag_bit(int j) { return 4 * (j & 7) + (j >> 3); }
constexpr size_t kTemplateFragDwords = (size_t)(kPlaneDwords / 2) * 64 * kFragDwords;  // 200 chunks

// Rotated-query tables (built once per engine, on the device by iris_query.hip;
// the host builders below are their reference):
//   TEMPLATES: dword [w*64 + 2k] = mask_k word w, [w*64 + 2k+1] = pattern_k word w   (400 x 64)
//   MASKS:     dword [w*32 + k]  = mask_k word w                                      (400 x 32)
//   SHARES:    dword [d*32 + k]  = rot_k[2d] | rot_k[2d+1] << 16                       (6400 x 32)
// k = 0..30 is rotation r = k - 15; slot 31 (and 62, 63) is zero.
constexpr int kTemplateTabStride = 64;
constexpr int kSlotTabStride = 32;

// Per-workgroup partial result of a search (24 B).
struct Partial {
    uint32_t num;
    uint32_t den;   // 0 = no candidate
    int32_t rot;    // k index 0..30
    uint32_t pad;
    uint64_t idx;   // template index relative to the searched range start
};

// Where a threshold-match pass appends its hits (iris_*_matches): every record whose best
// fraction num / den, divided in f64, is below `threshold` takes the next slot of `count` and,
// if that slot is inside `cap`, stores one Partial {num, den, rot, idx = range-relative index}
// at buf[slot].  The counter always counts, so a short buffer still yields the exact total.
struct MatchSink {
    Partial *buf;
    uint64_t cap;      // records buf holds
    uint64_t *count;   // device counter, zeroed on the stream before the launch
    double threshold;  // never NaN (the API refuses it)
};
// A top-k pass (iris_*_topk) takes the same struct, so the kernels keep one signature:
// buf = lists[units][k], cap = k (1..kTopkMax); count and threshold are unused.  Every unit (a
// wave that can hold candidates) stores its k best records, best first, empty entries (den = 0)
// last, at buf[unit * k + j]; launch_topk_merge then folds the lists.
constexpr uint32_t kTopkMax = 64;    // one list entry per lane
constexpr uint32_t kTopkFanIn = 64;  // lists one merge workgroup folds into one
inline MatchSink topk_sink(Partial *lists, uint32_t k) { return MatchSink{lists, k, nullptr, 0.0}; }
// A histogram pass (iris_*_histogram) takes it as well: count = counters[copies][nbins + 1], u64,
// zeroed on the stream before the launch, and cap = nbins | (copies - 1) << 32 (both powers of two);
// buf and threshold are unused.  A workgroup bins its records in LDS (bin = min(nbins - 1,
// num * nbins / den) of the best rotation, integers: num * nbins < 2^25, hist_count) and adds its non-zero
// words to copy blockIdx.x % copies: words 0 .. nbins - 1 the bins, word nbins the records without
// a valid rotation.  copies = 1 is the result itself; launch_hist_reduce sums more.
constexpr uint32_t kHistMaxBins = IRIS_HIST_MAX_BINS;
constexpr uint32_t kHistCopies = 64;  // the flush and its measurement
inline MatchSink hist_sink(uint64_t *counters, uint32_t nbins, uint32_t copies) {
    return MatchSink{nullptr, (uint64_t)nbins | (uint64_t)(copies - 1) << 32, counters, 0.0};
}
// whether s is a hist_sink the kernels' LDS histograms hold: counters, nbins a power of two up to kHistMaxBins
inline bool hist_sink_ok(const MatchSink &s) {
    const uint32_t nbins = (uint32_t)s.cap;
    return s.count && nbins >= 1 && nbins <= kHistMaxBins && (nbins & (nbins - 1)) == 0;
}
// A report pass (iris_template_report, iris_resolver_report*) feeds all three from one read of the database: a small DEVICE
// struct holds the three sinks and the pass's MatchSink points at it (report_sink: buf; the other
// fields are unused), so the kernels keep their signature and read the sinks once, after their K
// loop.  A part the call did not select is absent: match.count null, topk.cap 0, hist.count null.
struct ReportSinks {
    MatchSink match, topk, hist;
};
inline MatchSink report_sink(const ReportSinks *device_sinks) { return MatchSink{(Partial *)device_sinks, 0, nullptr, 0.0}; }

// ---------------------------------------------------------------- generator
// Counter-based synthetic data: limb = splitmix64 output number
// ctr+1 of the stream keyed by (seed, stream).  Templates: stream 0, pattern
// limb j of template t = ctr t*400 + j, mask limb j = ctr t*400 + 200 + j.
// Shares: stream 1, limb j of record t = ctr t*3200 + j (4 LE u16 per limb).
IRIS_HD inline uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
IRIS_HD inline uint64_t gen_key(uint64_t seed, uint64_t stream) {
    return mix64(seed ^ (0xD1B54A32D192ED03ULL * (stream + 1)));
}
IRIS_HD inline uint64_t gen_limb(uint64_t key, uint64_t ctr) {
    return mix64(key + (ctr + 1) * 0x9E3779B97F4A7C15ULL);
}

// ---------------------------------------------------------------- runtime configuration
// Environment knobs are read once, when a device opens (read_hooks, iris_host.cpp), into that
// device's Hooks; launchers take them from there, never from the environment.  The test-only
// hooks pin kernel variants or inject delays and faults: they are honoured only when
// IRIS_TEST_HOOKS=1 is also set, and otherwise ignored (iris_config reports both).
struct Hooks {
    // production knobs
    bool readahead = true;           // IRIS_READAHEAD=0: no read-ahead of host-output engine calls
    bool auto_resident = true;       // IRIS_AUTO_RESIDENT=0: host slices of read-only file mappings upload per call
    uint32_t group_timeout_ms = 0;   // IRIS_GROUP_TIMEOUT_MS: bound of a group exchange wait (0: auto)
    uint32_t resident_max_mb = 0;    // IRIS_RESIDENT_MAX_MB: resident file copies hold at most this (0: half the device)
    // test-only hooks (IRIS_TEST_HOOKS=1)
    bool test = false;
    int tiles_per_wave = 0;          // IRIS_TILES_PER_WAVE=1|4: pins the TILES kernels' variant (0: by range)
    bool fused_reduce = true;        // IRIS_FUSED_REDUCE=0: small searches launch the separate reduce
    int batch_kernel = 4;            // IRIS_BATCH_KERNEL=2|4: batched-query kernel shape (iris_batch.hip)
    int schedule = 0;                // IRIS_SCHEDULE=spin|yield|blocking (1|2|3): host wait mode
    bool load_pread = false;         // IRIS_LOAD_PREAD=1: file loads through the pinned-buffer path
    bool load_windows = false;       // IRIS_LOAD_WINDOWS=1: file loads DMA from registered page-cache windows
    uint32_t group_delay_us = 0;     // IRIS_GROUP_DELAY_US: side-stream spin before each group all-gather
    bool group_stall = false;        // IRIS_GROUP_STALL=1: a group all-gather waits on a peer that never comes
    bool group_unordered = false;    // IRIS_GROUP_UNORDERED=1: drop the exchange-buffer ordering (shows the race)
    int upload = 0;                  // IRIS_UPLOAD=pinned|runtime (1|2): the path of writes >= 8 MB (0: the faster lately)
    uint32_t ra_window = 0;          // IRIS_READAHEAD_WINDOW=1..64: chunks per read-ahead window (0: growing)
    uint32_t resident_budget_mb = 0; // IRIS_RESIDENT_BUDGET_MB: resident copies hold at most this (0: free memory)
    bool ra_packed = true;           // IRIS_READAHEAD_PACKED=0: masks read-ahead rows cross the host link unpacked
    uint32_t ra_window_max = 0;      // IRIS_READAHEAD_WINDOW_MAX=1..1024: cap of a read-ahead window, chunks (0: by records)
    bool search_share = true;        // IRIS_SEARCH_SHARE=0: asynchronous searches, match and top-k passes never register as guests
    uint32_t search_share_delay_us = 0;  // IRIS_SEARCH_SHARE_DELAY_US: device-stream spin ahead of a pass that can host
    bool search_share_even = false;  // IRIS_SEARCH_SHARE_EVEN=1: a pass that is nobody's guest sees no guest in odd tile groups
    uint32_t hist_copies = 0;        // IRIS_HIST_COPIES=1|2|..|64: counter copies of a histogram pass (0: kHistCopies; 1: straight into the result)
    uint32_t ignored = 0;            // bit i: test hook kHookNames[i] was set without IRIS_TEST_HOOKS=1
};
// The bound of forming a device group when IRIS_GROUP_TIMEOUT_MS is not set (iris_group.hip)
constexpr uint32_t kGroupInitTimeoutMs = 120000;
// Reads the environment (the Hooks a device opened now gets).
void read_hooks(Hooks *h);
// "key=value ..." of h plus the process-wide knobs (IRIS_COPY_HELPERS); returns the length.
size_t format_hooks(const Hooks &h, char *buf, size_t len);

// ---------------------------------------------------------------- launchers
// All asynchronous on `stream`; 0, or -1 for a refused argument or a failed launch.  Grouped by
// kernel family: a family's launcher sits with the functions that size its outputs (*_partials,
// *_units), the predicates its callers ask first (*_ok) and its operand structs.
struct LaunchRange {
    uint64_t first;  // first record index of the range
    uint64_t n;      // records in the range
};
// The 32-record tiles of a TILES database that a range touches: its first tile and their number
// (the first and the last may be partial).  iris_host.cpp: plain host code, tested on the CPU.
struct TileSpan {
    uint64_t tile0, ntiles;
};
TileSpan tile_span(LaunchRange r);
// Up to this many tiles a range runs its engine's K-split form, single-query and batched alike
// (the resolver's and the participants' 20 000-record chunks are 625 tiles).
constexpr uint64_t kMasksSplitTiles = 1024;
constexpr uint64_t kSharesSplitTiles = 4096;

// What a pass over a range does with each record's best rotation.  A family's launcher takes the
// pass as a value and picks its kernel's own mode constant; one it has no kernel for is refused.
//   Counts: the 31 numerators and denominators of every record
//   Search: the closest record -- one Partial per workgroup, which a reduce folds -- and,
//           if asked, every record's distance
//   Match:  every record under a threshold, appended to a MatchSink
//   Topk:   the k closest records of every unit (a wave that holds candidates), into topk_sink lists
//   Hist:   the distribution of the distances, into hist_sink counters
//   Report: Match, Topk and Hist together -- those of them its ReportSinks hold -- from one read
//           (the single-query template kernels, the fused masks kernel and the resolver kernel)
enum class Pass { Counts, Search, Match, Topk, Hist, Report };

// The operands of a single-query pass; what its mode does not write stays null.
struct PassOut {
    uint16_t *num_out = nullptr, *den_out = nullptr;  // Counts: [n][31] each (either may be null)
    double *dist_out = nullptr;                       // Search: null, or n distances
    Partial *partials = nullptr;                      // Search: the family's *_partials() records
    MatchSink sink{};                                 // Match, Topk, Hist: counters zeroed on the stream by the caller
                                                      // Report: report_sink of the device struct of the three
    PassOut(uint16_t *num, uint16_t *den) : num_out(num), den_out(den) {}
    PassOut(double *dist, Partial *parts) : dist_out(dist), partials(parts) {}
    PassOut(const MatchSink &s) : sink(s) {}
    PassOut(const ReportSinks *device_sinks) : sink(report_sink(device_sinks)) {}
    // whether the operands are the ones mode p writes (the launchers refuse a pass whose are not)
    bool fits(Pass p) const {
        const bool counts = num_out || den_out, search = partials || dist_out;
        return p == Pass::Counts ? !search : p == Pass::Search ? partials && !counts : !counts && !search;
    }
};

int check_launch();                        // 0 if the launch just made was accepted, else -1
int grid_stride_blocks(uint64_t total);    // workgroups of 256 for a grid-stride loop over `total` items

// -- record plumbing: reference records <-> a database's layout, every kind (LANES: iris_kernels.hip;
// TILES: launch_*_tiles_kind, iris_engines_mfma.hip)
int launch_pack(void *stream, const KindInfo &k, const void *staging, void *db, uint64_t t_first, uint64_t n);
int launch_unpack(void *stream, const KindInfo &k, const void *db, void *staging, uint64_t t_first, uint64_t n);
int launch_generate(void *stream, const KindInfo &k, void *db, uint64_t t_first, uint64_t n, uint64_t seed,
                    uint64_t global_index0);
int launch_pack_tiles_kind(void *stream, int kind, const void *staging, void *db, uint64_t t_first, uint64_t n);
int launch_unpack_tiles_kind(void *stream, int kind, const void *db, void *staging, uint64_t t_first, uint64_t n);
int launch_generate_tiles_kind(void *stream, int kind, void *db, uint64_t t_first, uint64_t n, uint64_t seed,
                               uint64_t global_index0);

// -- per-engine query tables built on the device from the query (iris_query.hip); q, qmask: host
int launch_query_template(void *stream, const void *q, uint32_t *tab, uint32_t *frag);
int launch_query_masks(void *stream, const void *qmask, uint32_t *tab, uint32_t *frag);
int launch_query_shares(void *stream, const void *q, uint32_t *tab, uint32_t *frag);
int launch_query_tiles(void *stream, const void *queries, uint32_t nq, uint32_t nqp, uint32_t *tiles);

// -- share preparation (iris_prepare.hip); rounds: ChaCha8 / 12 / 20 (anything else: -1)
constexpr int kMaxPrepParties = 64;
int launch_prepare_shares(void *stream, const void *templates, uint64_t m, uint64_t g0, const uint8_t key[32],
                          uint64_t nonce, uint32_t rounds, uint32_t parties, void *shares);
int launch_prepare_shares_tiles(void *stream, const void *templates, uint64_t m, uint64_t g0, const uint8_t key[32],
                                uint64_t nonce, uint32_t rounds, uint32_t parties, void *const *dbs,
                                const uint64_t *t_first);
int launch_prepare_direct(void *stream, const void *tdb, uint64_t t_first, uint64_t m, uint64_t g0,
                          const uint8_t key[32], uint64_t nonce, uint32_t rounds, uint32_t parties,
                          void *const *dbs, const uint64_t *s_first, void *masks, uint64_t m_first);

// -- template passes, LANES (template_kernel, iris_kernels.hip): one workgroup per 4 blocks of 64
// records, every mode.  *n_partials (if given) = search_partials(r), set for an empty range too;
// an empty range launches nothing.
uint32_t search_partials(LaunchRange r);      // partials a search writes
uint64_t template_topk_units(LaunchRange r);  // lists a top-k pass writes
int launch_template(Pass p, void *stream, const void *db, const void *qtab, LaunchRange r, const PassOut &o,
                    uint32_t *n_partials = nullptr);

// -- template passes, TILES (template_mfma_kernel, iris_mfma.hip): every mode runs the form its
// range asks for -- the K-split on small ranges, else one or four tiles per wave (IRIS_TILES_PER_WAVE
// pins one) -- on the same grid.  *n_partials (if given) = mfma_search_partials(h, r), set for an
// empty range too; an empty range launches nothing.
// fin (a search only, and only where fused_search_ok(): else -1): the fused finish of a small search
// (grids of at most kFusedReduceMax workgroups): the last workgroup to finish reduces the partials
// and writes the winner (idx + idx_base) to dst; ticket is a zeroed 4-KB device block (a two-level
// ticket) that the kernel leaves zeroed.  done != null (dst in coherent host memory): dst is written
// through to host memory and, once those stores have completed, seq is stored to *done (coherent
// host memory) -- a blocking caller spins on that word instead of waiting for the end of the kernel
// and the runtime's completion signal.
struct FusedFinish {
    uint32_t *ticket;
    Partial *dst;
    uint64_t idx_base;
    uint32_t *done;
    uint32_t seq;
};
constexpr uint32_t kFusedReduceMax = 4096;
bool fused_search_ok(const Hooks &h, LaunchRange r);
uint32_t mfma_search_partials(const Hooks &h, LaunchRange r);  // partials a search writes
uint64_t mfma_topk_units(const Hooks &h, LaunchRange r);       // lists a top-k pass writes
int launch_template_mfma(Pass p, const Hooks &h, void *stream, const void *db, const void *qfrag, LaunchRange r,
                         const PassOut &o, uint32_t *n_partials = nullptr, const FusedFinish *fin = nullptr);

// -- shared template passes, TILES (template_share_kernel, iris_mfma.hip): while a
// pass streams the database, a later pass of the same mode and range may register as its guest;
// every workgroup that starts after that computes both queries for its 16 tiles from one read of
// them, writes both results and marks its tile group in the guest's done array, and the guest's
// own launch skips the groups marked there.  A search's results are partials, a match pass's the
// hits appended to each query's sink, a top-k pass's each wave's list at unit blockIdx.x * 4 + wave
// of each query's topk_sink (mfma_topk_units(h, r) units; k may differ).  A pass hosts passes of
// its own mode only: the caller keeps them apart.  A report pass (iris_template_report_async) feeds,
// per query, the parts that query's ReportSinks hold -- the two queries' may differ in every field
// -- and each query's lists and histogram copies are written as its own launch would write them.
// The slot is device memory, zeroed before the hosting pass's launch and written once by
// launch_share_publish* (the fields, then ready with agent-scope release).  Nothing else is read
// while its writer runs: done words and what a pass wrote for its guest reach their readers (the
// guest's own launch and what follows it on the device stream) with the end of the hosting kernel.
struct GuestSlot {
    uint32_t ready;
    uint32_t pad;
    const void *frag;   // the guest's query fragments (a buffer of the sharing ring, not the engine's)
    Partial *partials;  // the guest's partials buffer (a search)
    uint32_t *done;     // the guest's done array, one word per workgroup
    MatchSink sink;     // the guest's sink (a match pass: its counter is zeroed ahead of the publish; a top-k pass: topk_sink;
                        // a report pass: report_sink of its device ReportSinks, complete ahead of the publish)
};
// whether a range runs the form that can share: 4 tiles per wave, no K-split, separate reduce
bool share_search_ok(const Hooks &h, LaunchRange r);
// Search, Match, Topk or Report where share_search_ok() (else -1): slot = this pass's guest slot (NULL:
// never hosts), own_done = NULL or the words an earlier pass set for the tile groups it computed
// for this query, count = NULL or a device counter of tile groups carried for guests.
int launch_template_share(Pass p, const Hooks &h, void *stream, const void *db, const void *qfrag, LaunchRange r,
                          const PassOut &o, uint32_t *n_partials, const GuestSlot *slot, const uint32_t *own_done,
                          unsigned long long *count);
// zeroes a pass's guest slot and, if given, its done array of n words
int launch_share_prepare(void *stream, GuestSlot *slot, uint32_t *done, uint32_t n);
// a search's registration; a match pass's, and a top-k pass's (sink = topk_sink(lists, k))
int launch_share_publish(void *stream, GuestSlot *slot, const void *frag, Partial *partials, uint32_t *done);
int launch_share_publish_match(void *stream, GuestSlot *slot, const void *frag, const MatchSink &sink, uint32_t *done);
// a report pass's registration is launch_share_publish_match with report_sink(device ReportSinks).
// What precedes it, and the pass's own launch: `sinks` stored at dst (device memory) and the
// `words` u64 counters at `zero` cleared (the histogram's copies and the match counter), one launch
int launch_report_prepare(void *stream, ReportSinks *dst, const ReportSinks &sinks, uint64_t *zero, uint64_t words);
// test hook IRIS_SEARCH_SHARE_DELAY_US: a one-thread kernel that spins for `ticks` of the wall clock
int launch_share_delay(void *stream, uint64_t ticks);

// -- two-query search rounds (template_multi_kernel): nq = 2 queries per streamed pass; partials [nq][*n_partials]
uint32_t multi_search_partials(LaunchRange r, int nq);
int launch_template_multi_search(void *stream, const void *db, const void *const *qfrags, int nq, LaunchRange r,
                                 Partial *partials, uint32_t *n_partials);

// -- what follows a pass (iris_kernels.hip)
// consumes partials; the winner's idx (range-relative) is offset by idx_base
int launch_reduce(void *stream, Partial *partials, uint32_t n_partials, Partial *out, uint64_t idx_base = 0);
// group search merge: out[q] = best of recv[s * stride + q], s < shards (indices already global)
int launch_group_merge(void *stream, const Partial *recv, uint32_t shards, uint32_t nq, uint32_t stride, Partial *out);
// dst[q][i] = sum over c < copies of src[q][c][i], q < nq, i < words (dst: device or pinned host memory)
int launch_hist_reduce(void *stream, const uint64_t *src, uint32_t words, uint32_t copies, uint32_t nq, uint64_t *dst);
// folds the `units` lists of k a top-k pass wrote at `lists` level by level (kTopkFanIn lists per
// workgroup, ping-pong between `lists` and `spare`, which holds topk_spare_lists(units) lists) and
// writes the final k records to `out`
inline uint64_t topk_spare_lists(uint64_t units) { return (units + kTopkFanIn - 1) / kTopkFanIn; }
int launch_topk_merge(void *stream, Partial *lists, Partial *spare, uint64_t units, uint32_t k, Partial *out);
// one level, `slots` queries that share `units` at a time (blockIdx.y): slot s reads src + s * src_stride
// and writes its topk_spare_lists(units) lists at dst + s * dst_stride
int launch_topk_merge_level(void *stream, const Partial *src, uint64_t units, uint32_t k, Partial *dst, uint32_t slots,
                            uint64_t src_stride, uint64_t dst_stride);

// -- MasksEngine and DistanceEngine rows, LANES (iris_kernels.hip)
int launch_masks(void *stream, const void *db, const void *qtab, LaunchRange r, uint16_t *out);
int launch_shares(void *stream, const void *db, const void *qtab, LaunchRange r, uint16_t *out);

// -- MasksEngine and DistanceEngine rows, TILES (iris_engines_mfma.hip)
// Completion word of a blocking device-output engine call: the kernel's last workgroup, once
// every workgroup's rows are stored, stores seq into the coherent host word done (ticket: the
// device's zeroed 4-KB ticket block, left zeroed).  The launcher sets armed when the kernel it
// chose signals (the small-range K-split kernels); otherwise the caller waits for the stream.
struct DoneSignal {
    uint32_t *ticket;
    uint32_t *done;
    uint32_t seq;
    bool armed;
};
// packed: the rows in the read-ahead's packed form (store_tile_packed): out holds r.n records of
// 32 B, then r.n escape rows of 31 u16 (no completion word)
int launch_masks_mfma(const Hooks &h, void *stream, const void *db, const void *qfrag, LaunchRange r, uint16_t *out,
                      DoneSignal *sig = nullptr, bool packed = false);
int launch_shares_mfma(const Hooks &h, void *stream, const void *db, const void *qfrag, LaunchRange r, uint16_t *out,
                       DoneSignal *sig = nullptr);
// nq DistanceEngine queries in one pass over a TILES share database (iris_shares_batch.hip):
// qfrags[q] = query q's fragments (as launch_shares_mfma's qfrag), rows of query q at out + q * r.n * 31.
// sig: as launch_shares_mfma's, armed when the last launch signals.
// forms (optional): the passes the call launched and the queries they held, by kernel form.
struct SharesBatchForms {
    uint32_t large = 0, large_queries = 0;    // shares_batch_kernel (passes of 2..4 queries)
    uint32_t split = 0, split_queries = 0;    // shares_batch_split_kernel (full groups)
    uint32_t single = 0;                      // launch_shares_mfma, one query each
};
int launch_shares_batch(const Hooks &h, void *stream, const void *db, const void *const *qfrags, uint32_t nq,
                        LaunchRange r, uint16_t *out, DoneSignal *sig = nullptr, SharesBatchForms *forms = nullptr);

// -- the fused resolver step, TILES (masks_mfma_kernel's resolving modes, iris_engines_mfma.hip): the
// masks pass whose rows are the denominators of shares[0..parts) (1..8 device arrays of r.n rows,
// summed), decoded in place of being stored.  Search, Match, Topk or Hist; every mode runs the same grid,
// masks_resolve_partials(h, r) workgroups at one or four tiles per wave; an empty range launches nothing.
uint32_t masks_resolve_partials(const Hooks &h, LaunchRange r);  // partials a search writes
uint64_t masks_topk_units(const Hooks &h, LaunchRange r);        // lists a top-k pass writes
int launch_masks_resolve(Pass p, const Hooks &h, void *stream, const void *db, const void *qfrag, LaunchRange r,
                         const uint16_t *const *shares, uint32_t parts, const PassOut &o);

// -- the resolver, denominators given (resolver_kernel, iris_resolver.hip): rows i < n of shares[0..parts)
// (1..8) summed and decoded against denoms.  Search, Match, Topk or Hist; one workgroup per 256 rows in
// every mode; n == 0 launches nothing.
uint32_t resolver_partials(uint64_t n);    // partials a search writes
uint64_t resolver_topk_units(uint64_t n);  // lists a top-k pass writes
int launch_resolver(Pass p, void *stream, const uint16_t *const *shares, uint32_t parts, const uint16_t *denoms, uint64_t n,
                    const PassOut &o);

// -- template batch passes, TILES (batch_lds_kernel, iris_batch.hip): the queries of g (g.nqg *
// g.qper, in qtiles' order, padding queries included) against r in one GEMM pass of the shape
// IRIS_BATCH_KERNEL picks, g.nqg * g.G workgroups in every mode; an empty range launches nothing.
struct BatchGeometry {
    uint64_t tile0, ntiles;
    uint32_t nqg, G;  // query groups, workgroups per query group
    uint32_t qper;    // queries per query group (nqg * qper results; at most the engine's padding)
};
BatchGeometry batch_geometry(const Hooks &h, LaunchRange r, uint32_t nq);
uint32_t batch_query_group();  // padding unit of a batched engine's queries
uint64_t batch_topk_units(const BatchGeometry &g);  // lists per query a top-k pass writes (its waves)
// A mode's operands (the others stay unset):
struct BatchPassOut {
    Partial *partials = nullptr, *out = nullptr;  // Search: g.G partials per query, which a reduce launched with
    uint64_t idx_base = 0;                        //   the pass folds into out[query] (idx + idx_base)
    const MatchSink *sinks = nullptr;             // Match: DEVICE array of one sink per query (a padding query's has cap 0)
    Partial *lists = nullptr;                     // Topk: query q's wave `unit` stores its k best at lists + q * stride
    uint64_t stride = 0;                          //   + unit * k (a padding query's lists stay empty); k 1..kTopkMax,
    uint32_t k = 0;                               //   stride >= batch_topk_units(g) * k
    uint64_t *counts = nullptr;                   // Hist: DEVICE rows [query][nbins + 1] of u64, zeroed on the stream by
    uint32_t nbins = 0;                           //   the caller (a padding query's row counts every record invalid);
                                                  //   nbins a power of two up to kHistMaxBins
    BatchPassOut(Partial *parts, Partial *res, uint64_t base = 0) : partials(parts), out(res), idx_base(base) {}
    BatchPassOut(const MatchSink *device_sinks) : sinks(device_sinks) {}
    BatchPassOut(Partial *l, uint64_t s, uint32_t kk) : lists(l), stride(s), k(kk) {}
    BatchPassOut(uint64_t *c, uint32_t bins) : counts(c), nbins(bins) {}
    // Report: the operands of the parts present, as above; an absent part's pointer (sinks, lists, counts) is null
    BatchPassOut(const MatchSink *device_sinks, Partial *l, uint64_t s, uint32_t kk, uint64_t *c, uint32_t bins)
        : sinks(device_sinks), lists(l), stride(s), k(kk), counts(c), nbins(bins) {}
};
int launch_batch(Pass p, const Hooks &h, void *stream, const void *db, const void *qtiles, LaunchRange r,
                 const BatchGeometry &g, const BatchPassOut &o);

// -- masks batch passes, TILES (masks_batch_kernel, iris_masks_batch.hip): m = 2..kMasksBatchG
// MasksEngine queries in one pass, the same slots, tiles per wave and grid in every mode.
constexpr int kMasksBatchG = 4;  // queries per pass
// The fused resolver step of a pass: shares[p] = participant p's query-major device array (nq slabs of
// r.n * 31 u16), q0 = the pass's first query (its slab); a search: dist_out = NULL or nq * r.n doubles
// (query-major), and query q0 + s writes masks_batch_partials() partials at partials + s * stride.
struct MasksBatchResolve {
    const uint16_t *const *shares;
    uint32_t parts;
    uint32_t q0;
    double *dist_out;
    Partial *partials;
    uint32_t stride;
};
bool masks_batch_runs(const Hooks &h, LaunchRange r);  // whether a range runs the batch kernel (else single-query launches)
uint32_t masks_batch_partials(const Hooks &h, LaunchRange r);  // upper bound of a query's partials
uint64_t masks_batch_topk_units(const Hooks &h, LaunchRange r, uint32_t m);  // lists per query a top-k pass writes
// A mode's operands, by constructor (launch_masks_batch refuses operands that are not its mode's):
struct MasksBatchOut {
    uint16_t *rows = nullptr;         // Search, no resolver step: rows of query s to rows + s * r.n * 31
    bool resolve = false;             // every other form: the fused resolver step rs
    MasksBatchResolve rs{};
    uint32_t *np = nullptr;           // Search with rs: *np = partials written per query
    const MatchSink *sinks = nullptr; // Match: sinks[s] is query s's (counters zeroed on the stream by the caller)
    Partial *lists = nullptr;         // Topk: every wave stores its k best of query s at lists + s * stride
    uint64_t stride = 0;              //   + wave * k (masks_batch_topk_units lists per query); k 1..kTopkMax
    uint32_t k = 0;
    const MatchSink *hists = nullptr; // Hist: hists[s] is query s's hist_sink (counters zeroed on the stream by the caller),
                                      //   every query's the same nbins and copies
    struct HistTag {};
    MasksBatchOut(uint16_t *out) : rows(out) {}
    MasksBatchOut(const MasksBatchResolve &r, uint32_t *n_partials) : resolve(true), rs(r), np(n_partials) {}
    MasksBatchOut(const uint16_t *const *shares, uint32_t parts, uint32_t q0, const MatchSink *match_sinks)
        : resolve(true), rs{shares, parts, q0, nullptr, nullptr, 0}, sinks(match_sinks) {}
    MasksBatchOut(const uint16_t *const *shares, uint32_t parts, uint32_t q0, Partial *l, uint64_t s, uint32_t kk)
        : resolve(true), rs{shares, parts, q0, nullptr, nullptr, 0}, lists(l), stride(s), k(kk) {}
    MasksBatchOut(const uint16_t *const *shares, uint32_t parts, uint32_t q0, const MatchSink *hist_sinks, HistTag)
        : resolve(true), rs{shares, parts, q0, nullptr, nullptr, 0}, hists(hist_sinks) {}
    // Report: reports[s] is query s's ReportSinks on the DEVICE (two or three parts, the same for every query, with one k,
    // nbins and copies), staged[s] the host copy they were staged from, which the launcher checks
    const ReportSinks *reports = nullptr, *staged = nullptr;
    MasksBatchOut(const uint16_t *const *shares, uint32_t parts, uint32_t q0, const ReportSinks *device_sinks,
                  const ReportSinks *host_copy)
        : resolve(true), rs{shares, parts, q0, nullptr, nullptr, 0}, reports(device_sinks), staged(host_copy) {}
};
int launch_masks_batch(Pass p, const Hooks &h, void *stream, const void *db, const void *const *qfrags, uint32_t m,
                       LaunchRange r, const MasksBatchOut &o);

// ---------------------------------------------------------------- host helpers (iris_host.cpp)
void bits_rotated(const uint64_t *in, int amount, uint64_t *out);
void encoded_rotated(const uint16_t *in, int amount, uint16_t *out);
void encode_template(const iris_template_t *t, uint16_t *out);
void build_template_table(const iris_template_t *q, uint32_t *tab);                  // 400*64 dwords
void build_template_frags(const iris_template_t *q, uint32_t *frag);                 // kTemplateFragDwords
void build_masks_frags(const uint64_t *const *vectors, int count, uint32_t *frag);    // kMaskFragUint4 uint4 (compact)
void build_query_tile(const iris_template_t *q, uint32_t *tile);                      // 6400 uint4 (TILES tile)
void build_shares_frags(const uint16_t *const *vectors, int count, uint32_t *frag);   // kShareFragUint4 uint4 + 64 int
void build_masks_table(const uint64_t *const *vectors, int count, uint32_t *tab);     // 400*32
void build_shares_table(const uint16_t *const *vectors, int count, uint32_t *tab);    // 6400*32
void build_masks_rotations(const uint64_t *query, uint32_t *tab);
void build_shares_rotations(const uint16_t *query, uint32_t *tab);
bool partial_better(const Partial &a, const Partial &b);
// memcpy split over a few persistent helper threads (copies of at least 256 KB)
void parallel_copy(void *dst, const void *src, size_t bytes, int lane = 0);  // lane: the device ordinal
// pread of [off, off + bytes) of fd into dst, split over the same helper threads; false if a read
// failed or the file ended early
bool parallel_pread(int fd, void *dst, size_t bytes, off_t off, int lane = 0);
// MasksEngine rows of n records in the read-ahead's packed form (store_tile_packed, iris_device.hpp:
// 32 B per record at pk, escaped rows in full at esc) expanded into [n][31] u16 at out, split over
// the same helper threads
void parallel_expand(uint16_t *out, const uint8_t *pk, const uint16_t *esc, size_t n, int lane = 0);
void expand_packed_rows(uint16_t *out, const uint8_t *pk, const uint16_t *esc, size_t n);  // one thread
// memcpy whose destination lines are written with non-temporal stores (AVX-512, >= 4 KB); one thread
void copy_nt(char *dst, const char *src, size_t n);
// dst[i] = src[0][i] + ... + src[k-1][i] mod 2^16 (k <= 8): one thread / the device's helper pool
void sum_u16(uint16_t *dst, const uint16_t *const *src, int k, size_t n);
void parallel_sum_u16(uint16_t *dst, const uint16_t *const *src, int k, size_t n, int lane = 0);

}  // namespace iris
