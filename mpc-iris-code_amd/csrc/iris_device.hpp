// iris_device.hpp — device helpers shared by the MFMA kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

#include "iris_internal.hpp"

namespace iris {

// Workgroups of one launch that fit on the current device at `per_cu` per CU
// (persistent grids); cached per device ordinal.
static inline uint64_t resident_blocks(int per_cu) {
    static std::atomic<int> cus[64];  // zero-initialised (static storage)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return (uint64_t)n * per_cu;
}

// Tiles per wave for a range of `ntiles` tiles: `big`, unless that leaves fewer waves
// than the chip holds at two workgroups per CU — then one, for 8x / 4x / 2x the waves
// (a participant-sized chunk of 20k records is only 625 tiles).  IRIS_TILES_PER_WAVE=1|4
// pins the small or the big variant (tests run both).
static inline int tiles_per_wave(const Hooks &h, uint64_t ntiles, int big) {
    if (h.tiles_per_wave) return h.tiles_per_wave == 1 ? 1 : big;
    return ntiles / big < (uint64_t)resident_blocks(2) * kWaveSlots ? 1 : big;
}

// The template kind's TILES record plumbing (iris_mfma.hip), launched with the other kinds' from
// launch_*_tiles_kind (iris_engines_mfma.hip): grid-stride loops over n * 2 * kPlaneGroups items
__global__ void __launch_bounds__(256) pack_tiles_kernel(const uint32_t *__restrict__ staging, uint4 *__restrict__ db, uint64_t t_first, uint64_t n);
__global__ void __launch_bounds__(256) unpack_tiles_kernel(const uint4 *__restrict__ db, uint32_t *__restrict__ staging, uint64_t t_first, uint64_t n);
__global__ void __launch_bounds__(256) generate_tiles_kernel(uint4 *__restrict__ db, uint64_t t_first, uint64_t n, uint64_t key, uint64_t global_index0);

// ---------------------------------------------------------------- primitives of the MFMA kernels
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4_nt __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

constexpr int kTile = 32;  // records of a TILES tile: the N of one 32x32 MFMA

// 16-B nontemporal load: a database stream that this launch reads once
__device__ __forceinline__ uint4 nt_load16(const uint4 *p) {
    const u32x4 v = __builtin_nontemporal_load((const u32x4 *)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
// 16-B copies through a vector type (a uint4 struct copy between address spaces is a memcpy that
// keeps its register copy in scratch memory)
__device__ __forceinline__ uint4 load16(const uint4 *p) {
    const u32x4 v = *(const u32x4 *)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void store16(uint4 *p, const uint4 &v) { *(u32x4 *)p = u32x4{v.x, v.y, v.z, v.w}; }

__device__ __forceinline__ v16f mfma_fp4(const v8i &a, const v8i &b, const v16f &c) {
    // cbsz = blgp = 4: both operands e2m1; scales 127 = 2^0 (e8m0)
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4, 4, 0, 127, 0, 127);
}
__device__ __forceinline__ v16i mfma_i8(const uint4 &a, const uint4 &b, const v16i &c) {
    const v4i av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w};
    const v4i bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w};
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, c, 0, 0, 0);
}

// MasksEngine operands of one 64-bit chunk: A from a compact query word, B from one dword of a mask
// tile (8 masks' nibbles) -- kMaskFragUint4, kMaskTileUint4 in iris_internal.hpp
__device__ __forceinline__ v8i mask_a(uint32_t w) {
    return v8i{(int)(w & 0x44444444u), (int)(w & 0x22222222u), (int)(w & 0x11111111u), (int)((w >> 3) & 0x11111111u),
               0, 0, 0, 0};
}
__device__ __forceinline__ v8i mask_b(uint32_t x) {
    return v8i{(int)(x & 0x11111111u), (int)(x & 0x22222222u), (int)(x & 0x44444444u), (int)((x >> 1) & 0x44444444u),
               0, 0, 0, 0};
}
__device__ __forceinline__ void mask_chunk(uint32_t x, const v8i &a, v16f &acc) { acc = mfma_fp4(a, mask_b(x), acc); }

// 16-B store written through the XCD's L2 (sc1: the line leaves L2 and is dropped there; the same
// cost as a plain 16-B store, MI355X_MICROARCH.md "stores of each flavour").
__device__ __forceinline__ void store16_wt(uint4 *dst, const uint4 &v) {
    const u32x4_nt w = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst), "v"(w) : "memory");
}

// Writes one 32-record tile's [32][31] u16 output rows.  In the 32x32 MFMA C
// layout lane l holds rows k = (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 0..15, of
// record (l & 31); `val(r)` returns that value.  A tile fully inside
// [first, end) whose output offset is 16-B aligned is staged through the
// wave's 2 KB LDS buffer and written with 124 16-byte stores (1984 B); other
// tiles fall back to per-element stores of their valid records.
// wt (a kernel that signals completion before it ends, DoneSignal): every row byte is written
// through L2 (sc1), so once the storing wave's vmcnt(0) wait returns the rows are in memory, where a
// reader on any XCD -- a kernel on another stream, a copy engine -- finds them without this launch's
// end-of-kernel write-back (nontemporal and plain stores stay dirty in the XCD's L2 until then).
template <class F>
__device__ __forceinline__ void store_tile_rows(uint16_t *__restrict__ out, uint16_t *lds, uint64_t tile_t0,
                                                uint64_t first, uint64_t end, bool tile_valid, int lane, F val,
                                                bool wt = false) {
    const int h = lane >> 5;
    const bool full = tile_valid && tile_t0 >= first && tile_t0 + 32 <= end && ((tile_t0 - first) & 7) == 0 &&
                      (((uintptr_t)out & 15) == 0);
    if (full) {  // wave-uniform
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (k < kRot) lds[(lane & 31) * kRot + k] = val(r);
        }
        uint4 *dst = (uint4 *)(out + (tile_t0 - first) * kRot);
        const uint4 *src = (const uint4 *)lds;
        // streamed out with nontemporal stores: the rows are not re-read by this launch
        constexpr int kStores = 32 * kRot * 2 / 16;
        if (wt) {  // wave-uniform
            for (int i = lane; i < kStores; i += 64) store16_wt(&dst[i], src[i]);
            return;
        }
        for (int i = lane; i < kStores; i += 64) {
            const uint4 v = src[i];
            const u32x4_nt w = {v.x, v.y, v.z, v.w};
            __builtin_nontemporal_store(w, (u32x4_nt *)&dst[i]);
        }
    } else {
        const uint64_t tg = tile_t0 + (lane & 31);
        if (!tile_valid || tg < first || tg >= end) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (k >= kRot) continue;
            if (wt)  // agent-scope relaxed store: global_store_short ... sc1
                __hip_atomic_store(&out[(tg - first) * kRot + k], val(r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                out[(tg - first) * kRot + k] = val(r);
        }
    }
}

// Writes one 32-record tile's MasksEngine rows in the packed form the read-ahead windows carry over
// the host link (32 B per record instead of 62, iris_api_engines.hip kPackedRecBytes): record i of the
// range [first, end) at pk + 32 i holds bytes 0..30 = row[k] - 64 B and byte 31 = B, where
// B = min_k row[k] >> 6 (den <= 12800, so B <= 200), whenever every row[k] - 64 B fits a byte;
// otherwise byte 31 is 0xFF and the row is stored in full at esc + 31 i.  Random masks never
// escape (the 31 rotations' counts span ~115-220); structured ones (a block of masked columns) do.
// In the 32x32 MFMA C layout lane l holds rows k = (r & 3) + 8 (r >> 2) + 4 h, h = l >> 5, of record
// l & 31, so its registers 4j..4j+3 are the record's bytes 8j + 4h .. +3 (record dword 2j + h); after
// swapping two dwords with its partner lane l ^ 32, half 0 holds the record's bytes 0..15 and half 1
// bytes 16..31, and a wave's 64 16-B stores cover a tile's 1024 B contiguously.
template <class F>
__device__ __forceinline__ void store_tile_packed(uint8_t *__restrict__ pk, uint16_t *__restrict__ esc, uint64_t tile_t0,
                                                  uint64_t first, uint64_t end, bool tile_valid, int lane, F val) {
    const int h = lane >> 5;
    uint32_t v[16];
    uint32_t lo = 0xFFFFu, hi = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int k = (r & 3) + 8 * (r >> 2) + 4 * h;
        v[r] = val(r);
        if (k < kRot) {
            lo = v[r] < lo ? v[r] : lo;
            hi = v[r] > hi ? v[r] : hi;
        }
    }
    const uint32_t plo = __shfl_xor(lo, 32), phi = __shfl_xor(hi, 32);
    lo = plo < lo ? plo : lo;
    hi = phi > hi ? phi : hi;
    const uint32_t b = lo >> 6, base = b << 6;
    const bool escape = hi - base > 255u;
    uint32_t dw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        dw[j] = ((v[4 * j] - base) & 0xFFu) | ((v[4 * j + 1] - base) & 0xFFu) << 8 | ((v[4 * j + 2] - base) & 0xFFu) << 16 |
                ((v[4 * j + 3] - base) & 0xFFu) << 24;
    if (h) dw[3] = (dw[3] & 0x00FFFFFFu) | (escape ? 0xFFu : b) << 24;  // byte 31: row k = 31 is the zero row
    const uint32_t sa = __shfl_xor(h ? dw[0] : dw[2], 32), sb = __shfl_xor(h ? dw[1] : dw[3], 32);
    const u32x4_nt w = h ? u32x4_nt{sa, dw[2], sb, dw[3]} : u32x4_nt{dw[0], sa, dw[1], sb};
    const uint64_t tg = tile_t0 + (lane & 31);
    if (!tile_valid || tg < first || tg >= end) return;
    __builtin_nontemporal_store(w, (u32x4_nt *)(pk + (tg - first) * 32 + 16 * h));
    if (escape) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (k < kRot) esc[(tg - first) * kRot + k] = (uint16_t)v[r];
        }
    }
}

// Shares TILES planes: 16 u16 elements (8 dwords) -> the low-byte and
// high-byte planes, each byte XOR 0x80 (the byte - 128 as i8), 16 B each.
__device__ __forceinline__ void split_bytes(const uint32_t *src8, uint4 &lo, uint4 &hi) {
    uint32_t l[4], hh[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t a = src8[2 * q], b = src8[2 * q + 1];  // elements 4q..4q+3
        // v_perm_b32: bytes 0-3 of the selector space are a's, 4-7 are b's
        l[q] = __builtin_amdgcn_perm(b, a, 0x06040200u) ^ 0x80808080u;   // a0 a2 b0 b2
        hh[q] = __builtin_amdgcn_perm(b, a, 0x07050301u) ^ 0x80808080u;  // a1 a3 b1 b3
    }
    lo = make_uint4(l[0], l[1], l[2], l[3]);
    hi = make_uint4(hh[0], hh[1], hh[2], hh[3]);
}

// Candidate order of the resolver / search argmin: exact fraction (u32 cross-
// multiplication, num and den < 2^16), then the lowest index; den = 0 is "no
// candidate" (NaN / +inf in the reference, never selected by a strict <).
// (__umul24: num, den < 2^16, so the 24-bit multiply's low 32 bits are the exact product, at
// full rate where a 32-bit v_mul_lo_u32 issues at a quarter)
__device__ __forceinline__ bool partial_better_dev(const Partial &a, const Partial &b) {
    if (a.den == 0) return false;
    if (b.den == 0) return true;
    const uint32_t l = __umul24(a.num, b.den), r = __umul24(b.num, a.den);
    if (l != r) return l < r;
    return a.idx < b.idx;
}
// as partial_better_dev, then the lower rotation (two candidates of one template)
__device__ __forceinline__ bool partial_better_rot(const Partial &a, const Partial &b) {
    if (a.den == 0) return false;
    if (b.den == 0) return true;
    const uint32_t l = __umul24(a.num, b.den), r = __umul24(b.num, a.den);
    if (l != r) return l < r;
    if (a.idx != b.idx) return a.idx < b.idx;
    return a.rot < b.rot;
}

__device__ __forceinline__ Partial partial_shfl_xor(const Partial &c, int off) {
    Partial o;
    o.num = __shfl_xor(c.num, off);
    o.den = __shfl_xor(c.den, off);
    o.rot = __shfl_xor(c.rot, off);
    o.pad = 0;
    const uint32_t lo = __shfl_xor((uint32_t)c.idx, off), hi = __shfl_xor((uint32_t)(c.idx >> 32), off);
    o.idx = ((uint64_t)hi << 32) | lo;
    return o;
}

__device__ __forceinline__ Partial partial_of(uint32_t num, uint32_t den, int rot, uint64_t idx) {
    Partial p;
    p.num = num;
    p.den = den;
    p.rot = rot;
    p.pad = 0;
    p.idx = idx;
    return p;
}
__device__ __forceinline__ Partial partial_none() { return partial_of(0, 0, 0, ~0ull); }

// The wave's best candidate in every lane: the 64-lane butterfly under `better` (the search order
// unless given: the LANES kernels and the batch kernel's rotation tie-break bring their own).
struct SearchOrder {
    __device__ __forceinline__ bool operator()(const Partial &a, const Partial &b) const { return partial_better_dev(a, b); }
};
struct RotationOrder {  // then the lower rotation: two candidates of one template
    __device__ __forceinline__ bool operator()(const Partial &a, const Partial &b) const { return partial_better_rot(a, b); }
};
template <class Better = SearchOrder>
__device__ __forceinline__ Partial wave_argmin(Partial c, Better better = Better()) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const Partial o = partial_shfl_xor(c, off);
        if (better(o, c)) c = o;
    }
    return c;
}
// One thread's fold of n waves' bests sh[0 .. n) into b
template <class Better = SearchOrder>
__device__ __forceinline__ void fold_waves(Partial &b, const Partial *sh, int n, Better better = Better()) {
    b = sh[0];
    for (int w = 1; w < n; ++w)
        if (better(sh[w], b)) b = sh[w];
}
// The workgroup's best of one candidate per thread (every thread calls this, sh: one entry per wave):
// each wave's butterfly, lane 0 of each wave to sh[], a barrier, and thread 0 folds the waves' bests
// into c.  True in thread 0 only.  nwaves: a constant (a workgroup sized at run time folds by
// hand, so that its wave count is not kept across the barrier).
template <class Better = SearchOrder>
__device__ __forceinline__ bool block_argmin(Partial &c, Partial *sh, int nwaves, Better better = Better()) {
    c = wave_argmin(c, better);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x != 0) return false;
    Partial b;
    fold_waves(b, sh, nwaves, better);
    c = b;
    return true;
}

// One template's best rotation from a 32x32 MFMA C tile: lane l holds rows
// k = (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 0..15, of template l & 31, and
// frac(r, num, den) yields row r's fraction.  Exact order (u32 cross-
// multiplication; den = 0 is no candidate), lowest rotation on ties; after the
// exchange with lane l ^ 32 both halves hold the template's best (k in 0..30).
template <class F>
__device__ __forceinline__ void best_rotation(int lane, F frac, uint32_t &bn, uint32_t &bd, int &br) {
    const int h = lane >> 5;
    bn = 0;
    bd = 0;
    br = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int k = (r & 3) + 8 * (r >> 2) + 4 * h;  // ascending in r within a half
        uint32_t nn, dd;
        frac(r, nn, dd);
        if (k < kRot && dd != 0 && (bd == 0 || __umul24(nn, bd) < __umul24(bn, dd))) {
            bn = nn;
            bd = dd;
            br = k;
        }
    }
    const uint32_t pn = __shfl_xor(bn, 32), pd = __shfl_xor(bd, 32);
    const int pr = __shfl_xor(br, 32);
    const uint32_t pl = __umul24(pn, bd), pr_ = __umul24(bn, pd);
    if (pd != 0 && (bd == 0 || pl < pr_ || (pl == pr_ && pr < br))) {
        bn = pn;
        bd = pd;
        br = pr;
    }
}

// Threshold matching (MatchSink, iris_internal.hpp).  The decision is the f64 comparison the
// caller would make on the search's own distance: one IEEE division per record, den = 0
// (distance +inf) never matches, not even under threshold = +inf.
// Sink: MatchSink, or a struct of the same fields whose pointers are global by type (GuestSink,
// iris_mfma.hip).
template <class Sink>
__device__ __forceinline__ bool match_hit(const Sink &m, bool valid, uint32_t num, uint32_t den) {
    return valid && den != 0 && (double)num / (double)den < m.threshold;
}

// Appends a wave's hits of T record groups (one candidate per lane and group; every lane of the
// wave calls this): a ballot per group finds them, lane 0 reserves the wave's slots with ONE
// agent-scope relaxed atomic add (none when the wave has no hit), and each hit whose slot lies
// inside the buffer stores its record.  Slot order depends on which wave adds first; the host
// sorts by index.
template <int T, class Sink>
__device__ __forceinline__ void append_matches(const Sink &m, int lane, const bool (&hit)[T],
                                               const uint32_t (&num)[T], const uint32_t (&den)[T], const int (&rot)[T],
                                               const uint64_t (&idx)[T]) {
    uint64_t mask[T];
    uint32_t total = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        mask[t] = __ballot(hit[t]);
        total += (uint32_t)__popcll(mask[t]);
    }
    if (total == 0) return;  // wave-uniform
    uint64_t base = 0;
    if (lane == 0) base = __hip_atomic_fetch_add(m.count, (uint64_t)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
    const uint64_t below = (1ull << lane) - 1;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const uint64_t slot = base + (uint64_t)__popcll(mask[t] & below);
        if (hit[t] && slot < m.cap) {
            auto *const p = m.buf + slot;  // field by field: a record in a typed address space has no operator=
            p->num = num[t];
            p->den = den[t];
            p->rot = rot[t];
            p->pad = 0;
            p->idx = idx[t];
        }
        base += (uint64_t)__popcll(mask[t]);
    }
}

// Histograms (iris_*_histogram; hist_sink, iris_internal.hpp).  A workgroup bins its records in an
// LDS histogram of `nbins` u32 counters and one more word for the records without a valid rotation,
// and adds the non-zero words to global memory once.  Every wave of the workgroup calls hist_zero,
// reaches a barrier, counts, reaches a second barrier and calls hist_flush: the callers place both
// barriers in workgroup-uniform control flow.
__device__ __forceinline__ uint32_t hist_sink_bins(const MatchSink &m) { return (uint32_t)m.cap; }
__device__ __forceinline__ uint64_t *hist_sink_copy(const MatchSink &m) {  // this workgroup's copy of the counters
    return m.count + (uint64_t)(blockIdx.x & (uint32_t)(m.cap >> 32)) * (hist_sink_bins(m) + 1);
}
__device__ __forceinline__ void hist_zero(uint32_t *lds, uint32_t nbins) {
    for (uint32_t i = threadIdx.x; i <= nbins; i += blockDim.x) lds[i] = 0;
}
// One record per lane (`counted` lanes only; every lane of the wave calls this).  The bin is the
// integer min(nbins - 1, floor(num * nbins / den)) with nbins <= 1024 a power of two.  Template
// passes: num <= den <= 12800, the product below 2^24.  Resolver passes: num <= 32767 (a u16 >> 1)
// and den <= 65535, the product at most 32767 * 1024 < 2^25 in u32; num > den (garbage shares, a
// distance above 1) joins the last bin by the same min.  Either way the quotient equals floor of
// the f64 distance times nbins (the header's rule; checked for every den in 1..65535 beside every
// bin edge, tests/test_resolver_histogram_abi.py); distance 1.0 joins the last bin.  den = 0: a
// ballot counts the wave's invalid records, one add.
__device__ __forceinline__ void hist_count(uint32_t *lds, uint32_t nbins, int lane, bool counted, uint32_t num,
                                           uint32_t den) {
    if (counted && den != 0) {
        const uint32_t b = num * nbins / den;
        atomicAdd(&lds[b < nbins ? b : nbins - 1], 1u);
    }
    const uint64_t inv = __ballot(counted && den == 0);
    if (inv != 0 && lane == 0) atomicAdd(&lds[nbins], (uint32_t)__popcll(inv));
}
// the workgroup's non-zero words -> dst (agent-scope relaxed u64 adds, as append_matches adds its
// counter; neighbouring lanes add to neighbouring words).  Counters: uint64_t *, or the same pointer
// global by type (the sharing pass, iris_mfma.hip)
template <class Counters>
__device__ __forceinline__ void hist_flush(const uint32_t *lds, uint32_t nbins, Counters dst) {
    for (uint32_t i = threadIdx.x; i <= nbins; i += blockDim.x) {
        const uint32_t v = lds[i];
        if (v != 0) __hip_atomic_fetch_add(dst + i, (uint64_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
template <int Q>
__device__ __forceinline__ uint32_t *hist_lds() {  // [Q][kHistMaxBins + 1], of the kernels that call it only
    __shared__ uint32_t h[Q * (kHistMaxBins + 1)];
    return h;
}

// Top-k (iris_*_topk).  A wave keeps its best candidates so far as ONE sorted list, entry j in
// lane j (`entry`; den = 0 is an empty entry, empties last), in the search order of
// partial_better_dev -- a total order, indices being unique.  It takes the place of the search
// form's running best.  Lanes >= k hold the overflow of earlier inserts and are never stored.
__device__ __forceinline__ Partial partial_readlane(const Partial &c, int src) {  // src: wave-uniform
    Partial o;
    o.num = (uint32_t)__builtin_amdgcn_readlane((int)c.num, src);
    o.den = (uint32_t)__builtin_amdgcn_readlane((int)c.den, src);
    o.rot = __builtin_amdgcn_readlane(c.rot, src);
    o.pad = 0;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)c.idx, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(c.idx >> 32), src);
    o.idx = ((uint64_t)hi << 32) | lo;
    return o;
}
// One record group's candidates (one per lane, `valid` lanes only; every lane of the wave calls
// this) against the wave's list: a ballot finds the candidates that beat the k-th entry (lane
// k - 1, broadcast once) -- after a short warm-up usually none, and the group costs one compare
// and one ballot.  Each set bit, in ascending lane order, is broadcast, its position is the
// number of entries that beat it (a popcount: the list is sorted), the entries from there on move
// up one lane and lane `pos` takes it; a candidate that an earlier insert of the same group
// pushed past k - 1 finds pos >= k and is dropped.
__device__ __forceinline__ void topk_insert(Partial &entry, uint32_t k, int lane, Partial c, bool valid) {
    if (!valid) c.den = 0;
    const Partial kth = partial_readlane(entry, (int)k - 1);
    uint64_t vote = __ballot(partial_better_dev(c, kth));
    while (vote) {  // wave-uniform
        const int src = __builtin_ctzll(vote);
        vote &= vote - 1;
        const Partial x = partial_readlane(c, src);
        const uint32_t pos = (uint32_t)__popcll(__ballot(partial_better_dev(entry, x)));
        if (pos >= k) continue;
        Partial up;
        up.num = __shfl_up(entry.num, 1);
        up.den = __shfl_up(entry.den, 1);
        up.rot = __shfl_up(entry.rot, 1);
        up.pad = 0;
        up.idx = ((uint64_t)__shfl_up((uint32_t)(entry.idx >> 32), 1) << 32) | __shfl_up((uint32_t)entry.idx, 1);
        if ((uint32_t)lane > pos) entry = up;
        else if ((uint32_t)lane == pos) entry = x;
    }
}
// The wave's list -> lists[unit][0..k) (topk_sink, iris_internal.hpp: buf = lists, cap = k): plain
// vector stores at a place only this wave writes, empty entries included, so the merge reads no
// stale record and nothing needs zeroing or an atomic.
__device__ __forceinline__ void topk_store(const MatchSink &m, uint64_t unit, int lane, const Partial &entry) {
    if ((uint64_t)lane < m.cap) m.buf[unit * m.cap + (uint64_t)lane] = entry;
}
// The same store into lists whose pointer is global by type (GlobalLists, iris_mfma.hip: the sharing
// pass's sink), field by field as append_matches stores its records.
template <class Lists>
__device__ __forceinline__ void topk_store_lists(const Lists &m, uint64_t unit, int lane, const Partial &entry) {
    if ((uint32_t)lane < m.k) {
        auto *const p = m.buf + (unit * m.k + (uint64_t)lane);
        p->num = entry.num;
        p->den = entry.den;
        p->rot = entry.rot;
        p->pad = 0;
        p->idx = entry.idx;
    }
}

// Report passes (iris_template_report; ReportSinks, iris_internal.hpp).  The pass's MatchSink points
// at the device struct of the three sinks: the fields the sinks' helpers read, through a pointer that
// is global by type -- a wave-uniform address, so they are scalar loads and every "is this part
// present" test is a scalar branch, the same for all waves of the workgroup.  Read after the K loop:
// nothing of it is carried across.
__device__ __forceinline__ ReportSinks report_sinks_load(const MatchSink &ms) {
    const __attribute__((address_space(1))) ReportSinks *const p = (const __attribute__((address_space(1))) ReportSinks *)ms.buf;
    ReportSinks r;
    r.match = MatchSink{p->match.buf, p->match.cap, p->match.count, p->match.threshold};
    r.topk = MatchSink{p->topk.buf, p->topk.cap, nullptr, 0.0};
    r.hist = MatchSink{nullptr, p->hist.cap, p->hist.count, 0.0};
    return r;
}
__device__ __forceinline__ bool report_has_match(const ReportSinks &r) { return r.match.count != nullptr; }
__device__ __forceinline__ bool report_has_topk(const ReportSinks &r) { return r.topk.cap != 0; }
__device__ __forceinline__ bool report_has_hist(const ReportSinks &r) { return r.hist.count != nullptr; }

// Last-workgroup reduction (a search's partials reduce without a second launch).  Thread 0
// publishes this workgroup's partial with agent-scope atomic stores (sc1: written through
// past the XCD's L2, coherent across the XCDs without an L2 writeback / invalidate -- a full
// __threadfence here drops every XCD's L2, the L2-resident query fragments with it, once per
// workgroup, and doubled a 20k-template search), waits for them to complete, and takes a
// ticket with an agent-scope atomic add; the workgroup that draws gridDim.x - 1 reads every
// partial with agent-scope (sc1) atomic loads (MI355X_MICROARCH.md, inter-workgroup
// visibility: the first hand-off row), folds them in the
// search order (exact fraction, then lowest index), writes the winner with idx + idx_base to
// fin.dst (pinned host or device memory) and resets the ticket for the next launch.
// at agent scope (sc1 stores / loads, the form of MI355X_MICROARCH.md's first hand-off row)
#define IRIS_FUSED_SCOPE __HIP_MEMORY_SCOPE_AGENT
__device__ __forceinline__ void publish_partial(Partial *p, const Partial &b) {
    uint64_t *w = (uint64_t *)p;
    __hip_atomic_store(w, (uint64_t)b.num | ((uint64_t)b.den << 32), __ATOMIC_RELAXED, IRIS_FUSED_SCOPE);
    __hip_atomic_store(w + 1, (uint64_t)(uint32_t)b.rot, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE);
    __hip_atomic_store(w + 2, b.idx, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE);
}
__device__ __forceinline__ Partial read_partial(const Partial *p) {
    uint64_t *w = (uint64_t *)p;
    const uint64_t a = __hip_atomic_load(w, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE);
    const uint64_t r = __hip_atomic_load(w + 1, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE);
    Partial q;
    q.num = (uint32_t)a;
    q.den = (uint32_t)(a >> 32);
    q.rot = (int32_t)(uint32_t)r;
    q.pad = 0;
    q.idx = __hip_atomic_load(w + 2, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE);
    return q;
}
constexpr uint32_t kTicketGroups = 8;    // sub-tickets of fold_partials_last
constexpr uint32_t kTicketStride = 64;   // words between tickets (256 B: separate lines)
// thread 0 holds this workgroup's winner b (the caller has not stored it)
__device__ __forceinline__ void fold_partials_last(Partial *partials, const Partial &b0, const FusedFinish &fin) {
    __shared__ int last;
    if (threadIdx.x == 0) {
        publish_partial(&partials[blockIdx.x], b0);
        // the stores are performed (vmcnt also counts stores on gfx9) before the ticket is taken;
        // a release fence at agent / system scope would add the L2 writeback this avoids
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // two-level ticket: workgroup b counts at sub-ticket b % 8 (its own 256-B line), the last
        // of each of those groups at the top word -- the same-address atomics of a launch are
        // serialised where they are performed, ~6 ns each, so 625 on one word cost ~4 us of tail
        const uint32_t c = blockIdx.x % kTicketGroups, groups = gridDim.x < kTicketGroups ? gridDim.x : kTicketGroups;
        const uint32_t members = (gridDim.x - c + kTicketGroups - 1) / kTicketGroups;
        uint32_t *sub = fin.ticket + kTicketStride * (1 + c);
        last = 0;
        if (__hip_atomic_fetch_add(sub, 1u, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE) == members - 1) {
            __hip_atomic_store(sub, 0u, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE);  // for the next launch
            last = __hip_atomic_fetch_add(fin.ticket, 1u, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE) == groups - 1;
        }
    }
    __syncthreads();
    if (!last) return;  // workgroup-uniform
    Partial c = partial_none();
    for (uint32_t i = threadIdx.x; i < gridDim.x; i += blockDim.x) {
        const Partial p = read_partial(&partials[i]);
        if (partial_better_dev(p, c)) c = p;
    }
    c = wave_argmin(c);
    __shared__ Partial sw[16];
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        Partial b;
        fold_waves(b, sw, (int)((blockDim.x + 63) / 64));
        if (b.den != 0) b.idx += fin.idx_base;
        __hip_atomic_store(fin.ticket, 0u, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE);  // for the next launch
        if (fin.done) {
            // write-through to the host, completed, then the sequence word the host polls
            uint64_t *w = (uint64_t *)fin.dst;
            __hip_atomic_store(w, (uint64_t)b.num | ((uint64_t)b.den << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(w + 1, (uint64_t)(uint32_t)b.rot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(w + 2, b.idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(fin.done, fin.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
            *fin.dst = b;
        }
    }
}

// Completion word of a blocking device-output call (DoneSignal): called by ONE thread of each
// workgroup once that workgroup's stores have completed (its waves waited for vmcnt(0)); the
// last workgroup to arrive (the two-level ticket of fold_partials_last) resets the ticket and
// stores the sequence number into the coherent host word the caller spins on.
__device__ __forceinline__ void signal_done_last(const DoneSignal &s) {
    const uint32_t c = blockIdx.x % kTicketGroups, groups = gridDim.x < kTicketGroups ? gridDim.x : kTicketGroups;
    const uint32_t members = (gridDim.x - c + kTicketGroups - 1) / kTicketGroups;
    uint32_t *sub = s.ticket + kTicketStride * (1 + c);
    if (__hip_atomic_fetch_add(sub, 1u, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE) != members - 1) return;
    __hip_atomic_store(sub, 0u, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE);  // for the next launch
    if (__hip_atomic_fetch_add(s.ticket, 1u, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE) != groups - 1) return;
    __hip_atomic_store(s.ticket, 0u, __ATOMIC_RELAXED, IRIS_FUSED_SCOPE);
    __hip_atomic_store(s.done, s.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace iris
