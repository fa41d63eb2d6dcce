// iris_api_engines.hip — the C ABI (include/iris_hip.h): engines.  Their query buffers, the u16
// engine calls with their read-ahead, the distance and masks batch engines' row calls, the arch
// plugin entry points and the query-table helpers.  Calls, locking and errors: see iris_api.hip.
#include <string.h>

#include <new>

#include "iris_handles.hpp"

using namespace iris;
using namespace iris_api;

namespace {

constexpr size_t kMaskFragBytes = kMaskFragUint4 * 16;
constexpr size_t kShareFragBytes = kShareFragUint4 * 16 + 32 * 8;

// A transient device DB holding host records (the host-slice engine forms).  Its memory is the
// device's cached workspace (grown on demand, kept until the device closes): a hipMalloc + hipFree
// per call cost a participant-sized upload call ~0.1 ms.  Callers hold the device lock.
struct TempDb {
    iris_db db;
};

int temp_db(iris_device *d, int kind, uint64_t cap, TempDb &t) {
    t.db.dev = d;
    t.db.k = kind_info(kind, IRIS_LAYOUT_TILES);
    t.db.cap = (cap + t.db.k.block - 1) / t.db.k.block * t.db.k.block;
    t.db.len = 0;
    const size_t bytes = std::max<uint64_t>(1, t.db.cap / t.db.k.block) * block_bytes(t.db.k);
    CHK(ensure(d, d->tempdb, bytes));
    t.db.data = d->tempdb.p;
    // the last block's records past the range stay zero (as a fresh database's)
    HIPCHK(hipMemsetAsync(t.db.data, 0, bytes, d->stream));
    return 0;
}

constexpr uint64_t kU16Chunk = 4ull << 20;  // records per engine launch of the host-output forms

// Enqueues the engine kernel over [first, first+n) of db, [n][31] u16 rows to the device buffer
// o, on `stream` (default: the device stream); nothing waits.  sig (TILES only): the kernel's
// completion word, if the kernel chosen signals one (sig->armed).
int enqueue_u16_engine(iris_engine *e, const iris_db *db, uint64_t first, uint64_t n, uint16_t *o,
                       hipStream_t stream = nullptr, DoneSignal *sig = nullptr, bool packed = false) {
    iris_device *d = e->dev;
    if (!stream) stream = d->stream;
    LaunchRange r{first, n};
    const bool tiles = db->k.layout == IRIS_LAYOUT_TILES;
    if (sig) sig->armed = false;
    if (e->kind == IRIS_KIND_MASKS)
        return timed(d, "masks", n, [&] {
            return tiles ? launch_masks_mfma(d->hooks, stream, db->data, e->qfrag, r, o, sig, packed)
                         : launch_masks(stream, db->data, e->qtab, r, o);
        }, stream);
    return timed(d, "shares", n, [&] {
        return tiles ? launch_shares_mfma(d->hooks, stream, db->data, e->qfrag, r, o, sig)
                     : launch_shares(stream, db->data, e->qtab, r, o);
    }, stream);
}

int run_u16_engine_pinned(iris_engine *e, const iris_db *db, uint64_t first, uint64_t n, uint16_t *out);

// Engine kernel over [first, first+n) of db, u16 [n][31] outputs to host.
int run_u16_engine(iris_engine *e, const iris_db *db, uint64_t first, uint64_t n, uint16_t *out) {
    iris_device *d = e->dev;
    if (db->k.layout == IRIS_LAYOUT_TILES) {
        // out of pinned host memory for the row buffers (nothing launched yet): the device-buffer form
        const int rc = run_u16_engine_pinned(e, db, first, n, out);
        if (rc != IRIS_E_NOMEM) return rc;
    }
    CHK(ensure(d, d->out_a, std::min<uint64_t>(n, kU16Chunk) * kRot * 2));
    for (uint64_t done = 0; done < n; done += kU16Chunk) {
        const uint64_t m = std::min<uint64_t>(kU16Chunk, n - done);
        CHK(enqueue_u16_engine(e, db, first + done, m, (uint16_t *)d->out_a.p));
        HIPCHK(hipMemcpyAsync(out + done * kRot, d->out_a.p, m * kRot * 2, hipMemcpyDeviceToHost, d->stream));
        CHK(sync(d));
    }
    return 0;
}

// The host-output form of the distance and masks batch engines: chunks of records whose nq slabs
// fit the device's row buffer; enqueue(done, m, o) computes records [done, done + m) of the call's
// range into o (query q's rows at o + q * m * 31), and slab q of a chunk is copied to its place in
// the caller's query-major array.
template <class F>
int batch_rows_to_host(iris_engine *e, uint64_t n, uint16_t *out, F &&enqueue) {
    iris_device *d = e->dev;
    const uint64_t ch = std::min<uint64_t>(n, kU16Chunk / e->nq / 32 * 32);  // whole tiles
    CHK(ensure(d, d->out_a, ch * e->nq * kRot * 2));
    for (uint64_t done = 0; done < n; done += ch) {
        const uint64_t m = std::min<uint64_t>(ch, n - done);
        uint16_t *o = (uint16_t *)d->out_a.p;
        CHK(enqueue(done, m, o));
        for (uint32_t q = 0; q < e->nq; ++q)
            HIPCHK(hipMemcpyAsync(out + ((uint64_t)q * n + done) * kRot, o + (uint64_t)q * m * kRot, m * kRot * 2,
                                  hipMemcpyDeviceToHost, d->stream));
        CHK(sync(d));
    }
    return 0;
}

// ---- read-ahead of host-output engine calls (iris_handles.hpp, Readahead)

// calls of at most this many records (62 MB of rows per buffer) go through the read-ahead
constexpr uint64_t kReadaheadMax = 1ull << 20;
// A MasksEngine window's rows cross the host link packed (store_tile_packed, iris_device.hpp): 32 B
// per record, then an escape row of 31 u16 per record that only rows spanning more than a byte
// use; the copy-out expands them into the caller's [u16; 31] (parallel_expand).  The resolver's
// 20 000-mask walk is bound by its rows crossing the host link (~44 GB/s: 23 us of a 28-us call
// with the rows unpacked).
constexpr size_t kPackedRecBytes = 32;
bool ra_packed(const iris_engine *e) { return e->kind == IRIS_KIND_MASKS && e->dev->hooks.ra_packed; }
// bytes of a read-ahead buffer per record
size_t ra_rec_bytes(const iris_engine *e) { return ra_packed(e) ? kPackedRecBytes + kRot * 2 : kRot * 2; }

// A walk's read-ahead windows grow geometrically: the walk's first window is one chunk, each later
// one twice the chunks of the window before it, up to kWindowRecords records (and kWindowRowsMax of
// rows per buffer).  Consecutive windows run on two side streams, so a window's kernel starts on
// the CUs the one before it leaves while it drains: the ramp and drain of a launch (~74 us of a
// 100k-share window's 446 us on one stream, profiles/r05u_shares_window_kernels.txt) no longer
// call for big windows, and a call waits for its whole window, so windows beyond ~160k records
// only delay the host (a 3M-mask walk: 1.03e9 records/s from C++ with windows up to 880k,
// profiles/r06c_walk_host_masks.txt; measured per cap in profiles/r06d_window_caps.txt).
constexpr uint64_t kWindowRecords = 160000;
constexpr size_t kWindowRowsMax = 64ull << 20;

uint64_t window_chunks_max(const iris_db *db, uint64_t n) {
    uint64_t w = std::max<uint64_t>(1, kWindowRecords / n);
    if (db->dev->hooks.ra_window_max) w = db->dev->hooks.ra_window_max;  // test hook: another cap
    return std::max<uint64_t>(1, std::min<uint64_t>(w, kWindowRowsMax / ((size_t)n * kRot * 2)));
}

// Records of a walk's window of chunks of n records that follows a window of `prev` records (0: the
// walk's first window), with `avail` records left in the run.
uint64_t window_records(const iris_db *db, uint64_t n, uint64_t prev, uint64_t avail) {
    uint64_t w = prev ? 2 * ((prev + n - 1) / n) : 1;
    if (db->dev->hooks.ra_window) w = db->dev->hooks.ra_window;  // test hook: a fixed window
    w = std::min(w, window_chunks_max(db, n));
    return std::min<uint64_t>(w * n, avail);
}

// TILES databases only: their kernels store the rows as 16-B runs (store_tile_rows), which the
// host link takes well; the LANES kernels' 2-byte stores would each be a host-link write.
// IRIS_READAHEAD=0 turns it off (Hooks::readahead; tests run both forms).
bool readahead_ok(const iris_db *db, uint64_t n) {
    return db->dev->hooks.readahead && n <= kReadaheadMax && db->k.layout == IRIS_LAYOUT_TILES;
}

// Waits for the engine's read-ahead kernels (side streams): the row buffers may be reused or freed
// when this returns.  The windows' rows stay valid (a change of the database changes its version).
int ra_wait(iris_engine *e) {
    Readahead &ra = e->ra;
    if (!ra.computed[0]) return 0;
    iris_device *d = e->dev;
    if (d->aux) HIPCHK(hipStreamSynchronize(d->aux));
    if (d->aux2) HIPCHK(hipStreamSynchronize(d->aux2));
    if (ra.on[0] == d->stream || ra.on[1] == d->stream) HIPCHK(hipStreamSynchronize(d->stream));
    if (d->profiling) fold_done(d);
    return 0;
}

constexpr size_t kRowsPoolMax = 8;

// A pinned row buffer of at least `bytes` from the device's pool (at most twice the size), else new.
int rows_take(iris_device *d, size_t bytes, void **p, size_t *got) {
    for (size_t i = 0; i < d->rows_pool.size(); ++i) {
        const size_t b = d->rows_pool[i].first;
        if (b >= bytes && b <= 2 * bytes) {
            *p = d->rows_pool[i].second;
            *got = b;
            d->rows_pool.erase(d->rows_pool.begin() + i);
            return 0;
        }
    }
    const hipError_t err = hipHostMalloc(p, bytes, hipHostMallocDefault);
    if (err != hipSuccess) return fail(IRIS_E_NOMEM, std::string("read-ahead rows: ") + hipGetErrorString(err));
    *got = bytes;
    return 0;
}

// Back to the pool; a full pool frees its oldest buffer, so the sizes callers use now stay
// pooled (a pool full of another walk's sizes cost every later walk two hipHostMalloc and two
// hipHostFree of ~0.8 ms each, profiles/r05_rows_pool_trace.txt).
void rows_give(iris_device *d, void *p, size_t bytes) {
    if (!p) return;
    if (d->rows_pool.size() >= kRowsPoolMax) {
        (void)hipHostFree(d->rows_pool.front().second);
        d->rows_pool.erase(d->rows_pool.begin());
    }
    d->rows_pool.emplace_back(bytes, p);
}

// records per kernel of the pinned-rows form (62 MB of rows per buffer)
constexpr uint64_t kPinnedRowsChunk = 1ull << 20;

// The host-output form for TILES databases: each chunk's kernel stores its rows straight into one
// of two pinned host buffers (16-B runs over the host link, as the read-ahead does), and the helper
// threads copy them to `out` while the next chunk's kernel runs.  The copy engines' D2H into a
// caller's pageable array ran at 3-8 GB/s on some boxes (profiles/r03_host_rows.txt).  MasksEngine
// rows cross the link packed, as the read-ahead's do (ra_packed), and are expanded on the way out.
int run_u16_engine_pinned(iris_engine *e, const iris_db *db, uint64_t first, uint64_t n, uint16_t *out) {
    iris_device *d = e->dev;
    const uint64_t ch = std::min<uint64_t>(n, kPinnedRowsChunk);
    const bool pk = ra_packed(e);
    const size_t want = std::max<size_t>((size_t)ch * ra_rec_bytes(e), 4096);
    void *rows[2] = {nullptr, nullptr};
    size_t got[2] = {0, 0};
    hipEvent_t ev[2] = {nullptr, nullptr};
    const int nb = n > ch ? 2 : 1;
    int rc = 0;
    for (int b = 0; b < nb && rc == 0; ++b) {
        rc = rows_take(d, want, &rows[b], &got[b]);
        if (rc == 0 && !(ev[b] = take_event(d))) rc = fail(IRIS_E_HIP, "hipEventCreate failed");
    }
    // chunk c's rows go to rows[c & 1]; its kernel is enqueued before chunk c - 1's rows are
    // copied out, and rows[c & 1] was last read by the (synchronous) copy of chunk c - 2
    auto launch = [&](uint64_t c) -> int {
        const uint64_t a = c * ch, m = std::min<uint64_t>(ch, n - a);
        CHK(enqueue_u16_engine(e, db, first + a, m, (uint16_t *)rows[c & 1], nullptr, nullptr, pk));
        HIPCHK(hipEventRecord(ev[c & 1], d->stream));
        return 0;
    };
    const uint64_t chunks = (n + ch - 1) / ch;
    if (rc == 0) rc = launch(0);
    for (uint64_t c = 0; c < chunks && rc == 0; ++c) {
        if (c + 1 < chunks) rc = launch(c + 1);
        if (rc == 0 && hipEventSynchronize(ev[c & 1]) != hipSuccess) rc = fail(IRIS_E_HIP, "hipEventSynchronize");
        if (rc == 0) {
            const uint64_t a = c * ch, m = std::min<uint64_t>(ch, n - a);
            if (pk) {
                const uint8_t *p = (const uint8_t *)rows[c & 1];
                parallel_expand(out + a * kRot, p, (const uint16_t *)(p + m * kPackedRecBytes), m, d->ordinal);
            } else {
                parallel_copy(out + a * kRot, rows[c & 1], (size_t)m * kRot * 2, d->ordinal);
            }
        }
    }
    // on failure a kernel may still be storing into the buffers: drain before they go back
    if (rc != 0) (void)hipStreamSynchronize(d->stream);
    for (int b = 0; b < nb; ++b) {
        rows_give(d, rows[b], got[b]);
        if (ev[b]) d->event_pool.push_back(ev[b]);
    }
    if (rc == 0 && d->profiling) fold_done(d);
    return rc;
}

void ra_release(iris_engine *e) {
    Readahead &ra = e->ra;
    if (!ra.computed[0]) return;
    (void)hipSetDevice(e->dev->ordinal);
    (void)ra_wait(e);  // no kernel writes the buffers any more: they go back to the pool
    for (int b = 0; b < 2; ++b) {
        rows_give(e->dev, ra.rows[b], ra.cap);
        (void)hipEventDestroy(ra.computed[b]);
    }
    ra = Readahead{};
}

// Enqueues the engine kernel over [first, first+n) of db on the buffer's side stream (or the busy
// device stream, below); it stores
// the rows straight into the pinned buffer rows[b] (over the host link, no copy-engine DMA) and
// records computed[b]; win[b] describes them from now on.  rows[b] is not being read: the host
// copies out synchronously.  grow = false: if the buffers are too small, launch nothing
// (*launched = false) rather than reallocate them under the other window's rows.  New buffers
// hold at least `reserve` records' rows: a new engine's first call (one chunk) sizes them for the
// windows a walk from there goes on to, so they are not reallocated at its second call.
int ra_launch(iris_engine *e, const iris_db *a, uint64_t first, uint64_t n, int b, bool grow = true,
              bool *launched = nullptr, uint64_t reserve = 0) {
    Readahead &ra = e->ra;
    iris_device *d = e->dev;
    if (launched) *launched = false;
    CHK(ensure_aux(d));
    if (!ra.computed[0])
        for (int i = 0; i < 2; ++i) HIPCHK(hipEventCreateWithFlags(&ra.computed[i], hipEventDisableTiming));
    const size_t rec = ra_rec_bytes(e);
    const size_t bytes = (size_t)n * rec;
    if (bytes > ra.cap) {
        if (!grow) return 0;
        CHK(ra_wait(e));  // no kernel in flight writes either buffer
        for (int i = 0; i < 2; ++i) rows_give(d, ra.rows[i], ra.cap);
        ra.rows[0] = ra.rows[1] = nullptr;
        ra.win[0].live = ra.win[1].live = false;
        ra.cap = 0;
        const size_t want = std::max({bytes, (size_t)reserve * rec, (size_t)4096});
        size_t got[2] = {0, 0};
        for (int i = 0; i < 2; ++i) CHK(rows_take(d, want, &ra.rows[i], &got[i]));
        ra.cap = std::min(got[0], got[1]);
    }
    // ordered after everything enqueued on the device stream so far: the engine's query tables
    // (built there when the engine was created) and any write to the database.  An idle device
    // stream (the steady state of a chunk walk: its work is all on the side stream) needs no
    // event -- the cross-stream wait costs ~10 us per launch (profiles/r03_readahead.txt)
    // buffer b's windows run on their own side stream: the next window's kernel is not queued
    // behind this one's drain (the two write different buffers and only read the database)
    // An engine's first window goes on the device stream itself, behind its query tables (built
    // there just before): no query of the stream and no cross-stream event, which had cost 6-35 us
    // of a walk's first call (profiles/r06ae_first_call_phases.txt).  Nothing of the engine is in
    // flight then; by its next launch the call has waited for this window, and a busy device
    // stream orders the side stream after everything on it, this window included.
    hipStream_t side = b ? d->aux2 : d->aux;
    if (!ra.on[0] && !ra.on[1]) {
        side = d->stream;
    } else {
        const hipError_t idle = hipStreamQuery(d->stream);
        if (idle != hipSuccess) {
            if (idle != hipErrorNotReady) return fail(IRIS_E_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(idle));
            if (!d->ra_order) HIPCHK(hipEventCreateWithFlags(&d->ra_order, hipEventDisableTiming));
            HIPCHK(hipEventRecord(d->ra_order, d->stream));
            HIPCHK(hipStreamWaitEvent(side, d->ra_order, 0));
        }
    }
    ra.win[b].live = false;
    ra.on[b] = side;
    CHK(enqueue_u16_engine(e, a, first, n, (uint16_t *)ra.rows[b], side, nullptr, ra_packed(e)));
    HIPCHK(hipEventRecord(ra.computed[b], side));
    ra.win[b] = Readahead::Window{a, a->version, first, n, true};
    d->ra_launches += 1;
    d->ra_records += n;
    d->ra_window_max = std::max(d->ra_window_max, n);
    if (launched) *launched = true;
    return 0;
}

// A host-output call on records [first, first+n) of db (records [0, end) exist).  Its rows come
// from a read-ahead window that holds them (same version of the same database), else they are
// computed now -- a whole window of consecutive chunks when the call continues a walk.  While a
// window's rows are copied out, the window after it is already computed into the other buffer
// (one launch of a growing number of chunks, window_records, on the other side stream), and a
// random-access caller never pays for rows it does not ask for.  The copy is the CPU's, split
// over helper threads: the copy engines' D2H of these 1.24 MB took 31 us on one box and
// 150-275 us (8 GB/s) on others, and queued behind the side stream's event it fell into the slow
// form on boxes that had the fast one (profiles/r03_host_rows.txt, r03_readahead.txt).
int readahead_u16_call(iris_engine *e, const iris_db *a, uint64_t first, uint64_t n, uint64_t end, uint16_t *out) {
    Readahead &ra = e->ra;
    iris_device *d = e->dev;
    auto holds = [&](int b) {
        const Readahead::Window &w = ra.win[b];
        return w.live && w.db == a && w.version == a->version && w.first <= first && first + n <= w.first + w.n;
    };
    int b = holds(0) ? 0 : holds(1) ? 1 : -1;
    // a walk: this call continues where the last one ended (or was read ahead for)
    const bool walk = b >= 0 || (ra.last_db == a && ra.last_version == a->version && ra.last_end == first);
    if (b < 0) {  // a miss: into the buffer whose window starts earlier (the one a walk has left)
        b = !ra.win[0].live ? 0 : !ra.win[1].live ? 1 : ra.win[0].first <= ra.win[1].first ? 0 : 1;
        // a walk's window follows the one the walk was in; a random-access call computes its range
        const uint64_t wn = walk ? window_records(a, n, ra.grow ? ra.grow : n, end - first) : n;
        // new buffers take the walk's largest window (not reallocated under it as the windows grow)
        const uint64_t reserve = std::min<uint64_t>(window_chunks_max(a, n) * n, end - first);
        CHK(ra_launch(e, a, first, std::max(wn, n), b, true, nullptr, reserve));
        ra.grow = std::max(wn, n);
    }
    const Readahead::Window w = ra.win[b];
    ra.last_db = a;
    ra.last_version = a->version;
    ra.last_end = first + n;
    // the walk's next window, into the other buffer (whose window the walk has left behind)
    const uint64_t next = w.first + w.n;
    if (walk && next < end) {
        const Readahead::Window &o = ra.win[b ^ 1];
        if (!(o.live && o.db == a && o.version == a->version && o.first == next)) {
            const uint64_t nn = window_records(a, n, w.n, end - next);
            bool launched = false;
            CHK(ra_launch(e, a, next, nn, b ^ 1, false, &launched));
            if (launched) ra.grow = nn;
        }
    }
    HIPCHK(hipEventSynchronize(ra.computed[b]));
    const uint64_t at = first - w.first;
    if (ra_packed(e)) {
        const uint8_t *pk = (const uint8_t *)ra.rows[b];
        parallel_expand(out, pk + at * kPackedRecBytes, (const uint16_t *)(pk + w.n * kPackedRecBytes) + at * kRot, n,
                        d->ordinal);
    } else {
        parallel_copy(out, (const char *)ra.rows[b] + (size_t)at * kRot * 2, (size_t)n * kRot * 2, d->ordinal);
    }
    if (d->profiling) fold_done(d);
    return 0;
}

constexpr size_t kQpoolMax = 16;

// A query buffer of at least `bytes`: a pooled one of up to twice the size, else hipMalloc.
int qbuf_take(iris_device *d, size_t bytes, void **p, size_t *got) {
    size_t best = SIZE_MAX, bi = 0;
    for (size_t i = 0; i < d->qpool.size(); ++i) {
        const size_t b = d->qpool[i].first;
        if (b >= bytes && b <= 2 * bytes && b < best) {
            best = b;
            bi = i;
        }
    }
    if (best != SIZE_MAX) {
        *p = d->qpool[bi].second;
        *got = best;
        d->qpool.erase(d->qpool.begin() + bi);
        return 0;
    }
    CHK(dev_malloc(d, p, bytes, "query buffer"));
    *got = bytes;
    return 0;
}

}  // namespace

void iris_api::engine_free(iris_engine *e) {
    if (!e) return;
    for (iris_engine *c : e->sub) engine_free(c);
    ra_release(e);
    if (e->qbuf) {
        iris_device *d = e->dev;
        // later users of the buffer are ordered after this engine's kernels on the device stream
        if (d->qpool.size() < kQpoolMax) d->qpool.emplace_back(e->qbuf_bytes, e->qbuf);
        else (void)hipFree(e->qbuf);
    }
    delete e->host_query;
    delete e;
}

namespace {

// A new engine whose query buffer holds [table | fragments | extra] (each 256-B aligned).
int engine_alloc(iris_device *dev, int kind, size_t tab_bytes, size_t frag_bytes, size_t extra_bytes,
                 iris_engine **out, void **extra = nullptr) {
    iris_engine *e = new (std::nothrow) iris_engine();
    if (!e) return fail(IRIS_E_NOMEM, "out of host memory");
    e->dev = dev;
    e->kind = kind;
    const size_t total = qalign(tab_bytes) + qalign(frag_bytes) + qalign(extra_bytes);
    int rc = qbuf_take(dev, total, &e->qbuf, &e->qbuf_bytes);
    if (rc != 0) {
        delete e;
        return rc;
    }
    char *base = (char *)e->qbuf;
    e->qtab = tab_bytes ? base : nullptr;
    e->qfrag = frag_bytes ? base + qalign(tab_bytes) : nullptr;
    if (extra) *extra = base + qalign(tab_bytes) + qalign(frag_bytes);
    *out = e;
    return 0;
}

// Uploads host-built tables (LANES table and, optionally, TILES fragments) of a new engine.
int engine_new(iris_device *dev, int kind, const void *table, size_t bytes, iris_engine **out,
               const void *frag = nullptr, size_t frag_bytes = 0) {
    iris_engine *e = nullptr;
    CHK(engine_alloc(dev, kind, bytes, frag ? frag_bytes : 0, 0, &e));
    hipError_t err = hipMemcpyAsync(e->qtab, table, bytes, hipMemcpyHostToDevice, dev->stream);
    if (err == hipSuccess && frag) err = hipMemcpyAsync(e->qfrag, frag, frag_bytes, hipMemcpyHostToDevice, dev->stream);
    if (err != hipSuccess) {
        engine_free(e);
        return fail(IRIS_E_HIP, std::string("upload query table: ") + hipGetErrorString(err));
    }
    *out = e;
    return 0;
}

// A new engine whose tables `build(stream, host_query, tab, frag)` fills from the host
// query passed in the kernel arguments (template and mask queries, iris_query.hip).
template <class B>
int engine_from_host_query(iris_device *dev, int kind, const void *query, size_t tab_bytes, size_t frag_bytes,
                           iris_engine **out, B &&build) {
    iris_engine *e = nullptr;
    CHK(engine_alloc(dev, kind, tab_bytes, frag_bytes, 0, &e));
    if (build(dev->stream, query, (uint32_t *)e->qtab, (uint32_t *)e->qfrag) != 0) {
        const hipError_t err = hipGetLastError();
        engine_free(e);
        return fail(IRIS_E_HIP, std::string("build query tables: ") + hipGetErrorString(err));
    }
    *out = e;
    return 0;
}

// Uploads a query (`qbytes` from the host) and builds the engine's tables from it
// on the device with `build(stream, query_dev, tab, frag)` (iris_query.hip).
template <class B>
int engine_from_query(iris_device *dev, int kind, const void *query, size_t qbytes, size_t tab_bytes,
                      size_t frag_bytes, iris_engine **out, B &&build) {
    iris_engine *e = nullptr;
    void *qdev = nullptr;
    CHK(engine_alloc(dev, kind, tab_bytes, frag_bytes, qbytes, &e, &qdev));
    hipError_t err = hipMemcpyAsync(qdev, query, qbytes, hipMemcpyHostToDevice, dev->stream);
    if (err != hipSuccess || build(dev->stream, qdev, (uint32_t *)e->qtab, (uint32_t *)e->qfrag) != 0) {
        if (err == hipSuccess) err = hipGetLastError();
        engine_free(e);
        return fail(IRIS_E_HIP, std::string("build query tables: ") + hipGetErrorString(err));
    }
    *out = e;
    return 0;
}

}  // namespace

int iris_api::template_engine_locked(iris_device *d, const iris_template_t *query, iris_engine **out) {
    // [LANES table | TILES fragments], both built by one launch
    iris_template_t *copy = new (std::nothrow) iris_template_t(*query);
    if (!copy) return fail(IRIS_E_NOMEM, "out of host memory");
    const int rc = engine_from_host_query(d, IRIS_KIND_TEMPLATES, query, kTemplateTabBytes, kTemplateFragDwords * 4,
                                          out, launch_query_template);
    if (rc != 0) {
        delete copy;
        return rc;
    }
    (*out)->host_query = copy;
    return 0;
}

int iris_api::masks_batch_args(iris_engine *e, const iris_db *db) {
    ARG(e && db, "NULL argument");
    ARG(e->kind == IRIS_KIND_MASKS && e->nq > 0, "not a masks batch engine (iris_masks_batch_engine_new)");
    ARG(db->k.kind == IRIS_KIND_MASKS, "a masks batch engine needs a masks database");
    ARG(e->dev == db->dev, "engine and database live on different devices");
    return 0;
}

extern "C" {

// ------------------------------------------------------------------ engines

int iris_masks_engine_new(iris_device_t *d, const uint64_t query_mask[IRIS_LIMBS], iris_engine_t **out) {
    IRIS_KEEP_DEVICE();
    ARG(d && query_mask && out, "NULL argument");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(engine_from_host_query(d, IRIS_KIND_MASKS, query_mask, (size_t)kPlaneDwords * kSlotTabStride * 4,
                               kMaskFragBytes, out, launch_query_masks));
    device_retain(d);
    return 0;
}

int iris_distance_engine_new(iris_device_t *d, const uint16_t query[IRIS_BITS], iris_engine_t **out) {
    IRIS_KEEP_DEVICE();
    ARG(d && query && out, "NULL argument");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(engine_from_query(d, IRIS_KIND_SHARES, query, IRIS_BITS * 2, (size_t)kShareDwords * kSlotTabStride * 4,
                          kShareFragBytes, out, launch_query_shares));
    device_retain(d);
    return 0;
}

int iris_template_engine_new(iris_device_t *d, const iris_template_t *query, iris_engine_t **out) {
    IRIS_KEEP_DEVICE();
    ARG(d && query && out, "NULL argument");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(template_engine_locked(d, query, out));
    device_retain(d);
    return 0;
}

int iris_engine_destroy(iris_engine_t *e) {
    IRIS_KEEP_DEVICE();
    if (!e) return 0;
    iris_device *d = e->dev;
    {
        std::lock_guard<std::recursive_mutex> g(d->mu);
        // no wait on the device stream: the query buffer goes back to the device's pool and its
        // reuse is stream-ordered; an engine that read ahead waits for its side-stream kernels
        // before its pinned row buffers go back (ra_release)
        engine_free(e);
    }
    device_release(d);
    return 0;
}

int iris_engine_batch_process(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint16_t *out) {
    IRIS_KEEP_DEVICE();
    ARG(e && db, "NULL argument");
    ARG(e->kind == IRIS_KIND_MASKS || e->kind == IRIS_KIND_SHARES, "batch_process needs a masks or distance engine");
    ARG(e->nq == 0, "a batch engine runs through iris_distance_batch_process / iris_masks_batch_process");
    ARG(db->k.kind == e->kind, "engine kind does not match the database kind");
    ARG(e->dev == db->dev, "engine and database live on different devices");
    std::lock_guard<std::recursive_mutex> g(e->dev->mu);
    CHK(set_device(e->dev));
    CHK(range_ok(db, first, n));
    if (n == 0) return 0;
    ARG(out, "out is NULL");
    if (readahead_ok(db, n)) return readahead_u16_call(e, db, first, n, db->len, out);
    CHK(ra_wait(e));
    return run_u16_engine(e, db, first, n, out);
}

int iris_engine_batch_process_device(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                                     uint16_t *out_device) {
    IRIS_KEEP_DEVICE();
    ARG(e && db, "NULL argument");
    ARG(e->kind == IRIS_KIND_MASKS || e->kind == IRIS_KIND_SHARES, "batch_process needs a masks or distance engine");
    ARG(e->nq == 0, "a batch engine runs through iris_distance_batch_process / iris_masks_batch_process");
    ARG(db->k.kind == e->kind, "engine kind does not match the database kind");
    ARG(e->dev == db->dev, "engine and database live on different devices");
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (n == 0) return 0;
    ARG(out_device, "out is NULL");
    // a participant-sized range: the kernel's last workgroup publishes a sequence word in coherent
    // host memory once every row is stored, and the call returns when it lands (as the small
    // search does) -- later work on the device stream, the rows' consumers, follows the kernel
    DoneSignal sig{};
    if (db->k.layout == IRIS_LAYOUT_TILES) CHK(done_signal(d, &sig));
    CHK(enqueue_u16_engine(e, db, first, n, out_device, nullptr, sig.done ? &sig : nullptr));
    if (!sig.armed) return sync(d);
    CHK(wait_done(d, sig.seq));
    if (d->profiling) fold_done(d);
    return 0;
}

int iris_engine_batch_process_host(iris_engine_t *e, const void *records, uint64_t n, uint16_t *out) {
    IRIS_KEEP_DEVICE();
    ARG(e, "engine is NULL");
    ARG(e->kind == IRIS_KIND_MASKS || e->kind == IRIS_KIND_SHARES, "batch_process needs a masks or distance engine");
    ARG(e->nq == 0, "a batch engine runs through iris_distance_batch_process / iris_masks_batch_process");
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    if (n == 0) return 0;
    ARG(records && out, "NULL argument");
    const KindInfo k = kind_info(e->kind);
    // a slice of an attached host array: run on its resident copy, nothing is uploaded
    const uintptr_t p = (uintptr_t)records;
    for (iris_db *a : d->attached) {
        if (a->k.kind != e->kind || p < a->host_base) continue;
        const uintptr_t off = p - a->host_base;
        if (off % k.rec_bytes != 0 || off / k.rec_bytes > a->host_n || n > a->host_n - off / k.rec_bytes) continue;
        if (readahead_ok(a, n)) return readahead_u16_call(e, a, off / k.rec_bytes, n, a->host_n, out);
        CHK(ra_wait(e));
        return run_u16_engine(e, a, off / k.rec_bytes, n, out);
    }
    // a slice of a read-only record file mapping (the reference's participant / resolver walk):
    // run on the device's resident copy of the file (iris_resident.hip)
    iris_db *rdb = nullptr;
    uint64_t rfirst = 0, rend = 0;
    CHK(resident_slice(d, e->kind, records, n, &rdb, &rfirst, &rend));
    if (rdb) {
        PinResident pin(d, rdb);  // a workspace allocation below may evict copies: not this one
        if (readahead_ok(rdb, n)) return readahead_u16_call(e, rdb, rfirst, n, rend, out);
        CHK(ra_wait(e));
        return run_u16_engine(e, rdb, rfirst, n, out);
    }
    const uint64_t ch = std::min<uint64_t>(n, 1ull << 20 >> (e->kind == IRIS_KIND_SHARES ? 4 : 0));
    TempDb t;
    CHK(temp_db(d, e->kind, ch, t));
    for (uint64_t done = 0; done < n; done += ch) {
        const uint64_t m = std::min<uint64_t>(ch, n - done);
        t.db.len = 0;
        CHK(db_write_locked(&t.db, 0, (const char *)records + done * k.rec_bytes, m));
        CHK(run_u16_engine(e, &t.db, 0, m, out + done * kRot));
    }
    return 0;
}

// ------------------------------------------------------------------ batched queries

int iris_template_batch_engine_new(iris_device_t *d, const iris_template_t *queries, uint32_t nq, iris_engine_t **out) {
    IRIS_KEEP_DEVICE();
    ARG(d && out && (nq == 0 || queries), "NULL argument");
    ARG(nq > 0, "a batch needs at least one query");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    if (nq <= kBatchStreamMax) {
        iris_engine *e = new (std::nothrow) iris_engine();
        if (!e) return fail(IRIS_E_NOMEM, "out of host memory");
        e->dev = d;
        e->kind = IRIS_KIND_TEMPLATES;
        e->nq = nq;
        for (uint32_t i = 0; i < nq; ++i) {
            iris_engine *c = nullptr;
            const int rc = template_engine_locked(d, queries + i, &c);
            if (rc != 0) {
                engine_free(e);
                return rc;
            }
            e->sub.push_back(c);
        }
        device_retain(d);
        *out = e;
        return 0;
    }
    const uint32_t qgs = batch_query_group();
    const uint32_t nqp = (nq + qgs - 1) / qgs * qgs;  // padded to the kernel's query groups (zero tiles: no candidate)
    const size_t tile_bytes = (size_t)16 * kPlaneGroups * 64;
    CHK(engine_from_query(d, IRIS_KIND_TEMPLATES, queries, (size_t)nq * sizeof(iris_template_t), 0,
                          (size_t)nqp * tile_bytes, out, [&](void *stream, const void *q, uint32_t *, uint32_t *frag) {
                              return launch_query_tiles(stream, q, nq, nqp, frag);
                          }));
    (*out)->nq = nq;
    device_retain(d);
    return 0;
}

// ------------------------------------------------------------------ batched DistanceEngine

// nq DistanceEngines (src/lib.rs:33-40) at once: one single-query engine per query (its LANES table
// and its TILES fragments, built by the same launch as iris_distance_engine_new's), run together.
int iris_distance_batch_engine_new(iris_device_t *d, const uint16_t *queries, uint32_t nq, iris_engine_t **out) {
    IRIS_KEEP_DEVICE();
    ARG(nq > 0 && nq <= IRIS_DISTANCE_BATCH_MAX, "a distance batch holds 1..IRIS_DISTANCE_BATCH_MAX (64) queries");
    ARG(d && queries && out, "NULL argument");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    iris_engine *e = new (std::nothrow) iris_engine();
    if (!e) return fail(IRIS_E_NOMEM, "out of host memory");
    e->dev = d;
    e->kind = IRIS_KIND_SHARES;
    e->nq = nq;
    for (uint32_t i = 0; i < nq; ++i) {
        iris_engine *c = nullptr;
        const int rc = engine_from_query(d, IRIS_KIND_SHARES, queries + (size_t)i * IRIS_BITS, IRIS_BITS * 2,
                                         (size_t)kShareDwords * kSlotTabStride * 4, kShareFragBytes, &c,
                                         launch_query_shares);
        if (rc != 0) {
            engine_free(e);
            return rc;
        }
        e->sub.push_back(c);
    }
    device_retain(d);
    *out = e;
    return 0;
}

static int distance_batch_args(iris_engine_t *e, const iris_db_t *db) {
    ARG(e && db, "NULL argument");
    ARG(e->kind == IRIS_KIND_SHARES && e->nq > 0, "not a distance batch engine (iris_distance_batch_engine_new)");
    ARG(db->k.kind == IRIS_KIND_SHARES, "a distance batch engine needs a share database");
    ARG(e->dev == db->dev, "engine and database live on different devices");
    return 0;
}

// Enqueues the batch over [first, first + n): query q's rows to the device array o + q * n * 31.
// TILES: the multi-query kernels (iris_shares_batch.hip); LANES: one single-query pass per query.
// sig (TILES only): the completion word, armed if the call's last kernel signals it.
static int enqueue_distance_batch(iris_engine *e, const iris_db *db, uint64_t first, uint64_t n, uint16_t *o,
                                  DoneSignal *sig = nullptr) {
    iris_device *d = e->dev;
    const LaunchRange r{first, n};
    if (sig) sig->armed = false;
    if (db->k.layout == IRIS_LAYOUT_TILES) {
        const void *frags[IRIS_DISTANCE_BATCH_MAX];
        for (uint32_t q = 0; q < e->nq; ++q) frags[q] = e->sub[q]->qfrag;
        SharesBatchForms forms;
        CHK(timed(d, "shares_batch", n * e->nq, [&] {
            return launch_shares_batch(d->hooks, d->stream, db->data, frags, e->nq, r, o, sig, &forms);
        }));
        if (d->profiling) {
            // which kernel forms the call ran: launches = passes, items = their rows, no time of
            // their own (the whole call is timed as "shares_batch")
            auto count = [&](const char *name, uint32_t passes, uint32_t queries) {
                if (!passes) return;
                KStat &s = d->stats[name];
                s.launches += passes;
                s.items += n * queries;
            };
            count("shares_batch_large", forms.large, forms.large_queries);
            count("shares_batch_split", forms.split, forms.split_queries);
            count("shares_batch_single", forms.single, forms.single);
        }
        return 0;
    }
    for (uint32_t q = 0; q < e->nq; ++q)
        CHK(timed(d, "shares_batch", n,
                  [&] { return launch_shares(d->stream, db->data, e->sub[q]->qtab, r, o + (uint64_t)q * n * kRot); }));
    return 0;
}

int iris_distance_batch_process_device(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                                       uint16_t *out_device) {
    IRIS_KEEP_DEVICE();
    CHK(distance_batch_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (n == 0) return 0;
    ARG(out_device, "out is NULL");
    // as iris_engine_batch_process_device: where the call's last kernel is a participant-sized
    // single-query one, the call returns on the completion word that kernel writes
    DoneSignal sig{};
    if (db->k.layout == IRIS_LAYOUT_TILES) CHK(done_signal(d, &sig));
    CHK(enqueue_distance_batch(e, db, first, n, out_device, sig.done ? &sig : nullptr));
    if (!sig.armed) return sync(d);
    CHK(wait_done(d, sig.seq));
    if (d->profiling) fold_done(d);
    return 0;
}

int iris_distance_batch_process(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint16_t *out) {
    IRIS_KEEP_DEVICE();
    CHK(distance_batch_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (n == 0) return 0;
    ARG(out, "out is NULL");
    return batch_rows_to_host(e, n, out, [&](uint64_t done, uint64_t m, uint16_t *o) {
        return enqueue_distance_batch(e, db, first + done, m, o);
    });
}

// ------------------------------------------------------------------ batched MasksEngine

// nq MasksEngines (src/lib.rs:55-67) at once: one single-query engine per query (its LANES table and
// its TILES fragments, built by the same launch as iris_masks_engine_new's), run together.
int iris_masks_batch_engine_new(iris_device_t *d, const uint64_t *query_masks, uint32_t nq, iris_engine_t **out) {
    IRIS_KEEP_DEVICE();
    ARG(nq > 0 && nq <= IRIS_MASKS_BATCH_MAX, "a masks batch holds 1..IRIS_MASKS_BATCH_MAX (64) queries");
    ARG(d && query_masks && out, "NULL argument");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    iris_engine *e = new (std::nothrow) iris_engine();
    if (!e) return fail(IRIS_E_NOMEM, "out of host memory");
    e->dev = d;
    e->kind = IRIS_KIND_MASKS;
    e->nq = nq;
    for (uint32_t i = 0; i < nq; ++i) {
        iris_engine *c = nullptr;
        const int rc = engine_from_host_query(d, IRIS_KIND_MASKS, query_masks + (size_t)i * IRIS_LIMBS,
                                              (size_t)kPlaneDwords * kSlotTabStride * 4, kMaskFragBytes, &c,
                                              launch_query_masks);
        if (rc != 0) {
            engine_free(e);
            return rc;
        }
        e->sub.push_back(c);
    }
    device_retain(d);
    *out = e;
    return 0;
}

// Enqueues the batch over [first, first + n): query q's rows to the device array o + q * n * 31.
// A group of queries runs one pass of the batch kernel ("masks_batch"), a single one the
// single-query kernel ("masks").
static int enqueue_masks_batch(iris_engine *e, const iris_db *db, uint64_t first, uint64_t n, uint16_t *o) {
    iris_device *d = e->dev;
    const MasksWalk w(e, db, first, n);
    for (MasksUnit u = w.unit(0); u.m; u = w.unit(u.q0 + u.m)) {
        if (u.m == 1) {
            CHK(enqueue_u16_engine(u.one, db, first, n, o + u.q0 * w.slab));
        } else {
            CHK(timed(d, "masks_batch", n * u.m, [&] {
                return launch_masks_batch(Pass::Search, d->hooks, d->stream, db->data, u.frags, u.m, w.r, o + u.q0 * w.slab);
            }));
        }
    }
    return 0;
}

int iris_masks_batch_process_device(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                                    uint16_t *out_device) {
    IRIS_KEEP_DEVICE();
    CHK(masks_batch_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (n == 0) return 0;
    ARG(out_device, "out is NULL");
    CHK(enqueue_masks_batch(e, db, first, n, out_device));
    return sync(d);
}

int iris_masks_batch_process(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint16_t *out) {
    IRIS_KEEP_DEVICE();
    CHK(masks_batch_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (n == 0) return 0;
    ARG(out, "out is NULL");
    return batch_rows_to_host(e, n, out, [&](uint64_t done, uint64_t m, uint16_t *o) {
        return enqueue_masks_batch(e, db, first + done, m, o);
    });
}

// ------------------------------------------------------------------ arch plugin

int iris_dot_bool_batch(iris_device_t *d, const uint64_t *a, uint64_t na, const uint64_t *b, uint64_t nb,
                        uint16_t *out) {
    IRIS_KEEP_DEVICE();
    ARG(d, "device is NULL");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    if (na == 0 || nb == 0) return 0;
    ARG(a && b && out, "NULL argument");
    TempDb t;
    CHK(temp_db(d, IRIS_KIND_MASKS, nb, t));
    CHK(db_write_locked(&t.db, 0, b, nb));
    std::vector<uint16_t> tmp(nb * kRot);
    std::vector<uint32_t> tab((size_t)kPlaneDwords * kSlotTabStride);
    std::vector<uint32_t> frag(kMaskFragBytes / 4);
    for (uint64_t i0 = 0; i0 < na; i0 += kRot) {
        const int cnt = (int)std::min<uint64_t>(kRot, na - i0);
        const uint64_t *ptrs[kRot];
        for (int k = 0; k < cnt; ++k) ptrs[k] = a + (i0 + k) * IRIS_LIMBS;
        build_masks_table(ptrs, cnt, tab.data());
        build_masks_frags(ptrs, cnt, frag.data());
        iris_engine *e = nullptr;
        CHK(engine_new(d, IRIS_KIND_MASKS, tab.data(), tab.size() * 4, &e, frag.data(), kMaskFragBytes));
        int rc = run_u16_engine(e, &t.db, 0, nb, tmp.data());
        engine_free(e);
        CHK(rc);
        for (uint64_t j = 0; j < nb; ++j)
            for (int k = 0; k < cnt; ++k) out[j * na + i0 + k] = tmp[j * kRot + k];
    }
    return 0;
}

int iris_dot_u16_batch(iris_device_t *d, const uint16_t *a, uint64_t na, const uint16_t *b, uint64_t nb,
                       uint16_t *out) {
    IRIS_KEEP_DEVICE();
    ARG(d, "device is NULL");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    if (na == 0 || nb == 0) return 0;
    ARG(a && b && out, "NULL argument");
    TempDb t;
    CHK(temp_db(d, IRIS_KIND_SHARES, nb, t));
    CHK(db_write_locked(&t.db, 0, b, nb));
    std::vector<uint16_t> tmp(nb * kRot);
    std::vector<uint32_t> tab((size_t)kShareDwords * kSlotTabStride);
    std::vector<uint32_t> frag(kShareFragBytes / 4);
    for (uint64_t i0 = 0; i0 < na; i0 += kRot) {
        const int cnt = (int)std::min<uint64_t>(kRot, na - i0);
        const uint16_t *ptrs[kRot];
        for (int k = 0; k < cnt; ++k) ptrs[k] = a + (i0 + k) * IRIS_BITS;
        build_shares_table(ptrs, cnt, tab.data());
        build_shares_frags(ptrs, cnt, frag.data());
        iris_engine *e = nullptr;
        CHK(engine_new(d, IRIS_KIND_SHARES, tab.data(), tab.size() * 4, &e, frag.data(), kShareFragBytes));
        int rc = run_u16_engine(e, &t.db, 0, nb, tmp.data());
        engine_free(e);
        CHK(rc);
        for (uint64_t j = 0; j < nb; ++j)
            for (int k = 0; k < cnt; ++k) out[j * na + i0 + k] = tmp[j * kRot + k];
    }
    return 0;
}

int iris_query_table_sizes(int kind, uint32_t nq, size_t *tab_bytes, size_t *frag_bytes) {
    ARG(tab_bytes && frag_bytes, "NULL argument");
    switch (kind) {
    case IRIS_KIND_TEMPLATES:
        ARG(nq == 0 || nq > kBatchStreamMax, "nq must be 0 (single query) or a tiled batch (> 3 queries)");
        *tab_bytes = nq ? 0 : (size_t)kPlaneDwords * kTemplateTabStride * 4;
        *frag_bytes = nq ? (size_t)(nq + batch_query_group() - 1) / batch_query_group() * batch_query_group() * 16 * kPlaneGroups * 64 : kTemplateFragDwords * 4;
        return 0;
    case IRIS_KIND_MASKS:
        *tab_bytes = (size_t)kPlaneDwords * kSlotTabStride * 4;
        *frag_bytes = kMaskFragBytes;
        return 0;
    case IRIS_KIND_SHARES:
        *tab_bytes = (size_t)kShareDwords * kSlotTabStride * 4;
        *frag_bytes = kShareFragBytes;
        return 0;
    default: return fail(IRIS_E_ARG, "unknown record kind");
    }
}

int iris_engine_query_tables(const iris_engine_t *e, void *tab, size_t tab_bytes, void *frag, size_t frag_bytes) {
    IRIS_KEEP_DEVICE();
    ARG(e, "engine is NULL");
    ARG(e->sub.empty(), "a streamed template batch (<= 3 queries), distance batch or masks batch engine holds one engine per query");
    size_t tb = 0, fb = 0;
    CHK(iris_query_table_sizes(e->kind, e->nq, &tb, &fb));
    ARG(tab_bytes == tb && frag_bytes == fb, "table sizes do not match the engine's layout");
    ARG((tb == 0 || tab) && frag, "NULL argument");
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    if (tb) HIPCHK(hipMemcpyAsync(tab, e->qtab, tb, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipMemcpyAsync(frag, e->qfrag, fb, hipMemcpyDeviceToHost, d->stream));
    return sync(d);
}

int iris_host_query_tables(int kind, const void *query, uint32_t nq, void *tab, size_t tab_bytes, void *frag,
                           size_t frag_bytes) {
    ARG(query, "query is NULL");
    size_t tb = 0, fb = 0;
    CHK(iris_query_table_sizes(kind, nq, &tb, &fb));
    ARG(tab_bytes == tb && frag_bytes == fb, "table sizes do not match the layout");
    ARG((tb == 0 || tab) && frag, "NULL argument");
    if (kind == IRIS_KIND_TEMPLATES && nq) {
        const size_t tile_dw = (size_t)4 * kPlaneGroups * 64;
        memset(frag, 0, fb);
        for (uint32_t i = 0; i < nq; ++i)
            build_query_tile((const iris_template_t *)query + i, (uint32_t *)frag + i * tile_dw);
    } else if (kind == IRIS_KIND_TEMPLATES) {
        build_template_table((const iris_template_t *)query, (uint32_t *)tab);
        build_template_frags((const iris_template_t *)query, (uint32_t *)frag);
    } else if (kind == IRIS_KIND_MASKS) {
        build_masks_rotations((const uint64_t *)query, (uint32_t *)tab);
        std::vector<uint64_t> rot((size_t)kRot * IRIS_LIMBS);
        const uint64_t *ptrs[kRot];
        for (int k = 0; k < kRot; ++k) {
            bits_rotated((const uint64_t *)query, k - 15, &rot[(size_t)k * IRIS_LIMBS]);
            ptrs[k] = &rot[(size_t)k * IRIS_LIMBS];
        }
        build_masks_frags(ptrs, kRot, (uint32_t *)frag);
    } else {
        build_shares_rotations((const uint16_t *)query, (uint32_t *)tab);
        std::vector<uint16_t> rot((size_t)kRot * IRIS_BITS);
        const uint16_t *ptrs[kRot];
        for (int k = 0; k < kRot; ++k) {
            encoded_rotated((const uint16_t *)query, k - 15, &rot[(size_t)k * IRIS_BITS]);
            ptrs[k] = &rot[(size_t)k * IRIS_BITS];
        }
        build_shares_frags(ptrs, kRot, (uint32_t *)frag);
    }
    return 0;
}

}  // extern "C"
