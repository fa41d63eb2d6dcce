// iris_api_search.hip — the C ABI (include/iris_hip.h): template counts, searches (blocking,
// asynchronous with their shared passes, batched) and distances.  The asynchronous search's handle
// lives by iris_pending.hpp.  Calls, locking and errors: see iris_api.hip.
#include <math.h>
#include <string.h>

#include "iris_pending.hpp"

using namespace iris;
using namespace iris_api;

int iris_api::template_args(iris_engine *e, const iris_db *db) {
    ARG(e && db, "NULL argument");
    ARG(e->kind == IRIS_KIND_TEMPLATES && e->nq == 0, "not a single-query template engine");
    ARG(db->k.kind == IRIS_KIND_TEMPLATES, "database does not hold templates");
    ARG(e->dev == db->dev, "engine and database live on different devices");
    return 0;
}

int iris_api::template_batch_args(iris_engine *e, const iris_db *db) {
    ARG(e && db, "NULL argument");
    ARG(e->kind == IRIS_KIND_TEMPLATES && e->nq > 0, "not a batched template engine");
    ARG(db->k.kind == IRIS_KIND_TEMPLATES, "database does not hold templates");
    // batches of up to kBatchStreamMax queries stream (any layout); the GEMM reads TILES
    ARG(db->k.layout == IRIS_LAYOUT_TILES || !e->sub.empty(),
        "batched search of more than 3 queries needs a template database in the TILES layout");
    ARG(e->dev == db->dev, "engine and database live on different devices");
    return 0;
}

namespace {

// A ring entry for the sharing pass about to be launched (*out = nullptr: the next entry is still in
// use, or the device has no memory to spare -- the pass then runs today's kernel and shares nothing).
int share_take(iris_device *d, uint32_t np, SharePass **out) {
    *out = nullptr;
    SharePass &s = d->share_ring[d->share_next];
    if (s.used) {
        // its kernel, and the kernel of the pass registered as its guest (whose registration wrote
        // the slot and whose hosting read qbuf and wrote done), must have ended; an entry taken again
        // since records a later point of the same stream in `ended`, which says no less
        if (hipEventQuery(s.ended) != hipSuccess) return 0;
        if (s.guest >= 0 && hipEventQuery(d->share_ring[s.guest].ended) != hipSuccess) return 0;
    }
    if (!d->share) {
        // at the highest priority, for the hardware queue: the runtime keeps its hardware queues per
        // priority and, once a process holds GPU_MAX_HW_QUEUES streams of one priority (4 by default;
        // a device with asynchronous searches has four itself), maps further streams onto the queues
        // in use.  A registration on the device stream's queue waits behind the pass that should
        // host it, and no search is ever carried (tests/test_gpu_seams.py met that).
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(hipStreamCreateWithPriority(&d->share, hipStreamNonBlocking, greatest));
    }
    if (!d->share_reg) HIPCHK(hipEventCreateWithFlags(&d->share_reg, hipEventDisableTiming));
    if (!d->share_count) {
        void *p = nullptr;
        if (dev_malloc(d, &p, 256, "sharing counter") != 0) return 0;
        d->share_count = (unsigned long long *)p;
        HIPCHK(hipMemsetAsync(p, 0, 256, d->stream));
    }
    if (!s.ended) HIPCHK(hipEventCreateWithFlags(&s.ended, hipEventDisableTiming));
    if (!s.slot) {
        void *p = nullptr;
        if (dev_malloc(d, &p, 256, "guest slot") != 0) return 0;
        s.slot = (iris::GuestSlot *)p;
    }
    if (!s.qbuf && dev_malloc(d, &s.qbuf, qalign(kTemplateTabBytes) + kTemplateFragDwords * 4, "shared query") != 0)
        return 0;
    if (ensure(d, s.done, (size_t)np * sizeof(uint32_t)) != 0) return 0;
    s.used = true;
    s.guest = -1;
    d->share_next = (d->share_next + 1) % kShareRing;
    *out = &s;
    return 0;
}

}  // namespace

int iris_api::share_join(iris_device *d, int share_host, const iris_db *db, uint64_t first, uint64_t n, uint32_t np,
                         const iris_template_t *query, hipEvent_t after, ShareKind kind, Partial *partials,
                         const MatchSink *sink, ShareJoin *out, const ReportPrep *prep) {
    *out = ShareJoin{};
    SharePass *sp = nullptr;
    if (d->hooks.search_share) CHK(share_take(d, np, &sp));
    if (!sp) return 0;
    const bool match = kind == kShareMatch;
    sp->db = db;
    sp->writes = db->writes;
    sp->first = first;
    sp->n = n;
    sp->kind = kind;
    // the pass before this one hosts it if it came from the same entry point and covers the same
    // records of the same database, unwritten since, has no guest yet and has not ended
    SharePass *host = share_host >= 0 ? &d->share_ring[share_host] : nullptr;
    const bool guest = host && host != sp && host->guest < 0 && host->kind == kind && host->db == db &&
                       host->writes == db->writes && host->first == first && host->n == n &&
                       hipEventQuery(host->ended) == hipErrorNotReady;
    // on the sharing stream: behind `after` (a search: the reduce that last read its partials
    // buffer), the slot (and done words) zeroed -- and a match pass's counter: on the device stream,
    // ahead of the pass's own launch, the zeroing would land after the hosting pass and wipe what it
    // counted for this one; a top-k pass's lists need no zeroing, every unit being stored once -- then, for a guest, its fragments built from the host copy of the query
    // (the engine's own buffer is built in device-stream order, behind the running pass) and the slot
    // of the hosting pass published
    if (after) HIPCHK(hipStreamWaitEvent(d->share, after, 0));
    if (launch_share_prepare(d->share, sp->slot, guest ? (uint32_t *)sp->done.p : nullptr, np) != 0)
        return fail(IRIS_E_HIP, "kernel launch failed: share_prepare");
    if (match) HIPCHK(hipMemsetAsync(sink->count, 0, sizeof(uint64_t), d->share));
    // a report pass's sinks and counters, for the same reason: the hosting pass reads the struct
    // once `ready` is published and adds into the counters from then on
    if (kind == kShareReport &&
        launch_report_prepare(d->share, (ReportSinks *)sink->buf, prep->sinks, prep->zero, prep->words) != 0)
        return fail(IRIS_E_HIP, "kernel launch failed: report_prepare");
    if (guest) {
        uint32_t *tab = (uint32_t *)sp->qbuf;
        uint32_t *frag = (uint32_t *)((char *)sp->qbuf + qalign(kTemplateTabBytes));
        if (launch_query_template(d->share, query, tab, frag) != 0 ||
            (sink ? launch_share_publish_match(d->share, host->slot, frag, *sink, (uint32_t *)sp->done.p)
                  : launch_share_publish(d->share, host->slot, frag, partials, (uint32_t *)sp->done.p)) != 0)
            return fail(IRIS_E_HIP, "kernel launch failed: share_publish");
        host->guest = (int)(sp - d->share_ring);
        d->share_regs[kind] += 1;
    }
    HIPCHK(hipEventRecord(d->share_reg, d->share));
    HIPCHK(hipStreamWaitEvent(d->stream, d->share_reg, 0));
    if (d->hooks.search_share_delay_us) {  // test hook: the next registration lands before this pass starts
        int khz = 0;
        HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, d->ordinal));
        if (launch_share_delay(d->stream, (uint64_t)d->hooks.search_share_delay_us * khz / 1000) != 0)
            return fail(IRIS_E_HIP, "kernel launch failed: share_delay");
    }
    out->sp = sp;
    out->own_done = guest ? (const uint32_t *)sp->done.p : nullptr;
    out->count = d->share_count + kind;
    return 0;
}

int iris_api::share_launched(iris_device *d, const ShareJoin &j) {
    if (!j.sp) return 0;
    HIPCHK(hipEventRecord(j.sp->ended, d->stream));
    d->share_last = (int)(j.sp - d->share_ring);
    return 0;
}

// Enqueues the search of [first, first+n) and its reduce, whose winner lands in
// `dst` (pinned host memory); nothing waits.  side = true (asynchronous
// searches): the reduce runs on the side stream over one of two alternating
// partials buffers, and `done` (if given) is recorded there after it.
int iris_api::search_enqueue(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, double *dist_dev,
                             Partial *dst, bool side, hipEvent_t done, uint64_t idx_base, uint32_t *host_done,
                             uint32_t seq, bool *flagged, bool share) {
    iris_device *d = e->dev;
    if (flagged) *flagged = false;
    if (n == 0) return 0;
    // only the latest search pass of the device can host, and only if this call finds it to be one
    // of the sharing form (set again below)
    const int share_host = d->share_last;
    d->share_last = -1;
    LaunchRange r{first, n};
    const int layout = db->k.layout;
    if (layout == IRIS_LAYOUT_TILES && fused_search_ok(d->hooks, r)) {
        // small range: the kernel's last workgroup reduces and writes dst itself (no reduce launch)
        CHK(ensure_ticket(d));
        CHK(ensure(d, d->partials, (size_t)mfma_search_partials(d->hooks, r) * sizeof(Partial)));
        const FusedFinish fin{(uint32_t *)d->ticket.p, dst, idx_base, host_done, seq};
        uint32_t written = 0;
        CHK(timed(d, "template_search", n, [&] {
            return launch_template_mfma(Pass::Search, d->hooks, d->stream, db->data, e->qfrag, r,
                                        {dist_dev, (Partial *)d->partials.p}, &written, &fin);
        }));
        if (flagged) *flagged = host_done != nullptr;
        if (!side) return 0;
        // later side-stream work (a group's all-gather) and `done` follow the kernel
        CHK(ensure_aux(d));
        const int b = d->apart_next;
        d->apart_next ^= 1;
        if (!d->apart_written[b]) HIPCHK(hipEventCreateWithFlags(&d->apart_written[b], hipEventDisableTiming));
        HIPCHK(hipEventRecord(d->apart_written[b], d->stream));
        HIPCHK(hipStreamWaitEvent(d->aux, d->apart_written[b], 0));
        if (done) HIPCHK(hipEventRecord(done, d->aux));
        return 0;
    }
    const uint32_t np = layout == IRIS_LAYOUT_TILES ? mfma_search_partials(d->hooks, r) : search_partials(r);
    const size_t pbytes = (size_t)std::max<uint32_t>(np, 1) * sizeof(Partial);
    DevBuf *buf = &d->partials;
    int b = 0;
    if (side) {
        CHK(ensure_aux(d));
        b = d->apart_next;
        d->apart_next ^= 1;
        buf = &d->apart[b];
        for (hipEvent_t *ev : {&d->apart_read[b], &d->apart_written[b]})
            if (!*ev) HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
        // the reduce that last read this buffer (two searches ago) precedes the overwrite
        HIPCHK(hipStreamWaitEvent(d->stream, d->apart_read[b], 0));
    }
    CHK(ensure(d, *buf, pbytes));
    Partial *part = (Partial *)buf->p;
    uint32_t written = 0;
    // the sharing form: asynchronous searches of large TILES ranges
    const bool share_form = share && side && layout == IRIS_LAYOUT_TILES && !dist_dev && e->host_query &&
                            share_search_ok(d->hooks, r);
    if (share_form) {
        ShareJoin j;
        CHK(share_join(d, share_host, db, first, n, np, e->host_query, d->apart_read[b], kShareSearch, part, nullptr,
                       &j));
        CHK(timed(d, "template_search", n, [&] {
            return launch_template_share(Pass::Search, d->hooks, d->stream, db->data, e->qfrag, r, {nullptr, part}, &written,
                                         j.sp ? j.sp->slot : nullptr, j.own_done, j.count);
        }));
        CHK(share_launched(d, j));
    } else {
        CHK(timed(d, "template_search", n, [&] {
            if (layout == IRIS_LAYOUT_TILES)
                return launch_template_mfma(Pass::Search, d->hooks, d->stream, db->data, e->qfrag, r, {dist_dev, part}, &written);
            return launch_template(Pass::Search, d->stream, db->data, e->qtab, r, {dist_dev, part}, &written);
        }));
    }
    if (!side)  // the reduce writes the winner straight into pinned host memory: no copy before the wait
        return timed(d, "reduce", written, [&] { return launch_reduce(d->stream, part, written, dst, idx_base); });
    HIPCHK(hipEventRecord(d->apart_written[b], d->stream));
    HIPCHK(hipStreamWaitEvent(d->aux, d->apart_written[b], 0));
    CHK(timed(d, "reduce", written, [&] { return launch_reduce(d->aux, part, written, dst, idx_base); }, d->aux));
    HIPCHK(hipEventRecord(d->apart_read[b], d->aux));
    if (done) HIPCHK(hipEventRecord(done, d->aux));
    return 0;
}

extern "C" {

int iris_template_counts(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint16_t *num_out,
                         uint16_t *den_out) {
    IRIS_KEEP_DEVICE();
    CHK(template_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (n == 0 || (!num_out && !den_out)) return 0;
    const uint64_t ch = 4ull << 20;
    const size_t bytes = std::min<uint64_t>(n, ch) * kRot * 2;
    CHK(ensure(d, d->out_a, bytes));
    CHK(ensure(d, d->out_b, bytes));
    for (uint64_t done = 0; done < n; done += ch) {
        const uint64_t m = std::min<uint64_t>(ch, n - done);
        LaunchRange r{first + done, m};
        uint16_t *na = num_out ? (uint16_t *)d->out_a.p : nullptr;
        uint16_t *da = den_out ? (uint16_t *)d->out_b.p : nullptr;
        CHK(timed(d, "template_counts", m, [&] {
            return db->k.layout == IRIS_LAYOUT_TILES
                       ? launch_template_mfma(Pass::Counts, d->hooks, d->stream, db->data, e->qfrag, r, {na, da})
                       : launch_template(Pass::Counts, d->stream, db->data, e->qtab, r, {na, da});
        }));
        if (num_out)
            HIPCHK(hipMemcpyAsync(num_out + done * kRot, d->out_a.p, m * kRot * 2, hipMemcpyDeviceToHost, d->stream));
        if (den_out)
            HIPCHK(hipMemcpyAsync(den_out + done * kRot, d->out_b.p, m * kRot * 2, hipMemcpyDeviceToHost, d->stream));
        CHK(sync(d));
    }
    return 0;
}

static int search_locked(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint64_t index_base,
                         double *dist_dev, iris_match_t *out) {
    iris_device *d = e->dev;
    CHK(ensure_host_result(d, sizeof(Partial)));
    // Without a device distances output the caller needs only the winner: a small (fused)
    // search publishes it with a sequence word in coherent host memory, and the call returns
    // as soon as that word lands -- no wait for the kernel's retirement and completion signal
    // (the kernel's tail is ordered before anything later enqueued on the stream).
    uint32_t *done_word = nullptr, seq = 0;
    if (!dist_dev) {
        CHK(ensure_host_done(d));
        done_word = d->host_done;
        seq = next_done_seq(d);
    }
    bool flagged = false;
    CHK(search_enqueue(e, db, first, n, dist_dev, (Partial *)d->host_result, false, nullptr, 0, done_word, seq,
                       &flagged));
    Partial res{};
    if (flagged) {
        CHK(wait_done(d, seq));
        if (d->profiling) fold_done(d);  // the timing events of earlier searches
    } else
        CHK(sync(d));
    if (n > 0) memcpy(&res, d->host_result, sizeof(Partial));
    if (out) match_from(res, n > 0, index_base + first, out);
    return 0;
}

// two queries in one streamed pass (TILES databases; LANES runs them one at a time)
static int pair_search_locked(iris_engine_t *a, iris_engine_t *b, const iris_db_t *db, uint64_t first, uint64_t n,
                              uint64_t index_base, iris_match_t *out) {
    if (db->k.layout != IRIS_LAYOUT_TILES) {
        CHK(search_locked(a, db, first, n, index_base, nullptr, out));
        return search_locked(b, db, first, n, index_base, nullptr, out + 1);
    }
    iris_device *d = a->dev;
    LaunchRange r{first, n};
    const uint32_t np = multi_search_partials(r, 2);
    CHK(ensure(d, d->partials, (size_t)std::max<uint32_t>(2 * np, 1) * sizeof(Partial)));
    CHK(ensure_host_result(d, 2 * sizeof(Partial)));
    const void *qf[2] = {a->qfrag, b->qfrag};
    uint32_t written = 0;
    CHK(timed(d, "template_batch", 2 * n, [&] {
        return launch_template_multi_search(d->stream, db->data, qf, 2, r, (Partial *)d->partials.p, &written);
    }));
    Partial res[2] = {};
    if (n > 0) {
        for (int q = 0; q < 2; ++q)
            CHK(timed(d, "reduce", written, [&] {
                return launch_reduce(d->stream, (Partial *)d->partials.p + (size_t)q * written, written,
                                     (Partial *)d->host_result + q);
            }));
    }
    CHK(sync(d));
    if (n > 0) memcpy(res, d->host_result, 2 * sizeof(Partial));
    for (int q = 0; q < 2; ++q) match_from(res[q], n > 0, index_base + first, &out[q]);
    return 0;
}

int iris_template_search(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint64_t index_base,
                         double *dist_out_device, iris_match_t *out) {
    IRIS_KEEP_DEVICE();
    CHK(template_args(e, db));
    std::lock_guard<std::recursive_mutex> g(e->dev->mu);
    CHK(set_device(e->dev));
    CHK(range_ok(db, first, n));
    ARG(out, "out is NULL");
    return search_locked(e, db, first, n, index_base, dist_out_device, out);
}

int iris_template_search_async(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                               uint64_t index_base, iris_pending_t **out) {
    IRIS_KEEP_DEVICE();
    CHK(template_args(e, db));
    ARG(out, "out is NULL");
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    iris_pending *p = nullptr;
    CHK(pending_new(d, kShareSearch, n, index_base + first, &p));
    if (n == 0) return pending_publish(p, out);
    int rc = take_result_slot(d, &p->slot);
    if (rc == 0) rc = pending_arm(p);
    if (rc == 0) rc = search_enqueue(e, db, first, n, nullptr, p->slot, true, p->ev, 0, nullptr, 0, nullptr, true);
    if (rc != 0) return pending_abandon(p, rc);
    return pending_publish(p, out);
}

int iris_pending_wait(iris_pending_t *pending, iris_match_t *out) {
    IRIS_KEEP_DEVICE();
    iris_pending *p = nullptr;
    CHK(pending_claim(pending, kShareSearch, &p));
    const hipError_t err = pending_await(p);
    Partial res{};  // copied before the lock is taken: the slot is this handle's alone
    if (p->n > 0 && err == hipSuccess) memcpy(&res, p->slot, sizeof(Partial));
    const uint64_t n = p->n, base = p->base;
    CHK(pending_retire(p, err, 0, [] { return 0; }));
    if (out) match_from(res, n > 0, base, out);
    return 0;
}

int iris_template_distances(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, double *out) {
    IRIS_KEEP_DEVICE();
    CHK(template_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (n == 0) return 0;
    ARG(out, "out is NULL");
    const uint64_t ch = 16ull << 20;
    CHK(ensure(d, d->out_a, std::min<uint64_t>(n, ch) * sizeof(double)));
    for (uint64_t done = 0; done < n; done += ch) {
        const uint64_t m = std::min<uint64_t>(ch, n - done);
        iris_match_t ignored;
        CHK(search_locked(e, db, first + done, m, 0, (double *)d->out_a.p, &ignored));
        HIPCHK(hipMemcpyAsync(out + done, d->out_a.p, m * sizeof(double), hipMemcpyDeviceToHost, d->stream));
        CHK(sync(d));
    }
    return 0;
}

int iris_template_batch_search(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint64_t index_base,
                               iris_match_t *out) {
    IRIS_KEEP_DEVICE();
    ARG(e && db && out, "NULL argument");
    CHK(template_batch_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (!e->sub.empty()) {
        uint32_t q = 0;
        for (; q + 2 <= e->nq; q += 2) CHK(pair_search_locked(e->sub[q], e->sub[q + 1], db, first, n, index_base, out + q));
        if (q < e->nq) CHK(search_locked(e->sub[q], db, first, n, index_base, nullptr, out + q));
        return 0;
    }
    LaunchRange r{first, n};
    const BatchGeometry geo = batch_geometry(d->hooks, r, e->nq);
    const uint32_t nqp = geo.nqg * geo.qper;
    std::vector<Partial> res(nqp);
    if (n > 0) {
        CHK(ensure(d, d->partials, (size_t)nqp * geo.G * sizeof(Partial)));
        CHK(ensure_host_result(d, (size_t)nqp * sizeof(Partial)));
        CHK(timed(d, "template_batch", n * e->nq, [&] {
            return launch_batch(Pass::Search, d->hooks, d->stream, db->data, e->qfrag, r, geo,
                                {(Partial *)d->partials.p, (Partial *)d->host_result});
        }));
    }
    CHK(sync(d));
    if (n > 0) memcpy(res.data(), d->host_result, nqp * sizeof(Partial));
    for (uint32_t q = 0; q < e->nq; ++q) match_from(res[q], n > 0, index_base + first, &out[q]);
    return 0;
}

}  // extern "C"
