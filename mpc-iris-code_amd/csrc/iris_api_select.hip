// iris_api_select.hip — the C ABI (include/iris_hip.h): threshold matching and top-k, single-query
// and batched, with the runners that turn launch units into match lists, the pipelined forms of
// the single-query template match and top-k (their handles live by iris_pending.hpp; here is only
// what a match or a top-k handle adds), the distance histograms of the template engines and of
// the resolver forms, and the combined pass that answers a match, a top-k and a histogram call of
// one probe from one read (iris_template_report, iris_resolver_report, iris_resolver_report_masks;
// pipelined: iris_template_report_async, whose running pass also serves the next submission),
// and of every probe of a template batch engine from one GEMM pass (iris_template_batch_report).
// Calls, locking and errors: see iris_api.hip.
#include <string.h>

#include "iris_pending.hpp"

using namespace iris;
using namespace iris_api;

extern "C" {

// ------------------------------------------------------------------ the single-query passes

// The kernel_stats name of a family's select pass; NULL for a mode the family has no pass for.
static const char *pass_name(Pass p, const char *match, const char *topk, const char *hist = nullptr,
                             const char *report = nullptr) {
    switch (p) {
    case Pass::Match: return match;
    case Pass::Topk: return topk;
    case Pass::Hist: return hist;
    case Pass::Report: return report;
    default: return nullptr;
    }
}

// One single-query template pass over r on the device stream, timed under its mode's name: the MFMA
// kernel on a TILES database (the engine's qfrag), the LANES kernel otherwise (its qtab).
static int launch_template_select(iris_device *d, const iris_db *db, const void *qtab, const void *qfrag, LaunchRange r,
                                  Pass p, const MatchSink &sink) {
    const char *name = pass_name(p, "template_match", "template_topk", "template_hist", "template_report");
    if (!name) return fail(IRIS_E_ARG, "no template pass of that mode");
    return timed(d, name, r.n, [&] {
        return db->k.layout == IRIS_LAYOUT_TILES ? launch_template_mfma(p, d->hooks, d->stream, db->data, qfrag, r, sink)
                                                 : launch_template(p, d->stream, db->data, qtab, r, sink);
    });
}

// The single-query masks form of a match, a top-k, a histogram or a report pass (sink: report_sink),
// on masks engine c and the shares of its query: a TILES database runs the fused masks_mfma_kernel; LANES the masks kernel into the
// workspace (the denominators) and then the resolver kernel.  *den: the denominators once they are
// enqueued -- a caller that launches again (the rerun of an overflowing list) while the workspace
// is still theirs keeps it, and they are not computed twice.
static int masks_single_launch(iris_device *d, const iris_engine *c, const iris_db *db, LaunchRange r,
                               const uint16_t *const *shares, uint32_t parts, Pass p, const MatchSink &sink,
                               const uint16_t **den) {
    const bool tiles = db->k.layout == IRIS_LAYOUT_TILES;
    const char *name = pass_name(p, tiles ? "masks_match" : "resolver_match", tiles ? "masks_topk" : "resolver_topk",
                                 tiles ? "masks_resolve_hist" : "resolver_hist", tiles ? "masks_report" : "resolver_report");
    if (!name) return fail(IRIS_E_ARG, "no masks pass of that mode");
    if (tiles)
        return timed(d, name, r.n, [&] {
            return launch_masks_resolve(p, d->hooks, d->stream, db->data, c->qfrag, r, shares, parts, sink);
        });
    if (!*den) CHK(enqueue_masks_denoms(c, db, r, den));
    return timed(d, name, r.n,
                 [&] { return launch_resolver(p, d->stream, shares, parts, *den, r.n, sink); });
}

// The pass of a pipelined match (kShareMatch) or top-k (kShareTopk) call over r into ms, on the
// device stream.  shared: a large TILES range -- the range the asynchronous search shares on, the
// hooks included -- runs the sharing form (§4.1) and takes a place in the ring; every other pass
// (the rerun of an overflowing match list among them) runs the blocking call's kernel and neither
// hosts nor is hosted.  query: the host copy a guest's fragments are built from.
// A report call (kShareReport): ms is report_sink of the pending's device ReportSinks and prep what
// that struct holds and the counters to clear -- on the sharing stream with a ring entry (share_join),
// else on the device stream; under IRIS_SEARCH_SHARE=0 a report runs the blocking call's kernel.
static int select_pass_enqueue(iris_device *d, const iris_db *db, LaunchRange r, const void *qtab, const void *qfrag,
                               const iris_template_t *query, ShareKind kind, const MatchSink &ms, bool shared,
                               const ReportPrep *prep = nullptr) {
    const bool match = kind == kShareMatch, report = kind == kShareReport;
    const Pass p = match ? Pass::Match : report ? Pass::Report : Pass::Topk;
    auto report_prepare = [&]() -> int {
        if (launch_report_prepare(d->stream, (ReportSinks *)ms.buf, prep->sinks, prep->zero, prep->words) != 0)
            return fail(IRIS_E_HIP, "kernel launch failed: report_prepare");
        return 0;
    };
    if (shared && db->k.layout == IRIS_LAYOUT_TILES && share_search_ok(d->hooks, r) && (!report || d->hooks.search_share)) {
        ShareJoin j;
        CHK(share_join(d, d->share_last, db, r.first, r.n, mfma_search_partials(d->hooks, r), query, nullptr, kind, nullptr,
                       &ms, &j, prep));
        d->share_last = -1;
        // a match pass's counter: share_join zeroes it on the sharing stream, but only with a ring entry
        if (match && !j.sp) HIPCHK(hipMemsetAsync(ms.count, 0, sizeof(uint64_t), d->stream));
        if (report && !j.sp) CHK(report_prepare());  // a report pass's struct and counters, likewise
        CHK(timed(d, pass_name(p, "template_match", "template_topk", nullptr, "template_report"), r.n, [&] {
            return launch_template_share(p, d->hooks, d->stream, db->data, qfrag, r, ms, nullptr,
                                         j.sp ? j.sp->slot : nullptr, j.own_done, j.count);
        }));
        return share_launched(d, j);
    }
    d->share_last = -1;  // only the device's latest pass can host
    if (match) HIPCHK(hipMemsetAsync(ms.count, 0, sizeof(uint64_t), d->stream));
    if (report) CHK(report_prepare());
    return launch_template_select(d, db, qtab, qfrag, r, p, ms);
}

// ------------------------------------------------------------------ threshold matching

// Records the first pass has room for when the caller's cap asks for fewer: a threshold that
// matters matches a handful of records, so this covers every sparse list in one pass (24 KB).
constexpr uint64_t kMatchFirstRoom = 1024;

static int matches_args(double threshold, const iris_match_t *out, uint64_t cap, const uint64_t *count) {
    ARG(threshold == threshold, "threshold is NaN");
    ARG(count, "count is NULL");
    ARG(cap == 0 || out, "out is NULL with cap > 0");
    return 0;
}

// One launch unit of a threshold-match call: queries q0 .. q0 + m - 1, whose hits one pass appends.
// launch(sinks) enqueues that pass (timed under its own names); sinks[s] is query q0 + s's.  A pass
// whose kernel takes more sinks than the unit has queries (the template batch GEMM's padding
// queries) asks for `pad` more after them: cap 0, no buffer, a zeroed counter of their own.
struct MatchUnit {
    uint32_t q0, m;
    std::function<int(const MatchSink *)> launch;
    uint32_t pad = 0;
};

// A first pass that one launch runs for all queries at once (the template batch GEMM), the units
// then being only what runs again: launch(sinks) takes nqp sinks, the queries' and the padding
// queries' after them.
struct MatchWhole {
    uint32_t nqp;
    std::function<int(const MatchSink *)> launch;
};

// What a combined pass adds to a threshold-match call whose first pass it rides on
// (iris_template_batch_report): the device's buffers are shared by region, and the other parts'
// work stands around the one wait.
struct MatchRider {
    size_t lists_bytes;             // of d->matches ahead of the queries' match regions (the top-k lists)
    size_t count_bytes;             // of d->match_count behind the counters (the histogram rows), zeroed with them
    std::function<int()> enqueue;   // on the stream behind the first pass: the merge levels, the rows' copy
    std::function<int()> taken;     // after the wait, before a rerun: their results off the pinned result, checked
};

// One threshold-match call of nq queries over n records each.  Every query has a counter of its
// own (all zeroed on the stream before the first launch) and a region of `room` records of the
// device's match buffer; the first pass -- `whole`, or else every unit's -- is enqueued before the
// one wait.  The counters always count, so a query whose hits did not fit reports how many there
// are: its unit -- that unit alone -- runs once more, its regions grown to exactly the reported
// counts (at most n records a query), one unit at a time, its records copied back before the next
// unit runs.  A query's records are then sorted by index -- the append order depends on which wave
// adds first -- and the min(count, cap) lowest become iris_match_t at out + q * cap as match_from
// fills them (idx + base).  cap == 0 needs no record, so never a second pass.  reuse_grown (the
// single-query calls): a buffer an earlier call grew is used in full by the first pass.  budget
// (0: none): the bytes all first-pass regions may take together, while a query keeps room for
// kMatchFirstRoom records -- a large cap times many queries asks for no more.
// ride (a combined pass, MatchRider): the match regions stand behind the lists; a buffer an earlier
// call grew is used in full behind them, nq equal regions; when a list overflows, the buffer grows
// once -- the lists' bytes and, where the budget allows, nq regions of the longest list -- so the
// next identical call is one pass; and the lists are held back until every unit has succeeded, so a
// failed call has written nothing (a second host copy of what the call returns: at most nq x cap records).
static int matches_run_units(iris_device *d, uint64_t n, uint64_t base, double threshold, iris_match_t *out, uint64_t cap,
                             uint64_t *counts, uint32_t nq, bool reuse_grown, const std::vector<MatchUnit> &units,
                             const MatchWhole *whole = nullptr, uint64_t budget = 0, const MatchRider *ride = nullptr) {
    const size_t lists_bytes = ride ? ride->lists_bytes : 0;
    for (uint32_t q = 0; q < nq; ++q) counts[q] = 0;
    if (n == 0) return 0;
    uint32_t nc = whole ? std::max(nq, whole->nqp) : nq;  // counters and first-pass sinks
    for (const MatchUnit &u : units) nc = std::max(nc, u.q0 + u.m + u.pad);
    const size_t count_bytes = nc * sizeof(uint64_t) + (ride ? ride->count_bytes : 0);
    CHK(ensure(d, d->match_count, count_bytes));
    CHK(ensure_host_result(d, nq * sizeof(uint64_t)));
    uint64_t room = 0;
    if (cap) {
        uint64_t want = cap;
        if (budget) want = std::min<uint64_t>(want, budget / (sizeof(Partial) * nq));
        room = std::min<uint64_t>(n, std::max<uint64_t>(want, kMatchFirstRoom));
        if (reuse_grown) room = std::max<uint64_t>(room, std::min<uint64_t>(n, d->matches.cap / sizeof(Partial)));
        if (ride && d->matches.cap > lists_bytes)  // never more than fits behind the lists
            room = std::max<uint64_t>(room, std::min<uint64_t>(n, (d->matches.cap - lists_bytes) / (sizeof(Partial) * nq)));
    }
    CHK(ensure(d, d->matches, lists_bytes + nq * room * sizeof(Partial)));
    uint64_t *cnt = (uint64_t *)d->match_count.p;
    Partial *regions = (Partial *)((char *)d->matches.p + lists_bytes);
    HIPCHK(hipMemsetAsync(cnt, 0, count_bytes, d->stream));
    std::vector<MatchSink> sinks;  // by query; a unit's own during its rerun
    std::vector<uint64_t> total, off, held_at;
    std::vector<iris_match_t> held;  // ride: the lists until every unit has succeeded
    try {
        sinks.resize(nc);
        total.resize(nq);
        if (ride) held_at.resize(nq);
        off.reserve(kMasksBatchG + 1);
    } catch (const std::bad_alloc &) {
        return fail(IRIS_E_NOMEM, "out of host memory");
    }
    for (uint32_t q = 0; q < nc; ++q)
        sinks[q] = q < nq ? MatchSink{regions + q * room, room, cnt + q, threshold}
                          : MatchSink{nullptr, 0, cnt + q, threshold};
    if (whole) {
        CHK(whole->launch(sinks.data()));
    } else {
        for (const MatchUnit &u : units) CHK(u.launch(sinks.data() + u.q0));
    }
    if (ride) CHK(ride->enqueue());
    HIPCHK(hipMemcpyAsync(d->host_result, cnt, nq * sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
    CHK(sync(d));
    memcpy(total.data(), d->host_result, nq * sizeof(uint64_t));
    for (uint32_t q = 0; q < nq; ++q)
        if (total[q] > n) return fail(IRIS_E_HIP, "match pass counted more records than the range holds");
    if (ride) CHK(ride->taken());
    // query q's total[q] records at src -> counts[q] and its list
    std::vector<Partial> recs;
    auto finish = [&](uint32_t q, const Partial *src) -> int {
        counts[q] = total[q];
        const uint64_t take = std::min(total[q], cap);
        if (take == 0) return 0;
        try {
            recs.resize(total[q]);
            if (ride) {
                held_at[q] = held.size();
                held.resize(held.size() + take);
            }
        } catch (const std::bad_alloc &) {
            return fail(IRIS_E_NOMEM, "out of host memory");
        }
        HIPCHK(hipMemcpyAsync(recs.data(), src, total[q] * sizeof(Partial), hipMemcpyDeviceToHost, d->stream));
        CHK(sync(d));
        match_list(recs.data(), total[q], take, base, ride ? held.data() + held_at[q] : out + q * cap);
        return 0;
    };
    auto overflows = [&](const MatchUnit &u) {
        for (uint32_t s = 0; cap && s < u.m; ++s)
            if (total[u.q0 + s] > room) return true;
        return false;
    };
    // the units whose lists fit first: a rerun below may replace the buffer their records are in
    for (const MatchUnit &u : units) {
        if (overflows(u)) continue;
        for (uint32_t s = 0; s < u.m; ++s) CHK(finish(u.q0 + s, regions + (u.q0 + s) * room));
    }
    if (ride && cap) {  // the first-pass room of the next identical call
        const uint64_t longest = *std::max_element(total.begin(), total.end());
        const uint64_t all = (uint64_t)nq * longest * sizeof(Partial);
        if (longest > room && (!budget || all <= budget)) CHK(ensure(d, d->matches, lists_bytes + all));
    }
    for (const MatchUnit &u : units) {
        if (!overflows(u)) continue;
        off.assign(u.m + 1, 0);
        for (uint32_t s = 0; s < u.m; ++s) off[s + 1] = off[s] + total[u.q0 + s];
        CHK(ensure(d, d->matches, lists_bytes + off[u.m] * sizeof(Partial)));
        for (uint32_t s = 0; s < u.m + u.pad; ++s)
            sinks[s] = s < u.m ? MatchSink{(Partial *)d->matches.p + off[s], total[u.q0 + s], cnt + u.q0 + s, threshold}
                               : MatchSink{nullptr, 0, cnt + u.q0 + s, threshold};
        HIPCHK(hipMemsetAsync(cnt + u.q0, 0, u.m * sizeof(uint64_t), d->stream));
        CHK(u.launch(sinks.data()));
        HIPCHK(hipMemcpyAsync(d->host_result, cnt + u.q0, u.m * sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
        CHK(sync(d));
        if (memcmp(d->host_result, total.data() + u.q0, u.m * sizeof(uint64_t)) != 0)
            return fail(IRIS_E_HIP, "match pass counts differ between two runs");
        for (uint32_t s = 0; s < u.m; ++s) CHK(finish(u.q0 + s, (const Partial *)d->matches.p + off[s]));
    }
    for (uint32_t q = 0; ride && q < nq; ++q)
        if (const uint64_t take = std::min(total[q], cap))
            memcpy(out + q * cap, held.data() + held_at[q], take * sizeof(iris_match_t));
    return 0;
}

// The single-query calls: one unit of one query.
static int matches_run(iris_device *d, uint64_t n, uint64_t base, double threshold, iris_match_t *out, uint64_t cap,
                       uint64_t *count, const std::function<int(const MatchSink &)> &launch) {
    const std::vector<MatchUnit> unit{MatchUnit{0, 1, [&](const MatchSink *ms) { return launch(ms[0]); }}};
    return matches_run_units(d, n, base, threshold, out, cap, count, 1, true, unit);
}

// iris_template_search's threshold sibling (header: "threshold matching")
int iris_template_matches(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint64_t index_base,
                          double threshold, iris_match_t *out, uint64_t cap, uint64_t *count) {
    IRIS_KEEP_DEVICE();
    CHK(matches_args(threshold, out, cap, count));  // the value arguments first: refused whatever the handles
    CHK(template_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const LaunchRange r{first, n};
    return matches_run(d, n, index_base + first, threshold, out, cap, count, [&](const MatchSink &ms) {
        return launch_template_select(d, db, e->qtab, e->qfrag, r, Pass::Match, ms);
    });
}

// ------------------------------------------------------------------ pipelined threshold matching

// iris_template_matches_async .. iris_pending_matches_wait (the handle's life:
// iris_pending.hpp).  The pass appends into the pending's device buffer; its side-stream step takes
// the counter and the first kMatchInline records to the pending's pinned slot.
struct iris_pending_matches : iris_pending {
    const iris_db *db = nullptr;  // the caller keeps it alive and unmodified until the wait
    uint64_t first = 0, cap = 0, room = 0;
    double threshold = 0;
    iris_template_t query;  // an overflowing list runs the pass again after the engine may be gone
};

static uint64_t *match_counter(const MatchBufs &b) { return (uint64_t *)b.dev.p; }
static Partial *match_records(const MatchBufs &b) { return (Partial *)((char *)b.dev.p + kMatchRecOff); }

// The pass of a pending over its range into its buffers; shared: the submission (the rerun of an
// overflowing list never shares).
static int match_pass_enqueue(iris_device *d, const iris_pending_matches *p, const void *qtab, const void *qfrag,
                              bool shared) {
    const MatchSink ms{match_records(p->bufs), p->room, match_counter(p->bufs), p->threshold};
    return select_pass_enqueue(d, p->db, LaunchRange{p->first, p->n}, qtab, qfrag, &p->query, kShareMatch, ms, shared);
}

int iris_template_matches_async(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint64_t index_base,
                                double threshold, uint64_t cap, iris_pending_t **out) {
    IRIS_KEEP_DEVICE();
    ARG(threshold == threshold, "threshold is NaN");  // the value arguments first, as iris_template_matches
    ARG(out, "out is NULL");
    CHK(template_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (!e->host_query) return fail(IRIS_E_ARG, "engine keeps no host copy of its query");
    iris_pending_matches *p = nullptr;
    CHK(pending_new(d, kShareMatch, n, index_base + first, &p));
    p->db = db;
    p->first = first;
    p->cap = cap;
    p->threshold = threshold;
    p->query = *e->host_query;
    if (n == 0) return pending_publish(p, out);
    p->room = std::min<uint64_t>(n, std::max<uint64_t>(cap, kMatchFirstRoom));
    int rc = bufs_take(d, kMatchPool, kMatchRecOff + p->room * sizeof(Partial), p);
    if (rc == 0) rc = pending_arm(p);
    if (rc == 0) rc = match_pass_enqueue(d, p, e->qtab, e->qfrag, true);
    if (rc == 0) rc = pending_side_begin(p);
    if (rc == 0) {  // the counter and the first records to the pinned slot
        const size_t bytes = kMatchRecOff + std::min<uint64_t>(p->room, kMatchInline) * sizeof(Partial);
        rc = pending_side_chk(p, hipMemcpyAsync(p->bufs.host, p->bufs.dev.p, bytes, hipMemcpyDeviceToHost, d->aux));
    }
    if (rc == 0) rc = pending_side_end(p);
    if (rc != 0) return pending_abandon(p, rc);
    return pending_publish(p, out);
}

// The list of a pending whose pass has ended (caller holds the device lock): `total` is the
// counter's value.
static int pending_matches_finish(iris_pending_matches *p, uint64_t total, iris_match_t *out) {
    iris_device *d = p->dev;
    const uint64_t take = std::min(total, p->cap);
    if (take == 0) return 0;
    std::vector<Partial> recs;
    try {
        recs.resize(total);
    } catch (const std::bad_alloc &) {
        return fail(IRIS_E_NOMEM, "out of host memory");
    }
    if (total <= std::min<uint64_t>(p->room, kMatchInline)) {
        memcpy(recs.data(), (const char *)p->bufs.host + kMatchRecOff, total * sizeof(Partial));
    } else {
        CHK(set_device(d));
        if (total > p->room) {
            // the list did not fit: the pass once more, blocking and unshared, the buffer grown to
            // exactly the reported count and the query's tables built again from the host copy
            void *q = nullptr;
            CHK(dev_malloc(d, &q, qalign(kTemplateTabBytes) + kTemplateFragDwords * 4, "match rerun query"));
            uint32_t *tab = (uint32_t *)q, *frag = (uint32_t *)((char *)q + qalign(kTemplateTabBytes));
            p->room = total;
            int rc = ensure(d, p->bufs.dev, kMatchRecOff + total * sizeof(Partial));
            if (rc == 0 && launch_query_template(d->stream, &p->query, tab, frag) != 0)
                rc = fail(IRIS_E_HIP, "kernel launch failed: query tables");
            if (rc == 0) rc = match_pass_enqueue(d, p, tab, frag, false);
            uint64_t again = 0;
            if (rc == 0 && hipMemcpyAsync(&again, match_counter(p->bufs), sizeof(again), hipMemcpyDeviceToHost, d->stream) !=
                               hipSuccess)
                rc = fail(IRIS_E_HIP, "hipMemcpyAsync failed");
            const int rs = sync(d);
            (void)hipFree(q);
            CHK(rc);
            CHK(rs);
            if (again != total) return fail(IRIS_E_HIP, "match pass counts differ between two runs");
        }
        // the rest on the second side stream, which carries nothing of a template pipeline: the
        // device stream and the first side stream may hold the passes submitted since
        HIPCHK(hipMemcpyAsync(recs.data(), match_records(p->bufs), total * sizeof(Partial), hipMemcpyDeviceToHost, d->aux2));
        HIPCHK(hipStreamSynchronize(d->aux2));
    }
    match_list(recs.data(), total, take, p->base, out);
    return 0;
}

int iris_pending_matches_wait(iris_pending_t *pending, iris_match_t *out, uint64_t *count) {
    IRIS_KEEP_DEVICE();
    iris_pending_matches *p = nullptr;
    CHK(pending_claim(pending, kShareMatch, &p));
    int rc = 0;
    if (!count) rc = fail(IRIS_E_ARG, "count is NULL");
    else if (p->cap && !out) rc = fail(IRIS_E_ARG, "out is NULL with cap > 0");
    return pending_retire(p, pending_await(p), rc, [&]() -> int {
        uint64_t total = 0;
        if (p->n > 0) memcpy(&total, p->bufs.host, sizeof(total));
        if (total > p->n) return fail(IRIS_E_HIP, "match pass counted more records than the range holds");
        CHK(pending_matches_finish(p, total, out));
        *count = total;
        return 0;
    });
}

// iris_resolver_search's threshold sibling
int iris_resolver_matches(iris_device_t *d, const uint16_t *const *shares, uint32_t parts, const uint16_t *denoms,
                          uint64_t n, uint64_t index_base, double threshold, iris_match_t *out, uint64_t cap,
                          uint64_t *count) {
    IRIS_KEEP_DEVICE();
    CHK(matches_args(threshold, out, cap, count));
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    ARG(d, "NULL argument");
    CHK(share_args(shares, parts, n, denoms != nullptr));
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    return matches_run(d, n, index_base, threshold, out, cap, count, [&](const MatchSink &ms) {
        return timed(d, "resolver_match", n, [&] { return launch_resolver(Pass::Match, d->stream, shares, parts, denoms, n, ms); });
    });
}

// iris_resolver_search_masks' threshold sibling: TILES runs the fused masks_mfma_kernel<MASKS_MATCH>;
// LANES the masks kernel into a workspace and then the resolver match kernel.
int iris_resolver_matches_masks(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                                const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                                double threshold, iris_match_t *out, uint64_t cap, uint64_t *count) {
    IRIS_KEEP_DEVICE();
    CHK(matches_args(threshold, out, cap, count));
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    CHK(single_masks_args(e, db, "iris_resolver_batch_matches_masks"));
    CHK(share_args(shares_device, parts, n));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const LaunchRange r{first, n};
    const uint16_t *den = nullptr;
    return matches_run(d, n, index_base, threshold, out, cap, count, [&](const MatchSink &ms) {
        return masks_single_launch(d, e, db, r, shares_device, parts, Pass::Match, ms, &den);
    });
}

// ------------------------------------------------------------------ top-k

static int topk_args(uint32_t k, const iris_match_t *out, const uint32_t *count) {
    ARG(k >= 1 && k <= IRIS_TOPK_MAX, "k must be 1..IRIS_TOPK_MAX (64)");
    ARG(out, "out is NULL");
    ARG(count, "count is NULL");
    return 0;
}

// the lists a single-query template top-k pass over r (not empty) writes
static uint64_t template_topk_lists(const iris_device *d, const iris_db *db, LaunchRange r) {
    return db->k.layout == IRIS_LAYOUT_TILES ? mfma_topk_units(d->hooks, r) : template_topk_units(r);
}

// One top-k call over n records: `launch` enqueues the pass whose `units` waves each store their
// k best at the lists it is given (the device's match buffer: units lists, then the merge's spare
// lists), the merge levels follow on the stream and the last one writes k records to the pinned
// host result -- 24 k bytes whatever n is -- and the call waits once.  The list is sorted with the
// empty entries (den = 0) last, so the count is the length of its valid prefix.
static int topk_run(iris_device *d, uint64_t n, uint64_t base, uint32_t k, iris_match_t *out, uint32_t *count,
                    uint64_t units, const std::function<int(const MatchSink &)> &launch) {
    *count = 0;
    if (n == 0) return 0;
    CHK(ensure(d, d->matches, (units + topk_spare_lists(units)) * k * sizeof(Partial)));
    CHK(ensure_host_result(d, (size_t)k * sizeof(Partial)));
    Partial *lists = (Partial *)d->matches.p, *spare = lists + units * k;
    CHK(launch(topk_sink(lists, k)));
    CHK(timed(d, "topk_merge", units,
              [&] { return launch_topk_merge(d->stream, lists, spare, units, k, (Partial *)d->host_result); }));
    CHK(sync(d));
    *count = topk_list((const Partial *)d->host_result, k, base, out);
    return 0;
}

// iris_template_search's top-k sibling (header: "top-k")
int iris_template_topk(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint64_t index_base,
                       uint32_t k, iris_match_t *out, uint32_t *count) {
    IRIS_KEEP_DEVICE();
    CHK(topk_args(k, out, count));  // the value arguments first: refused whatever the handles
    CHK(template_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const LaunchRange r{first, n};
    const uint64_t units = n ? template_topk_lists(d, db, r) : 0;
    return topk_run(d, n, index_base + first, k, out, count, units, [&](const MatchSink &ts) {
        return launch_template_select(d, db, e->qtab, e->qfrag, r, Pass::Topk, ts);
    });
}

// ------------------------------------------------------------------ pipelined top-k

// iris_template_topk_async .. iris_pending_topk_wait (the handle's life:
// iris_pending.hpp).  The pass stores its lists into the pending's device buffer; its side-stream
// step is the merge, whose last level writes the k records to the pending's pinned slot -- as the
// blocking call's writes the device's pinned result.
struct iris_pending_topk : iris_pending {
    uint32_t k = 0;
};

int iris_template_topk_async(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint64_t index_base,
                             uint32_t k, iris_pending_t **out) {
    IRIS_KEEP_DEVICE();
    ARG(k >= 1 && k <= IRIS_TOPK_MAX, "k must be 1..IRIS_TOPK_MAX (64)");  // the value arguments first
    ARG(out, "out is NULL");
    CHK(template_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (!e->host_query) return fail(IRIS_E_ARG, "engine keeps no host copy of its query");
    iris_pending_topk *p = nullptr;
    CHK(pending_new(d, kShareTopk, n, index_base + first, &p));
    p->k = k;
    if (n == 0) return pending_publish(p, out);
    const LaunchRange r{first, n};
    const uint64_t units = template_topk_lists(d, db, r);
    int rc = bufs_take(d, kTopkPool, (units + topk_spare_lists(units)) * k * sizeof(Partial), p);
    if (rc == 0) rc = pending_arm(p);
    Partial *lists = (Partial *)p->bufs.dev.p, *spare = lists + units * k;
    if (rc == 0)
        rc = select_pass_enqueue(d, db, r, e->qtab, e->qfrag, e->host_query, kShareTopk, topk_sink(lists, k), true);
    if (rc == 0) rc = pending_side_begin(p);
    if (rc == 0)  // the merge, whose last level writes the pinned slot
        rc = timed(d, "topk_merge", units,
                   [&] { return launch_topk_merge(d->aux, lists, spare, units, k, (Partial *)p->bufs.host); }, d->aux);
    if (rc == 0) rc = pending_side_end(p);
    if (rc != 0) return pending_abandon(p, rc);
    return pending_publish(p, out);
}

int iris_pending_topk_wait(iris_pending_t *pending, iris_match_t *out, uint32_t *count) {
    IRIS_KEEP_DEVICE();
    iris_pending_topk *p = nullptr;
    CHK(pending_claim(pending, kShareTopk, &p));
    int rc = 0;
    if (!out) rc = fail(IRIS_E_ARG, "out is NULL");
    else if (!count) rc = fail(IRIS_E_ARG, "count is NULL");
    return pending_retire(p, pending_await(p), rc, [&] {
        *count = p->n > 0 ? topk_list((const Partial *)p->bufs.host, p->k, p->base, out) : 0;
        return 0;
    });
}

// iris_resolver_search's top-k sibling
int iris_resolver_topk(iris_device_t *d, const uint16_t *const *shares, uint32_t parts, const uint16_t *denoms,
                       uint64_t n, uint64_t index_base, uint32_t k, iris_match_t *out, uint32_t *count) {
    IRIS_KEEP_DEVICE();
    CHK(topk_args(k, out, count));
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    ARG(d, "NULL argument");
    CHK(share_args(shares, parts, n, denoms != nullptr));
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    return topk_run(d, n, index_base, k, out, count, resolver_topk_units(n), [&](const MatchSink &ts) {
        return timed(d, "resolver_topk", n, [&] { return launch_resolver(Pass::Topk, d->stream, shares, parts, denoms, n, ts); });
    });
}

// iris_resolver_search_masks' top-k sibling: TILES runs the fused masks_mfma_kernel<MASKS_TOPK>;
// LANES the masks kernel into a workspace and then the resolver top-k kernel.
int iris_resolver_topk_masks(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                             const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base, uint32_t k,
                             iris_match_t *out, uint32_t *count) {
    IRIS_KEEP_DEVICE();
    CHK(topk_args(k, out, count));
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    CHK(single_masks_args(e, db, "iris_resolver_batch_topk_masks"));
    CHK(share_args(shares_device, parts, n));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const LaunchRange r{first, n};
    const uint64_t units = db->k.layout != IRIS_LAYOUT_TILES ? resolver_topk_units(n) : n ? masks_topk_units(d->hooks, r) : 0;
    const uint16_t *den = nullptr;
    return topk_run(d, n, index_base, k, out, count, units, [&](const MatchSink &ts) {
        return masks_single_launch(d, e, db, r, shares_device, parts, Pass::Topk, ts, &den);
    });
}

// A launch unit of a batched top-k call: m queries from q0 on (a masks pass: m <= kMasksBatchG; the
// template batch GEMM: all of them) whose pass writes `lists` lists of k records per query;
// launch(base, stride) enqueues the pass(es), query q0 + s storing its lists at base + s * stride.
// A pass whose kernel writes lists for more queries than the unit has (the GEMM's padding queries)
// asks for `pad` more regions after them; nobody reads those.
struct TopkUnit {
    uint32_t q0, m;
    uint64_t lists;
    std::function<int(Partial *, uint64_t)> launch;
    uint32_t pad = 0;
};

// A merge launch takes at most this many queries (blockIdx.y, launch_topk_merge_level)
constexpr uint32_t kTopkMergeSlots = 65535;

// The merge levels of m queries whose `lists` lists of k records each stand `stride` records apart
// from `region` on (the spare lists behind each query's own), on the stream: one launch per level
// for the queries together (launch_topk_merge_level; more than kTopkMergeSlots queries: one launch
// per kTopkMergeSlots of them).  The last level writes query s's k records at res + s * k.
static int topk_merge_enqueue(iris_device *d, Partial *region, uint64_t lists, uint64_t stride, uint32_t k, uint32_t m,
                              Partial *res) {
    Partial *src = region, *dst = region + lists * k;
    for (uint64_t left = lists;;) {
        const uint64_t groups = topk_spare_lists(left);
        const bool last = groups == 1;
        for (uint32_t s0 = 0; s0 < m; s0 += kTopkMergeSlots) {
            const uint32_t slots = std::min(kTopkMergeSlots, m - s0);
            CHK(timed(d, "topk_merge", left * slots, [&] {
                return launch_topk_merge_level(d->stream, src + s0 * stride, left, k,
                                               last ? res + (size_t)s0 * k : dst + s0 * stride, slots, stride,
                                               last ? k : stride);
            }));
        }
        if (last) return 0;
        left = groups;
        std::swap(src, dst);
    }
}

// topk_run for the nq queries of a batch engine.  One lists region of the device's match buffer
// -- per query of a unit its lists and then the merge's spare lists, (lists + spare) * k records
// -- serves every unit in stream order: a unit's merge has consumed the
// region before the next unit's pass writes it.  Each unit's pass is followed by its merge levels,
// one launch per level for the unit's queries together (launch_topk_merge_level; a unit of more
// than kTopkMergeSlots queries: one launch per kTopkMergeSlots of them); the last level
// writes query q's k records at q * k of the pinned host result.  The call waits once; every
// query's count is the length of its list's valid prefix.
static int topk_run_units(iris_device *d, uint64_t n, uint64_t base, uint32_t k, iris_match_t *out, uint32_t *counts,
                          uint32_t nq, const std::vector<TopkUnit> &units) {
    for (uint32_t q = 0; q < nq; ++q) counts[q] = 0;
    if (n == 0) return 0;
    uint64_t room = 0;
    for (const TopkUnit &u : units) room = std::max(room, (uint64_t)(u.m + u.pad) * (u.lists + topk_spare_lists(u.lists)) * k);
    CHK(ensure(d, d->matches, room * sizeof(Partial)));
    CHK(ensure_host_result(d, (size_t)nq * k * sizeof(Partial)));
    Partial *region = (Partial *)d->matches.p, *res = (Partial *)d->host_result;
    for (const TopkUnit &u : units) {
        const uint64_t stride = (u.lists + topk_spare_lists(u.lists)) * k;
        CHK(u.launch(region, stride));
        CHK(topk_merge_enqueue(d, region, u.lists, stride, k, u.m, res + (size_t)u.q0 * k));
    }
    CHK(sync(d));
    for (uint32_t q = 0; q < nq; ++q) counts[q] = topk_list(res + (size_t)q * k, k, base, out + (size_t)q * k);
    return 0;
}

// iris_resolver_batch_search_masks' top-k sibling, with iris_resolver_batch_matches_masks' dispatch:
// TILES ranges the batch kernel runs walk the queries in groups of kMasksBatchG, each group one pass
// of masks_batch_kernel<BATCH_TOPK> ("masks_batch_topk") storing every wave's list per query, a
// single left-over query one fused single-query pass on its slab; other TILES ranges one such pass
// per query; LANES the masks kernel into the workspace and the resolver top-k kernel per query.
int iris_resolver_batch_topk_masks(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                                   const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base, uint32_t k,
                                   iris_match_t *out, uint32_t *counts) {
    IRIS_KEEP_DEVICE();
    ARG(k >= 1 && k <= IRIS_TOPK_MAX, "k must be 1..IRIS_TOPK_MAX (64)");
    ARG(out, "out is NULL");
    ARG(counts, "counts is NULL");
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    CHK(masks_batch_args(e, db));
    CHK(share_args(shares_device, parts, n));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const MasksWalk w(e, db, first, n);
    std::vector<TopkUnit> units;
    for (MasksUnit u = w.unit(0); n && u.m; u = w.unit(u.q0 + u.m)) {
        if (u.m > 1) {
            units.push_back(TopkUnit{u.q0, u.m, masks_batch_topk_units(d->hooks, w.r, u.m), [=](Partial *lists, uint64_t stride) {
                return timed(d, "masks_batch_topk", n * u.m, [&] {
                    return launch_masks_batch(Pass::Topk, d->hooks, d->stream, db->data, u.frags, u.m, w.r,
                                              {shares_device, parts, u.q0, lists, stride, k});
                });
            }});
        } else {
            // one query through the single-query forms, on its slab of every part
            const uint64_t lists = w.tiles ? masks_topk_units(d->hooks, w.r) : resolver_topk_units(n);
            units.push_back(TopkUnit{u.q0, 1, lists, [=](Partial *buf, uint64_t) {
                const uint16_t *sl[8], *den = nullptr;
                w.slabs(u.q0, shares_device, parts, sl);
                return masks_single_launch(d, u.one, db, w.r, sl, parts, Pass::Topk, topk_sink(buf, k), &den);
            }});
        }
    }
    return topk_run_units(d, n, index_base, k, out, counts, e->nq, units);
}

// iris_resolver_batch_search_masks' threshold sibling, and that call's dispatch: TILES ranges the
// batch kernel runs walk the queries in groups of kMasksBatchG, each group one pass of
// masks_batch_kernel<BATCH_MATCH> ("masks_batch_match") appending to the group's sinks, a single
// left-over query one fused single-query pass; other TILES ranges one such pass per query; LANES
// the masks kernel into the workspace and the resolver match kernel per query.  A launch unit -- a
// group or a single query -- is what matches_run_units runs again when one of its lists overflows.
int iris_resolver_batch_matches_masks(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                                      const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                                      double threshold, iris_match_t *out, uint64_t cap, uint64_t *counts) {
    IRIS_KEEP_DEVICE();
    CHK(matches_args(threshold, out, cap, counts));
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    CHK(masks_batch_args(e, db));
    CHK(share_args(shares_device, parts, n));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const MasksWalk w(e, db, first, n);
    std::vector<MatchUnit> units;
    for (MasksUnit u = w.unit(0); n && u.m; u = w.unit(u.q0 + u.m)) {
        if (u.m > 1) {
            units.push_back(MatchUnit{u.q0, u.m, [=](const MatchSink *ms) {
                return timed(d, "masks_batch_match", n * u.m, [&] {
                    return launch_masks_batch(Pass::Match, d->hooks, d->stream, db->data, u.frags, u.m, w.r,
                                              {shares_device, parts, u.q0, ms});
                });
            }});
        } else {
            // one query through the single-query forms, on its slab of every part
            units.push_back(MatchUnit{u.q0, 1, [=](const MatchSink *ms) {
                const uint16_t *sl[8], *den = nullptr;
                w.slabs(u.q0, shares_device, parts, sl);
                return masks_single_launch(d, u.one, db, w.r, sl, parts, Pass::Match, ms[0], &den);
            }});
        }
    }
    return matches_run_units(d, n, index_base, threshold, out, cap, counts, e->nq, false, units);
}

// The bytes the first pass of iris_template_batch_matches gives all queries' regions together (a
// design constant): 1024 queries with a large cap then ask for 256 MiB, not for
// cap x 1024 records.
constexpr uint64_t kBatchMatchBudget = 256ull << 20;

// The GEMM's match passes (iris_template_batch_matches, and the reruns of iris_template_batch_report).
// The sinks cross to the device from pinned memory, so the copy is a plain asynchronous one on the
// stream: the device's pinned result words past the nq counts the call reads back.  The caller has
// ensured d->match_sinks (batch_padded(nq) sinks) and the pinned result up to the staged sinks' end.
static uint32_t batch_padded(uint32_t nq) {  // the engine's padded queries (zero tiles)
    const uint32_t bq = batch_query_group();
    return (nq + bq - 1) / bq * bq;
}
static size_t batch_stage_off(uint32_t nq) { return (nq * sizeof(uint64_t) + 63) / 64 * 64; }
// the sinks of queries q0 .. q0 + m - 1 and of the padding queries that fill their last block
// (host) -> their places in the device array; every pass but the first follows a wait, so the
// staged sinks are never overwritten in flight
static int batch_sinks_stage(iris_device *d, uint32_t nq, uint32_t q0, uint32_t m, const MatchSink *ms) {
    const uint32_t mp = batch_padded(m);
    MatchSink *stage = (MatchSink *)((char *)d->host_result + batch_stage_off(nq)) + q0;
    memcpy(stage, ms, mp * sizeof(MatchSink));
    HIPCHK(hipMemcpyAsync((MatchSink *)d->match_sinks.p + q0, stage, mp * sizeof(MatchSink), hipMemcpyHostToDevice, d->stream));
    return 0;
}
// those sinks staged, then the match pass over those queries' tiles
static int batch_match_pass(iris_device *d, const iris_engine *e, const iris_db *db, LaunchRange r, uint32_t q0, uint32_t m,
                            const MatchSink *ms) {
    const size_t tile_bytes = (size_t)16 * kPlaneGroups * 64;
    CHK(batch_sinks_stage(d, e->nq, q0, m, ms));
    const BatchGeometry geo = batch_geometry(d->hooks, r, m);
    return timed(d, "template_batch_match", r.n * m, [&] {
        return launch_batch(Pass::Match, d->hooks, d->stream, db->data, (const char *)e->qfrag + q0 * tile_bytes, r, geo,
                            (const MatchSink *)d->match_sinks.p + q0);
    });
}
// what runs again when a list overflows: the aligned blocks of batch_query_group() queries
static std::vector<MatchUnit> batch_match_units(iris_device *d, const iris_engine *e, const iris_db *db, LaunchRange r) {
    const uint32_t bq = batch_query_group(), nq = e->nq;
    std::vector<MatchUnit> units;
    for (uint32_t q0 = 0; q0 < nq; q0 += bq) {
        const uint32_t m = std::min(bq, nq - q0);
        units.push_back(MatchUnit{q0, m, [=](const MatchSink *ms) { return batch_match_pass(d, e, db, r, q0, m, ms); }, bq - m});
    }
    return units;
}

// iris_template_batch_search's threshold sibling, and that call's checks and dispatch.  Engines of
// up to kBatchStreamMax queries: one single-query match pass per query ("template_match"), all
// enqueued before the one wait.  The GEMM: one launch of batch_lds_kernel<..., BL_MATCH>
// ("template_batch_match") over all query groups, every query appending to its own sink of the
// device array d->match_sinks; what runs again when a list overflows is the aligned block of
// batch_query_group() queries, independent of the kernel shape, launched on its own query tiles.
int iris_template_batch_matches(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint64_t index_base,
                                double threshold, iris_match_t *out, uint64_t cap, uint64_t *counts) {
    IRIS_KEEP_DEVICE();
    CHK(matches_args(threshold, out, cap, counts));  // the value arguments first: refused whatever the handles
    CHK(template_batch_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const uint32_t nq = e->nq;
    const LaunchRange r{first, n};
    const uint64_t base = index_base + first;
    std::vector<MatchUnit> units;
    if (!e->sub.empty()) {
        for (uint32_t q = 0; n && q < nq; ++q) {
            const iris_engine *c = e->sub[q];
            units.push_back(MatchUnit{q, 1, [=](const MatchSink *ms) {
                return launch_template_select(d, db, c->qtab, c->qfrag, r, Pass::Match, ms[0]);
            }});
        }
        return matches_run_units(d, n, base, threshold, out, cap, counts, nq, false, units, nullptr, kBatchMatchBudget);
    }
    const uint32_t nqp = batch_padded(nq);
    if (n) {
        CHK(ensure(d, d->match_sinks, nqp * sizeof(MatchSink)));
        CHK(ensure_host_result(d, batch_stage_off(nq) + nqp * sizeof(MatchSink)));
        units = batch_match_units(d, e, db, r);
    }
    const MatchWhole whole{nqp, [=](const MatchSink *ms) { return batch_match_pass(d, e, db, r, 0, nq, ms); }};
    return matches_run_units(d, n, base, threshold, out, cap, counts, nq, false, units, &whole, kBatchMatchBudget);
}

// iris_template_batch_search's top-k sibling, with iris_template_batch_matches' checks and dispatch.
// Engines of up to kBatchStreamMax queries: one single-query top-k pass per query ("template_topk")
// and its merge, all enqueued before the one wait.  The GEMM: one launch of
// batch_lds_kernel<..., BL_TOPK> ("template_batch_topk") over all query groups, every wave storing
// one list per query of its own -- 8 G lists a query in both kernel shapes -- and then the merge
// levels for all queries together.  The lists region holds nqp (8 G + ceil(8 G / 64)) k records
// (DESIGN.md 4.14); top-k always fits, so there is no overflow rule and no second pass.
int iris_template_batch_topk(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint64_t index_base,
                             uint32_t k, iris_match_t *out, uint32_t *counts) {
    IRIS_KEEP_DEVICE();
    ARG(k >= 1 && k <= IRIS_TOPK_MAX, "k must be 1..IRIS_TOPK_MAX (64)");  // the value arguments first
    ARG(out, "out is NULL");
    ARG(counts, "counts is NULL");
    CHK(template_batch_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const uint32_t nq = e->nq;
    const LaunchRange r{first, n};
    const uint64_t base = index_base + first;
    std::vector<TopkUnit> units;
    if (!e->sub.empty()) {
        const uint64_t lists = n ? template_topk_lists(d, db, r) : 0;
        for (uint32_t q = 0; n && q < nq; ++q) {
            const iris_engine *c = e->sub[q];
            units.push_back(TopkUnit{q, 1, lists, [=](Partial *buf, uint64_t) {
                return launch_template_select(d, db, c->qtab, c->qfrag, r, Pass::Topk, topk_sink(buf, k));
            }});
        }
        return topk_run_units(d, n, base, k, out, counts, nq, units);
    }
    if (n) {
        const BatchGeometry geo = batch_geometry(d->hooks, r, nq);
        units.push_back(TopkUnit{0, nq, batch_topk_units(geo), [=](Partial *lists, uint64_t stride) {
            return timed(d, "template_batch_topk", n * nq, [&] {
                return launch_batch(Pass::Topk, d->hooks, d->stream, db->data, e->qfrag, r, geo, {lists, stride, k});
            });
        }, geo.nqg * geo.qper - nq});
    }
    return topk_run_units(d, n, base, k, out, counts, nq, units);
}

// ------------------------------------------------------------------ histograms

static int hist_args(uint32_t nbins, const uint64_t *bins, const uint64_t *invalid) {
    ARG(nbins >= 1 && nbins <= IRIS_HIST_MAX_BINS && (nbins & (nbins - 1)) == 0,
        "nbins must be a power of two in 1..IRIS_HIST_MAX_BINS (1024)");
    ARG(bins, "bins is NULL");
    ARG(invalid, "invalid is NULL");
    return 0;
}

// Whether each of the nq rows of nbins + 1 counters at res adds up to the range.
static int hist_rows_check(const uint64_t *res, uint64_t n, uint32_t nbins, uint32_t nq) {
    const size_t words = (size_t)nbins + 1;
    for (uint32_t q = 0; q < nq; ++q) {
        uint64_t sum = 0;
        for (size_t i = 0; i < words; ++i) sum += res[q * words + i];
        if (sum != n) return fail(IRIS_E_HIP, "histogram pass did not count every record of the range once");
    }
    return 0;
}

// checked rows -> the caller's arrays
static void hist_rows_write(const uint64_t *res, uint32_t nbins, uint32_t nq, uint64_t *bins, uint64_t *invalid) {
    const size_t words = (size_t)nbins + 1;
    for (uint32_t q = 0; q < nq; ++q) {
        memcpy(bins + (size_t)q * nbins, res + q * words, nbins * sizeof(uint64_t));
        invalid[q] = res[q * words + nbins];
    }
}

// The nq rows of nbins + 1 counters at res (bins, then the invalid count; null: the pinned host
// result) -> the caller's arrays, once every row adds up to the range: nothing is written before that.
static int hist_finish(iris_device *d, uint64_t n, uint32_t nbins, uint32_t nq, uint64_t *bins, uint64_t *invalid,
                       const uint64_t *res = nullptr) {
    if (!res) res = (const uint64_t *)d->host_result;
    CHK(hist_rows_check(res, n, nbins, nq));
    hist_rows_write(res, nbins, nq, bins, invalid);
    return 0;
}

// the histograms of an empty range
static int hist_empty(uint32_t nq, uint32_t nbins, uint64_t *bins, uint64_t *invalid) {
    memset(bins, 0, (size_t)nq * nbins * sizeof(uint64_t));
    memset(invalid, 0, nq * sizeof(uint64_t));
    return 0;
}

// One histogram call of nq queries over n records each (iris_template_histogram: nq = 1; a batch
// engine of up to kBatchStreamMax queries; the resolver forms).  Query q has `copies` copies of its
// nbins + 1 counters in the device's counter buffer, all zeroed on the stream first; enqueue(sinks)
// launches every pass of the call, sinks[q] being query q's -- a pass ("template_hist", ...) adds every
// workgroup's LDS histogram to copy blockIdx.x % copies -- "hist_reduce" sums the copies of all
// queries straight into the pinned host result, and the call waits once.  copies = 1 (the
// IRIS_HIST_COPIES=1 test hook): the passes add into the result itself and a copy brings it back
// (DESIGN.md 4.17 and 4.18 have both measured).  A histogram always fits, so there is no second pass.
static int hist_run_all(iris_device *d, uint64_t n, uint32_t nbins, uint64_t *bins, uint64_t *invalid, uint32_t nq,
                        const std::function<int(const MatchSink *)> &enqueue) {
    if (n == 0) return hist_empty(nq, nbins, bins, invalid);
    const uint32_t words = nbins + 1, copies = d->hooks.hist_copies ? d->hooks.hist_copies : kHistCopies;
    const size_t row = (size_t)copies * words;
    CHK(ensure(d, d->match_count, nq * row * sizeof(uint64_t)));
    CHK(ensure_host_result(d, (size_t)nq * words * sizeof(uint64_t)));
    uint64_t *cnt = (uint64_t *)d->match_count.p;
    HIPCHK(hipMemsetAsync(cnt, 0, nq * row * sizeof(uint64_t), d->stream));
    std::vector<MatchSink> sinks(nq);
    for (uint32_t q = 0; q < nq; ++q) sinks[q] = hist_sink(cnt + q * row, nbins, copies);
    CHK(enqueue(sinks.data()));
    if (copies > 1)
        CHK(timed(d, "hist_reduce", nq * row, [&] {
            return launch_hist_reduce(d->stream, cnt, words, copies, nq, (uint64_t *)d->host_result);
        }));
    else
        HIPCHK(hipMemcpyAsync(d->host_result, cnt, (size_t)nq * words * sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
    CHK(sync(d));
    return hist_finish(d, n, nbins, nq, bins, invalid);
}

// hist_run_all of one single-query pass per query: launch(q, sink) enqueues query q's
static int hist_run(iris_device *d, uint64_t n, uint32_t nbins, uint64_t *bins, uint64_t *invalid, uint32_t nq,
                    const std::function<int(uint32_t, const MatchSink &)> &launch) {
    return hist_run_all(d, n, nbins, bins, invalid, nq, [&](const MatchSink *sinks) {
        for (uint32_t q = 0; q < nq; ++q) CHK(launch(q, sinks[q]));
        return 0;
    });
}

// iris_template_search's histogram sibling (header: "histograms")
int iris_template_histogram(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint32_t nbins,
                            uint64_t *bins, uint64_t *invalid) {
    IRIS_KEEP_DEVICE();
    CHK(hist_args(nbins, bins, invalid));  // the value arguments first: refused whatever the handles
    CHK(template_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const LaunchRange r{first, n};
    return hist_run(d, n, nbins, bins, invalid, 1, [&](uint32_t, const MatchSink &hs) {
        return launch_template_select(d, db, e->qtab, e->qfrag, r, Pass::Hist, hs);
    });
}

// iris_template_batch_search's histogram sibling, with iris_template_batch_matches' checks and
// dispatch.  Engines of up to kBatchStreamMax queries: one single-query histogram pass per query
// ("template_hist"), all enqueued before the one wait.  The GEMM: one launch of
// batch_lds_kernel<..., BL_HIST> ("template_batch_hist") over all query groups; a workgroup adds its
// queries' LDS histograms once, after its walk, straight into the rows of the device's counter
// buffer -- one row per padded query, the padding queries' rows ignored -- and a copy brings the nq
// rows back.
int iris_template_batch_histogram(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint32_t nbins,
                                  uint64_t *bins, uint64_t *invalid) {
    IRIS_KEEP_DEVICE();
    CHK(hist_args(nbins, bins, invalid));  // the value arguments first: refused whatever the handles
    CHK(template_batch_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const uint32_t nq = e->nq;
    const LaunchRange r{first, n};
    if (!e->sub.empty())
        return hist_run(d, n, nbins, bins, invalid, nq, [&](uint32_t q, const MatchSink &hs) {
            return launch_template_select(d, db, e->sub[q]->qtab, e->sub[q]->qfrag, r, Pass::Hist, hs);
        });
    if (n == 0) return hist_empty(nq, nbins, bins, invalid);
    const BatchGeometry geo = batch_geometry(d->hooks, r, nq);
    const size_t words = (size_t)nbins + 1, rows = (size_t)geo.nqg * geo.qper;
    CHK(ensure(d, d->match_count, rows * words * sizeof(uint64_t)));
    CHK(ensure_host_result(d, nq * words * sizeof(uint64_t)));
    uint64_t *cnt = (uint64_t *)d->match_count.p;
    HIPCHK(hipMemsetAsync(cnt, 0, rows * words * sizeof(uint64_t), d->stream));
    CHK(timed(d, "template_batch_hist", n * nq,
              [&] { return launch_batch(Pass::Hist, d->hooks, d->stream, db->data, e->qfrag, r, geo, {cnt, nbins}); }));
    HIPCHK(hipMemcpyAsync(d->host_result, cnt, nq * words * sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
    CHK(sync(d));
    return hist_finish(d, n, nbins, nq, bins, invalid);
}

// iris_resolver_search's histogram sibling (header: "resolver histograms"): resolver_kernel's
// histogram mode ("resolver_hist"), one workgroup per 256 rows, through hist_run's counter copies.
int iris_resolver_histogram(iris_device_t *d, const uint16_t *const *shares, uint32_t parts, const uint16_t *denoms,
                            uint64_t n, uint32_t nbins, uint64_t *bins, uint64_t *invalid) {
    IRIS_KEEP_DEVICE();
    CHK(hist_args(nbins, bins, invalid));  // the value arguments first: refused whatever the handles
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    ARG(d, "NULL argument");
    CHK(share_args(shares, parts, n, denoms != nullptr));
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    return hist_run(d, n, nbins, bins, invalid, 1, [&](uint32_t, const MatchSink &hs) {
        return timed(d, "resolver_hist", n, [&] { return launch_resolver(Pass::Hist, d->stream, shares, parts, denoms, n, hs); });
    });
}

// iris_resolver_search_masks' histogram sibling: TILES runs the fused masks_mfma_kernel<MASKS_HIST>
// ("masks_resolve_hist"); LANES the masks kernel into the workspace and then the resolver kernel's
// histogram mode ("resolver_hist").
int iris_resolver_histogram_masks(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                                  const uint16_t *const *shares_device, uint32_t parts, uint32_t nbins, uint64_t *bins,
                                  uint64_t *invalid) {
    IRIS_KEEP_DEVICE();
    CHK(hist_args(nbins, bins, invalid));  // the value arguments first: refused whatever the handles
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    CHK(single_masks_args(e, db, "iris_resolver_batch_histogram_masks"));
    CHK(share_args(shares_device, parts, n));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const LaunchRange r{first, n};
    return hist_run(d, n, nbins, bins, invalid, 1, [&](uint32_t, const MatchSink &hs) {
        const uint16_t *den = nullptr;
        return masks_single_launch(d, e, db, r, shares_device, parts, Pass::Hist, hs, &den);
    });
}

// iris_resolver_batch_search_masks' histogram sibling, with iris_resolver_batch_matches_masks'
// dispatch: TILES ranges the batch kernel runs walk the queries in groups of kMasksBatchG, each group
// one pass of masks_batch_kernel<BATCH_HIST> ("masks_batch_hist") into the group's sinks, a single
// left-over query one fused single-query pass; other TILES ranges one such pass per query; LANES the
// masks kernel into the workspace and the resolver kernel per query.  Every pass is enqueued before
// the one hist_reduce over all nq rows and the one wait.
int iris_resolver_batch_histogram_masks(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                                        const uint16_t *const *shares_device, uint32_t parts, uint32_t nbins,
                                        uint64_t *bins, uint64_t *invalid) {
    IRIS_KEEP_DEVICE();
    CHK(hist_args(nbins, bins, invalid));  // the value arguments first: refused whatever the handles
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    CHK(masks_batch_args(e, db));
    CHK(share_args(shares_device, parts, n));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const MasksWalk w(e, db, first, n);
    return hist_run_all(d, n, nbins, bins, invalid, e->nq, [&](const MatchSink *hs) {
        for (MasksUnit u = w.unit(0); u.m; u = w.unit(u.q0 + u.m)) {
            if (u.m > 1) {
                CHK(timed(d, "masks_batch_hist", n * u.m, [&] {
                    return launch_masks_batch(Pass::Hist, d->hooks, d->stream, db->data, u.frags, u.m, w.r,
                                              {shares_device, parts, u.q0, hs + u.q0, MasksBatchOut::HistTag{}});
                }));
                continue;
            }
            // one query through the single-query forms, on its slab of every part
            const uint16_t *sl[8], *den = nullptr;
            w.slabs(u.q0, shares_device, parts, sl);
            CHK(masks_single_launch(d, u.one, db, w.r, sl, parts, Pass::Hist, hs[u.q0], &den));
        }
        return 0;
    });
}

// ------------------------------------------------------------------ combined passes

// The pinned host result of a report call: the staged ReportSinks, the match counter, the merged
// top-k list, the histogram row -- disjoint, each at a 64-byte boundary.
constexpr size_t kReportCountOff = 128, kReportTopkOff = 192;
constexpr size_t kReportHistOff = kReportTopkOff + kTopkMax * sizeof(Partial);
static_assert(sizeof(ReportSinks) <= kReportCountOff && kReportHistOff % 64 == 0, "report result layout");
// The device's counter buffer of a report call: the match counter, then (a line on) the histogram's copies
constexpr size_t kReportHistWord = 8;

// The passes of one report call, whichever family runs them: launch(p, sink) enqueues the family's
// pass of mode p over the call's range, timed under the family's own names -- Pass::Report with
// report_sink of the device's ReportSinks, Pass::Match / Topk / Hist with that part's sink, as the
// sibling call launches it.  units: the lists a top-k (or report) pass writes, 0 for an empty range.
struct ReportPasses {
    uint64_t units;
    std::function<int(Pass, const MatchSink &)> launch;
};

// Two or three parts of a report call over n records (not none) from ONE pass ("template_report",
// "masks_report", "resolver_report").  The device's buffers are shared by region: d->matches holds
// the top-k lists (and the merge's spare lists) and behind them the match records; d->match_count
// the match counter and behind it the histogram's copies; the pinned result as laid out above.
// The pass is followed on the stream by the top-k merge, the histogram's reduce (copies = 1: a
// copy) and the copy of the match counter, and the call waits once.  A match list that overflows
// its room (matches_run_units' rule: the caller's cap or kMatchFirstRoom, a grown buffer in full,
// cap = 0 never) runs again alone, as the family's plain match pass whose room is the reported
// count; its ensure() may replace d->matches, so the top-k list and the histogram are taken off
// the pinned result first.  That ensure() grows the buffer by the lists' bytes as well, so a caller
// with a steady list length reruns once, not in every call.  Nothing reaches *rep or its arrays before every part has succeeded.
static int report_run(iris_device *d, uint64_t n, uint64_t base, iris_report_t *rep, const ReportPasses &ps) {
    const bool want_match = rep->parts & IRIS_REPORT_MATCHES, want_topk = rep->parts & IRIS_REPORT_TOPK,
               want_hist = rep->parts & IRIS_REPORT_HIST;
    const uint64_t cap = want_match ? rep->matches_cap : 0;
    const uint32_t k = want_topk ? rep->k : 0, nbins = want_hist ? rep->nbins : 0;
    const uint64_t units = want_topk ? ps.units : 0;
    const size_t lists_bytes = (units + topk_spare_lists(units)) * k * sizeof(Partial);
    const uint32_t words = nbins + 1, copies = !want_hist ? 0 : d->hooks.hist_copies ? d->hooks.hist_copies : kHistCopies;
    uint64_t room = 0;
    if (cap) {
        room = std::min<uint64_t>(n, std::max<uint64_t>(cap, kMatchFirstRoom));
        if (d->matches.cap > lists_bytes)  // reuse_grown: what an earlier call grew, behind the lists
            room = std::max<uint64_t>(room, std::min<uint64_t>(n, (d->matches.cap - lists_bytes) / sizeof(Partial)));
    }
    CHK(ensure(d, d->matches, lists_bytes + room * sizeof(Partial)));
    CHK(ensure(d, d->match_count, (kReportHistWord + (size_t)copies * words) * sizeof(uint64_t)));
    CHK(ensure(d, d->match_sinks, sizeof(ReportSinks)));
    CHK(ensure_host_result(d, kReportHistOff + (size_t)kHistMaxBins * sizeof(uint64_t) + sizeof(uint64_t)));
    Partial *lists = (Partial *)d->matches.p, *spare = lists + units * k;
    Partial *records = (Partial *)((char *)d->matches.p + lists_bytes);
    uint64_t *cnt = (uint64_t *)d->match_count.p, *hist = cnt + kReportHistWord;
    char *res = (char *)d->host_result;
    HIPCHK(hipMemsetAsync(cnt, 0, (kReportHistWord + (size_t)copies * words) * sizeof(uint64_t), d->stream));
    // the sinks cross to the device from pinned memory, as a template batch match pass's do
    ReportSinks *stage = (ReportSinks *)res;
    *stage = ReportSinks{};
    if (want_match) stage->match = MatchSink{records, room, cnt, rep->threshold};
    if (want_topk) stage->topk = topk_sink(lists, k);
    if (want_hist) stage->hist = hist_sink(hist, nbins, copies);
    const ReportSinks *dsinks = (const ReportSinks *)d->match_sinks.p;
    HIPCHK(hipMemcpyAsync((void *)dsinks, stage, sizeof(ReportSinks), hipMemcpyHostToDevice, d->stream));
    CHK(ps.launch(Pass::Report, report_sink(dsinks)));
    if (want_topk)
        CHK(timed(d, "topk_merge", units, [&] {
            return launch_topk_merge(d->stream, lists, spare, units, k, (Partial *)(res + kReportTopkOff));
        }));
    if (want_hist) {
        if (copies > 1)
            CHK(timed(d, "hist_reduce", (uint64_t)copies * words, [&] {
                return launch_hist_reduce(d->stream, hist, words, copies, 1, (uint64_t *)(res + kReportHistOff));
            }));
        else
            HIPCHK(hipMemcpyAsync(res + kReportHistOff, hist, words * sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
    }
    if (want_match)
        HIPCHK(hipMemcpyAsync(res + kReportCountOff, cnt, sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
    CHK(sync(d));
    // every part's result off the pinned words: a rerun below reuses them
    uint64_t total = 0;
    Partial best[kTopkMax];
    std::vector<uint64_t> row;
    std::vector<Partial> recs;
    if (want_match) {
        memcpy(&total, res + kReportCountOff, sizeof(total));
        if (total > n) return fail(IRIS_E_HIP, "match pass counted more records than the range holds");
    }
    if (want_topk) memcpy(best, res + kReportTopkOff, k * sizeof(Partial));
    const uint64_t take = std::min(total, cap);
    try {
        if (want_hist) row.assign((const uint64_t *)(res + kReportHistOff), (const uint64_t *)(res + kReportHistOff) + words);
        if (take) recs.resize(total);
    } catch (const std::bad_alloc &) {
        return fail(IRIS_E_NOMEM, "out of host memory");
    }
    if (want_hist) {
        uint64_t sum = 0;
        for (uint32_t i = 0; i < words; ++i) sum += row[i];
        if (sum != n) return fail(IRIS_E_HIP, "histogram pass did not count every record of the range once");
    }
    if (take) {
        if (total > room) {  // the matches part alone once more, its room the reported count
            // grown past the lists too: the next such call finds room for this list behind them (reuse_grown)
            CHK(ensure(d, d->matches, lists_bytes + total * sizeof(Partial)));
            records = (Partial *)d->matches.p;
            HIPCHK(hipMemsetAsync(cnt, 0, sizeof(uint64_t), d->stream));
            CHK(ps.launch(Pass::Match, MatchSink{records, total, cnt, rep->threshold}));
            HIPCHK(hipMemcpyAsync(res + kReportCountOff, cnt, sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
            CHK(sync(d));
            if (memcmp(res + kReportCountOff, &total, sizeof(total)) != 0)
                return fail(IRIS_E_HIP, "match pass counts differ between two runs");
        }
        HIPCHK(hipMemcpyAsync(recs.data(), records, total * sizeof(Partial), hipMemcpyDeviceToHost, d->stream));
        CHK(sync(d));
    }
    if (want_match) {
        if (take) match_list(recs.data(), total, take, base, rep->matches);
        rep->matches_count = total;
    }
    if (want_topk) rep->topk_count = topk_list(best, k, base, rep->topk);
    if (want_hist) {
        memcpy(rep->bins, row.data(), nbins * sizeof(uint64_t));
        rep->invalid = row[nbins];
    }
    return 0;
}

// The value arguments of a report call, refused whatever the handles: the struct, its parts, then
// each selected part under its sibling's rules.
static int report_args(iris_report_t *rep) {
    ARG(rep, "report is NULL");
    const uint32_t all = IRIS_REPORT_MATCHES | IRIS_REPORT_TOPK | IRIS_REPORT_HIST;
    ARG(rep->parts != 0 && (rep->parts & ~all) == 0, "parts must be one or more of IRIS_REPORT_MATCHES, _TOPK, _HIST");
    if (rep->parts & IRIS_REPORT_MATCHES) CHK(matches_args(rep->threshold, rep->matches, rep->matches_cap, &rep->matches_count));
    if (rep->parts & IRIS_REPORT_TOPK) CHK(topk_args(rep->k, rep->topk, &rep->topk_count));
    if (rep->parts & IRIS_REPORT_HIST) CHK(hist_args(rep->nbins, rep->bins, &rep->invalid));
    return 0;
}

// A report call once its arguments, handles and range stand (the device locked and current), for
// every family.  One part: that sibling's own pass through its own runner, its count through a
// local -- a failed call leaves the struct as it was.  An empty range: zeros, nothing launched.
// Otherwise report_run.
static int report_dispatch(iris_device *d, uint64_t n, uint64_t base, iris_report_t *rep, const ReportPasses &ps) {
    if (rep->parts == IRIS_REPORT_MATCHES) {
        uint64_t count = 0;
        CHK(matches_run(d, n, base, rep->threshold, rep->matches, rep->matches_cap, &count,
                        [&](const MatchSink &ms) { return ps.launch(Pass::Match, ms); }));
        rep->matches_count = count;
        return 0;
    }
    if (rep->parts == IRIS_REPORT_TOPK) {
        uint32_t count = 0;
        CHK(topk_run(d, n, base, rep->k, rep->topk, &count, ps.units,
                     [&](const MatchSink &ts) { return ps.launch(Pass::Topk, ts); }));
        rep->topk_count = count;
        return 0;
    }
    if (rep->parts == IRIS_REPORT_HIST)
        return hist_run(d, n, rep->nbins, rep->bins, &rep->invalid, 1,
                        [&](uint32_t, const MatchSink &hs) { return ps.launch(Pass::Hist, hs); });
    if (n == 0) {  // nothing is launched
        if (rep->parts & IRIS_REPORT_MATCHES) rep->matches_count = 0;
        if (rep->parts & IRIS_REPORT_TOPK) rep->topk_count = 0;
        if (rep->parts & IRIS_REPORT_HIST) CHK(hist_empty(1, rep->nbins, rep->bins, &rep->invalid));
        return 0;
    }
    return report_run(d, n, base, rep, ps);
}

// Several of iris_template_matches, iris_template_topk and iris_template_histogram for one probe from
// one read of the range (header: "combined passes").
int iris_template_report(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint64_t index_base,
                         void *report) {
    IRIS_KEEP_DEVICE();
    iris_report_t *const rep = (iris_report_t *)report;
    CHK(report_args(rep));  // the value arguments first: refused whatever the handles
    CHK(template_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const LaunchRange r{first, n};
    return report_dispatch(d, n, index_base + first, rep, {n ? template_topk_lists(d, db, r) : 0, [&](Pass p, const MatchSink &s) {
        return launch_template_select(d, db, e->qtab, e->qfrag, r, p, s);
    }});
}

// ------------------------------------------------------------------ pipelined reports

// iris_template_report_async .. iris_pending_report_wait (the handle's life:
// iris_pending.hpp).  One device buffer per pending, from kReportPool (the "fit" pick: k and nbins
// change from call to call):
//   [0, kReportSinksBytes)   the ReportSinks the pass (and the pass that hosts it) reads
//   hist copies              copies x (nbins + 1) u64 (no histogram part: none)
//   the match counter        8 bytes, straight behind them: one region to clear
//   the match records        room = min(n, max(cap, kMatchFirstRoom)) of them (cap 0: none)
//   the top-k lists          units lists of k and the merge's spare lists
// and one pinned slot (kReportSlotBytes): the counter and the first kMatchInline records, the merged
// k records at kReportSlotTopkOff, the histogram row at kReportSlotHistOff.  Behind the pass, on the
// side stream: the merge (its last level into the slot), the histogram's reduce (copies = 1: a copy)
// into the slot, the copy of the counter and the inline records.
constexpr size_t kReportSinksBytes = 128;
static_assert(sizeof(ReportSinks) <= kReportSinksBytes, "report buffer layout");
struct iris_pending_report : iris_pending {
    const iris_db *db = nullptr;  // the caller keeps it alive and unmodified until the wait
    uint64_t first = 0, cap = 0, room = 0;
    double threshold = 0;
    uint32_t parts = 0, k = 0, nbins = 0, copies = 0;
    size_t cnt_off = 0, rec_off = 0;  // of the device buffer: the match counter, the records
    iris_template_t query;  // an overflowing match list runs its pass again after the engine may be gone
};

int iris_template_report_async(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint64_t index_base,
                               const void *report, iris_pending_t **out) {
    IRIS_KEEP_DEVICE();
    // the in scalars only, under iris_template_report's rules and in its order; the pointers wait for the wait
    const iris_report_t *const rep = (const iris_report_t *)report;
    ARG(rep, "report is NULL");
    const uint32_t parts = rep->parts, all = IRIS_REPORT_MATCHES | IRIS_REPORT_TOPK | IRIS_REPORT_HIST;
    ARG(parts != 0 && (parts & ~all) == 0, "parts must be one or more of IRIS_REPORT_MATCHES, _TOPK, _HIST");
    const bool want_match = parts & IRIS_REPORT_MATCHES, want_topk = parts & IRIS_REPORT_TOPK,
               want_hist = parts & IRIS_REPORT_HIST;
    const double threshold = rep->threshold;
    const uint64_t cap = want_match ? rep->matches_cap : 0;
    const uint32_t k = want_topk ? rep->k : 0, nbins = want_hist ? rep->nbins : 0;
    if (want_match) ARG(threshold == threshold, "threshold is NaN");
    if (want_topk) ARG(k >= 1 && k <= IRIS_TOPK_MAX, "k must be 1..IRIS_TOPK_MAX (64)");
    if (want_hist)
        ARG(nbins >= 1 && nbins <= IRIS_HIST_MAX_BINS && (nbins & (nbins - 1)) == 0,
            "nbins must be a power of two in 1..IRIS_HIST_MAX_BINS (1024)");
    ARG(out, "out is NULL");
    CHK(template_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (!e->host_query) return fail(IRIS_E_ARG, "engine keeps no host copy of its query");
    iris_pending_report *p = nullptr;
    CHK(pending_new(d, kShareReport, n, index_base + first, &p));
    p->db = db;
    p->first = first;
    p->cap = cap;
    p->threshold = threshold;
    p->parts = parts;
    p->k = k;
    p->nbins = nbins;
    p->query = *e->host_query;
    if (n == 0) return pending_publish(p, out);
    const LaunchRange r{first, n};
    const uint64_t units = want_topk ? template_topk_lists(d, db, r) : 0;
    const uint32_t words = nbins + 1;
    p->copies = !want_hist ? 0 : d->hooks.hist_copies ? d->hooks.hist_copies : kHistCopies;
    p->room = cap ? std::min<uint64_t>(n, std::max<uint64_t>(cap, kMatchFirstRoom)) : 0;
    const size_t hist_bytes = (size_t)p->copies * words * sizeof(uint64_t);
    p->cnt_off = kReportSinksBytes + hist_bytes;
    p->rec_off = p->cnt_off + sizeof(uint64_t);
    const size_t lists_off = p->rec_off + p->room * sizeof(Partial);
    int rc = bufs_take(d, kReportPool, lists_off + (units + topk_spare_lists(units)) * k * sizeof(Partial), p);
    if (rc == 0) rc = pending_arm(p);
    if (rc != 0) return pending_abandon(p, rc);
    char *dev = (char *)p->bufs.dev.p, *slot = (char *)p->bufs.host;
    uint64_t *hist = (uint64_t *)(dev + kReportSinksBytes), *cnt = (uint64_t *)(dev + p->cnt_off);
    Partial *records = (Partial *)(dev + p->rec_off), *lists = (Partial *)(dev + lists_off), *spare = lists + units * k;
    ReportPrep prep{ReportSinks{}, hist, (uint64_t)p->copies * words + 1};
    if (want_match) prep.sinks.match = MatchSink{records, p->room, cnt, threshold};
    if (want_topk) prep.sinks.topk = topk_sink(lists, k);
    if (want_hist) prep.sinks.hist = hist_sink(hist, nbins, p->copies);
    rc = select_pass_enqueue(d, db, r, e->qtab, e->qfrag, e->host_query, kShareReport, report_sink((const ReportSinks *)dev),
                             true, &prep);
    if (rc == 0) rc = pending_side_begin(p);
    if (rc == 0 && want_topk)  // the merge, whose last level writes the pinned slot
        rc = timed(d, "topk_merge", units, [&] {
            return launch_topk_merge(d->aux, lists, spare, units, k, (Partial *)(slot + kReportSlotTopkOff));
        }, d->aux);
    if (rc == 0 && want_hist) {
        if (p->copies > 1)
            rc = timed(d, "hist_reduce", (uint64_t)p->copies * words, [&] {
                return launch_hist_reduce(d->aux, hist, words, p->copies, 1, (uint64_t *)(slot + kReportSlotHistOff));
            }, d->aux);
        else
            rc = pending_side_chk(p, hipMemcpyAsync(slot + kReportSlotHistOff, hist, words * sizeof(uint64_t),
                                                    hipMemcpyDeviceToHost, d->aux));
    }
    if (rc == 0 && want_match) {  // the counter and the first records
        const size_t bytes = sizeof(uint64_t) + std::min<uint64_t>(p->room, kMatchInline) * sizeof(Partial);
        rc = pending_side_chk(p, hipMemcpyAsync(slot, cnt, bytes, hipMemcpyDeviceToHost, d->aux));
    }
    if (rc == 0) rc = pending_side_end(p);
    if (rc != 0) return pending_abandon(p, rc);
    return pending_publish(p, out);
}

// The `total` match records of a pending whose pass has ended -> recs (caller holds the device lock).
// A list longer than its room: the matches part alone once more, blocking and unshared, as a plain
// match pass into the buffer grown to the reported count (the top-k list and the histogram row are
// off the slot by then), the query's tables built again from the host copy.
static int pending_report_records(iris_pending_report *p, uint64_t total, Partial *recs) {
    iris_device *d = p->dev;
    if (total <= std::min<uint64_t>(p->room, kMatchInline)) {
        memcpy(recs, (const char *)p->bufs.host + kMatchRecOff, total * sizeof(Partial));
        return 0;
    }
    CHK(set_device(d));
    if (total > p->room) {
        void *q = nullptr;
        CHK(dev_malloc(d, &q, qalign(kTemplateTabBytes) + kTemplateFragDwords * 4, "match rerun query"));
        uint32_t *tab = (uint32_t *)q, *frag = (uint32_t *)((char *)q + qalign(kTemplateTabBytes));
        p->room = total;
        p->cnt_off = 0;
        p->rec_off = kMatchRecOff;
        int rc = ensure(d, p->bufs.dev, kMatchRecOff + total * sizeof(Partial));
        uint64_t *cnt = (uint64_t *)p->bufs.dev.p;
        if (rc == 0 && launch_query_template(d->stream, &p->query, tab, frag) != 0)
            rc = fail(IRIS_E_HIP, "kernel launch failed: query tables");
        if (rc == 0)
            rc = select_pass_enqueue(d, p->db, LaunchRange{p->first, p->n}, tab, frag, &p->query, kShareMatch,
                                     MatchSink{(Partial *)((char *)p->bufs.dev.p + kMatchRecOff), total, cnt, p->threshold},
                                     false);
        uint64_t again = 0;
        if (rc == 0 && hipMemcpyAsync(&again, cnt, sizeof(again), hipMemcpyDeviceToHost, d->stream) != hipSuccess)
            rc = fail(IRIS_E_HIP, "hipMemcpyAsync failed");
        const int rs = sync(d);
        (void)hipFree(q);
        CHK(rc);
        CHK(rs);
        if (again != total) return fail(IRIS_E_HIP, "match pass counts differ between two runs");
    }
    // on the second side stream, which carries nothing of a template pipeline (iris_pending_matches_wait)
    HIPCHK(hipMemcpyAsync(recs, (const char *)p->bufs.dev.p + p->rec_off, total * sizeof(Partial), hipMemcpyDeviceToHost,
                          d->aux2));
    HIPCHK(hipStreamSynchronize(d->aux2));
    return 0;
}

int iris_pending_report_wait(iris_pending_t *pending, void *report) {
    IRIS_KEEP_DEVICE();
    iris_pending_report *p = nullptr;
    CHK(pending_claim(pending, kShareReport, &p));
    iris_report_t *const rep = (iris_report_t *)report;
    const bool want_match = p->parts & IRIS_REPORT_MATCHES, want_topk = p->parts & IRIS_REPORT_TOPK,
               want_hist = p->parts & IRIS_REPORT_HIST;
    // the struct must be the submission's: the arrays' sizes follow from these fields
    int rc = 0;
    if (!rep) rc = fail(IRIS_E_ARG, "report is NULL");
    else if (rep->parts != p->parts) rc = fail(IRIS_E_ARG, "parts differs from the submission's");
    else if (want_match && rep->matches_cap != p->cap) rc = fail(IRIS_E_ARG, "matches_cap differs from the submission's");
    else if (want_topk && rep->k != p->k) rc = fail(IRIS_E_ARG, "k differs from the submission's");
    else if (want_hist && rep->nbins != p->nbins) rc = fail(IRIS_E_ARG, "nbins differs from the submission's");
    else if (want_match && p->cap && !rep->matches) rc = fail(IRIS_E_ARG, "out is NULL with cap > 0");
    else if (want_topk && !rep->topk) rc = fail(IRIS_E_ARG, "out is NULL");
    else if (want_hist && !rep->bins) rc = fail(IRIS_E_ARG, "bins is NULL");
    return pending_retire(p, pending_await(p), rc, [&]() -> int {
        const uint64_t n = p->n;
        const uint32_t k = p->k, nbins = p->nbins;
        // every part's result off the slot and checked before anything reaches *rep: a rerun replaces the buffers
        uint64_t total = 0;
        Partial best[kTopkMax];
        std::vector<uint64_t> row;
        std::vector<Partial> recs;
        const char *slot = (const char *)p->bufs.host;
        if (n > 0) {
            if (want_match) memcpy(&total, slot, sizeof(total));
            if (total > n) return fail(IRIS_E_HIP, "match pass counted more records than the range holds");
            if (want_topk) memcpy(best, slot + kReportSlotTopkOff, k * sizeof(Partial));
        }
        const uint64_t take = std::min(total, p->cap);
        try {
            if (want_hist && n > 0)
                row.assign((const uint64_t *)(slot + kReportSlotHistOff), (const uint64_t *)(slot + kReportSlotHistOff) + nbins + 1);
            else if (want_hist)
                row.assign((size_t)nbins + 1, 0);
            if (take) recs.resize(total);
        } catch (const std::bad_alloc &) {
            return fail(IRIS_E_NOMEM, "out of host memory");
        }
        if (want_hist) CHK(hist_rows_check(row.data(), n, nbins, 1));
        if (take) CHK(pending_report_records(p, total, recs.data()));
        if (want_match) {
            if (take) match_list(recs.data(), total, take, p->base, rep->matches);
            rep->matches_count = total;
        }
        if (want_topk) rep->topk_count = n > 0 ? topk_list(best, k, p->base, rep->topk) : 0;
        if (want_hist) hist_rows_write(row.data(), nbins, 1, rep->bins, &rep->invalid);
        return 0;
    });
}

// ------------------------------------------------------------------ resolver reports

// iris_resolver_matches, iris_resolver_topk and iris_resolver_histogram for one probe from one read
// of the share rows (header: "resolver reports"): resolver_kernel's report mode ("resolver_report").
int iris_resolver_report(iris_device_t *d, const uint16_t *const *shares, uint32_t parts, const uint16_t *denoms,
                         uint64_t n, uint64_t index_base, void *report) {
    IRIS_KEEP_DEVICE();
    iris_report_t *const rep = (iris_report_t *)report;
    CHK(report_args(rep));  // the value arguments first: refused whatever the handles
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    ARG(d, "NULL argument");
    CHK(share_args(shares, parts, n, denoms != nullptr));
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    return report_dispatch(d, n, index_base, rep, {resolver_topk_units(n), [&](Pass p, const MatchSink &s) {
        const char *name = pass_name(p, "resolver_match", "resolver_topk", "resolver_hist", "resolver_report");
        return timed(d, name, n, [&] { return launch_resolver(p, d->stream, shares, parts, denoms, n, s); });
    }});
}

// The masks sibling: TILES runs the fused masks_mfma_kernel<MASKS_REPORT> ("masks_report"); LANES
// the masks kernel into the workspace, once per call -- the rerun of an overflowing match list
// reuses the denominators -- and then resolver_kernel's report mode.
int iris_resolver_report_masks(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                               const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base, void *report) {
    IRIS_KEEP_DEVICE();
    iris_report_t *const rep = (iris_report_t *)report;
    CHK(report_args(rep));  // the value arguments first: refused whatever the handles
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    CHK(single_masks_args(e, db, "iris_resolver_batch_report_masks"));
    CHK(share_args(shares_device, parts, n));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const LaunchRange r{first, n};
    const uint64_t units = db->k.layout != IRIS_LAYOUT_TILES ? resolver_topk_units(n) : n ? masks_topk_units(d->hooks, r) : 0;
    const uint16_t *den = nullptr;
    return report_dispatch(d, n, index_base, rep, {units, [&](Pass p, const MatchSink &s) {
        return masks_single_launch(d, e, db, r, shares_device, parts, p, s, &den);
    }});
}

// ------------------------------------------------------------------ template batch reports

static int batch_report_args(const iris_batch_report_t *rep) {
    ARG(rep, "report is NULL");
    const uint32_t all = IRIS_REPORT_MATCHES | IRIS_REPORT_TOPK | IRIS_REPORT_HIST;
    ARG(rep->parts != 0 && (rep->parts & ~all) == 0, "parts must be one or more of IRIS_REPORT_MATCHES, _TOPK, _HIST");
    ARG(rep->reserved == 0, "reserved must be 0");
    if (rep->parts & IRIS_REPORT_MATCHES) CHK(matches_args(rep->threshold, rep->matches, rep->matches_cap, rep->matches_counts));
    if (rep->parts & IRIS_REPORT_TOPK) CHK(topk_args(rep->k, rep->topk, rep->topk_counts));
    if (rep->parts & IRIS_REPORT_HIST) CHK(hist_args(rep->nbins, rep->bins, rep->invalid));
    return 0;
}

// Two or three parts for the queries of a GEMM engine over r (not empty) from ONE pass of
// batch_lds_kernel<..., BL_REPORT> ("template_batch_report").  The device's buffers are shared by
// region: d->matches holds the lists region of iris_template_batch_topk -- nqp (8 G + ceil(8 G / 64)) k
// records -- and behind it the queries' match regions; d->match_count nqp counters and behind them
// the histogram rows [nqp][nbins + 1], which the workgroups add into as in BL_HIST; the pinned
// result the nq counts, the staged sinks, the merged lists [nq][k] and the nq rows, each at a
// 64-byte boundary.  The merge levels of all queries and the rows' copy follow the pass on the
// stream, and the call waits once.  With a matches part the call is a threshold-match call
// (matches_run_units) whose first pass is the report pass: its room, overflow and rerun rules are
// iris_template_batch_matches', the rerun that call's plain match pass over the block.  The merged
// lists and the rows are taken off the pinned result before a rerun; nothing reaches the caller's
// arrays before every part has succeeded.
static int batch_report_run(iris_device *d, const iris_engine *e, const iris_db *db, LaunchRange r, uint64_t base,
                            const iris_batch_report_t *rep) {
    const bool want_match = rep->parts & IRIS_REPORT_MATCHES, want_topk = rep->parts & IRIS_REPORT_TOPK,
               want_hist = rep->parts & IRIS_REPORT_HIST;
    const uint32_t nq = e->nq, nqp = batch_padded(nq);
    const uint32_t k = want_topk ? rep->k : 0, nbins = want_hist ? rep->nbins : 0;
    const BatchGeometry geo = batch_geometry(d->hooks, r, nq);
    const uint64_t lists = want_topk ? batch_topk_units(geo) : 0, stride = (lists + topk_spare_lists(lists)) * k;
    const size_t lists_bytes = (size_t)nqp * stride * sizeof(Partial);
    const size_t words = (size_t)nbins + 1, rows_bytes = want_hist ? nqp * words * sizeof(uint64_t) : 0;
    const auto line = [](size_t b) { return (b + 63) / 64 * 64; };
    const size_t topk_off = line(batch_stage_off(nq) + nqp * sizeof(MatchSink));
    const size_t hist_off = line(topk_off + (size_t)nq * k * sizeof(Partial));
    CHK(ensure_host_result(d, hist_off + (want_hist ? nq * words * sizeof(uint64_t) : 0)));
    if (want_match) CHK(ensure(d, d->match_sinks, nqp * sizeof(MatchSink)));
    // the buffers' addresses are read when a step is enqueued: matches_run_units ensures them first
    const auto rows_dev = [=] { return (uint64_t *)d->match_count.p + nqp; };
    const auto report_pass = [=](const MatchSink *ms) -> int {  // ms: the nqp sinks; null without a matches part
        if (ms) CHK(batch_sinks_stage(d, nq, 0, nq, ms));
        return timed(d, "template_batch_report", r.n * nq, [&] {
            return launch_batch(Pass::Report, d->hooks, d->stream, db->data, e->qfrag, r, geo,
                                {ms ? (const MatchSink *)d->match_sinks.p : nullptr, want_topk ? (Partial *)d->matches.p : nullptr,
                                 stride, k, want_hist ? rows_dev() : nullptr, nbins});
        });
    };
    const auto enqueue = [=]() -> int {
        char *res = (char *)d->host_result;
        if (want_topk) CHK(topk_merge_enqueue(d, (Partial *)d->matches.p, lists, stride, k, nq, (Partial *)(res + topk_off)));
        if (want_hist)
            HIPCHK(hipMemcpyAsync(res + hist_off, rows_dev(), nq * words * sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
        return 0;
    };
    std::vector<Partial> best;
    std::vector<uint64_t> rows, mcounts;
    const auto taken = [&]() -> int {
        const char *res = (const char *)d->host_result;
        try {
            if (want_topk) best.assign((const Partial *)(res + topk_off), (const Partial *)(res + topk_off) + (size_t)nq * k);
            if (want_hist) rows.assign((const uint64_t *)(res + hist_off), (const uint64_t *)(res + hist_off) + nq * words);
        } catch (const std::bad_alloc &) {
            return fail(IRIS_E_NOMEM, "out of host memory");
        }
        return want_hist ? hist_rows_check(rows.data(), r.n, nbins, nq) : 0;
    };
    if (want_match) {
        try {
            mcounts.resize(nq);
        } catch (const std::bad_alloc &) {
            return fail(IRIS_E_NOMEM, "out of host memory");
        }
        const MatchWhole whole{nqp, report_pass};
        const MatchRider ride{lists_bytes, rows_bytes, enqueue, taken};
        CHK(matches_run_units(d, r.n, base, rep->threshold, rep->matches, rep->matches_cap, mcounts.data(), nq, false,
                              batch_match_units(d, e, db, r), &whole, kBatchMatchBudget, &ride));
        memcpy(rep->matches_counts, mcounts.data(), nq * sizeof(uint64_t));
    } else {
        const size_t count_bytes = nqp * sizeof(uint64_t) + rows_bytes;
        CHK(ensure(d, d->matches, lists_bytes));
        CHK(ensure(d, d->match_count, count_bytes));
        HIPCHK(hipMemsetAsync(d->match_count.p, 0, count_bytes, d->stream));
        CHK(report_pass(nullptr));
        CHK(enqueue());
        CHK(sync(d));
        CHK(taken());
    }
    if (want_topk)
        for (uint32_t q = 0; q < nq; ++q)
            rep->topk_counts[q] = topk_list(best.data() + (size_t)q * k, k, base, rep->topk + (size_t)q * k);
    if (want_hist) hist_rows_write(rows.data(), nbins, nq, rep->bins, rep->invalid);  // checked in taken()
    return 0;
}

// Several of iris_template_batch_matches, iris_template_batch_topk and iris_template_batch_histogram
// for every probe of a batch engine from one pass over the range (header: "template batch reports").
// One part: the sibling call itself.  Engines of up to kBatchStreamMax queries: one single-query
// report per query (report_dispatch, either layout), each waiting once.  The GEMM: batch_report_run.
int iris_template_batch_report(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n, uint64_t index_base,
                               void *report) {
    IRIS_KEEP_DEVICE();
    const iris_batch_report_t *const rep = (const iris_batch_report_t *)report;
    CHK(batch_report_args(rep));  // the value arguments first: refused whatever the handles
    CHK(template_batch_args(e, db));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (rep->parts == IRIS_REPORT_MATCHES)
        return iris_template_batch_matches(e, db, first, n, index_base, rep->threshold, rep->matches, rep->matches_cap,
                                           rep->matches_counts);
    if (rep->parts == IRIS_REPORT_TOPK)
        return iris_template_batch_topk(e, db, first, n, index_base, rep->k, rep->topk, rep->topk_counts);
    if (rep->parts == IRIS_REPORT_HIST) return iris_template_batch_histogram(e, db, first, n, rep->nbins, rep->bins, rep->invalid);
    const bool want_match = rep->parts & IRIS_REPORT_MATCHES, want_topk = rep->parts & IRIS_REPORT_TOPK,
               want_hist = rep->parts & IRIS_REPORT_HIST;
    const uint32_t nq = e->nq;
    if (n == 0) {  // nothing is launched
        if (want_match) memset(rep->matches_counts, 0, nq * sizeof(uint64_t));
        if (want_topk) memset(rep->topk_counts, 0, nq * sizeof(uint32_t));
        if (want_hist) CHK(hist_empty(nq, rep->nbins, rep->bins, rep->invalid));
        return 0;
    }
    const LaunchRange r{first, n};
    if (e->sub.empty()) return batch_report_run(d, e, db, r, index_base + first, rep);
    const uint64_t units = template_topk_lists(d, db, r);
    iris_report_t ones[kBatchStreamMax] = {};
    for (uint32_t q = 0; q < nq; ++q) {
        const iris_engine *c = e->sub[q];
        iris_report_t &one = ones[q];
        one.parts = rep->parts;
        if (want_match) {
            one.threshold = rep->threshold;
            one.matches_cap = rep->matches_cap;
            one.matches = rep->matches_cap ? rep->matches + q * rep->matches_cap : nullptr;
        }
        if (want_topk) {
            one.k = rep->k;
            one.topk = rep->topk + (size_t)q * rep->k;
        }
        if (want_hist) {
            one.nbins = rep->nbins;
            one.bins = rep->bins + (size_t)q * rep->nbins;
        }
        CHK(report_dispatch(d, n, index_base + first, &one, {units, [&](Pass p, const MatchSink &s) {
            return launch_template_select(d, db, c->qtab, c->qfrag, r, p, s);
        }}));
    }
    for (uint32_t q = 0; q < nq; ++q) {  // the counts once every query has succeeded
        if (want_match) rep->matches_counts[q] = ones[q].matches_count;
        if (want_topk) rep->topk_counts[q] = ones[q].topk_count;
        if (want_hist) rep->invalid[q] = ones[q].invalid;
    }
    return 0;
}

// ------------------------------------------------------------------ masks batch reports

// Two or three parts for the nq queries of a masks batch engine over w.r (not empty), every launch
// unit of the walk (MasksWalk, as the sibling calls split) from ONE pass: a group of 2..4 queries
// masks_batch_kernel<BATCH_REPORT> ("masks_batch_report"), a single query the single-query report
// pass on its slab ("masks_report"; LANES "masks" + "resolver_report").  The device's buffers are
// shared by region, as batch_report_run shares them: d->matches holds ONE lists region -- per query
// of a unit its lists and the merge's spare lists, sized for the largest unit -- and behind it the
// queries' match regions; d->match_count the nq match counters and behind them every query's
// histogram copies; d->match_sinks the ReportSinks[nq], staged through the pinned result and copied
// once; the pinned result the nq counts, the staged sinks, the merged lists [nq][k] and the nq rows,
// each at a 64-byte boundary.  A unit's pass is followed by its merge levels, so the region serves
// every unit in stream order (topk_run_units' argument: a unit's merge has consumed the region
// before the next unit's pass writes it; the match regions and counters are per query and never
// shared).  One hist_reduce over all nq rows (copies = 1: a copy) follows the last unit, and the
// call waits once.  With a matches part the call is a threshold-match call (matches_run_units) whose
// first pass is all units' report passes: room, overflow and rerun are
// iris_resolver_batch_matches_masks', the rerun that call's plain match pass of the one unit.  On
// LANES a rerun reuses the denominators where the workspace still holds that query's (the last
// query enqueued).  Nothing reaches the caller's arrays before every part has succeeded.
static int masks_batch_report_run(iris_device *d, const iris_engine *e, const iris_db *db, const MasksWalk &w,
                                  const uint16_t *const *shares, uint32_t parts, uint64_t base,
                                  const iris_batch_report_t *rep) {
    const bool want_match = rep->parts & IRIS_REPORT_MATCHES, want_topk = rep->parts & IRIS_REPORT_TOPK,
               want_hist = rep->parts & IRIS_REPORT_HIST;
    const uint32_t nq = e->nq;
    const uint64_t n = w.r.n;
    const uint32_t k = want_topk ? rep->k : 0, nbins = want_hist ? rep->nbins : 0;
    const uint32_t copies = !want_hist ? 0 : d->hooks.hist_copies ? d->hooks.hist_copies : kHistCopies;
    const size_t words = (size_t)nbins + 1, row = (size_t)copies * words;
    const size_t rows_bytes = want_hist ? nq * row * sizeof(uint64_t) : 0;
    // the lists a unit's pass writes per query, and the region the largest unit takes
    const auto unit_lists = [&](const MasksUnit &u) -> uint64_t {
        if (!want_topk) return 0;
        return u.m > 1 ? masks_batch_topk_units(d->hooks, w.r, u.m) : w.tiles ? masks_topk_units(d->hooks, w.r) : resolver_topk_units(n);
    };
    uint64_t region = 0;
    for (MasksUnit u = w.unit(0); u.m; u = w.unit(u.q0 + u.m)) {
        const uint64_t lists = unit_lists(u);
        region = std::max(region, (uint64_t)u.m * (lists + topk_spare_lists(lists)) * k);
    }
    const size_t lists_bytes = region * sizeof(Partial);
    const auto line = [](size_t b) { return (b + 63) / 64 * 64; };
    const size_t stage_off = line(nq * sizeof(uint64_t));
    const size_t topk_off = line(stage_off + nq * sizeof(ReportSinks));
    const size_t hist_off = line(topk_off + (size_t)nq * k * sizeof(Partial));
    CHK(ensure_host_result(d, hist_off + (want_hist ? nq * words * sizeof(uint64_t) : 0)));
    CHK(ensure(d, d->match_sinks, nq * sizeof(ReportSinks)));
    // the buffers' addresses are read when a step is enqueued: matches_run_units ensures them first
    const auto rows_dev = [=] { return (uint64_t *)d->match_count.p + nq; };
    struct {  // LANES: the query whose denominators the workspace holds
        const uint16_t *den = nullptr;
        uint32_t q = 0;
    } held;
    // one unit's pass of mode p: Report on the unit's device sinks, Match (the rerun) into ms
    const auto unit_pass = [&](const MasksUnit &u, Pass p, const MatchSink *ms, const ReportSinks *stage) -> int {
        const ReportSinks *dsinks = (const ReportSinks *)d->match_sinks.p + u.q0;
        if (u.m > 1) {
            if (p == Pass::Report)
                return timed(d, "masks_batch_report", n * u.m, [&] {
                    return launch_masks_batch(Pass::Report, d->hooks, d->stream, db->data, u.frags, u.m, w.r,
                                              {shares, parts, u.q0, dsinks, stage + u.q0});
                });
            return timed(d, "masks_batch_match", n * u.m, [&] {
                return launch_masks_batch(Pass::Match, d->hooks, d->stream, db->data, u.frags, u.m, w.r, {shares, parts, u.q0, ms});
            });
        }
        // one query through the single-query forms, on its slab of every part
        const uint16_t *sl[8];
        w.slabs(u.q0, shares, parts, sl);
        const uint16_t *den = !w.tiles && held.den && held.q == u.q0 ? held.den : nullptr;
        CHK(masks_single_launch(d, u.one, db, w.r, sl, parts, p, p == Pass::Report ? report_sink(dsinks) : ms[0], &den));
        held.den = den;
        held.q = u.q0;
        return 0;
    };
    // every unit's report pass and merge: ms = the nq match sinks, null without a matches part
    const auto report_passes = [&](const MatchSink *ms) -> int {
        char *res = (char *)d->host_result;
        ReportSinks *stage = (ReportSinks *)(res + stage_off);
        for (MasksUnit u = w.unit(0); u.m; u = w.unit(u.q0 + u.m)) {
            const uint64_t lists = unit_lists(u), stride = (lists + topk_spare_lists(lists)) * k;
            for (uint32_t s = 0; s < u.m; ++s) {
                ReportSinks &x = stage[u.q0 + s];
                x = ReportSinks{};
                if (ms) x.match = ms[u.q0 + s];
                if (want_topk) x.topk = topk_sink((Partial *)d->matches.p + s * stride, k);
                if (want_hist) x.hist = hist_sink(rows_dev() + (u.q0 + s) * row, nbins, copies);
            }
        }
        // the sinks cross to the device from pinned memory, as a template batch match pass's do
        HIPCHK(hipMemcpyAsync(d->match_sinks.p, stage, nq * sizeof(ReportSinks), hipMemcpyHostToDevice, d->stream));
        for (MasksUnit u = w.unit(0); u.m; u = w.unit(u.q0 + u.m)) {
            CHK(unit_pass(u, Pass::Report, nullptr, stage));
            if (!want_topk) continue;
            const uint64_t lists = unit_lists(u), stride = (lists + topk_spare_lists(lists)) * k;
            CHK(topk_merge_enqueue(d, (Partial *)d->matches.p, lists, stride, k, u.m, (Partial *)(res + topk_off) + (size_t)u.q0 * k));
        }
        return 0;
    };
    const auto enqueue = [&]() -> int {  // behind the last unit: the rows
        if (!want_hist) return 0;
        char *res = (char *)d->host_result;
        if (copies > 1)
            return timed(d, "hist_reduce", nq * row, [&] {
                return launch_hist_reduce(d->stream, rows_dev(), (uint32_t)words, copies, nq, (uint64_t *)(res + hist_off));
            });
        HIPCHK(hipMemcpyAsync(res + hist_off, rows_dev(), nq * words * sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
        return 0;
    };
    std::vector<Partial> best;
    std::vector<uint64_t> rows, mcounts;
    const auto taken = [&]() -> int {
        const char *res = (const char *)d->host_result;
        try {
            if (want_topk) best.assign((const Partial *)(res + topk_off), (const Partial *)(res + topk_off) + (size_t)nq * k);
            if (want_hist) rows.assign((const uint64_t *)(res + hist_off), (const uint64_t *)(res + hist_off) + nq * words);
        } catch (const std::bad_alloc &) {
            return fail(IRIS_E_NOMEM, "out of host memory");
        }
        return want_hist ? hist_rows_check(rows.data(), n, nbins, nq) : 0;
    };
    if (want_match) {
        std::vector<MatchUnit> units;
        try {
            mcounts.resize(nq);
            for (MasksUnit u = w.unit(0); u.m; u = w.unit(u.q0 + u.m))
                units.push_back(MatchUnit{u.q0, u.m, [&unit_pass, u](const MatchSink *ms) { return unit_pass(u, Pass::Match, ms, nullptr); }});
        } catch (const std::bad_alloc &) {
            return fail(IRIS_E_NOMEM, "out of host memory");
        }
        const MatchWhole whole{nq, report_passes};
        const MatchRider ride{lists_bytes, rows_bytes, enqueue, taken};
        CHK(matches_run_units(d, n, base, rep->threshold, rep->matches, rep->matches_cap, mcounts.data(), nq, false, units, &whole,
                              0, &ride));
        memcpy(rep->matches_counts, mcounts.data(), nq * sizeof(uint64_t));
    } else {
        const size_t count_bytes = nq * sizeof(uint64_t) + rows_bytes;
        CHK(ensure(d, d->matches, lists_bytes));
        CHK(ensure(d, d->match_count, count_bytes));
        HIPCHK(hipMemsetAsync(d->match_count.p, 0, count_bytes, d->stream));
        CHK(report_passes(nullptr));
        CHK(enqueue());
        CHK(sync(d));
        CHK(taken());
    }
    if (want_topk)
        for (uint32_t q = 0; q < nq; ++q)
            rep->topk_counts[q] = topk_list(best.data() + (size_t)q * k, k, base, rep->topk + (size_t)q * k);
    if (want_hist) hist_rows_write(rows.data(), nbins, nq, rep->bins, rep->invalid);  // checked in taken()
    return 0;
}

// Several of iris_resolver_batch_matches_masks, iris_resolver_batch_topk_masks and
// iris_resolver_batch_histogram_masks for every probe of a masks batch engine from one pass over the
// masks and the share slabs (header: "masks batch reports").  One part: the sibling call itself.
// Otherwise masks_batch_report_run.
int iris_resolver_batch_report_masks(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                                     const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                                     void *report) {
    IRIS_KEEP_DEVICE();
    const iris_batch_report_t *const rep = (const iris_batch_report_t *)report;
    CHK(batch_report_args(rep));  // the value arguments first: refused whatever the handles
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    CHK(masks_batch_args(e, db));
    CHK(share_args(shares_device, parts, n));
    for (uint32_t p = 0; n && p < parts; ++p) ARG(((uintptr_t)shares_device[p] & 1) == 0, "share array is not 2-byte aligned");
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (rep->parts == IRIS_REPORT_MATCHES)
        return iris_resolver_batch_matches_masks(e, db, first, n, shares_device, parts, index_base, rep->threshold, rep->matches,
                                                 rep->matches_cap, rep->matches_counts);
    if (rep->parts == IRIS_REPORT_TOPK)
        return iris_resolver_batch_topk_masks(e, db, first, n, shares_device, parts, index_base, rep->k, rep->topk,
                                              rep->topk_counts);
    if (rep->parts == IRIS_REPORT_HIST)
        return iris_resolver_batch_histogram_masks(e, db, first, n, shares_device, parts, rep->nbins, rep->bins, rep->invalid);
    if (n == 0) {  // nothing is launched
        if (rep->parts & IRIS_REPORT_MATCHES) memset(rep->matches_counts, 0, e->nq * sizeof(uint64_t));
        if (rep->parts & IRIS_REPORT_TOPK) memset(rep->topk_counts, 0, e->nq * sizeof(uint32_t));
        if (rep->parts & IRIS_REPORT_HIST) CHK(hist_empty(e->nq, rep->nbins, rep->bins, rep->invalid));
        return 0;
    }
    const MasksWalk w(e, db, first, n);
    return masks_batch_report_run(d, e, db, w, shares_device, parts, index_base, rep);
}

}  // extern "C"
