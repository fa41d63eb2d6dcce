// iris_api_resolver.hip — the C ABI (include/iris_hip.h): the resolver step on device arrays, on
// the masks database (single query and masks batch engine) and on host arrays.  Calls, locking and
// errors: see iris_api.hip.
#include <string.h>

#include "iris_handles.hpp"

using namespace iris;
using namespace iris_api;

// The share arrays of a resolver call: 1..8 parts and, unless the range is empty, the table of
// arrays and every part's array.  denoms: a call that also takes a denominators array passes
// `denoms != nullptr` (NULL is refused with the table, "NULL argument"); the *_masks calls leave it
// true.  A call with another check between its parts and its arrays keeps its own parts check there.
int iris_api::share_args(const uint16_t *const *shares, uint32_t parts, uint64_t n, bool denoms) {
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    ARG(n == 0 || (shares && denoms), "NULL argument");
    for (uint32_t p = 0; n && p < parts; ++p) ARG(shares[p], "NULL share array");
    return 0;
}

// The engine and database of a single-query *_masks call; a masks batch engine is sent to `batch_call`.
int iris_api::single_masks_args(const iris_engine *e, const iris_db *db, const char *batch_call) {
    ARG(e && db, "NULL argument");
    ARG(e->kind == IRIS_KIND_MASKS && db->k.kind == IRIS_KIND_MASKS, "needs a masks engine and a masks database");
    ARG(e->nq == 0, std::string("a masks batch engine runs through ") + batch_call);
    ARG(e->dev == db->dev, "engine and database live on different devices");
    return 0;
}

// The LANES form of the *_masks calls: the engine's masks kernel over r into the device's row
// workspace; *den = the denominators the resolver kernel enqueued next reads there.
int iris_api::enqueue_masks_denoms(const iris_engine *c, const iris_db *db, LaunchRange r, const uint16_t **den) {
    iris_device *d = c->dev;
    CHK(ensure(d, d->out_a, std::max<uint64_t>(r.n, 1) * kRot * 2));
    CHK(timed(d, "masks", r.n, [&] { return launch_masks(d->stream, db->data, c->qtab, r, (uint16_t *)d->out_a.p); }));
    *den = (const uint16_t *)d->out_a.p;
    return 0;
}

extern "C" {

static int resolver_finish(iris_device *d, uint32_t np, Partial *res) {
    if (np) {
        CHK(ensure_host_result(d, sizeof(Partial)));
        CHK(timed(d, "reduce", np, [&] { return launch_reduce(d->stream, (Partial *)d->partials.p, np, (Partial *)d->host_result); }));
    }
    CHK(sync(d));
    if (np) memcpy(res, d->host_result, sizeof(Partial));
    return 0;
}


// Partial.idx values of one launch are row indices of that launch; chunked
// host calls merge the per-chunk winners on the host in chunk order.
int iris_resolver_search(iris_device_t *d, const uint16_t *const *shares, uint32_t parts, const uint16_t *denoms,
                         uint64_t n, uint64_t index_base, double *dist_out_device, iris_match_t *out) {
    IRIS_KEEP_DEVICE();
    ARG(d && out, "NULL argument");
    CHK(share_args(shares, parts, n, denoms != nullptr));
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    const uint32_t np = resolver_partials(n);
    CHK(ensure(d, d->partials, (size_t)std::max<uint32_t>(np, 1) * sizeof(Partial)));
    CHK(timed(d, "resolver", n, [&] {
        return launch_resolver(Pass::Search, d->stream, shares, parts, denoms, n, {dist_out_device, (Partial *)d->partials.p});
    }));
    Partial res{};
    CHK(resolver_finish(d, n ? np : 0, &res));
    match_from(res, n > 0, index_base, out);
    return 0;
}

// The resolver step with the denominators computed on the fly from the masks
// database (src/main.rs:510-519 + 597-621): TILES runs the fused
// masks_mfma_kernel<MASKS_RESOLVE>; LANES the masks kernel into a workspace
// and then the resolver kernel.
int iris_resolver_search_masks(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                               const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                               double *dist_out_device, iris_match_t *out) {
    IRIS_KEEP_DEVICE();
    ARG(e && db && out, "NULL argument");
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    CHK(single_masks_args(e, db, "iris_resolver_batch_search_masks"));
    CHK(share_args(shares_device, parts, n));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    LaunchRange r{first, n};
    Partial res{};
    if (db->k.layout == IRIS_LAYOUT_TILES) {
        const uint32_t np = n ? masks_resolve_partials(d->hooks, r) : 0;
        CHK(ensure(d, d->partials, (size_t)std::max<uint32_t>(np, 1) * sizeof(Partial)));
        CHK(timed(d, "masks_resolve", n, [&] {
            return launch_masks_resolve(Pass::Search, d->hooks, d->stream, db->data, e->qfrag, r, shares_device, parts,
                                        {dist_out_device, (Partial *)d->partials.p});
        }));
        CHK(resolver_finish(d, np, &res));
    } else {
        const uint16_t *den = nullptr;
        CHK(enqueue_masks_denoms(e, db, r, &den));
        const uint32_t np = resolver_partials(n);
        CHK(ensure(d, d->partials, (size_t)std::max<uint32_t>(np, 1) * sizeof(Partial)));
        CHK(timed(d, "resolver", n, [&] {
            return launch_resolver(Pass::Search, d->stream, shares_device, parts, den, n, {dist_out_device, (Partial *)d->partials.p});
        }));
        CHK(resolver_finish(d, n ? np : 0, &res));
    }
    match_from(res, n > 0, index_base, out);
    return 0;
}

// The fused resolver step (iris_resolver_search_masks) for every query of a masks batch engine in
// one pass over the masks: shares_device[p] holds nq slabs of n rows (what
// iris_distance_batch_process_device wrote for participant p).  Every query's partials get a run
// of their own, each run is reduced into its slot of the pinned result, and the call waits once.
int iris_resolver_batch_search_masks(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                                     const uint16_t *const *shares_device, uint32_t parts, uint64_t index_base,
                                     double *dist_out_device, iris_match_t *out) {
    IRIS_KEEP_DEVICE();
    ARG(out, "NULL argument");
    CHK(masks_batch_args(e, db));
    CHK(share_args(shares_device, parts, n));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    const uint32_t nq = e->nq;
    if (n == 0) {
        for (uint32_t q = 0; q < nq; ++q) match_from(Partial{}, false, index_base, &out[q]);
        return 0;
    }
    const MasksWalk w(e, db, first, n);
    // partials: one run of `stride` per query (LANES: the resolver kernel's)
    const uint32_t stride = !w.tiles ? resolver_partials(n)
                                     : std::max(masks_resolve_partials(d->hooks, w.r),
                                                w.batch ? masks_batch_partials(d->hooks, w.r) : 0u);
    CHK(ensure(d, d->partials, (size_t)nq * stride * sizeof(Partial)));
    CHK(ensure_host_result(d, (size_t)nq * sizeof(Partial)));
    Partial *parts_dev = (Partial *)d->partials.p, *res = (Partial *)d->host_result;
    auto reduce = [&](uint32_t q, uint32_t np) {
        return timed(d, "reduce", np, [&] { return launch_reduce(d->stream, parts_dev + (size_t)q * stride, np, res + q); });
    };
    for (MasksUnit u = w.unit(0); u.m; u = w.unit(u.q0 + u.m)) {
        Partial *pq = parts_dev + (size_t)u.q0 * stride;
        if (u.m > 1) {
            const MasksBatchResolve rs{shares_device, parts, u.q0, dist_out_device, pq, stride};
            uint32_t np = 0;
            CHK(timed(d, "masks_batch_resolve", n * u.m, [&] {
                return launch_masks_batch(Pass::Search, d->hooks, d->stream, db->data, u.frags, u.m, w.r, {rs, &np});
            }));
            for (uint32_t s = 0; s < u.m; ++s) CHK(reduce(u.q0 + s, np));
            continue;
        }
        // one query through the single-query forms, on its slab of every part
        const uint16_t *sl[8];
        w.slabs(u.q0, shares_device, parts, sl);
        double *dist = dist_out_device ? dist_out_device + (uint64_t)u.q0 * n : nullptr;
        if (w.tiles) {
            CHK(timed(d, "masks_resolve", n, [&] {
                return launch_masks_resolve(Pass::Search, d->hooks, d->stream, db->data, u.one->qfrag, w.r, sl, parts, {dist, pq});
            }));
            CHK(reduce(u.q0, masks_resolve_partials(d->hooks, w.r)));
        } else {
            const uint16_t *den = nullptr;
            CHK(enqueue_masks_denoms(u.one, db, w.r, &den));
            CHK(timed(d, "resolver", n, [&] { return launch_resolver(Pass::Search, d->stream, sl, parts, den, n, {dist, pq}); }));
            CHK(reduce(u.q0, resolver_partials(n)));
        }
    }
    CHK(sync(d));
    for (uint32_t q = 0; q < nq; ++q) match_from(res[q], true, index_base, &out[q]);
    return 0;
}

// The resolver step from host share arrays and the resident masks database (src/main.rs:510-519 +
// 597-621, the shares as they arrive from the participants): the helper threads sum each chunk's
// parts into a pinned upload slot (62 B per record over the host link), the copy engine moves it to a
// device staging slot, and the fused masks + resolve kernel computes the denominators on the fly
// against the summed rows; each chunk's winner is reduced into its own pinned result slot, the host
// fills the next slot meanwhile, and the call waits once.  LANES databases run chunk by chunk through
// iris_resolver_search_masks.
int iris_resolver_search_masks_host(iris_engine_t *e, const iris_db_t *db, uint64_t first, uint64_t n,
                                    const uint16_t *const *shares, uint32_t parts, uint64_t index_base,
                                    iris_match_t *out) {
    IRIS_KEEP_DEVICE();
    ARG(e && db && out, "NULL argument");
    ARG(parts >= 1 && parts <= 8, "parts must be 1..8");
    CHK(single_masks_args(e, db, "iris_resolver_batch_search_masks"));
    CHK(share_args(shares, parts, n));
    iris_device *d = e->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    iris_match_t best;
    match_from(Partial{}, false, 0, &best);
    if (n == 0) {
        *out = best;
        return 0;
    }
    const size_t row = (size_t)kRot * 2;
    const uint64_t ch = std::min<uint64_t>(n, kUploadSlot / row / 64 * 64);
    const uint64_t chunks = (n + ch - 1) / ch;
    CHK(ensure_upin(d));
    CHK(ensure(d, d->staging, kUploadSlots * (size_t)ch * row));
    const bool tiles = db->k.layout == IRIS_LAYOUT_TILES;
    uint32_t np_max = 1;
    for (uint64_t c = 0; tiles && c < chunks; ++c)
        np_max = std::max(np_max, masks_resolve_partials(d->hooks, LaunchRange{first + c * ch, std::min(ch, n - c * ch)}));
    if (tiles) {
        CHK(ensure(d, d->partials, (size_t)np_max * sizeof(Partial)));
        CHK(ensure_host_result(d, (size_t)chunks * sizeof(Partial)));
    }
    Partial *res = (Partial *)d->host_result;
    int rc = 0;
    for (uint64_t c = 0; c < chunks && rc == 0; ++c) {
        const uint64_t a = c * ch, m = std::min<uint64_t>(ch, n - a);
        const int b = (int)(c % kUploadSlots);
        // pinned slot b was last read by the copy of chunk c - kUploadSlots
        if (c >= (uint64_t)kUploadSlots && hipEventSynchronize(d->upin_ev[b]) != hipSuccess) {
            rc = fail(IRIS_E_HIP, "hipEventSynchronize");
            break;
        }
        const uint16_t *src[8];
        for (uint32_t p = 0; p < parts; ++p) src[p] = shares[p] + a * kRot;
        parallel_sum_u16((uint16_t *)d->upin[b], src, (int)parts, m * kRot, d->ordinal);
        char *stage = (char *)d->staging.p + (size_t)b * ch * row;
        if (hipMemcpyAsync(stage, d->upin[b], m * row, hipMemcpyHostToDevice, d->stream) != hipSuccess ||
            hipEventRecord(d->upin_ev[b], d->stream) != hipSuccess) {
            rc = fail(IRIS_E_HIP, "hipMemcpyAsync upload");
            break;
        }
        const uint16_t *dsum = (const uint16_t *)stage;
        if (!tiles) {  // the summed rows through the LANES form, one chunk at a time
            iris_match_t cm;
            rc = iris_resolver_search_masks(e, db, first + a, m, &dsum, 1, index_base + a, nullptr, &cm);
            if (rc == 0) {
                iris_match_t pair[2] = {best, cm};
                rc = iris_match_merge(pair, 2, &best);
            }
            continue;
        }
        const LaunchRange r{first + a, m};
        const uint32_t np = masks_resolve_partials(d->hooks, r);
        rc = timed(d, "masks_resolve", m, [&] {
            return launch_masks_resolve(Pass::Search, d->hooks, d->stream, db->data, e->qfrag, r, &dsum, 1,
                                        {nullptr, (Partial *)d->partials.p});
        });
        // the chunk's winner, its index offset to the call's records, into result slot c
        if (rc == 0)
            rc = timed(d, "reduce", np, [&] { return launch_reduce(d->stream, (Partial *)d->partials.p, np, res + c, a); });
    }
    const int rs = sync(d);  // the pinned slots are free again and every chunk's winner is in place
    CHK(rc);
    CHK(rs);
    for (uint64_t c = 0; tiles && c < chunks; ++c) {
        iris_match_t pair[2] = {best, {}};
        match_from(res[c], true, index_base, &pair[1]);
        CHK(iris_match_merge(pair, 2, &best));
    }
    *out = best;
    return 0;
}

// The resolver step over host arrays (the participants' rows as they arrive, src/main.rs:597-621):
// the helper threads sum a chunk's parts (the wrapping u16 sum the kernel would take first,
// src/main.rs:601-605) into one pinned upload slot beside a copy of its denominators -- 124 B per
// record cross the host link instead of 62 (P + 1) -- the copy engine moves the slot into a device
// staging slot, and the records are decoded + reduced there (the reduce writes the chunk's winner, its index already
// offset, into a pinned result slot), while the host fills the other slot with the next chunk; the
// call waits once, at the end, and merges the chunks' winners in chunk order.  The runtime's own
// copy of a pageable source ran at 29-30 GB/s for some caller arrays and 53-55 GB/s for others
// (profiles/r04_host_upload.txt, r06am_host_resolver.txt), so, as large database writes do, the
// call takes whichever of the two forms was faster lately (a tuner of its own, resolver_tune).
static int resolver_host_pinned(iris_device *d, const uint16_t *const *shares, uint32_t parts, const uint16_t *denoms,
                                uint64_t n, uint64_t index_base, iris_match_t *out) {
    iris_match_t best;
    match_from(Partial{}, false, 0, &best);
    const size_t row = (size_t)kRot * 2;
    const uint32_t arrays = 2;
    // records per slot (the parts' summed rows, then the denominators), a multiple of 64
    const uint64_t ch = std::min<uint64_t>(n, std::max<uint64_t>(64, kUploadSlot / (arrays * row) / 64 * 64));
    const uint64_t chunks = (n + ch - 1) / ch;
    const size_t slot = (size_t)ch * arrays * row;
    CHK(ensure_upin(d));
    CHK(ensure(d, d->staging, kUploadSlots * slot));
    CHK(ensure(d, d->partials, (size_t)std::max<uint32_t>(resolver_partials(ch), 1) * sizeof(Partial)));
    CHK(ensure_host_result(d, (size_t)chunks * sizeof(Partial)));
    Partial *res = (Partial *)d->host_result;
    int rc = 0;
    for (uint64_t c = 0; c < chunks && rc == 0; ++c) {
        const uint64_t a = c * ch, m = std::min<uint64_t>(ch, n - a);
        const int b = (int)(c % kUploadSlots);
        // pinned slot b was last read by the copy of chunk c - kUploadSlots (the previous call's
        // copies ended with its sync)
        if (c >= (uint64_t)kUploadSlots && hipEventSynchronize(d->upin_ev[b]) != hipSuccess) {
            rc = fail(IRIS_E_HIP, "hipEventSynchronize");
            break;
        }
        char *pin = (char *)d->upin[b];
        const uint16_t *src[8];
        for (uint32_t p = 0; p < parts; ++p) src[p] = shares[p] + a * kRot;
        parallel_sum_u16((uint16_t *)pin, src, (int)parts, m * kRot, d->ordinal);
        parallel_copy(pin + m * row, (const char *)(denoms + a * kRot), m * row, d->ordinal);
        char *stage = (char *)d->staging.p + (size_t)b * slot;
        if (hipMemcpyAsync(stage, pin, (size_t)arrays * m * row, hipMemcpyHostToDevice, d->stream) != hipSuccess ||
            hipEventRecord(d->upin_ev[b], d->stream) != hipSuccess) {
            rc = fail(IRIS_E_HIP, "hipMemcpyAsync upload");
            break;
        }
        const uint16_t *dsum = (const uint16_t *)stage;
        const uint16_t *dden = (const uint16_t *)(stage + m * row);
        const uint32_t np = resolver_partials(m);
        rc = timed(d, "resolver", m, [&] {
            return launch_resolver(Pass::Search, d->stream, &dsum, 1, dden, m, {nullptr, (Partial *)d->partials.p});
        });
        // the chunk's winner, its index offset to the call's records, into result slot c
        if (rc == 0)
            rc = timed(d, "reduce", np, [&] { return launch_reduce(d->stream, (Partial *)d->partials.p, np, res + c, a); });
    }
    const int rs = sync(d);  // the pinned slots are free again and every chunk's winner is in place
    CHK(rc);
    CHK(rs);
    for (uint64_t c = 0; c < chunks; ++c) {
        iris_match_t pair[2] = {best, {}};
        match_from(res[c], true, index_base, &pair[1]);
        CHK(iris_match_merge(pair, 2, &best));
    }
    *out = best;
    return 0;
}

// The runtime's copy of each pageable array into device staging, one chunk of up to 1M records at a
// time, and the device-input resolver on it.
static int resolver_host_runtime(iris_device *d, const uint16_t *const *shares, uint32_t parts, const uint16_t *denoms,
                                 uint64_t n, uint64_t index_base, iris_match_t *out) {
    const uint64_t ch = std::min<uint64_t>(n, 1ull << 20);
    const size_t row = (size_t)kRot * 2;
    CHK(ensure(d, d->staging, std::max<uint64_t>(ch, 1) * row * (parts + 1)));
    iris_match_t best;
    match_from(Partial{}, false, 0, &best);
    for (uint64_t done = 0; done < n; done += ch) {
        const uint64_t m = std::min<uint64_t>(ch, n - done);
        const uint16_t *dev_sh[8];
        for (uint32_t p = 0; p <= parts; ++p) {
            uint16_t *dst = (uint16_t *)((char *)d->staging.p + (size_t)p * ch * row);
            HIPCHK(hipMemcpyAsync(dst, (p < parts ? shares[p] : denoms) + done * kRot, m * row, hipMemcpyHostToDevice,
                                  d->stream));
            if (p < parts) dev_sh[p] = dst;
        }
        const uint16_t *dden = (const uint16_t *)((char *)d->staging.p + (size_t)parts * ch * row);
        iris_match_t cm;
        CHK(iris_resolver_search(d, dev_sh, parts, dden, m, index_base + done, nullptr, &cm));
        iris_match_t pair[2] = {best, cm};
        CHK(iris_match_merge(pair, 2, &best));
    }
    *out = best;
    return 0;
}

int iris_resolver_search_host(iris_device_t *d, const uint16_t *const *shares, uint32_t parts, const uint16_t *denoms,
                              uint64_t n, uint64_t index_base, iris_match_t *out) {
    IRIS_KEEP_DEVICE();
    ARG(d && out, "NULL argument");
    CHK(share_args(shares, parts, n, denoms != nullptr));
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    if (n == 0) {
        match_from(Partial{}, false, 0, out);
        return 0;
    }
    const size_t bytes = (size_t)n * kRot * 2 * (parts + 1);
    if (d->hooks.upload == 1 || d->hooks.upload == 2 || bytes < kUploadTuneMin)  // test hook, or small: one path
        return (d->hooks.upload == 1 ? resolver_host_pinned : resolver_host_runtime)(d, shares, parts, denoms, n,
                                                                                      index_base, out);
    UploadTune &u = d->resolver_tune;
    const int path = u.pick();
    const auto t0 = std::chrono::steady_clock::now();
    int rc = path == 0 ? resolver_host_pinned(d, shares, parts, denoms, n, index_base, out)
                       : resolver_host_runtime(d, shares, parts, denoms, n, index_base, out);
    if (rc == IRIS_E_NOMEM && path == 0 && d->upin_cap < kUploadSlot) {  // no pinned slots: the runtime's copy
        u.no_pinned = true;
        return resolver_host_runtime(d, shares, parts, denoms, n, index_base, out);
    }
    CHK(rc);
    u.record(path, (double)bytes / std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}

}  // extern "C"
