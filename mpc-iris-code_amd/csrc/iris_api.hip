// iris_api.hip — the C ABI (include/iris_hip.h): devices, device-resident
// databases with their uploads, and host helpers.  Engines are in
// iris_api_engines.hip, searches in iris_api_search.hip, the resolver step in
// iris_api_resolver.hip, threshold matching and top-k in iris_api_select.hip.
//
// Every call is blocking and serialised per device (one HIP stream per
// device).  Errors never throw across the ABI: they return a negative status
// and set a thread-local message (iris_last_error).
#include <math.h>
#include <stdio.h>
#include <ctype.h>
#include <string.h>
#include <unistd.h>

#include <new>

#include "iris_handles.hpp"

using namespace iris;
using namespace iris_api;

namespace {

constexpr size_t kUploadPieceMin = 4ull << 20;  // a write is cut into at least 4 slots of at least this

int db_write_runtime(iris_db *db, uint64_t index, const void *records, uint64_t n);

}  // namespace

// The device's pinned upload slots (kUploadSlot bytes each) and their events, allocated once.
int iris_api::ensure_upin(iris_device *d) {
    if (d->upin_cap >= kUploadSlot) return 0;
    CHK(sync(d));  // no copy uses the old buffers any more
    for (int b = 0; b < kUploadSlots; ++b)
        if (d->upin[b]) HIPCHK(hipHostFree(d->upin[b]));
    for (int b = 0; b < kUploadSlots; ++b) d->upin[b] = nullptr;
    for (int b = 0; b < kUploadSlots; ++b) {
        const hipError_t e = hipHostMalloc(&d->upin[b], kUploadSlot, hipHostMallocDefault);
        if (e != hipSuccess) {
            d->upin[b] = nullptr;
            return fail(IRIS_E_NOMEM, std::string("hipHostMalloc upload buffer: ") + hipGetErrorString(e));
        }
    }
    for (int b = 0; b < kUploadSlots; ++b)
        if (!d->upin_ev[b]) HIPCHK(hipEventCreateWithFlags(&d->upin_ev[b], hipEventDisableTiming));
    d->upin_cap = kUploadSlot;
    return 0;
}

// A large write through pinned slots: the helper threads copy each slot's records from the
// caller's pageable array into one of two pinned buffers, the copy engine moves it to one of two
// device staging slots and the pack kernel stores it, while the host already fills the other
// pinned buffer.  The runtime's copy of a pageable source ran at 29-30 GB/s for some caller arrays
// and 53 GB/s for others; this path moved 48-52 GB/s for both (profiles/r04_host_upload.txt).
// Writes of 8 MB and more take whichever of the two was faster lately (UploadTune);
// IRIS_UPLOAD=pinned|runtime (test hook) pins one.
int iris_api::db_write_pinned(iris_db *db, uint64_t index, const void *records, uint64_t n, const SlotFill *fill) {
    iris_device *d = db->dev;
    const KindInfo &k = db->k;
    db_written(db);
    // at least four slots per write (so the host's copy of one overlaps the copy engine's of another)
    const size_t piece = std::min(kUploadSlot, std::max(kUploadPieceMin, (size_t)n * k.rec_bytes / 4));
    const uint64_t ch = std::max<uint64_t>(64, piece / k.rec_bytes / 64 * 64);
    const size_t slot = (size_t)ch * k.rec_bytes;
    CHK(ensure_upin(d));  // host first: an IRIS_E_NOMEM with the slots in place is the device's
    CHK(ensure(d, d->staging, kUploadSlots * slot));
    int rc = 0;
    uint64_t c = 0;
    for (uint64_t done = 0; done < n && rc == 0; done += ch, ++c) {
        const uint64_t m = std::min<uint64_t>(ch, n - done);
        const int b = (int)(c % kUploadSlots);
        // pinned buffer b was last read by the copy of slot c - kUploadSlots (this call) or by the previous
        // call's copies (which ended with a sync)
        if (c >= (uint64_t)kUploadSlots && hipEventSynchronize(d->upin_ev[b]) != hipSuccess) {
            rc = fail(IRIS_E_HIP, "hipEventSynchronize");
            break;
        }
        if (fill) {
            if (!(*fill)(d->upin[b], (size_t)done * k.rec_bytes, (size_t)m * k.rec_bytes)) {
                rc = fail(IRIS_E_IO, "read failed (I/O error, or the file shrank under the load)");
                break;
            }
        } else {
            parallel_copy(d->upin[b], (const char *)records + done * k.rec_bytes, (size_t)m * k.rec_bytes, d->ordinal);
        }
        void *stage = (char *)d->staging.p + (size_t)b * slot;
        if (hipMemcpyAsync(stage, d->upin[b], (size_t)m * k.rec_bytes, hipMemcpyHostToDevice, d->stream) != hipSuccess) {
            rc = fail(IRIS_E_HIP, "hipMemcpyAsync upload");
            break;
        }
        if (hipEventRecord(d->upin_ev[b], d->stream) != hipSuccess) {
            rc = fail(IRIS_E_HIP, "hipEventRecord");
            break;
        }
        rc = timed(d, "pack", m, [&] { return launch_pack(d->stream, k, stage, db->data, index + done, m); });
    }
    const int rs = sync(d);  // the pinned buffers are free again when the call returns
    CHK(rc);
    CHK(rs);
    db->len = std::max(db->len, index + n);
    return 0;
}

int iris_api::db_store_locked(iris_db *db, uint64_t index, const void *records, uint64_t n) {
    iris_device *d = db->dev;
    if (index > db->len) return fail(IRIS_E_RANGE, "iris_db_write: index beyond the end of the database");
    if (n > db->cap - index) return fail(IRIS_E_RANGE, "iris_db_write: database capacity exceeded");
    if (n == 0) return 0;
    ARG(records != nullptr, "iris_db_write: records is NULL");
    db_written(db);
    const KindInfo &k = db->k;
    const size_t bytes = (size_t)n * k.rec_bytes;
    if (d->hooks.upload == 1 && bytes >= kUploadTuneMin) return db_write_pinned(db, index, records, n);
    if (d->hooks.upload == 0 && bytes >= kUploadTuneMin) {
        // the faster path for this caller's arrays, as measured on its recent writes
        UploadTune &u = d->upload_tune;
        const int path = u.pick();
        const auto t0 = std::chrono::steady_clock::now();
        int rc = path == 0 ? db_write_pinned(db, index, records, n) : db_write_runtime(db, index, records, n);
        if (rc == IRIS_E_NOMEM && path == 0 && d->upin_cap < kUploadSlot) {
            // no pinned host memory for the slots: the runtime's copy from now on (a device
            // allocation failure is the caller's error and leaves the tuner as it was)
            u.no_pinned = true;
            return db_write_runtime(db, index, records, n);
        }
        CHK(rc);
        u.record(path, (double)bytes / std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        return 0;
    }
    return db_write_runtime(db, index, records, n);
}

int iris_api::db_write_locked(iris_db *db, uint64_t index, const void *records, uint64_t n) {
    db_detach(db);
    return db_store_locked(db, index, records, n);
}

int iris_api::range_ok(const iris_db *db, uint64_t first, uint64_t n) {
    if (first > db->len || n > db->len - first) return fail(IRIS_E_RANGE, "record range outside the database");
    return 0;
}

namespace {

// The runtime's copy of the pageable source, through one 256-MB staging chunk at a time.
int db_write_runtime(iris_db *db, uint64_t index, const void *records, uint64_t n) {
    iris_device *d = db->dev;
    const KindInfo &k = db->k;
    const uint64_t ch = chunk_records(k);
    CHK(ensure(d, d->staging, std::min<uint64_t>(n, ch) * k.rec_bytes));
    for (uint64_t done = 0; done < n; done += ch) {
        const uint64_t m = std::min<uint64_t>(ch, n - done);
        HIPCHK(hipMemcpyAsync(d->staging.p, (const char *)records + done * k.rec_bytes, m * k.rec_bytes,
                              hipMemcpyHostToDevice, d->stream));
        CHK(timed(d, "pack", m, [&] { return launch_pack(d->stream, k, d->staging.p, db->data, index + done, m); }));
        CHK(sync(d));  // staging is reused by the next chunk
    }
    db->len = std::max(db->len, index + n);
    return 0;
}

double rust_f64_min(double a, double b) {
    if (isnan(a)) return b;
    if (isnan(b)) return a;
    return a < b ? a : b;
}

// The host NUMA node the device hangs off (sysfs of its PCI function); a one-node host is node 0;
// -1 when unknown.
int device_numa_node(int ordinal) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus) - 1, ordinal) != hipSuccess) return -1;
    for (char *c = bus; *c; ++c) *c = (char)tolower((unsigned char)*c);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    int node = -1;
    if (FILE *f = fopen(path.c_str(), "r")) {
        if (fscanf(f, "%d", &node) != 1) node = -1;
        fclose(f);
    }
    if (node < 0 && access("/sys/devices/system/node/node1", F_OK) != 0 && access("/sys/devices/system/node/node0", F_OK) == 0)
        node = 0;
    return node;
}

void device_teardown(iris_device *d) {
    {
        std::lock_guard<std::recursive_mutex> g(d->mu);
        (void)hipSetDevice(d->ordinal);
        resident_drop_all(d);
        (void)hipStreamSynchronize(d->stream);
        for (DevBuf *b : {&d->partials, &d->result, &d->staging, &d->out_a, &d->out_b, &d->ticket, &d->tempdb,
                          &d->matches, &d->match_count, &d->match_sinks})
            if (b->p) (void)hipFree(b->p);
        side_sync(d);
        for (MatchBufs &m : d->match_free)
            if (m.dev.p) (void)hipFree(m.dev.p);
        for (MatchBufs &m : d->topk_free)
            if (m.dev.p) (void)hipFree(m.dev.p);
        for (MatchBufs &m : d->report_free)
            if (m.dev.p) (void)hipFree(m.dev.p);
        for (int b = 0; b < 2; ++b) {
            if (d->apart[b].p) (void)hipFree(d->apart[b].p);
            if (d->apart_read[b]) (void)hipEventDestroy(d->apart_read[b]);
            if (d->apart_written[b]) (void)hipEventDestroy(d->apart_written[b]);
        }
        for (int b = 0; b < kUploadRing; ++b) {
            if (d->upin[b]) (void)hipHostFree(d->upin[b]);
            if (d->upin_ev[b]) (void)hipEventDestroy(d->upin_ev[b]);
        }
        for (SharePass &s : d->share_ring) {
            if (s.slot) (void)hipFree(s.slot);
            if (s.done.p) (void)hipFree(s.done.p);
            if (s.qbuf) (void)hipFree(s.qbuf);
            if (s.ended) (void)hipEventDestroy(s.ended);
        }
        if (d->share_count) (void)hipFree(d->share_count);
        if (d->share_reg) (void)hipEventDestroy(d->share_reg);
        if (d->share) (void)hipStreamDestroy(d->share);
        if (d->aux) (void)hipStreamDestroy(d->aux);
        if (d->aux2) (void)hipStreamDestroy(d->aux2);
        if (d->host_result) (void)hipHostFree(d->host_result);
        if (d->host_done) (void)hipHostFree(d->host_done);
        for (void *b : d->slot_blocks) (void)hipHostFree(b);
        for (auto &q : d->qpool) (void)hipFree(q.second);
        d->qpool.clear();
        for (auto &q : d->rows_pool) (void)hipHostFree(q.second);
        d->rows_pool.clear();
        if (d->ra_order) (void)hipEventDestroy(d->ra_order);
        for (auto &p : d->pending) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
        for (auto e : d->event_pool) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(d->stream);
    }
    delete d;
}

}  // namespace

void iris_api::device_retain(iris_device *d) { d->refs.fetch_add(1, std::memory_order_relaxed); }
void iris_api::device_release(iris_device *d) {
    if (d->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) device_teardown(d);
}

// ================================================================== C ABI

extern "C" {

const char *iris_last_error(void) { return g_err.c_str(); }
#ifndef IRIS_BUILD_KNOBS
#define IRIS_BUILD_KNOBS ""
#endif
// "iris-hip X (gfx950)", plus " knobs: -DIRIS_..." when the build set compile-time knobs
const char *iris_version(void) {
    static const std::string v = std::string("iris-hip 0.3.0 (gfx950)") +
                                 (sizeof(IRIS_BUILD_KNOBS) > 1 ? std::string(" knobs: ") + IRIS_BUILD_KNOBS : std::string());
    return v.c_str();
}

int iris_config(const iris_device_t *d, char *buf, size_t len, size_t *needed) {
    ARG(buf || len == 0, "NULL buffer");
    Hooks now;
    if (!d) read_hooks(&now);
    std::string s(format_hooks(d ? d->hooks : now, nullptr, 0), '\0');
    format_hooks(d ? d->hooks : now, &s[0], s.size() + 1);
    if (d) {
        s += " numa_node=" + std::to_string(d->numa_node);
        char r[96];  // large writes' measured rates (GB/s) through the pinned slots / the runtime's copy
        snprintf(r, sizeof(r), " upload_gbps=%.1f/%.1f", d->upload_tune.gbps[0] / 1e9, d->upload_tune.gbps[1] / 1e9);
        s += r;
        uint64_t rc = 0, rbytes = 0;
        int via_fd = 0;
        std::string skip;
        {
            std::lock_guard<std::recursive_mutex> g(const_cast<iris_device *>(d)->mu);
            resident_stats(d, &rc, &rbytes, &via_fd);
            skip = d->resident_skip;
            // read-ahead windows since the last iris_device_reset_stats: launches, records computed,
            // the largest window (records)
            s += " readahead_windows=" + std::to_string(d->ra_launches) + "/" + std::to_string(d->ra_records) + "/" +
                 std::to_string(d->ra_window_max);
        }
        s += " resident=" + std::to_string(rc) + "/" + std::to_string(rbytes) + " resident_via_fd=" + std::to_string(via_fd);
        uint64_t ab_pending = 0, ab_total = 0;  // RCCL inits abandoned on a formation timeout: pending/total
        abandoned_inits(d->ordinal, &ab_pending, &ab_total);
        s += " abandoned_inits=" + std::to_string(ab_pending) + "/" + std::to_string(ab_total);
        if (!skip.empty()) {  // one token: spaces and '=' replaced
            for (char &c : skip)
                if (c == ' ' || c == '=') c = '_';
            s += " resident_skip=" + skip;
        }
    }
    if (buf && len) {
        const size_t n = std::min(len - 1, s.size());
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    if (needed) *needed = s.size();
    return 0;
}

int iris_device_count(int *count) {
    ARG(count, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count = n;
    return 0;
}

int iris_device_open(int ordinal, iris_device_t **out) {
    IRIS_KEEP_DEVICE();
    ARG(out, "out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(IRIS_E_NODEV, "no HIP device visible");
    if (ordinal < 0 || ordinal >= n) return fail(IRIS_E_NODEV, "device ordinal out of range");
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, ordinal));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(IRIS_E_NODEV, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950");
    iris_device *d = new (std::nothrow) iris_device();
    if (!d) return fail(IRIS_E_NOMEM, "out of host memory");
    d->ordinal = ordinal;
    read_hooks(&d->hooks);  // the environment's knobs, once (iris_config reports them)
    if (d->hooks.ignored) {  // said once per process: a test hook in a production environment does nothing
        static std::once_flag warned;
        std::call_once(warned, [&] {
            char buf[512];
            format_hooks(d->hooks, buf, sizeof(buf));
            fprintf(stderr, "iris-hip: test-only hooks ignored (IRIS_TEST_HOOKS is not 1): %s\n", strstr(buf, "ignored="));
        });
    }
    hipError_t e = hipSetDevice(ordinal);
    // test hook IRIS_SCHEDULE = spin | yield | blocking: how host waits on this device behave
    // (takes effect only before the process's first context on the device)
    if (d->hooks.schedule) {
        const unsigned f = d->hooks.schedule == 1   ? hipDeviceScheduleSpin
                           : d->hooks.schedule == 2 ? hipDeviceScheduleYield
                                                    : hipDeviceScheduleBlockingSync;
        (void)hipSetDeviceFlags(f);
        (void)hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
    if (e == hipSuccess) d->numa_node = device_numa_node(ordinal);
    if (e != hipSuccess) {
        delete d;
        return fail(IRIS_E_HIP, std::string("stream create: ") + hipGetErrorString(e));
    }
    *out = d;
    return 0;
}

int iris_device_close(iris_device_t *d) {
    IRIS_KEEP_DEVICE();
    if (!d) return 0;
    device_release(d);  // torn down now, or when its last database / engine is destroyed
    return 0;
}

int iris_device_synchronize(iris_device_t *d) {
    IRIS_KEEP_DEVICE();
    ARG(d, "device is NULL");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    resident_sweep(d);  // copies of mappings that are gone free their memory (at most once a second)
    return sync(d);
}

int iris_device_stream(iris_device_t *d, void **stream) {
    ARG(d && stream, "NULL argument");
    *stream = (void *)d->stream;
    return 0;
}

int iris_device_memory(iris_device_t *d, size_t *free_bytes, size_t *total_bytes) {
    IRIS_KEEP_DEVICE();
    ARG(d && free_bytes && total_bytes, "NULL argument");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    HIPCHK(hipMemGetInfo(free_bytes, total_bytes));
    return 0;
}

int iris_device_set_profiling(iris_device_t *d, int enabled) {
    IRIS_KEEP_DEVICE();
    ARG(d, "device is NULL");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    d->profiling = enabled != 0;
    return 0;
}

int iris_device_kernel_stats(iris_device_t *d, const char *kernel, uint64_t *launches, double *total_ms,
                             uint64_t *items) {
    IRIS_KEEP_DEVICE();
    ARG(d && kernel, "NULL argument");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    const int shared = !strcmp(kernel, "search_shared")  ? kShareSearch
                       : !strcmp(kernel, "match_shared") ? kShareMatch
                       : !strcmp(kernel, "topk_shared")  ? kShareTopk
                       : !strcmp(kernel, "report_shared") ? kShareReport
                                                         : -1;
    if (shared >= 0) {
        // shared passes: launches = searches (match, top-k passes) registered as guests, items = tile groups
        // carried for them (a device counter, read behind whatever the device stream holds); no time
        // of its own
        unsigned long long carried = 0;
        if (d->share_count) {
            CHK(set_device(d));
            HIPCHK(hipMemcpyAsync(&carried, d->share_count + shared, sizeof(carried), hipMemcpyDeviceToHost, d->stream));
            HIPCHK(hipStreamSynchronize(d->stream));
        }
        if (launches) *launches = d->share_regs[shared];
        if (total_ms) *total_ms = 0;
        if (items) *items = carried;
        return 0;
    }
    auto it = d->stats.find(kernel);
    KStat s = it == d->stats.end() ? KStat{} : it->second;
    if (launches) *launches = s.launches;
    if (total_ms) *total_ms = s.ms;
    if (items) *items = s.items;
    return 0;
}

int iris_device_kernel_stats_largest(iris_device_t *d, const char *kernel, uint64_t *items, double *ms) {
    IRIS_KEEP_DEVICE();
    ARG(d && kernel, "NULL argument");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    fold_done(d);
    auto it = d->stats.find(kernel);
    KStat s = it == d->stats.end() ? KStat{} : it->second;
    if (items) *items = s.max_items;
    if (ms) *ms = s.max_ms;
    return 0;
}

int iris_device_reset_stats(iris_device_t *d) {
    IRIS_KEEP_DEVICE();
    ARG(d, "device is NULL");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    d->stats.clear();
    d->ra_launches = d->ra_records = d->ra_window_max = 0;
    for (uint64_t &r : d->share_regs) r = 0;
    if (d->share_count) {
        CHK(set_device(d));
        HIPCHK(hipMemsetAsync(d->share_count, 0, kShareKinds * sizeof(*d->share_count), d->stream));
    }
    return 0;
}

int iris_device_alloc(iris_device_t *d, size_t bytes, void **ptr) {
    IRIS_KEEP_DEVICE();
    ARG(d && ptr, "NULL argument");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    return dev_malloc(d, ptr, std::max<size_t>(bytes, 1), "iris_device_alloc");
}

int iris_device_free(iris_device_t *d, void *ptr) {
    IRIS_KEEP_DEVICE();
    ARG(d, "device is NULL");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    if (ptr) HIPCHK(hipFree(ptr));
    return 0;
}

int iris_memcpy_d2h(iris_device_t *d, void *host, const void *device, size_t bytes) {
    IRIS_KEEP_DEVICE();
    ARG(d && (bytes == 0 || (host && device)), "NULL argument");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    HIPCHK(hipMemcpyAsync(host, device, bytes, hipMemcpyDeviceToHost, d->stream));
    return sync(d);
}

int iris_memcpy_h2d(iris_device_t *d, void *device, const void *host, size_t bytes) {
    IRIS_KEEP_DEVICE();
    ARG(d && (bytes == 0 || (host && device)), "NULL argument");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    HIPCHK(hipMemcpyAsync(device, host, bytes, hipMemcpyHostToDevice, d->stream));
    return sync(d);
}

// ------------------------------------------------------------------ databases

int iris_db_create(iris_device_t *d, int kind, uint64_t capacity, iris_db_t **out) {
    return iris_db_create_ex(d, kind, capacity, IRIS_LAYOUT_DEFAULT, out);
}

int iris_db_create_ex(iris_device_t *d, int kind, uint64_t capacity, int layout, iris_db_t **out) {
    IRIS_KEEP_DEVICE();
    ARG(d && out, "NULL argument");
    CHK(check_kind(kind));
    if (layout == IRIS_LAYOUT_DEFAULT) layout = IRIS_LAYOUT_TILES;
    ARG(layout == IRIS_LAYOUT_LANES || layout == IRIS_LAYOUT_TILES, "unknown layout");
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    iris_db *db = new (std::nothrow) iris_db();
    if (db) db->version = next_db_version();
    if (!db) return fail(IRIS_E_NOMEM, "out of host memory");
    db_written(db);
    db->dev = d;
    db->k = kind_info(kind, layout);
    const uint64_t blocks = std::max<uint64_t>(1, capacity / db->k.block + (capacity % db->k.block != 0));
    size_t bytes = 0;
    if (__builtin_mul_overflow(blocks, (uint64_t)block_bytes(db->k), &bytes)) {
        delete db;
        return fail(IRIS_E_NOMEM, "database capacity overflows the address space");
    }
    db->cap = capacity == 0 ? 0 : blocks * db->k.block;
    // the caller's database before cached file copies (evicted least recently used first)
    if (dev_malloc(d, &db->data, bytes, "database") != 0) {
        delete db;
        return IRIS_E_NOMEM;
    }
    // zeroed padding records: a zero mask gives den = 0, i.e. "no candidate"
    hipError_t e = hipMemsetAsync(db->data, 0, bytes, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) {
        (void)hipFree(db->data);
        delete db;
        return fail(IRIS_E_HIP, std::string("memset database: ") + hipGetErrorString(e));
    }
    device_retain(d);
    *out = db;
    return 0;
}

int iris_db_layout(const iris_db_t *db, int *layout) {
    ARG(db && layout, "NULL argument");
    *layout = db->k.layout;
    return 0;
}

int iris_db_destroy(iris_db_t *db) {
    IRIS_KEEP_DEVICE();
    if (!db) return 0;
    iris_device *d = db->dev;
    {
        std::lock_guard<std::recursive_mutex> g(d->mu);
        (void)hipSetDevice(d->ordinal);
        (void)hipStreamSynchronize(d->stream);
        side_sync(d);  // a read-ahead kernel may still read it
        db_detach(db);
        if (db->data) (void)hipFree(db->data);
    }
    delete db;
    device_release(d);
    return 0;
}

int iris_db_len(const iris_db_t *db, uint64_t *len) {
    ARG(db && len, "NULL argument");
    *len = db->len;
    return 0;
}

int iris_db_capacity(const iris_db_t *db, uint64_t *cap) {
    ARG(db && cap, "NULL argument");
    *cap = db->cap;
    return 0;
}

int iris_db_kind(const iris_db_t *db, int *kind) {
    ARG(db && kind, "NULL argument");
    *kind = db->k.kind;
    return 0;
}

int iris_db_append(iris_db_t *db, const void *records, uint64_t n) {
    IRIS_KEEP_DEVICE();
    ARG(db, "database is NULL");
    std::lock_guard<std::recursive_mutex> g(db->dev->mu);
    CHK(set_device(db->dev));
    return db_write_locked(db, db->len, records, n);
}

int iris_db_write(iris_db_t *db, uint64_t index, const void *records, uint64_t n) {
    IRIS_KEEP_DEVICE();
    ARG(db, "database is NULL");
    std::lock_guard<std::recursive_mutex> g(db->dev->mu);
    CHK(set_device(db->dev));
    return db_write_locked(db, index, records, n);
}

int iris_db_read(const iris_db_t *db, uint64_t first, uint64_t n, void *records) {
    IRIS_KEEP_DEVICE();
    ARG(db, "database is NULL");
    iris_device *d = db->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    CHK(range_ok(db, first, n));
    if (n == 0) return 0;
    ARG(records, "records is NULL");
    const KindInfo &k = db->k;
    if ((size_t)n * k.rec_bytes >= kUploadTuneMin && ensure_upin(d) == 0) {
        // the upload slots run backwards: slot c is unpacked and copied into pinned buffer c % 2 by the
        // device while the helper threads copy slot c - 1 into the caller's array
        const uint64_t ch = std::max<uint64_t>(64, kUploadSlot / k.rec_bytes / 64 * 64);
        const size_t slot = (size_t)ch * k.rec_bytes;
        CHK(ensure(d, d->staging, kUploadSlots * slot));
        const uint64_t chunks = (n + ch - 1) / ch;
        int rc = 0;
        auto enqueue = [&](uint64_t c) -> int {
            const int b = (int)(c % kUploadSlots);
            const uint64_t a = c * ch, m = std::min<uint64_t>(ch, n - a);
            void *stage = (char *)d->staging.p + (size_t)b * slot;
            CHK(timed(d, "unpack", m, [&] { return launch_unpack(d->stream, k, db->data, stage, first + a, m); }));
            HIPCHK(hipMemcpyAsync(d->upin[b], stage, (size_t)m * k.rec_bytes, hipMemcpyDeviceToHost, d->stream));
            HIPCHK(hipEventRecord(d->upin_ev[b], d->stream));
            return 0;
        };
        rc = enqueue(0);
        for (uint64_t c = 0; c < chunks && rc == 0; ++c) {
            // pinned buffer (c + 1) % slots was last read by the (synchronous) copy-out of slot c + 1 - slots
            if (c + 1 < chunks) rc = enqueue(c + 1);
            if (rc == 0 && hipEventSynchronize(d->upin_ev[c % kUploadSlots]) != hipSuccess) rc = fail(IRIS_E_HIP, "hipEventSynchronize");
            if (rc == 0) {
                const uint64_t a = c * ch, m = std::min<uint64_t>(ch, n - a);
                parallel_copy((char *)records + a * k.rec_bytes, d->upin[c % kUploadSlots], (size_t)m * k.rec_bytes, d->ordinal);
            }
        }
        const int rs = sync(d);
        CHK(rc);
        return rs;
    }
    const uint64_t ch = chunk_records(k);
    CHK(ensure(d, d->staging, std::min<uint64_t>(n, ch) * k.rec_bytes));
    for (uint64_t done = 0; done < n; done += ch) {
        const uint64_t m = std::min<uint64_t>(ch, n - done);
        CHK(timed(d, "unpack", m, [&] { return launch_unpack(d->stream, k, db->data, d->staging.p, first + done, m); }));
        HIPCHK(hipMemcpyAsync((char *)records + done * k.rec_bytes, d->staging.p, m * k.rec_bytes,
                              hipMemcpyDeviceToHost, d->stream));
        CHK(sync(d));
    }
    return 0;
}

int iris_db_generate(iris_db_t *db, uint64_t n, uint64_t seed, uint64_t global_index0) {
    IRIS_KEEP_DEVICE();
    ARG(db, "database is NULL");
    iris_device *d = db->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    if (n > db->cap - db->len) return fail(IRIS_E_RANGE, "iris_db_generate: database capacity exceeded");
    if (n == 0) return 0;
    db_detach(db);
    CHK(timed(d, "generate", n, [&] { return launch_generate(d->stream, db->k, db->data, db->len, n, seed, global_index0); }));
    CHK(sync(d));
    db->len += n;
    return 0;
}

int iris_db_truncate(iris_db_t *db, uint64_t len) {
    IRIS_KEEP_DEVICE();
    ARG(db, "database is NULL");
    std::lock_guard<std::recursive_mutex> g(db->dev->mu);
    if (len > db->len) return fail(IRIS_E_RANGE, "iris_db_truncate: len beyond the current length");
    if (len != db->len) db_detach(db);
    db->len = len;
    return 0;
}

int iris_db_attach_host(iris_db_t *db, const void *host, uint64_t n, int upload) {
    IRIS_KEEP_DEVICE();
    ARG(db && (host || n == 0), "NULL argument");
    iris_device *d = db->dev;
    std::lock_guard<std::recursive_mutex> g(d->mu);
    CHK(set_device(d));
    db_detach(db);
    const size_t rb = db->k.rec_bytes;
    if (upload) {
        ARG(db->len == 0, "iris_db_attach_host(upload): the database must be empty");
        CHK(db_write_locked(db, 0, host, n));
    } else {
        ARG(db->len == n, "iris_db_attach_host: the database must hold exactly the n records of the host array");
        // the caller's promise (e.g. the same file loaded with iris_db_load_file) is spot-checked
        const uint64_t probe[3] = {0, n / 2, n ? n - 1 : 0};
        std::vector<char> rec(rb);
        for (int i = 0; i < 3 && n; ++i) {
            CHK(iris_db_read(db, probe[i], 1, rec.data()));
            if (memcmp(rec.data(), (const char *)host + probe[i] * rb, rb) != 0)
                return fail(IRIS_E_ARG, "iris_db_attach_host: record " + std::to_string(probe[i]) +
                                            " of the database differs from the host array");
        }
    }
    if (n == 0) return 0;
    db->host_base = (uintptr_t)host;
    db->host_n = n;
    db->version = next_db_version();
    d->attached.push_back(db);
    return 0;
}

int iris_db_detach_host(iris_db_t *db) {
    IRIS_KEEP_DEVICE();
    ARG(db, "database is NULL");
    std::lock_guard<std::recursive_mutex> g(db->dev->mu);
    db_detach(db);
    return 0;
}

int iris_db_clear(iris_db_t *db) {
    IRIS_KEEP_DEVICE();
    ARG(db, "database is NULL");
    std::lock_guard<std::recursive_mutex> g(db->dev->mu);
    CHK(set_device(db->dev));
    db_detach(db);
    const size_t bytes = std::max<uint64_t>(1, db->cap / db->k.block) * block_bytes(db->k);
    HIPCHK(hipMemsetAsync(db->data, 0, bytes, db->dev->stream));
    CHK(sync(db->dev));
    db->len = 0;
    return 0;
}

// ------------------------------------------------------------------ host helpers

int iris_bits_rotated(const uint64_t in[IRIS_LIMBS], int32_t amount, uint64_t out[IRIS_LIMBS]) {
    ARG(in && out, "NULL argument");
    bits_rotated(in, amount, out);
    return 0;
}

int iris_encoded_rotated(const uint16_t in[IRIS_BITS], int32_t amount, uint16_t out[IRIS_BITS]) {
    ARG(in && out, "NULL argument");
    if (in == out) {
        std::vector<uint16_t> tmp(in, in + IRIS_BITS);
        encoded_rotated(tmp.data(), amount, out);
    } else {
        encoded_rotated(in, amount, out);
    }
    return 0;
}

int iris_encode(const iris_template_t *t, uint16_t out[IRIS_BITS]) {
    ARG(t && out, "NULL argument");
    encode_template(t, out);
    return 0;
}

int iris_decode_distance(const uint16_t distances[IRIS_ROTATIONS], const uint16_t denominators[IRIS_ROTATIONS],
                         double *out) {
    ARG(distances && denominators && out, "NULL argument");
    double acc = INFINITY;
    for (int k = 0; k < kRot; ++k) {
        const uint16_t n = distances[k], dd = denominators[k];
        const uint16_t uneq = (uint16_t)((uint16_t)(dd - n) / 2);  // src/lib.rs:104
        acc = rust_f64_min(acc, (double)uneq / (double)dd);        // src/lib.rs:105-106
    }
    *out = acc;
    return 0;
}

int iris_match_merge(const iris_match_t *recs, uint64_t count, iris_match_t *out) {
    ARG(out && (count == 0 || recs), "NULL argument");
    iris_match_t best;
    match_from(Partial{}, false, 0, &best);
    for (uint64_t i = 0; i < count; ++i) {
        const iris_match_t &c = recs[i];
        if (c.den == 0 || c.index == UINT64_MAX) continue;
        bool take = best.den == 0;
        if (!take) {
            const uint64_t l = (uint64_t)c.num * best.den, r = (uint64_t)best.num * c.den;
            take = l < r || (l == r && c.index < best.index);
        }
        if (take) best = c;
    }
    *out = best;
    return 0;
}

// iris_match_merge's top-k counterpart, host only: the k first records of the search order
// (exact fraction, then lowest index) among `count` records that carry global indices.
int iris_topk_merge(const iris_match_t *recs, uint64_t nrecords, uint32_t k, iris_match_t *out, uint32_t *count) {
    ARG(k >= 1 && k <= IRIS_TOPK_MAX, "k must be 1..IRIS_TOPK_MAX (64)");
    ARG(out, "out is NULL");
    ARG(count, "count is NULL");
    ARG(nrecords == 0 || recs, "records is NULL");
    std::vector<const iris_match_t *> v;
    try {
        v.reserve(nrecords);
    } catch (const std::bad_alloc &) {
        return fail(IRIS_E_NOMEM, "out of host memory");
    }
    for (uint64_t i = 0; i < nrecords; ++i)
        if (recs[i].den != 0 && recs[i].index != UINT64_MAX) v.push_back(&recs[i]);
    std::sort(v.begin(), v.end(), [](const iris_match_t *a, const iris_match_t *b) { return a->index < b->index; });
    for (size_t i = 1; i < v.size(); ++i) ARG(v[i]->index != v[i - 1]->index, "two records carry the same index");
    const size_t take = std::min<size_t>(k, v.size());
    std::partial_sort(v.begin(), v.begin() + take, v.end(), [](const iris_match_t *a, const iris_match_t *b) {
        const uint64_t l = (uint64_t)a->num * b->den, r = (uint64_t)b->num * a->den;
        return l != r ? l < r : a->index < b->index;
    });
    for (size_t i = 0; i < take; ++i) out[i] = *v[i];
    *count = (uint32_t)take;
    return 0;
}

}  // extern "C"
