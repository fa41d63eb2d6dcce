// iris_pending.hpp — the life of a pending handle, from the submission of
// iris_template_search_async, iris_template_matches_async, iris_template_topk_async or
// iris_template_report_async to its wait: what a handle owns, and the one copy of every step the
// four submit / wait pairs share.
//
// A submission runs, under the device lock: pending_new; for an empty range pending_publish at once
// (such a handle owns no event and no buffers); else its slot or buffers (take_result_slot,
// bufs_take), pending_arm, the pass on the device stream, then between pending_side_begin and
// pending_side_end what follows the pass on the side stream (a search: search_enqueue orders its own
// reduce there and records the event); on any failure pending_abandon, else pending_publish.
// A wait runs pending_claim, its own argument checks (an error there still consumes the handle),
// pending_await, and pending_retire around whatever reads the buffers.
#pragma once
#include <new>

#include "iris_handles.hpp"

// iris_template_matches_async's handle extends it (iris_pending_matches, iris_api_select.hip), as does
// iris_template_topk_async's (iris_pending_topk) and iris_template_report_async's
// (iris_pending_report), and `kind` tells each wait which one it was given
struct iris_pending {
    ShareKind kind = kShareSearch;
    iris_device *dev = nullptr;
    hipEvent_t ev = nullptr;        // recorded behind the last side-stream step (null for an empty range)
    uint64_t n = 0, base = 0;       // range size; index_base + first
    iris::Partial *slot = nullptr;  // a search: the pinned host slot the reduce writes
    MatchBufs bufs;                 // a match or top-k pass: its device buffer and pinned slot ...
    std::vector<MatchBufs> *home = nullptr;  // ... and the free list they go back to (null: none taken)
};

namespace iris_api {

// The entry points of a kind of pending, and the prefix of an error of its side-stream steps
struct PendingCalls {
    const char *submit, *wait, *side;
};
inline constexpr PendingCalls kPendingCalls[kShareKinds] = {
    {"iris_template_search_async", "iris_pending_wait", nullptr},
    {"iris_template_matches_async", "iris_pending_matches_wait", "enqueue match copy: "},
    {"iris_template_topk_async", "iris_pending_topk_wait", "enqueue top-k merge: "},
    {"iris_template_report_async", "iris_pending_report_wait", "enqueue report results: "}};

// A free list of (device buffer, pinned slot) pairs: its pinned slots come in blocks of `slots`
// (d->slot_blocks, as take_result_slot's), the device buffers on first use.
struct BufPool {
    std::vector<MatchBufs> iris_device::*list;
    size_t slot_bytes;
    int slots;
    const char *what;  // in the message of a failed hipHostMalloc
    bool fit;          // the pick rule, below
};
inline constexpr BufPool kMatchPool{&iris_device::match_free, kMatchSlotBytes, 64, "match slots", false};
inline constexpr BufPool kTopkPool{&iris_device::topk_free, kTopkSlotBytes, 32, "top-k slots", true};
inline constexpr BufPool kReportPool{&iris_device::report_free, kReportSlotBytes, 16, "report slots", true};

// A pair for p whose device buffer holds dev_bytes (caller holds the device lock)
inline int bufs_take(iris_device *d, const BufPool &pool, size_t dev_bytes, iris_pending *p) {
    std::vector<MatchBufs> &list = d->*pool.list;
    if (list.empty()) {
        void *blk = nullptr;
        hipError_t e = hipHostMalloc(&blk, pool.slots * pool.slot_bytes, hipHostMallocDefault);
        if (e != hipSuccess)
            return fail(IRIS_E_NOMEM, std::string("hipHostMalloc ") + pool.what + ": " + hipGetErrorString(e));
        d->slot_blocks.push_back(blk);
        for (int i = pool.slots - 1; i >= 0; --i) list.push_back(MatchBufs{DevBuf{}, (char *)blk + (size_t)i * pool.slot_bytes});
    }
    size_t pick = list.size() - 1;  // the one returned last: a steady pipeline keeps to a few
    if (pool.fit) {
        // the one returned last whose buffer is large enough, else one that has no buffer yet: growing
        // a buffer frees it, and hipFree waits for the device -- for the very pass that could have
        // hosted this one (a top-k pass's k, and so the size, changes from call to call)
        for (size_t i = list.size(); i-- > 0;)
            if (list[i].dev.cap >= dev_bytes) {
                pick = i;
                break;
            }
        if (list[pick].dev.cap < dev_bytes)
            for (size_t i = list.size(); i-- > 0;)
                if (!list[i].dev.p) {
                    pick = i;
                    break;
                }
    }
    MatchBufs b = list[pick];
    list.erase(list.begin() + pick);
    const int rc = ensure(d, b.dev, dev_bytes);
    if (rc != 0) {
        list.push_back(b);
        return rc;
    }
    p->bufs = b;
    p->home = &list;
    return 0;
}

// What p owns goes back to the device's lists (caller holds the device lock).  drain: whatever was
// enqueued may still write it, so the streams are waited for first.
inline void pending_give(iris_pending *p, bool drain) {
    iris_device *d = p->dev;
    if (drain && (p->home || p->slot)) {
        (void)hipStreamSynchronize(d->stream);
        side_sync(d);
    }
    if (p->home) p->home->push_back(p->bufs);
    if (p->slot) d->free_slots.push_back(p->slot);
    if (p->ev) d->event_pool.push_back(p->ev);
}

template <class T>
int pending_new(iris_device *d, ShareKind kind, uint64_t n, uint64_t base, T **out) {
    T *p = new (std::nothrow) T();
    if (!p) return fail(IRIS_E_NOMEM, "out of host memory");
    p->kind = kind;
    p->dev = d;
    p->n = n;
    p->base = base;
    *out = p;
    return 0;
}

// a non-empty range: the handle's event and the device's side streams
inline int pending_arm(iris_pending *p) {
    p->ev = take_event(p->dev);
    if (!p->ev) return fail(IRIS_E_HIP, "hipEventCreate failed");
    return ensure_aux(p->dev);
}

inline int pending_side_chk(const iris_pending *p, hipError_t err) {
    if (err == hipSuccess) return 0;
    return fail(IRIS_E_HIP, std::string(kPendingCalls[p->kind].side) + hipGetErrorString(err));
}

// Behind the pass, on the side stream (the next pass is not held up): what is enqueued on d->aux
// between the two follows the pass, and the handle's event follows that.
inline int pending_side_begin(const iris_pending *p) {
    CHK(pending_side_chk(p, hipEventRecord(p->ev, p->dev->stream)));
    return pending_side_chk(p, hipStreamWaitEvent(p->dev->aux, p->ev, 0));
}

inline int pending_side_end(const iris_pending *p) { return pending_side_chk(p, hipEventRecord(p->ev, p->dev->aux)); }

// a failed submission: rc, with the handle gone
template <class T>
int pending_abandon(T *p, int rc) {
    pending_give(p, true);
    delete p;
    return rc;
}

template <class T>
int pending_publish(T *p, iris_pending **out) {
    device_retain(p->dev);
    *out = p;
    return 0;
}

// The handle a wait was given, as the kind that wait serves; a refusal leaves the handle alive.
template <class T>
int pending_claim(iris_pending *pending, ShareKind kind, T **out) {
    ARG(pending, "pending is NULL");
    const PendingCalls &c = kPendingCalls[pending->kind];
    ARG(pending->kind == kind, std::string("pending of ") + c.submit + ": " + c.wait + " waits for it");
    *out = static_cast<T *>(pending);
    return 0;
}

// waits for this pass and its side-stream steps only: later enqueued work keeps running
inline hipError_t pending_await(const iris_pending *p) { return p->ev ? hipEventSynchronize(p->ev) : hipSuccess; }

// The end of a wait: err is pending_await's, rc the wait's own argument checks'.  Under the device
// lock, finish() reads the buffers (only if neither failed); then everything goes back to the lists
// -- after a failed event only once nothing can still write it -- and the handle and its hold on the
// device go.  The event's error wins and is reported after the release.
template <class T, class F>
int pending_retire(T *p, hipError_t err, int rc, F &&finish) {
    iris_device *d = p->dev;
    {
        std::lock_guard<std::recursive_mutex> g(d->mu);
        if (rc == 0 && err == hipSuccess) rc = finish();
        pending_give(p, err != hipSuccess);
        fold_done(d);
    }
    delete p;
    device_release(d);
    if (err != hipSuccess) return fail(IRIS_E_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(err));
    return rc;
}

}  // namespace iris_api
