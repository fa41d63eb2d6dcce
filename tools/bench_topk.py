"""Measurement: top-k (iris_template_topk, iris_resolver_topk_masks, iris_resolver_topk) against the
search it is the sibling of, against today's alternative, and at its adversarial order.

On one device, in one process, on generated TILES databases far past the Infinity Cache (10M records
by default), for k in {1, 16, 64}:

  1. templates  10M random templates (seed 42) with 8 planted near-copies of the query:
                (a) iris_template_topk, (b) iris_template_search, (c) today's alternative --
                iris_template_search with dist_out_device, the copy back of the n doubles and
                np.argpartition + a sort of the k on the host.
     resolve    the inputs of `bench.py --workload resolve-masks` (masks seed 20251015, query mask
                seed 20251016, 3 parts of uniform u16 rows from default_rng(20251015)):
                (a) iris_resolver_topk_masks, (b) iris_resolver_search_masks.
     The calls of a group are timed interleaved with their order rotated every repetition, after a
     warm-up of each, with a host clock around the blocking calls; then each side's launches are
     timed with HIP events in a pass of its own (kernel_stats: "template_topk" + "topk_merge"
     against "template_search" + "reduce"; "masks_topk" + "topk_merge" against "masks_resolve" +
     "reduce").  The table gives medians, each call's spread ((max - min) / median), the ratio
     (a)/(b) on host and device times with the streaming kernel and the merge launches apart, and
     whether (a) beats (c) by more than (c)'s own spread (required).
  2. adversarial order (reported): resolver rows whose distance strictly decreases with the index --
     every row beats all before it -- through iris_resolver_topk (den = 12800 rows) and through
     iris_resolver_topk_masks (all-ones masks), beside the same rows in ascending order.
  3. a 20 000-record template call against the search of the same range (reported).

Before anything is timed the lists are checked: the planted indices lead the template list, every
list is sorted by (distance, index), a prefix of the k = 64 list, and its head is the search's
result.  No number is printed if they differ.

(Plain bench.py at the parent commit and at the branch, alternating, is a job of its own.)

usage: python tools/bench_topk.py [n=10000000] [reps=15]"""
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402

ROT = 31
PARTS = 3
BENCH_SEED = 20251015  # bench.py's SEED
KS = (1, 16, 64)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def spread(ts):
    return (max(ts) - min(ts)) / float(np.median(ts))


def med(ts):
    return float(np.median(ts)) * 1e3


def gen_records(dev, kind, n, seed):
    with ih.Database(dev, kind, max(n, 1)) as g:
        g.generate(n, seed)
        return g.read(0, n)


def planted_record(query, rotation, flips):
    p = ih.Bits(query[:200]).rotated(rotation).limbs.copy()
    m = ih.Bits(query[200:]).rotated(rotation).limbs
    p[7] ^= np.uint64(flips)
    return np.concatenate([p, m])


def device_ms(dev, fn, names, reps):
    """Device time per call of each named launch family: HIP-event times summed over reps calls."""
    dev.reset_stats()
    dev.set_profiling(True)
    for _ in range(reps):
        fn()
    dev.set_profiling(False)
    return {k: dev.kernel_stats(k)[1] / reps for k in names}


def interleaved(calls, reps):
    """calls: {label: fn} -> {label: [seconds]}; the order is rotated every repetition."""
    labels = list(calls)
    for _ in range(3):
        for l in labels:
            calls[l]()
    ts = {l: [] for l in labels}
    for r in range(reps):
        for i in range(len(labels)):
            l = labels[(i + r) % len(labels)]
            ts[l].append(timed(calls[l]))
    return ts


def listed_ok(lst, k, full, best):
    key = [(m.distance, m.index) for m in lst]
    return (len(lst) == k and key == sorted(key) and [bytes(m) for m in lst] == [bytes(m) for m in full[:k]]
            and bytes(lst[0]) == bytes(best))


def report(title, n, k, ts, dev_a, dev_b, stream_a, stream_b, alt=None):
    a, b = med(ts["topk"]), med(ts["search"])
    da, db_ = sum(dev_a.values()), sum(dev_b.values())
    print(f"\n{title}: n = {n}, k = {k}, {len(ts['topk'])} interleaved repetitions")
    print(f"   (a) top-k   host {a:9.4f} ms  spread {spread(ts['topk']):6.1%}   device {da:9.4f} ms  {dev_a}")
    print(f"   (b) search  host {b:9.4f} ms  spread {spread(ts['search']):6.1%}   device {db_:9.4f} ms  {dev_b}")
    print(f"   (a)/(b): host {a / b:.4f}, device {da / db_:.4f}; streaming kernel {dev_a[stream_a] / dev_b[stream_b]:.4f}, "
          f"merge launches {dev_a['topk_merge']:.4f} ms against the reduce's {dev_b['reduce']:.4f} ms")
    if alt is not None:
        c, sc = med(ts[alt]), spread(ts[alt])
        ok = a < c * (1.0 - sc)
        print(f"   (c) search + dist_out_device + {n * 8 / 1e6:.0f} MB copy back + argpartition: host {c:9.4f} ms  spread {sc:6.1%}"
              f"  = {c / a:.2f} x (a); required (a) < (c) by more than (c)'s spread: {'holds' if ok else 'FAILS'}")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 15, 15)
    dev = ih.Device(0)
    print(f"library: {ih.load_library().iris_version().decode()}")

    # ---------------------------------------------------------------- templates
    tdb = ih.Database(dev, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES)
    tdb.generate(n, 42)
    query = gen_records(dev, ih.KIND_TEMPLATES, 1, 43)[0]
    sites = sorted({(n // 9) * (k + 1) + 17 * k for k in range(8)})
    for k, s in enumerate(sites):
        tdb.write(s, planted_record(query, 4 * k - 14, 0x00FF00FF00FF00FF >> k)[None, :])
    eng = ih.TemplateEngine(dev, query)
    full = eng.topk(tdb, 64)
    best = eng.search(tdb)
    if sorted(m.index for m in full[:8]) != sites or not all(listed_ok(eng.topk(tdb, k), k, full, best) for k in KS):
        print("template top-k lists differ from the planted sites / the search: no numbers")
        return 1
    dist_ptr = dev.alloc(n * 8)
    dist = np.empty(n, np.float64)
    eng.search(tdb, dist_out_device=dist_ptr)
    dev.d2h(dist, dist_ptr)
    if [m.index for m in full] != list(np.lexsort((np.arange(n), dist))[:64]):
        print("the k = 64 list differs from the sort of the search's own distances: no numbers")
        return 1
    print(f"results: the {len(sites)} planted records lead every list; the k = 64 list equals the sort of the distances")

    for k in KS:
        def alternative():
            eng.search(tdb, dist_out_device=dist_ptr)
            dev.d2h(dist, dist_ptr)
            part = np.argpartition(dist, k)[:k] if k < n else np.arange(n)
            return part[np.lexsort((part, dist[part]))]

        ts = interleaved({"topk": lambda: eng.topk(tdb, k), "search": lambda: eng.search(tdb), "alt": alternative}, reps)
        dev_a = device_ms(dev, lambda: eng.topk(tdb, k), ("template_topk", "topk_merge"), reps)
        dev_b = device_ms(dev, lambda: eng.search(tdb), ("template_search", "reduce"), reps)
        report("1. templates, iris_template_topk against iris_template_search", n, k, ts, dev_a, dev_b,
               "template_topk", "template_search", alt="alt")

    # 3. a 20 000-record call
    small = min(20000, n)
    for k in KS:
        ts = interleaved({"topk": lambda: eng.topk(tdb, k, n=small), "search": lambda: eng.search(tdb, n=small)}, 4 * reps)
        print(f"\n3. {small} records, k = {k}: top-k {med(ts['topk']) * 1e3:.1f} us (spread {spread(ts['topk']):.1%}), "
              f"search {med(ts['search']) * 1e3:.1f} us (spread {spread(ts['search']):.1%})")
    eng.close()
    dev.free(dist_ptr)
    tdb.close()

    # ---------------------------------------------------------------- resolve-masks
    rng = np.random.default_rng(BENCH_SEED)
    shares = rng.integers(0, 65536, (PARTS, n, ROT), dtype=np.uint16)
    ptrs = []
    for p in range(PARTS):
        ptrs.append(dev.alloc(n * ROT * 2))
        dev.h2d(ptrs[p], shares[p])
    del shares
    mdb = ih.Database(dev, ih.KIND_MASKS, n, ih.LAYOUT_TILES)
    mdb.generate(n, BENCH_SEED)
    qmask = gen_records(dev, ih.KIND_MASKS, 1, BENCH_SEED + 1)[0]
    me = ih.MasksEngine(dev, qmask)
    full = me.topk(mdb, ptrs, 64)
    best = me.resolve(mdb, ptrs)
    if not all(listed_ok(me.topk(mdb, ptrs, k), k, full, best) for k in KS):
        print("resolver top-k lists are not sorted prefixes led by the search's result: no numbers")
        return 1
    for k in KS:
        ts = interleaved({"topk": lambda: me.topk(mdb, ptrs, k), "search": lambda: me.resolve(mdb, ptrs)}, reps)
        dev_a = device_ms(dev, lambda: me.topk(mdb, ptrs, k), ("masks_topk", "topk_merge"), reps)
        dev_b = device_ms(dev, lambda: me.resolve(mdb, ptrs), ("masks_resolve", "reduce"), reps)
        report("1. resolve-masks, iris_resolver_topk_masks against iris_resolver_search_masks", n, k, ts, dev_a, dev_b,
               "masks_topk", "masks_resolve")
    me.close()
    mdb.close()

    # ---------------------------------------------------------------- 2. adversarial order
    # distance u / 12800 with u strictly monotonic in the row: 12800 distinct values at most, so the
    # rows come in runs of ceil(n / 6400) equal distances; within a run the lower index is better, so
    # in the descending order the first row of every run inserts (and in a list of k, k runs' worth)
    run = -(-n // 6400)
    ones = np.full(200, ~np.uint64(0))
    odb = ih.Database(dev, ih.KIND_MASKS, n, ih.LAYOUT_TILES)
    chunk = 1 << 18
    for lo in range(0, n, chunk):
        odb.append(np.tile(ones, (min(chunk, n - lo), 1)))
    oe = ih.MasksEngine(dev, ones)
    den_ptr = dev.alloc(n * ROT * 2)
    dev.h2d(den_ptr, np.full((n, ROT), 12800, np.uint16))
    for label, u in (("descending (every run's first row inserts)", 6400 - np.arange(n) // run),
                     ("ascending", 1 + np.arange(n) // run)):
        total = ((12800 - 2 * u) & 0xFFFF).astype(np.uint16)
        dev.h2d(ptrs[0], np.repeat(total[:, None], ROT, axis=1))
        for k in KS:
            tp = [timed(lambda: ih.resolver_topk(dev, ptrs[:1], den_ptr, n, k)) for _ in range(reps)]
            tf = [timed(lambda: oe.topk(odb, ptrs[:1], k)) for _ in range(reps)]
            ts_ = [timed(lambda: oe.resolve(odb, ptrs[:1])) for _ in range(reps)]
            print(f"\n2. adversarial order, {label}, k = {k}: iris_resolver_topk {med(tp):.3f} ms (spread {spread(tp):.1%}); "
                  f"iris_resolver_topk_masks {med(tf):.3f} ms (spread {spread(tf):.1%}) against its search "
                  f"{med(ts_):.3f} ms (spread {spread(ts_):.1%})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
