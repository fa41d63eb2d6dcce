"""Measurement: threshold matching (iris_template_matches, iris_resolver_matches_masks) against the
search it is the sibling of, against today's alternative, and at its worst case.

On one device, in one process, on generated TILES databases far past the Infinity Cache (10M records
by default):

  1. cost over the search
     templates  10M random templates (seed 42) with 8 planted near-copies of the query, threshold
                0.375 (only the planted records match): iris_template_matches against
                iris_template_search.
     resolve    the inputs of `bench.py --workload resolve-masks` (masks seed 20251015, query mask
                seed 20251016, 3 parts of uniform u16 rows from default_rng(20251015)), the threshold
                taken from one dist_out_device run so that fewer than 0.01 % of the records match:
                iris_resolver_matches_masks against iris_resolver_search_masks.
     Each pair is timed interleaved (a, b, a, b, ...) after a warm-up of both, with a host clock
     around the blocking calls; then each side's launches are timed with HIP events in a pass of
     its own (kernel_stats: "template_match" against "template_search" + "reduce", "masks_match"
     against "masks_resolve" + "reduce").  The table gives medians, the ratio and each side's
     spread ((max - min) / median).  Condition: matches <= 1.03 x search, on the device times.
  3. worst case (reported, not bounded): threshold = +inf over the templates -- every record is
     appended, the pass runs twice (the first buffer is sized from cap) and the host sorts 10M
     records.  Device time of the passes from kernel_stats; the remainder of the call (the copy
     back of 24 B per match, the sort by index, the conversion) from the host clock; a count-only
     call (cap = 0: one pass, nothing copied or sorted) beside it.
  4. today's alternative: iris_template_search with dist_out_device, the copy back of the n
     doubles and a numpy filter at the same threshold.

Before anything is timed the lists are checked: the planted indices exactly, the resolver list
against a numpy filter of the dist_out_device distances, and the +inf count against the number of
finite distances.  No number is printed if they differ.

(Measurement 2 of the feature's plan -- plain bench.py at the parent commit and at the branch,
alternating -- is a job of its own, not part of this tool.)

usage: python tools/bench_matches.py [n=10000000] [reps=15]"""
import ctypes
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
INF = float("inf")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def spread(ts):
    return (max(ts) - min(ts)) / float(np.median(ts))


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
    """Median-free device time per call: the sum of the named launches' HIP-event times over reps calls."""
    dev.reset_stats()
    dev.set_profiling(True)
    for _ in range(reps):
        fn()
    dev.set_profiling(False)
    stats = {k: dev.kernel_stats(k) for k in names}
    return sum(s[1] for s in stats.values()) / reps, {k: s[0] / reps for k, s in stats.items()}


def compare(dev, title, n, a, b, a_names, b_names, reps):
    """a = the matches call, b = the search call."""
    for _ in range(3):
        a()
        b()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a))
        tb.append(timed(b))
    da, la = device_ms(dev, a, a_names, reps)
    db_, lb = device_ms(dev, b, b_names, reps)
    ma, mb = float(np.median(ta)) * 1e3, float(np.median(tb)) * 1e3
    print(f"\n1. {title}: n = {n}, {reps} interleaved repetitions")
    print("                 host ms (median)  spread   device ms / call   launches / call")
    print(f"   matches       {ma:10.4f}      {spread(ta):6.1%}   {da:10.4f}         {la}")
    print(f"   search        {mb:10.4f}      {spread(tb):6.1%}   {db_:10.4f}         {lb}")
    print(f"   ratio matches / search: host {ma / mb:.4f}, device {da / db_:.4f}")
    print(f"   condition (matches <= 1.03 x search, device times): {'holds' if da <= 1.03 * db_ else 'FAILS'}"
          f"; on host times: {'holds' if ma <= 1.03 * mb else 'FAILS'}")
    return ma, mb


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    reps = max(reps, 10)
    dev = ih.Device(0)
    lib = ih.load_library()
    print(f"library: {lib.iris_version().decode()}")

    # ---------------------------------------------------------------- templates
    tdb = ih.Database(dev, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES)
    tdb.generate(n, 42)
    query = gen_records(dev, ih.KIND_TEMPLATES, 1, 43)[0]
    sites = sorted({(n // 9) * (k + 1) + 17 * k for k in range(8)})
    for k, s in enumerate(sites):
        tdb.write(s, planted_record(query, 4 * k - 14, 0x00FF00FF00FF00FF >> k)[None, :])
    eng = ih.TemplateEngine(dev, query)
    thr = 0.375
    got, count = eng.matches(tdb, thr)
    if count != len(sites) or [m.index for m in got] != sites:
        print(f"template matches {[m.index for m in got]} differ from the planted {sites}: no numbers")
        return 1
    dist_ptr = dev.alloc(n * 8)
    dist = np.empty(n, np.float64)
    eng.search(tdb, dist_out_device=dist_ptr)
    dev.d2h(dist, dist_ptr)
    if list(np.flatnonzero(dist < thr)) != sites:
        print("the distances' filter differs from the planted sites: no numbers")
        return 1
    finite = int(np.isfinite(dist).sum())
    cnt = ctypes.c_uint64()

    def count_only(t):
        rc = lib.iris_template_matches(eng.handle, tdb.handle, 0, n, 0, t, None, 0, ctypes.byref(cnt))
        assert rc == 0, rc
        return cnt.value

    if count_only(INF) != finite:
        print(f"+inf count {cnt.value} differs from the {finite} finite distances: no numbers")
        return 1
    print(f"results: the {len(sites)} planted records at threshold {thr}; {finite} of {n} at +inf")

    m_ms, s_ms = compare(dev, "templates, iris_template_matches against iris_template_search", n,
                         lambda: eng.matches(tdb, thr), lambda: eng.search(tdb),
                         ("template_match",), ("template_search", "reduce"), reps)

    # 4. today's alternative
    def alternative():
        eng.search(tdb, dist_out_device=dist_ptr)
        dev.d2h(dist, dist_ptr)
        return np.flatnonzero(dist < thr)

    for _ in range(2):
        alternative()
    talt = [timed(alternative) for _ in range(reps)]
    alt = float(np.median(talt)) * 1e3
    print(f"\n4. today's alternative (search with dist_out_device + {n * 8 / 1e6:.0f} MB copy back + numpy filter): "
          f"{alt:.3f} ms (spread {spread(talt):.1%}) = {alt / m_ms:.1f} x iris_template_matches ({m_ms:.3f} ms)")

    # 3. worst case
    out = (ih.Match * n)()

    def dense():
        rc = lib.iris_template_matches(eng.handle, tdb.handle, 0, n, 0, INF, out, n, ctypes.byref(cnt))
        assert rc == 0 and cnt.value == finite, (rc, cnt.value)

    dense()  # grows the buffer: these calls run one pass; the two-pass call is timed below on a fresh device
    small = (ih.Match * 10)()
    tdense = [timed(dense) for _ in range(3)]
    kd, ld = device_ms(dev, dense, ("template_match",), 3)
    tcount = [timed(lambda: count_only(INF)) for _ in range(3)]
    kc, lc = device_ms(dev, lambda: count_only(INF), ("template_match",), 3)
    wall = float(np.median(tdense)) * 1e3
    print(f"\n3. worst case, threshold = +inf ({finite} matches, {finite * 24 / 1e6:.0f} MB of records):")
    print(f"   full list, buffer already grown: {wall:.1f} ms per call; device passes {kd:.3f} ms "
          f"({ld['template_match']:.0f} launch per call); copy back + sort by index + conversion {wall - kd:.1f} ms")
    print(f"   count only (cap = 0, one pass, nothing copied): {float(np.median(tcount)) * 1e3:.3f} ms per call, "
          f"device {kc:.3f} ms")
    eng.close()
    dev.free(dist_ptr)
    del out
    tdb.close()

    # a fresh device handle starts from an empty match buffer: the forced second pass, timed once
    dev2 = ih.Device(0)
    tdb2 = ih.Database(dev2, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES)
    tdb2.generate(n, 42)
    eng2 = ih.TemplateEngine(dev2, query)
    eng2.matches(tdb2, thr)
    dev2.reset_stats()
    dev2.set_profiling(True)
    t0 = time.perf_counter()
    rc = lib.iris_template_matches(eng2.handle, tdb2.handle, 0, n, 0, INF, small, 10, ctypes.byref(cnt))
    t2 = (time.perf_counter() - t0) * 1e3
    dev2.set_profiling(False)
    launches, kms, _ = dev2.kernel_stats("template_match")
    assert rc == 0
    print(f"   first dense call on a device (cap = 10; buffer grown to the count, second pass, partial sort): "
          f"{t2:.1f} ms, {launches} passes, device {kms:.3f} ms")
    eng2.close()
    tdb2.close()
    dev2.close()

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
    dist_ptr = dev.alloc(n * 8)
    dist = np.empty(n, np.float64)
    me.resolve(mdb, ptrs, dist_out_device=dist_ptr)
    dev.d2h(dist, dist_ptr)
    # Uniform random rows decode to distance 0 in about 2^-15 of the (record, rotation) cells, so ~0.1 %
    # of these records sit at exactly 0: the largest threshold under which fewer than 0.01 % match is
    # the distance at rank n / 20000 of the sorted list, which here is 0.0 itself (nothing matches).
    # The next f64 above it is timed too: every zero-distance record matches, a list ten times longer
    # than the bound asks for.
    k = max(1, n // 20000)  # 0.005 % of the records
    rthr = float(np.partition(dist, k)[k])
    for label, t in (("rank n / 20000 of the distances", rthr), ("the next f64 above it", float(np.nextafter(rthr, INF)))):
        want = np.flatnonzero(dist < t)
        got, count = me.matches(mdb, ptrs, t)
        if count != len(want) or [m.index for m in got] != list(want):
            print("resolver matches differ from the filter of the dist_out_device distances: no numbers")
            return 1
        print(f"\nresults: resolve-masks threshold {t!r} ({label}): {count} of {n} records ({count / n:.4%}) match, "
              "equal to the filter of the search's own distances")
        compare(dev, f"resolve-masks at {t!r}, iris_resolver_matches_masks against iris_resolver_search_masks", n,
                lambda: me.matches(mdb, ptrs, t), lambda: me.resolve(mdb, ptrs),
                ("masks_match",), ("masks_resolve", "reduce"), reps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
