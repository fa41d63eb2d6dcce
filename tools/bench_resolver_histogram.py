"""Measurement: the resolver histograms (iris_resolver_histogram, iris_resolver_histogram_masks,
iris_resolver_batch_histogram_masks) against the searches they are the siblings of, against the
count-only dense match passes they replace, and the two forms of the flush against each other.

On one device, in one process, on tools/bench_masks_batch.py's inputs -- a generated TILES masks
database far past the Infinity Cache (10M records by default), 3 parts of query-major device share
arrays holding a repeated block of uniform random u16 (their decoded distances spread from 0 to far
above 1) -- every table timed interleaved (a, b, c, ..., a, ...) after a warm-up of all, with a host
clock around the blocking calls, then each side's launches with HIP events in a pass of its own
(kernel_stats); tools/bench_histogram.py's table():

  1. fused form, per nbins in {64, 1024}:
       copies   iris_resolver_histogram_masks as shipped ("masks_resolve_hist" + "hist_reduce")
       direct   the same call on a device opened with IRIS_HIST_COPIES=1: every workgroup adds
                straight into the result, on a database of its own with the same records
       search   iris_resolver_search_masks ("masks_resolve" + "reduce")
       dense    iris_resolver_matches_masks, threshold = +inf, cap = 0 ("masks_match")
  2. denominators given, per nbins in {64, 1024}: iris_resolver_histogram ("resolver_hist" +
     "hist_reduce") on both devices against iris_resolver_search ("resolver" + "reduce") and
     iris_resolver_matches(+inf, cap = 0) ("resolver_match"), over the first query's own rows.
  3. batch form, 4 and 16 queries at 1024 bins: iris_resolver_batch_histogram_masks
     ("masks_batch_hist" + "hist_reduce") on both devices against iris_resolver_batch_search_masks,
     iris_resolver_batch_matches_masks(+inf, cap = 0) and nq single-query histogram calls.
Condition, every table: the shipped histogram is not slower than the dense match pass beyond that
pass's spread (host clock), and not slower on the device.

Before anything is timed the histograms are checked against np.bincount of the search's own
dist_out_device distances, binned by the header's rule.  No number is printed if they differ.

usage: python tools/bench_resolver_histogram.py [n=10000000] [reps=15] [max batch=16]"""
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402
from bench_histogram import open_hooked, table, want_hist  # noqa: E402

INF = float("inf")
ROT = 31
PARTS = 3


def verdict(res, hist="copies", dense="dense"):
    h, m = res[hist], res[dense]
    ok = h[1] <= m[1] and h[0] <= m[0] * (1 + m[2])
    print(f"   condition (shipped histogram <= dense match pass: device times, and host within the pass's spread): "
          f"{'holds' if ok else 'FAILS'}")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 15, 5)
    nqm = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    dev = ih.Device(0)
    direct = open_hooked(IRIS_HIST_COPIES=1)
    print(f"library: {ih.load_library().iris_version().decode()}")
    print(f"direct device: hist_copies={direct.config()['hist_copies']}")

    dbs = {}
    for d in (dev, direct):
        dbs[d] = ih.Database(d, ih.KIND_MASKS, n, ih.LAYOUT_TILES)
        dbs[d].generate(n, 7)
    mdb, ddb = dbs[dev], dbs[direct]
    queries = np.random.default_rng(3).integers(0, 2**64, (nqm, ih.LIMBS), dtype=np.uint64)
    slab_bytes = nqm * n * ROT * 2
    ptrs = []
    for p in range(PARTS):  # one array per part, filled with a repeated block of random u16
        ptr = dev.alloc(slab_bytes)
        rows = np.random.default_rng(p).integers(0, 2**16, 1 << 24, dtype=np.uint16)
        for off in range(0, slab_bytes, rows.nbytes):
            dev.h2d(ptr + off, rows[:min(rows.size, (slab_bytes - off) // 2)])
        ptrs.append(ptr)
    slab = lambda q: [p + q * n * ROT * 2 for p in ptrs]  # noqa: E731
    eng, deng = ih.MasksEngine(dev, queries[0]), ih.MasksEngine(direct, queries[0])

    # the first query's denominators and distances
    den_ptr, dist_ptr = dev.alloc(n * ROT * 2), dev.alloc(n * 8)
    with ih.MasksBatchEngine(dev, queries[:1]) as one:
        one.batch_process_device(mdb, den_ptr)
    dist = np.empty(n, np.float64)
    eng.resolve(mdb, slab(0), dist_out_device=dist_ptr)
    dev.d2h(dist, dist_ptr)
    dev.free(dist_ptr)
    for nbins in (64, 1024):
        want = want_hist(dist, nbins)
        got = [eng.histogram(mdb, slab(0), nbins), deng.histogram(ddb, slab(0), nbins),
               ih.resolver_histogram(dev, slab(0), den_ptr, n, nbins), ih.resolver_histogram(direct, slab(0), den_ptr, n, nbins)]
        for bins, invalid in got:
            if not (bins == want[0]).all() or invalid != want[1]:
                print(f"histogram at {nbins} bins differs from the bincount of the search's distances: no numbers")
                return 1
    w = want_hist(dist, 1024)[0]
    nz = np.flatnonzero(w)
    print(f"results: every form equals np.bincount of the search's distances; at 1024 bins {len(nz)} non-zero bins, "
          f"{nz[0]}..{nz[-1]}, {int(w[1023])} records in the last (distance >= 1023/1024)")

    print(f"\n1. fused form, n = {n}, {PARTS} parts")
    for nbins in (64, 1024):
        res = table([("copies", dev, lambda: eng.histogram(mdb, slab(0), nbins), ("masks_resolve_hist", "hist_reduce")),
                         ("direct", direct, lambda: deng.histogram(ddb, slab(0), nbins), ("masks_resolve_hist",)),
                         ("search", dev, lambda: eng.resolve(mdb, slab(0)), ("masks_resolve", "reduce")),
                         ("dense", dev, lambda: eng.matches(mdb, slab(0), INF, cap=0), ("masks_match",))],
                        reps, f"nbins = {nbins}")
        c, d, s, m = (res[k] for k in ("copies", "direct", "search", "dense"))
        print(f"   ratios (device): copies / search {c[1] / s[1]:.4f}, direct / search {d[1] / s[1]:.4f}, "
              f"copies / dense match {c[1] / m[1]:.4f}, direct / dense match {d[1] / m[1]:.4f}, direct / copies {d[1] / c[1]:.4f}")
        print(f"   ratios (host):   copies / search {c[0] / s[0]:.4f}, direct / search {d[0] / s[0]:.4f}, "
              f"copies / dense match {c[0] / m[0]:.4f}, direct / copies {d[0] / c[0]:.4f}")
        verdict(res)

    print(f"\n2. denominators given, n = {n}, {PARTS} parts")
    for nbins in (64, 1024):
        res = table([("copies", dev, lambda: ih.resolver_histogram(dev, slab(0), den_ptr, n, nbins), ("resolver_hist", "hist_reduce")),
                         ("direct", direct, lambda: ih.resolver_histogram(direct, slab(0), den_ptr, n, nbins), ("resolver_hist",)),
                         ("search", dev, lambda: ih.resolver_search_device(dev, slab(0), den_ptr, n), ("resolver", "reduce")),
                         ("dense", dev, lambda: ih.resolver_matches(dev, slab(0), den_ptr, n, INF, cap=0), ("resolver_match",))],
                        reps, f"nbins = {nbins}")
        c, d, s, m = (res[k] for k in ("copies", "direct", "search", "dense"))
        print(f"   ratios (device): copies / search {c[1] / s[1]:.4f}, direct / search {d[1] / s[1]:.4f}, "
              f"copies / dense match {c[1] / m[1]:.4f}, direct / copies {d[1] / c[1]:.4f}")
        print(f"   ratios (host):   copies / search {c[0] / s[0]:.4f}, copies / dense match {c[0] / m[0]:.4f}, "
              f"direct / copies {d[0] / c[0]:.4f}")
        verdict(res)
    dev.free(den_ptr)

    print(f"\n3. batch form, n = {n}, 1024 bins")
    for nq in (4, 16):
        if nq > nqm:
            continue
        singles = [ih.MasksEngine(dev, q) for q in queries[:nq]]
        with ih.MasksBatchEngine(dev, queries[:nq]) as be, ih.MasksBatchEngine(direct, queries[:nq]) as dbe:
            bins, invalid = be.histogram(mdb, ptrs, 1024)
            dbins, dinvalid = dbe.histogram(ddb, ptrs, 1024)
            want = want_hist(dist, 1024)
            s3 = singles[nq - 1].histogram(mdb, slab(nq - 1), 1024)
            if (not (bins[0] == want[0]).all() or invalid[0] != want[1] or not (bins.sum(axis=1) + invalid == n).all()
                    or bins.tobytes() != dbins.tobytes() or invalid.tobytes() != dinvalid.tobytes()
                    or s3[0].tobytes() != bins[nq - 1].tobytes() or s3[1] != invalid[nq - 1]):
                print("batch histogram differs: no numbers")
                return 1

            def each():
                for q, s in enumerate(singles):
                    s.histogram(mdb, slab(q), 1024)

            res = table([("copies", dev, lambda: be.histogram(mdb, ptrs, 1024), ("masks_batch_hist", "masks_resolve_hist", "hist_reduce")),
                             ("direct", direct, lambda: dbe.histogram(ddb, ptrs, 1024), ("masks_batch_hist", "masks_resolve_hist")),
                             ("search", dev, lambda: be.resolve(mdb, ptrs), ("masks_batch_resolve", "masks_resolve", "reduce")),
                             ("dense", dev, lambda: be.matches(mdb, ptrs, INF, cap=0), ("masks_batch_match", "masks_match")),
                             ("singles", dev, each, ("masks_resolve_hist", "hist_reduce"))],
                            min(reps, 9), f"{nq} queries")
            c, d, s, m, e = (res[k] for k in ("copies", "direct", "search", "dense", "singles"))
            print(f"   ratios (device): copies / search {c[1] / s[1]:.4f}, copies / dense match {c[1] / m[1]:.4f}, "
                  f"direct / copies {d[1] / c[1]:.4f}, copies / {nq} single calls {c[1] / e[1]:.4f}")
            print(f"   ratios (host):   copies / search {c[0] / s[0]:.4f}, copies / dense match {c[0] / m[0]:.4f}, "
                  f"direct / copies {d[0] / c[0]:.4f}, copies / {nq} single calls {c[0] / e[0]:.4f}")
            verdict(res)
        for s in singles:
            s.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
