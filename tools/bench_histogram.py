"""Measurement: distance histograms (iris_template_histogram, iris_template_batch_histogram) against
the searches they are the siblings of, against the count-only dense match pass, and the two forms of
the flush against each other.

On one device, in one process, on a generated TILES database far past the Infinity Cache (10M
records by default):

  1. single query, per nbins in {64, 1024}, timed interleaved (a, b, c, d, a, ...) after a warm-up
     of all, with a host clock around the blocking calls, then each side's launches with HIP events
     in a pass of its own (kernel_stats):
       copies   iris_template_histogram as shipped: every workgroup adds its LDS histogram to copy
                blockIdx.x % 64 of the counters, hist_reduce sums the copies ("template_hist" +
                "hist_reduce")
       direct   the same call on a device opened with IRIS_HIST_COPIES=1: every workgroup adds
                straight into the result ("template_hist"), on a database of its own with the same
                records
       search   iris_template_search ("template_search" + "reduce"), which this feature leaves alone
       dense    iris_template_matches, threshold = +inf, cap = 0: the count-only dense match pass,
                one global atomic per wave ("template_match")
     Condition: the shipped histogram is not slower than the dense match pass (device times).
  2. batch, for 4, 64 and 1024 queries at 1024 bins: iris_template_batch_histogram
     ("template_batch_hist") against iris_template_batch_search ("template_batch" + "batch_reduce"
     by the host clock) and iris_template_batch_matches with an empty list (threshold 0, cap 0).

Before anything is timed the histograms are checked against np.bincount of the search's own
dist_out_device distances, binned by the header's rule.  No number is printed if they differ.

usage: python tools/bench_histogram.py [n=10000000] [reps=15] [max batch=1024]"""
import os
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402

INF = float("inf")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def spread(ts):
    return (max(ts) - min(ts)) / float(np.median(ts))


def gen_records(dev, n, seed):
    with ih.Database(dev, ih.KIND_TEMPLATES, max(n, 1)) as g:
        g.generate(n, seed)
        return g.read(0, n)


def open_hooked(**env):
    """Device 0 with test hooks, set for the open alone."""
    old = {k: os.environ.get(k) for k in list(env) + ["IRIS_TEST_HOOKS"]}
    os.environ["IRIS_TEST_HOOKS"] = "1"
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return ih.Device(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def device_ms(dev, fn, names, reps):
    """Device time per call: the sum of the named launches' HIP-event times over reps calls."""
    dev.reset_stats()
    dev.set_profiling(True)
    for _ in range(reps):
        fn()
    dev.set_profiling(False)
    return {k: dev.kernel_stats(k)[1] / reps for k in names}


def want_hist(dist, nbins):
    finite = np.isfinite(dist)
    b = np.minimum(nbins - 1, np.floor(dist[finite] * nbins)).astype(np.int64)
    return np.bincount(b, minlength=nbins).astype(np.uint64), int((~finite).sum())


def table(rows, reps, note):
    """rows: (label, device the call runs on, call, kernel names)."""
    for _, _, fn, _ in rows:
        for _ in range(3):
            fn()
    host = [[] for _ in rows]
    for _ in range(reps):
        for h, (_, _, fn, _) in zip(host, rows):
            h.append(timed(fn))
    print(f"   {note}, {reps} interleaved repetitions")
    print("                 host ms (median)  spread   device ms / call (by launch name)")
    out = {}
    for h, (label, dev, fn, names) in zip(host, rows):
        dms = device_ms(dev, fn, names, min(reps, 10))
        out[label] = (float(np.median(h)) * 1e3, sum(dms.values()), spread(h))  # host ms, device ms, host spread
        parts = ", ".join(f"{k} {v:.4f}" for k, v in dms.items())
        print(f"   {label:<10}    {out[label][0]:10.4f}      {spread(h):6.1%}   {out[label][1]:10.4f}   ({parts})")
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 15, 5)
    max_batch = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    dev = ih.Device(0)
    direct = open_hooked(IRIS_HIST_COPIES=1)
    print(f"library: {ih.load_library().iris_version().decode()}")
    print(f"direct device: hist_copies={direct.config()['hist_copies']}")

    tdb = ih.Database(dev, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES)
    tdb.generate(n, 42)
    ddb = ih.Database(direct, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES)
    ddb.generate(n, 42)
    queries = gen_records(dev, max(max_batch, 1), 43)
    eng, deng = ih.TemplateEngine(dev, queries[0]), ih.TemplateEngine(direct, queries[0])

    dist_ptr = dev.alloc(n * 8)
    dist = np.empty(n, np.float64)
    eng.search(tdb, dist_out_device=dist_ptr)
    dev.d2h(dist, dist_ptr)
    dev.free(dist_ptr)
    for nbins in (64, 1024):
        want, want_invalid = want_hist(dist, nbins)
        for e, d in ((eng, tdb), (deng, ddb)):
            bins, invalid = e.histogram(d, nbins)
            if not (bins == want).all() or invalid != want_invalid:
                print(f"histogram at {nbins} bins differs from the bincount of the search's distances: no numbers")
                return 1
    nz = np.flatnonzero(want_hist(dist, 1024)[0])
    print(f"results: both forms equal np.bincount of the search's distances; at 1024 bins {len(nz)} non-zero bins, "
          f"{nz[0]}..{nz[-1]}")

    print(f"\n1. single query, n = {n}")
    for nbins in (64, 1024):
        res = table([("copies", dev, lambda: eng.histogram(tdb, nbins), ("template_hist", "hist_reduce")),
                     ("direct", direct, lambda: deng.histogram(ddb, nbins), ("template_hist",)),
                     ("search", dev, lambda: eng.search(tdb), ("template_search", "reduce")),
                     ("dense", dev, lambda: eng.matches(tdb, INF, cap=0), ("template_match",))],
                    reps, f"nbins = {nbins}")
        c, d, s, m = (res[k] for k in ("copies", "direct", "search", "dense"))
        print(f"   ratios (device): copies / search {c[1] / s[1]:.4f}, direct / search {d[1] / s[1]:.4f}, "
              f"copies / dense match {c[1] / m[1]:.4f}, direct / dense match {d[1] / m[1]:.4f}")
        print(f"   ratios (host):   copies / search {c[0] / s[0]:.4f}, direct / search {d[0] / s[0]:.4f}")
        print(f"   condition (shipped histogram <= dense match pass, device times): {'holds' if c[1] <= m[1] else 'FAILS'}")
    eng.close()
    deng.close()
    ddb.close()
    direct.close()

    print(f"\n2. batch, n = {n}, 1024 bins")
    for nq in (4, 64, 1024):
        if nq > max_batch:
            continue
        with ih.TemplateBatchEngine(dev, queries[:nq]) as be:
            bins, invalid = be.histogram(tdb, 1024)
            want, want_invalid = want_hist(dist, 1024)
            if not (bins[0] == want).all() or invalid[0] != want_invalid or not (bins.sum(axis=1) + invalid == n).all():
                print("batch histogram differs: no numbers")
                return 1
            r = 3 if nq >= 1024 else min(reps, 7)
            res = table([("histogram", dev, lambda: be.histogram(tdb, 1024), ("template_batch_hist",)),
                         ("search", dev, lambda: be.search(tdb), ("template_batch",)),
                         ("matches", dev, lambda: be.matches(tdb, 0.0, cap=0), ("template_batch_match",))],
                        r, f"{nq} queries")
            h, s, m = (res[k] for k in ("histogram", "search", "matches"))
            print(f"   ratios (host): histogram / search {h[0] / s[0]:.4f}, histogram / matches {h[0] / m[0]:.4f}, "
                  f"matches / search {m[0] / s[0]:.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
