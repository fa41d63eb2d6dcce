"""Measurement: the combined pass (iris_template_report) against the sibling calls it replaces
(iris_template_matches, iris_template_topk, iris_template_histogram).

On one device, in one process, on a generated TILES database far past the Infinity Cache (10M
records by default) and on a 20 000-record range of it (the K-split form): for every subset of two
or three parts, k in {1, 16, 64}, nbins in {64, 1024}, a threshold that matches a handful (0.3, room
for 1024) and the dense count-only case (threshold 2.0, cap = 0), the report call and the separate
calls are timed interleaved (report, a, b, c, report, ...) after a warm-up of all, with a host clock
around the blocking calls; then each side's launches with HIP events in a pass of its own
(kernel_stats).

Per case one line: the report's median, the sum of the siblings' medians, what the one call saves,
the siblings' spread in this run (the sum of their max - min), and the verdict of the standing rule
for a combining call -- faster than the calls it replaces by more than their spread.

Before anything is timed each part of the report is compared with its sibling's output.  No number
is printed if they differ.

usage: python tools/bench_report.py [n=10000000] [reps=15] [small n=20000]"""
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402

KS = (1, 16, 64)
NBINS = (64, 1024)
THRESHOLDS = ((0.3, 1024, "sparse"), (2.0, 0, "dense"))
SIBLING_NAMES = {"m": ("template_match",), "t": ("template_topk", "topk_merge"), "h": ("template_hist", "hist_reduce")}
REPORT_NAMES = ("template_report", "topk_merge", "hist_reduce", "template_match")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def device_ms(dev, fn, names, reps):
    dev.reset_stats()
    dev.set_profiling(True)
    for _ in range(reps):
        fn()
    dev.set_profiling(False)
    return sum(dev.kernel_stats(k)[1] for k in names) / reps


def cases():
    """(subset, threshold, cap, label, k, nbins): a part's argument is None where the subset lacks it."""
    for subset in ("mt", "mh", "th", "mth"):
        for thr, cap, label in (THRESHOLDS if "m" in subset else ((None, None, "-"),)):
            for k in (KS if "t" in subset else (None,)):
                for nbins in (NBINS if "h" in subset else (None,)):
                    yield subset, thr, cap, label, k, nbins


def same(a, b):
    return [(m.index, m.num, m.den, m.rotation, m.distance) for m in a] == \
           [(m.index, m.num, m.den, m.rotation, m.distance) for m in b]


def run_size(dev, eng, db, first, n, reps):
    print(f"\nn = {n} (records {first} .. {first + n}), {reps} interleaved repetitions; ms")
    print("   parts  matches  k    nbins | report host  siblings host  saved   siblings' spread  verdict |"
          " report device  siblings device")
    failed = []
    for subset, thr, cap, label, k, nbins in cases():
        report = lambda: eng.report(db, threshold=thr, cap=cap, k=k, nbins=nbins, first=first, n=n)  # noqa: E731
        sib = {}
        if "m" in subset:
            sib["m"] = lambda: eng.matches(db, thr, first=first, n=n, cap=cap)  # noqa: E731
        if "t" in subset:
            sib["t"] = lambda: eng.topk(db, k, first=first, n=n)  # noqa: E731
        if "h" in subset:
            sib["h"] = lambda: eng.histogram(db, nbins, first=first, n=n)  # noqa: E731
        r = report()
        if "m" in subset:
            got, count = sib["m"]()
            if count != r.matches_count or not same(got, r.matches):
                print("the report's matches differ from iris_template_matches': no numbers")
                return None
        if "t" in subset and not same(sib["t"](), r.topk):
            print("the report's top-k differs from iris_template_topk's: no numbers")
            return None
        if "h" in subset:
            bins, invalid = sib["h"]()
            if not (bins == r.bins).all() or invalid != r.invalid:
                print("the report's histogram differs from iris_template_histogram's: no numbers")
                return None
        calls = [report] + list(sib.values())
        for fn in calls:
            for _ in range(3):
                fn()
        host = [[] for _ in calls]
        for _ in range(reps):
            for h, fn in zip(host, calls):
                h.append(timed(fn))
        rep_ms = float(np.median(host[0]))
        sib_ms = sum(float(np.median(h)) for h in host[1:])
        sib_spread = sum(max(h) - min(h) for h in host[1:])
        ok = sib_ms - rep_ms > sib_spread
        dreps = min(reps, 5)
        rep_dev = device_ms(dev, report, REPORT_NAMES, dreps)
        sib_dev = sum(device_ms(dev, fn, SIBLING_NAMES[key], dreps) for key, fn in sib.items())
        print(f"   {subset:<5}  {label:<7}  {str(k or '-'):<3}  {str(nbins or '-'):<5} | {rep_ms:10.4f}  {sib_ms:13.4f}  "
              f"{sib_ms - rep_ms:6.4f}  {sib_spread:16.4f}  {'faster' if ok else 'NOT FASTER':<10} | "
              f"{rep_dev:13.4f}  {sib_dev:15.4f}")
        if not ok:
            failed.append((subset, label, k, nbins))
    return failed


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 15, 5)
    small = int(sys.argv[3]) if len(sys.argv) > 3 else 20_000
    dev = ih.Device(0)
    print(f"library: {ih.load_library().iris_version().decode()}")
    db = ih.Database(dev, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES)
    db.generate(n, 42)
    with ih.Database(dev, ih.KIND_TEMPLATES, 1) as g:
        g.generate(1, 43)
        query = g.read(0, 1)[0]
    eng = ih.TemplateEngine(dev, query)
    search = [timed(lambda: eng.search(db)) for _ in range(reps + 3)][3:]
    print(f"iris_template_search over n = {n}: host ms median {float(np.median(search)):.4f}")
    failed = []
    for first, m in ((0, n), (min(64, n - min(small, n)), min(small, n))):
        f = run_size(dev, eng, db, first, m, reps)
        if f is None:
            return 1
        failed += [(m,) + c for c in f]
    print(f"\nstanding rule (no measured form slower than the calls it replaces): "
          f"{'holds in every case' if not failed else 'FAILS in ' + repr(failed)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
