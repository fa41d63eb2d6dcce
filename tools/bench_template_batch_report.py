"""Measurement: the template batch report (iris_template_batch_report) against the sibling batch
calls it replaces (iris_template_batch_matches, iris_template_batch_topk,
iris_template_batch_histogram).

On one device, in one process, on a generated TILES database far past the Infinity Cache (10M
records by default), for engines of 4, 64 and 1024 generated queries: for every subset of two or
three parts, k in {1, 16, 64}, nbins in {64, 1024}, a threshold that matches nothing or a handful
(0.3, room for 1024 a query) and the dense count-only case (threshold 2.0, cap = 0), the report call
and the separate calls are timed interleaved (report, a, b, c, report, ...) after a warm-up of all,
with a host clock around the blocking C calls into arrays allocated once; then each side's launches
with HIP events in a pass of its own (kernel_stats).  A call of 1024 queries over 10M records takes
seconds, so engines of more than `full` queries run a selection of the cases (WIDE_CASES) unless
`full` says otherwise.

Per case one line: the report's median, the sum of the siblings' medians, their ratio, what the one
call saves, the siblings' spread in this run (the sum of their max - min), and the verdict of the
standing rule for a combining call -- faster than the calls it replaces by more than their spread.

Before anything is timed each part of the report is compared with its sibling's output, byte for
byte.  No number is printed if they differ.

usage: python tools/bench_template_batch_report.py [n=10000000] [reps=9] [nqs=4,64,1024] [full=64]"""
import ctypes
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
WIDE_CASES = [("mth", 0.3, 1024, "sparse", 16, 1024), ("mth", 2.0, 0, "dense", 64, 1024), ("th", None, None, "-", 16, 64),
              ("mt", 0.3, 1024, "sparse", 1, None), ("mh", 2.0, 0, "dense", None, 64)]
SIBLING_NAMES = {"m": ("template_batch_match",), "t": ("template_batch_topk", "topk_merge"), "h": ("template_batch_hist",)}
REPORT_NAMES = ("template_batch_report", "topk_merge", "template_batch_match")
BITS = {"m": ih.REPORT_MATCHES, "t": ih.REPORT_TOPK, "h": ih.REPORT_HIST}


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


class Arrays:
    """The output arrays of one side (the report's or the siblings'), allocated once per case."""

    def __init__(self, nq, cap, k, nbins):
        self.matches = (ih.Match * max(nq * (cap or 0), 1))()
        self.matches_counts = (ctypes.c_uint64 * nq)()
        self.topk = (ih.Match * (nq * (k or 1)))()
        self.topk_counts = (ctypes.c_uint32 * nq)()
        self.bins = np.zeros((nq, nbins or 1), np.uint64)
        self.invalid = np.zeros(nq, np.uint64)

    def parts(self, subset, nq, cap, k):
        out = []
        if "m" in subset:
            counts = list(self.matches_counts)
            out += [counts] + [bytes(self.matches)[32 * q * cap:32 * (q * cap + min(counts[q], cap))] for q in range(nq)]
        if "t" in subset:
            counts = list(self.topk_counts)
            out += [counts] + [bytes(self.topk)[32 * q * k:32 * (q * k + counts[q])] for q in range(nq)]
        if "h" in subset:
            out += [self.bins.tobytes(), self.invalid.tobytes()]
        return out


def check(rc):
    if rc != 0:
        raise RuntimeError(ih.load_library().iris_last_error().decode(errors="replace"))


def run_engine(dev, eng, db, n, reps, selection):
    lib = ih.load_library()
    nq = eng.nq
    u64p = ctypes.POINTER(ctypes.c_uint64)
    print(f"\nnq = {nq}, n = {n}, {reps} interleaved repetitions; ms")
    print("   parts  matches  k    nbins | report host  siblings host  ratio   saved      siblings' spread  verdict    |"
          " report device  siblings device")
    failed = []
    for subset, thr, cap, label, k, nbins in selection:
        mine, theirs = Arrays(nq, cap, k, nbins), Arrays(nq, cap, k, nbins)
        r = ih.BatchReport()
        r.parts = sum(BITS[c] for c in subset)
        if "m" in subset:
            r.threshold, r.matches_cap, r.matches_counts = thr, cap, mine.matches_counts
            r.matches = mine.matches if cap else None
        if "t" in subset:
            r.k, r.topk, r.topk_counts = k, mine.topk, mine.topk_counts
        if "h" in subset:
            r.nbins, r.bins, r.invalid = nbins, mine.bins.ctypes.data_as(u64p), mine.invalid.ctypes.data_as(u64p)
        report = lambda: check(lib.iris_template_batch_report(eng.handle, db.handle, 0, n, 0, ctypes.byref(r)))  # noqa: E731
        sib = {}
        if "m" in subset:
            sib["m"] = lambda: check(lib.iris_template_batch_matches(  # noqa: E731
                eng.handle, db.handle, 0, n, 0, thr, theirs.matches if cap else None, cap, theirs.matches_counts))
        if "t" in subset:
            sib["t"] = lambda: check(lib.iris_template_batch_topk(  # noqa: E731
                eng.handle, db.handle, 0, n, 0, k, theirs.topk, theirs.topk_counts))
        if "h" in subset:
            sib["h"] = lambda: check(lib.iris_template_batch_histogram(  # noqa: E731
                eng.handle, db.handle, 0, n, nbins, theirs.bins.ctypes.data_as(ctypes.c_void_p),
                theirs.invalid.ctypes.data_as(ctypes.c_void_p)))
        calls = [report] + list(sib.values())
        for fn in calls:  # the first call of each is also the warm-up
            fn()
        if mine.parts(subset, nq, cap, k) != theirs.parts(subset, nq, cap, k):
            print(f"the report's parts differ from the sibling calls' ({subset} {label} {k} {nbins}): no numbers")
            return None
        slow = timed(report) > 500.0  # seconds per call: one warm-up and one device pass are enough
        for fn in calls:
            for _ in range(0 if slow else 2):
                fn()
        host = [[] for _ in calls]
        for _ in range(reps):
            for h, fn in zip(host, calls):
                h.append(timed(fn))
        rep_ms = float(np.median(host[0]))
        sib_ms = sum(float(np.median(h)) for h in host[1:])
        sib_spread = sum(max(h) - min(h) for h in host[1:])
        ok = sib_ms - rep_ms > sib_spread
        dreps = 1 if slow else min(reps, 5)
        rep_dev = device_ms(dev, report, REPORT_NAMES, dreps)
        sib_dev = sum(device_ms(dev, fn, SIBLING_NAMES[key], dreps) for key, fn in sib.items())
        print(f"   {subset:<5}  {label:<7}  {str(k or '-'):<3}  {str(nbins or '-'):<5} | {rep_ms:11.3f}  {sib_ms:13.3f}  "
              f"{rep_ms / sib_ms:5.3f}  {sib_ms - rep_ms:9.3f}  {sib_spread:16.3f}  "
              f"{'faster' if ok else 'slower' if rep_ms >= sib_ms else 'NOT FASTER':<10} | {rep_dev:13.3f}  {sib_dev:15.3f}",
              flush=True)
        if not ok:
            failed.append((nq, subset, label, k, nbins))
    return failed


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 9, 3)
    nqs = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "4,64,1024").split(",")]
    full = int(sys.argv[4]) if len(sys.argv) > 4 else 64
    dev = ih.Device(0)
    print(f"library: {ih.load_library().iris_version().decode()}")
    db = ih.Database(dev, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES)
    db.generate(n, 42)
    with ih.Database(dev, ih.KIND_TEMPLATES, max(nqs)) as g:
        g.generate(max(nqs), 43)
        queries = g.read(0, max(nqs))
    failed = []
    for nq in nqs:
        with ih.TemplateBatchEngine(dev, queries[:nq]) as eng:
            search = [timed(lambda: eng.search(db)) for _ in range(4)][1:]
            print(f"\niris_template_batch_search, nq = {nq}, n = {n}: host ms median {float(np.median(search)):.3f}")
            f = run_engine(dev, eng, db, n, reps, list(cases()) if nq <= full else WIDE_CASES)
        if f is None:
            return 1
        failed += f
    print(f"\nstanding rule (faster than the calls it replaces by more than their spread): "
          f"{'holds in every case' if not failed else 'MISSED in ' + repr(failed)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
