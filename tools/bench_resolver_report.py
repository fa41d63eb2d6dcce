"""Measurement: the resolver reports (iris_resolver_report_masks, iris_resolver_report) against the
sibling calls they replace (iris_resolver_{matches,topk,histogram}_masks and
iris_resolver_{matches,topk,histogram}).

On one device, in one process, on a generated TILES masks database far past the Infinity Cache (10M
masks by default) with 3 participants' uniform random share rows, and on a 20 000-mask range of it:
for every subset of two or three parts, k in {1, 16, 64}, nbins in {64, 1024}, a sparse match list
(threshold 1e-5: with uniform shares the records with uneq = 0 in some rotation, about one in a
thousand; the 1024 lowest indices and the exact total) and the dense count-only case (threshold 2.0,
cap = 0), the report call and the separate calls are timed interleaved (report, a, b, c, report,
...) after a warm-up of all, with a host clock around the blocking calls; then each side's launches
with HIP events in a pass of its own (kernel_stats).  The same runs are then made for iris_resolver_report,
the denominators given: the masks engine's own rows, kept on the device.

Per case one line: the report's median, the sum of the siblings' medians, what the one call saves,
the siblings' spread in this run (the sum of their max - min), and the verdict of the standing rule
for a combining call -- faster than the calls it replaces by more than their spread.

Before anything is timed each part of the report is compared with its sibling's output.  No number
is printed if they differ.

Exit status: 0; 1 if a part differs from its sibling's; 2 if a case is slower than the calls it
replaces on its median.

usage: python tools/bench_resolver_report.py [n=10000000] [reps=15] [small n=20000]"""
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402

ROT, PARTS, SEED = 31, 3, 42
KS = (1, 16, 64)
NBINS = (64, 1024)
THRESHOLDS = ((1e-5, 1024, "sparse"), (2.0, 0, "dense"))
# kernel_stats names of each side: (the masks calls on TILES, the calls with denominators given)
SIBLING_NAMES = {
    "masks": {"m": ("masks_match",), "t": ("masks_topk", "topk_merge"), "h": ("masks_resolve_hist", "hist_reduce")},
    "plain": {"m": ("resolver_match",), "t": ("resolver_topk", "topk_merge"), "h": ("resolver_hist", "hist_reduce")},
}
REPORT_NAMES = {"masks": ("masks_report", "topk_merge", "hist_reduce", "masks_match"),
                "plain": ("resolver_report", "topk_merge", "hist_reduce", "resolver_match")}


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


class MasksForm:
    """iris_resolver_report_masks and its siblings over records [first, first + n)."""
    key = "masks"

    def __init__(self, eng, db, ptrs, first, n):
        self.eng, self.db, self.first, self.n = eng, db, first, n
        self.ptrs = [p + first * ROT * 2 for p in ptrs]

    def report(self, thr, cap, k, nbins):
        return self.eng.report(self.db, self.ptrs, threshold=thr, cap=cap, k=k, nbins=nbins, first=self.first, n=self.n)

    def matches(self, thr, cap):
        return self.eng.matches(self.db, self.ptrs, thr, first=self.first, n=self.n, cap=cap)

    def topk(self, k):
        return self.eng.topk(self.db, self.ptrs, k, first=self.first, n=self.n)

    def histogram(self, nbins):
        return self.eng.histogram(self.db, self.ptrs, nbins, first=self.first, n=self.n)


class PlainForm:
    """iris_resolver_report and its siblings over rows [first, first + n) of the arrays."""
    key = "plain"

    def __init__(self, dev, ptrs, den_ptr, first, n):
        self.dev, self.n = dev, n
        self.ptrs, self.den = [p + first * ROT * 2 for p in ptrs], den_ptr + first * ROT * 2

    def report(self, thr, cap, k, nbins):
        return ih.resolver_report(self.dev, self.ptrs, self.den, self.n, threshold=thr, cap=cap, k=k, nbins=nbins)

    def matches(self, thr, cap):
        return ih.resolver_matches(self.dev, self.ptrs, self.den, self.n, thr, cap=cap)

    def topk(self, k):
        return ih.resolver_topk(self.dev, self.ptrs, self.den, self.n, k)

    def histogram(self, nbins):
        return ih.resolver_histogram(self.dev, self.ptrs, self.den, self.n, nbins)


def run_size(dev, form, reps):
    print(f"\n{form.key}: n = {form.n}, {reps} interleaved repetitions; ms")
    print("   parts  matches  k    nbins | report host  siblings host  saved   siblings' spread  verdict |"
          " report device  siblings device")
    failed = []
    for subset, thr, cap, label, k, nbins in cases():
        report = lambda: form.report(thr, cap, k, nbins)  # noqa: E731
        sib = {}
        if "m" in subset:
            sib["m"] = lambda: form.matches(thr, cap)  # noqa: E731
        if "t" in subset:
            sib["t"] = lambda: form.topk(k)  # noqa: E731
        if "h" in subset:
            sib["h"] = lambda: form.histogram(nbins)  # noqa: E731
        r = report()
        if "m" in subset:
            got, count = sib["m"]()
            if count != r.matches_count or not same(got, r.matches):
                print("the report's matches differ from the sibling's: no numbers")
                return None
        if "t" in subset and not same(sib["t"](), r.topk):
            print("the report's top-k differs from the sibling's: no numbers")
            return None
        if "h" in subset:
            bins, invalid = sib["h"]()
            if not (bins == r.bins).all() or invalid != r.invalid:
                print("the report's histogram differs from the sibling's: no numbers")
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
        rep_dev = device_ms(dev, report, REPORT_NAMES[form.key], dreps)
        sib_dev = sum(device_ms(dev, fn, SIBLING_NAMES[form.key][key], dreps) for key, fn in sib.items())
        print(f"   {subset:<5}  {label:<7}  {str(k or '-'):<3}  {str(nbins or '-'):<5} | {rep_ms:10.4f}  {sib_ms:13.4f}  "
              f"{sib_ms - rep_ms:6.4f}  {sib_spread:16.4f}  {'faster' if ok else 'NOT FASTER':<10} | "
              f"{rep_dev:13.4f}  {sib_dev:15.4f}", flush=True)
        if not ok:
            failed.append((form.key, form.n, subset, label, k, nbins, "median" if sib_ms <= rep_ms else "spread"))
    return failed


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 15, 5)
    small = min(int(sys.argv[3]) if len(sys.argv) > 3 else 20_000, n)
    dev = ih.Device(0)
    print(f"library: {ih.load_library().iris_version().decode()}")
    db = ih.Database(dev, ih.KIND_MASKS, n, ih.LAYOUT_TILES)
    db.generate(n, SEED)
    with ih.Database(dev, ih.KIND_MASKS, 1) as g:
        g.generate(1, SEED + 1)
        qmask = g.read(0, 1)[0]
    rng = np.random.default_rng(SEED)
    ptrs = []
    for p in range(PARTS):  # uniform shares, generated and uploaded in pieces
        ptrs.append(dev.alloc(n * ROT * 2))
        for lo in range(0, n, 1 << 20):
            m = min(1 << 20, n - lo)
            dev.h2d(ptrs[p] + lo * ROT * 2, rng.integers(0, 65536, (m, ROT), dtype=np.uint16))
    den_ptr = dev.alloc(n * ROT * 2)
    with ih.MasksBatchEngine(dev, qmask[None, :]) as be:
        be.batch_process_device(db, den_ptr)
    eng = ih.MasksEngine(dev, qmask)
    search = [timed(lambda: eng.resolve(db, ptrs)) for _ in range(reps + 3)][3:]
    print(f"iris_resolver_search_masks over n = {n}, {PARTS} parts: host ms median {float(np.median(search)):.4f}")
    failed = []
    for first, m in ((0, n), (min(64, n - small), small)):
        for form in (MasksForm(eng, db, ptrs, first, m), PlainForm(dev, ptrs, den_ptr, first, m)):
            f = run_size(dev, form, reps)
            if f is None:
                return 1
            failed += f
    print(f"\nstanding rule (no measured form slower than the calls it replaces): "
          f"{'holds in every case' if not failed else 'FAILS in ' + repr(failed)}")
    return 2 if any(f[-1] == "median" for f in failed) else 0  # a miss on a sibling's spread alone is reported, not failed


if __name__ == "__main__":
    sys.exit(main())
