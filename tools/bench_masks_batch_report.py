"""Measurement: the masks batch report (iris_resolver_batch_report_masks) against the sibling batch
calls it replaces (iris_resolver_batch_{matches,topk,histogram}_masks).

On one device, in one process, on a generated TILES masks database far past the Infinity Cache (10M
masks by default) with 3 participants' uniform random query-major share rows (nq slabs of n rows
per participant, uploaded from one random 64-MiB block), and on a 20 000-mask range of it (the resolver's
chunk: single-query passes, no batch kernel): for nq in {2, 3, 4, 5, 16, 64} queries, subsets of
two or three parts, k in {1, 16, 64}, nbins in {64, 1024}, a sparse match list (threshold 1e-5: with
uniform shares the records with uneq = 0 in some rotation, about one in a thousand; cap 16 384 holds
every list of 10M records, so neither side runs a second pass) and the dense count-only case
(threshold 2.0, cap = 0), the report call and the separate calls are timed interleaved (report, a,
b, c, report, ...) after a warm-up of all, with a host clock around the blocking C calls (ctypes,
the output arrays allocated once per case); then each side's launches with HIP events in a pass of
its own (kernel_stats).  All three parts get the full k x nbins matrix; the two-part subsets k = 16
and 64 bins, and the top-k + histogram subset every k; 64 queries k = 16 alone.

Per case one line: the report's median, the sum of the siblings' medians, what the one call saves,
the siblings' spread in this run (the sum of their max - min), and the verdict of the standing rule
for a combining call -- faster than the calls it replaces by more than their spread.

Before anything is timed each part of the report is compared with its sibling's output, byte for
byte.  No number is printed if they differ.

Exit status: 0; 1 if a part differs from its sibling's; 2 if a case is slower than the calls it
replaces on its median.

usage: python tools/bench_masks_batch_report.py [n=10000000] [reps=9] [small n=20000] [nq,nq,...]"""
import ctypes
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402

ROT, PARTS, SEED = 31, 3, 42
NQS = (2, 3, 4, 5, 16, 64)
THRESHOLDS = ((1e-5, 16384, "sparse"), (2.0, 0, "dense"))
SIBLING_NAMES = {"m": ("masks_batch_match", "masks_match"), "t": ("masks_batch_topk", "masks_topk", "topk_merge"),
                 "h": ("masks_batch_hist", "masks_resolve_hist", "hist_reduce")}
REPORT_NAMES = ("masks_batch_report", "masks_report", "topk_merge", "hist_reduce", "masks_batch_match", "masks_match")


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


def cases(nq):
    """(subset, threshold, cap, label, k, nbins): a part's argument is None where the subset lacks it."""
    ks = (16,) if nq == 64 else (1, 16, 64)
    for thr, cap, label in THRESHOLDS:
        for k in ks:
            for nbins in (64, 1024):
                yield "mth", thr, cap, label, k, nbins
        yield "mt", thr, cap, label, 16, None
        yield "mh", thr, cap, label, None, 64
    for k in ks:
        yield "th", None, None, "-", k, 64
    yield "th", None, None, "-", 16, 1024


class Calls:
    """The raw C calls of one case over records [first, first + n) for the first nq queries, into
    arrays allocated here: report() and the selected siblings."""

    def __init__(self, eng, db, ptrs, first, n, subset, thr, cap, k, nbins):
        lib = ih.load_library()
        nq = eng.nq
        arr = (ctypes.c_void_p * PARTS)(*ptrs)
        h = (eng.handle, db.handle, first, n, arr, PARTS)
        self.out, self.sib = {}, {}
        r = ih.BatchReport()
        for side in ("report", "sibling"):
            o = {}
            if "m" in subset:
                o["m"] = ((ih.Match * max(nq * cap, 1))(), (ctypes.c_uint64 * nq)())
            if "t" in subset:
                o["t"] = ((ih.Match * (nq * k))(), (ctypes.c_uint32 * nq)())
            if "h" in subset:
                o["h"] = (np.zeros((nq, nbins), np.uint64), np.zeros(nq, np.uint64))
            self.out[side] = o
        o = self.out["report"]
        if "m" in subset:
            r.parts |= ih.REPORT_MATCHES
            r.threshold, r.matches_cap, r.matches_counts = thr, cap, o["m"][1]
            r.matches = o["m"][0] if cap else None
        if "t" in subset:
            r.parts |= ih.REPORT_TOPK
            r.k, r.topk, r.topk_counts = k, o["t"][0], o["t"][1]
        if "h" in subset:
            r.parts |= ih.REPORT_HIST
            r.nbins = nbins
            r.bins = o["h"][0].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
            r.invalid = o["h"][1].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        self.struct = r

        def check(rc):
            if rc != 0:
                raise RuntimeError(lib.iris_last_error().decode())

        self.report = lambda: check(lib.iris_resolver_batch_report_masks(*h, 0, ctypes.byref(r)))
        s = self.out["sibling"]
        if "m" in subset:
            self.sib["m"] = lambda: check(lib.iris_resolver_batch_matches_masks(*h, 0, thr, s["m"][0] if cap else None, cap,
                                                                               s["m"][1]))
        if "t" in subset:
            self.sib["t"] = lambda: check(lib.iris_resolver_batch_topk_masks(*h, 0, k, s["t"][0], s["t"][1]))
        if "h" in subset:
            self.sib["h"] = lambda: check(lib.iris_resolver_batch_histogram_masks(
                *h, nbins, s["h"][0].ctypes.data_as(ctypes.c_void_p), s["h"][1].ctypes.data_as(ctypes.c_void_p)))

    def equal(self):
        a, b = self.out["report"], self.out["sibling"]
        for key in a:
            if key == "h":
                if a[key][0].tobytes() != b[key][0].tobytes() or a[key][1].tobytes() != b[key][1].tobytes():
                    return False
            elif bytes(a[key][0]) != bytes(b[key][0]) or list(a[key][1]) != list(b[key][1]):
                return False
        return True


def run_size(dev, eng, db, ptrs, first, n, reps):
    print(f"\nnq = {eng.nq}, n = {n}, {reps} interleaved repetitions; ms")
    print("   parts  matches  k    nbins | report host  siblings host  saved    siblings' spread  verdict    |"
          " report device  siblings device")
    failed = []
    for subset, thr, cap, label, k, nbins in cases(eng.nq):
        c = Calls(eng, db, ptrs, first, n, subset, thr, cap, k, nbins)
        calls = [c.report] + list(c.sib.values())
        for fn in calls:
            for _ in range(3):
                fn()
        if not c.equal():
            print(f"   {subset} {label} k={k} nbins={nbins}: the report differs from its siblings: no numbers")
            return None
        host = [[] for _ in calls]
        for _ in range(reps):
            for h, fn in zip(host, calls):
                h.append(timed(fn))
        rep_ms = float(np.median(host[0]))
        sib_ms = sum(float(np.median(h)) for h in host[1:])
        sib_spread = sum(max(h) - min(h) for h in host[1:])
        ok = sib_ms - rep_ms > sib_spread
        dreps = min(reps, 3)
        rep_dev = device_ms(dev, c.report, REPORT_NAMES, dreps)
        sib_dev = sum(device_ms(dev, fn, SIBLING_NAMES[key], dreps) for key, fn in c.sib.items())
        print(f"   {subset:<5}  {label:<7}  {str(k or '-'):<3}  {str(nbins or '-'):<5} | {rep_ms:10.4f}  {sib_ms:13.4f}  "
              f"{sib_ms - rep_ms:7.4f}  {sib_spread:16.4f}  {'faster' if ok else 'NOT FASTER':<10} | "
              f"{rep_dev:13.4f}  {sib_dev:15.4f}", flush=True)
        if not ok:
            failed.append((eng.nq, n, subset, label, k, nbins, "median" if sib_ms <= rep_ms else "spread"))
    return failed


class Uniform:
    """A device array of uniform random u16: one 64-MiB block, uploaded over and over (nq slabs of
    10M rows are 40 GB a participant at 64 queries; what a pass reads is what matters here)."""

    def __init__(self, dev, nbytes):
        self.dev, self.ptr = dev, dev.alloc(nbytes)
        block = np.random.default_rng(SEED).integers(0, 65536, 1 << 25, dtype=np.uint16)
        for lo in range(0, nbytes, block.nbytes):
            dev.h2d(self.ptr + lo, block[:min(block.nbytes, nbytes - lo) // 2])

    def close(self):
        self.dev.free(self.ptr)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 9, 9)
    small = min(int(sys.argv[3]) if len(sys.argv) > 3 else 20_000, n)
    nqs = tuple(int(x) for x in sys.argv[4].split(",")) if len(sys.argv) > 4 else NQS
    dev = ih.Device(0)
    print(f"library: {ih.load_library().iris_version().decode()}")
    db = ih.Database(dev, ih.KIND_MASKS, n, ih.LAYOUT_TILES)
    db.generate(n, SEED)
    with ih.Database(dev, ih.KIND_MASKS, max(nqs)) as g:
        g.generate(max(nqs), SEED + 1)
        qmasks = g.read(0, max(nqs))
    failed = []
    for nq in nqs:
        # query-major arrays of nq slabs are laid out for this nq and this range
        for first, m in ((0, n), (min(64, n - small), small)):
            owners = [Uniform(dev, nq * m * ROT * 2) for _ in range(PARTS)]
            ptrs = [o.ptr for o in owners]  # row i of a slab is record first + i
            with ih.MasksBatchEngine(dev, qmasks[:nq]) as eng:
                f = run_size(dev, eng, db, ptrs, first, m, reps)
            for o in owners:
                o.close()
            if f is None:
                return 1
            failed += f
    print(f"\nstanding rule (no measured case slower than the calls it replaces): "
          f"{'holds in every case' if not failed else 'FAILS in ' + repr(failed)}")
    return 2 if any(f[-1] == "median" for f in failed) else 0  # a miss on a sibling's spread alone is reported, not failed


if __name__ == "__main__":
    sys.exit(main())
