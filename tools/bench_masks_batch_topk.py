"""Measurement: batched top-k (iris_resolver_batch_topk_masks) against the batched search it is the
sibling of and against the single-query top-k calls it replaces.

On one device, in one process, on tools/bench_masks_batch.py's inputs -- a generated TILES masks
database far past the Infinity Cache (10M records by default), 3 parts of query-major device share
arrays holding a repeated block of uniform random u16 -- for nq in 2, 3, 4, 5, 8, 16 and k in 1, 16,
64:

  (a) one iris_resolver_batch_topk_masks call of a MasksBatchEngine of nq queries;
  (b) one iris_resolver_batch_search_masks call on the same engine and inputs;
  (c) nq back-to-back iris_resolver_topk_masks calls on nq prebuilt MasksEngines, each on its slab
      of every part.

All three are timed in the same run, interleaved with the order rotated every repetition (a b c,
b c a, c a b, ...) after a warm-up of each shape (at least three rounds and half a second), with a
host clock around the blocking C calls (output buffers allocated once, outside the clock); the
table gives medians and each side's spread ((max - min) / median of its repetitions).  The same at
n = 20 000 (the resolver's chunk: below the batch kernel's range, every query runs the
single-query pass inside the call).  The device time of (a)'s and (b)'s launches and the share of
(a)'s merge launches come from kernel_stats (HIP events, a pass of its own).

Conditions: at the large range (a) < (c) x (1 - spread(c)) for every (nq, k); at 20 000
(a) <= (c) x (1 + spread(c)).  (a) / (b) is reported, not bounded.

Before anything is timed the batched lists and counts are compared, byte for byte, with the
single-query calls' at 20 000 and 300 000 records; no number is printed if they differ.

usage: python tools/bench_masks_batch_topk.py [n=10000000] [reps=15]"""
import ctypes
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402

NQS = (2, 3, 4, 5, 8, 16)
KS = (1, 16, 64)
ROT = 31
PARTS = 3
WARM_S = 0.5  # warm-up of each (nq, k) before its timed repetitions


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def spread(ts):
    return (max(ts) - min(ts)) / float(np.median(ts))


class Calls:
    """The three C calls over [0, n) for the first nq queries, into buffers allocated once."""

    def __init__(self, lib, db, batches, singles, share_ptrs, nqmax):
        self.lib, self.db, self.batches, self.singles, self.ptrs = lib, db, batches, singles, share_ptrs
        self.out = (ih.Match * (nqmax * ih.TOPK_MAX))()
        self.one = (ih.Match * ih.TOPK_MAX)()
        self.best = (ih.Match * nqmax)()
        self.counts = (ctypes.c_uint32 * nqmax)()
        self.count = ctypes.c_uint32()
        self.arr = (ctypes.c_void_p * PARTS)(*share_ptrs)

    def a(self, nq, n, k):
        rc = self.lib.iris_resolver_batch_topk_masks(self.batches[nq].handle, self.db.handle, 0, n, self.arr, PARTS, 0, k,
                                                     self.out, self.counts)
        assert rc == 0, (rc, self.lib.iris_last_error())

    def b(self, nq, n):
        rc = self.lib.iris_resolver_batch_search_masks(self.batches[nq].handle, self.db.handle, 0, n, self.arr, PARTS, 0,
                                                       None, self.best)
        assert rc == 0, (rc, self.lib.iris_last_error())

    def c(self, nq, n, k, keep=None):
        slab = n * ROT * 2
        for q in range(nq):
            arr = (ctypes.c_void_p * PARTS)(*[p + q * slab for p in self.ptrs])
            rc = self.lib.iris_resolver_topk_masks(self.singles[q].handle, self.db.handle, 0, n, arr, PARTS, 0, k, self.one,
                                                   ctypes.byref(self.count))
            assert rc == 0, (rc, self.lib.iris_last_error())
            if keep is not None:
                keep.append((self.count.value, bytes(self.one)[:32 * self.count.value]))


def device_ms(dev, fn, names, reps=3):
    dev.reset_stats()
    dev.set_profiling(True)
    for _ in range(reps):
        fn()
    dev.set_profiling(False)
    stats = {k: dev.kernel_stats(k) for k in names}
    return {k: s[1] / reps for k, s in stats.items()}, {k: s[0] // reps for k, s in stats.items() if s[0]}


def check_results(calls, nq, sizes, k=64):
    for n in sizes:
        singles = []
        calls.c(nq, n, k, singles)
        calls.a(nq, n, k)
        raw = bytes(calls.out)
        for q, (count, recs) in enumerate(singles):
            if calls.counts[q] != count or count != k or raw[q * k * 32:q * k * 32 + len(recs)] != recs:
                print(f"batched list of query {q} differs from the single-query call's at n = {n}: no numbers")
                return False
    return True


def measure(dev, calls, n, nqs, k, reps):
    rows = []
    for nq in nqs:
        fa, fb, fc = (lambda: calls.a(nq, n, k)), (lambda: calls.b(nq, n)), (lambda: calls.c(nq, n, k))
        warm_until, w = time.perf_counter() + WARM_S, 0
        while w < 3 or time.perf_counter() < warm_until:  # every shape, and long enough for the clocks to settle
            fa(), fb(), fc()
            w += 1
        ts = ([], [], [])
        fs = (fa, fb, fc)
        for i in range(reps):  # interleaved, the order rotated so that no side always follows the same other
            for j in range(3):
                s = (i + j) % 3
                ts[s].append(timed(fs[s]))
        ta, tb, tc = ts
        da, la = device_ms(dev, fa, ("masks_batch_topk", "masks_topk", "topk_merge"))
        db_, _ = device_ms(dev, fb, ("masks_batch_resolve", "masks_resolve", "reduce"))
        ma, mb, mc = (float(np.median(x)) * 1e3 for x in (ta, tb, tc))
        rows.append({"nq": nq, "a": ma, "b": mb, "c": mc, "sa": spread(ta), "sb": spread(tb), "sc": spread(tc),
                     "da": sum(da.values()), "merge": da["topk_merge"], "db": sum(db_.values()), "launches": la})
    return rows


def show(title, n, k, rows, strict):
    print(f"\n{title}: n = {n} masks, k = {k}")
    print(" nq   (a) ms  spread   (b) ms  spread   (c) ms  spread   (a)/(b)  (a)/(c)   device (a)  its merge  device (b)"
          "   (a)'s launches")
    for r in rows:
        print(f"{r['nq']:3d}  {r['a']:7.3f}  {r['sa']:6.1%}  {r['b']:7.3f}  {r['sb']:6.1%}  "
              f"{r['c']:7.3f}  {r['sc']:6.1%}  {r['a'] / r['b']:8.4f}  {r['a'] / r['c']:7.4f}  {r['da']:10.3f}  "
              f"{r['merge']:9.3f}  {r['db']:10.3f}   {r['launches']}")
    if strict:
        bad = [r["nq"] for r in rows if not r["a"] < r["c"] * (1 - r["sc"])]
        print(f"condition (a) < (c) x (1 - spread(c)), every nq: {'holds' if not bad else f'FAILS at nq = {bad}'}")
    else:
        bad = [r["nq"] for r in rows if r["a"] > r["c"] * (1 + r["sc"])]
        print(f"condition (a) <= (c) x (1 + spread(c)), every nq: {'holds' if not bad else f'FAILS at nq = {bad}'}")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 15, 15)
    small = 20_000
    nqm = max(NQS)
    dev = ih.Device(0)
    lib = ih.load_library()
    db = ih.Database(dev, ih.KIND_MASKS, n, ih.LAYOUT_TILES)
    db.generate(n, 7)
    queries = np.random.default_rng(3).integers(0, 2**64, (nqm, ih.LIMBS), dtype=np.uint64)
    singles = [ih.MasksEngine(dev, q) for q in queries]
    batches = {nq: ih.MasksBatchEngine(dev, queries[:nq]) for nq in NQS}
    slab_bytes = nqm * n * ROT * 2
    share_ptrs = []
    for p in range(PARTS):  # one array per part, filled with a repeated block of random u16
        ptr = dev.alloc(slab_bytes)
        rows = np.random.default_rng(p).integers(0, 2**16, 1 << 24, dtype=np.uint16)
        for off in range(0, slab_bytes, rows.nbytes):
            dev.h2d(ptr + off, rows[:min(rows.size, (slab_bytes - off) // 2)])
        share_ptrs.append(ptr)
    calls = Calls(lib, db, batches, singles, share_ptrs, nqm)

    if not check_results(calls, nqm, (small, min(n, 300_000))):
        return 1
    print(f"results: {nqm} batched lists and counts equal the single-query calls' at n = {small} and {min(n, 300_000)}")
    print(f"library: {lib.iris_version().decode()}", flush=True)

    for k in KS:
        show("large range", n, k, measure(dev, calls, n, NQS, k, reps), True)
        sys.stdout.flush()
    for k in KS:
        show("resolver chunk", small, k, measure(dev, calls, small, NQS, k, max(reps, 51)), False)
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
