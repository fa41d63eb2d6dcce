"""Measurement: template batch top-k (iris_template_batch_topk) against the batched search it is
the sibling of and against the single-query top-k calls it replaces.

On one device, in one process, on a generated TILES template database far past the Infinity Cache
(10M records by default), for nq in 4, 16, 64 generated queries x k in 1, 16, 64, and for 1024
queries at k = 16:

  (a) one iris_template_batch_topk call of a TemplateBatchEngine of nq queries;
  (b) one iris_template_batch_search call on the same engine;
  (c) nq back-to-back iris_template_topk calls on nq prebuilt TemplateEngines.

All three are timed in the same run, interleaved with the order rotated every repetition (a b c,
b c a, c a b, ...) after a warm-up of each shape, with a host clock around the blocking C calls
(output buffers allocated once, outside the clock); the table gives medians and each call's own
spread ((max - min) / median of its repetitions).  Repetitions: `reps` (default 9) up to 16 queries,
5 at 64, 3 at 1024, where one call takes seconds; warm-up rounds 3, 2 and 1.  1 + q % 8 near-copies
of query q are written into the database at scattered records, so every list starts with known
records (generated templates lie near 0.47-0.49 from any query).  The device time of (a)'s and (b)'s
launches comes from kernel_stats (HIP events, a pass of its own), (a)'s split into the pass and the
merge levels.

Required: (a) is faster than (c) by more than (c)'s own spread, for every (nq, k).  (a) / (b) is
reported, on device times too.

Before anything is timed the batched lists and counts at k = 16 are compared, byte for byte, with the
single-query calls' for 16 and for 64 queries; no number is printed if they differ.

usage: python tools/bench_template_batch_topk.py [n=10000000] [reps=9] [nq,nq,...] [k,k,...]"""
import ctypes
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402

NQS = (4, 16, 64, 1024)
KS = (1, 16, 64)
K_WIDE = 16  # the one k of 1024 queries
KMAX = 64


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def spread(ts):
    return (max(ts) - min(ts)) / float(np.median(ts))


def schedule(nq, reps):
    """(warm-up rounds, repetitions) of one shape."""
    if nq <= 16:
        return 3, reps
    return (2, 5) if nq <= 64 else (1, 3)


class Calls:
    """The three C calls over [0, n) for the first nq queries, into buffers allocated once."""

    def __init__(self, lib, db, batches, singles, nqmax):
        self.lib, self.db, self.batches, self.singles = lib, db, batches, singles
        self.out = (ih.Match * (nqmax * KMAX))()
        self.one = (ih.Match * KMAX)()
        self.best = (ih.Match * nqmax)()
        self.counts = (ctypes.c_uint32 * nqmax)()
        self.count = ctypes.c_uint32()

    def a(self, nq, n, k):
        rc = self.lib.iris_template_batch_topk(self.batches[nq].handle, self.db.handle, 0, n, 0, k, self.out, self.counts)
        assert rc == 0, (rc, self.lib.iris_last_error())

    def b(self, nq, n):
        rc = self.lib.iris_template_batch_search(self.batches[nq].handle, self.db.handle, 0, n, 0, self.best)
        assert rc == 0, (rc, self.lib.iris_last_error())

    def c(self, nq, n, k, keep=None):
        for q in range(nq):
            rc = self.lib.iris_template_topk(self.singles[q].handle, self.db.handle, 0, n, 0, k, self.one,
                                             ctypes.byref(self.count))
            assert rc == 0, (rc, self.lib.iris_last_error())
            if keep is not None:
                keep.append((self.count.value, bytes(self.one)[:32 * self.count.value]))


def device_ms(dev, fn, names, reps):
    dev.reset_stats()
    dev.set_profiling(True)
    for _ in range(reps):
        fn()
    dev.set_profiling(False)
    stats = {k: dev.kernel_stats(k) for k in names}
    return {k: s[1] / reps for k, s in stats.items()}, {k: s[0] // reps for k, s in stats.items() if s[0]}


def check_results(calls, n, nqs, k=16):
    for nq in nqs:
        singles = []
        calls.c(nq, n, k, singles)
        calls.a(nq, n, k)
        raw = bytes(calls.out)
        for q, (count, recs) in enumerate(singles):
            if calls.counts[q] != count or raw[q * k * 32:q * k * 32 + len(recs)] != recs:
                print(f"batched list of query {q} of {nq} differs from the single-query call's: no numbers")
                return False
    return True


def measure(dev, calls, n, nq, k, reps):
    fa, fb, fc = (lambda: calls.a(nq, n, k)), (lambda: calls.b(nq, n)), (lambda: calls.c(nq, n, k))
    warm, r = schedule(nq, reps)
    for _ in range(warm):
        fa(), fb(), fc()
    ts = ([], [], [])
    fs = (fa, fb, fc)
    for i in range(r):  # interleaved, the order rotated so that no call always follows the same other
        for j in range(3):
            x = (i + j) % 3
            ts[x].append(timed(fs[x]))
    ta, tb, tc = ts
    dreps = 3 if nq <= 64 else 1
    da, la = device_ms(dev, fa, ("template_batch_topk", "topk_merge"), dreps)
    db_, _ = device_ms(dev, fb, ("template_batch",), dreps)
    ma, mb, mc = (float(np.median(x)) * 1e3 for x in (ta, tb, tc))
    return {"nq": nq, "k": k, "reps": r, "a": ma, "b": mb, "c": mc, "sa": spread(ta), "sb": spread(tb), "sc": spread(tc),
            "pass": da["template_batch_topk"], "merge": da["topk_merge"], "db": db_["template_batch"], "launches": la}


def show(n, rows):
    print(f"\nn = {n} templates")
    print("  nq   k reps    (a) ms  spread    (b) ms  spread    (c) ms  spread   (a)/(b)  (a)/(c)   dev pass  dev merge  merge %"
          "    dev (b)  dev (a)/(b)   (a)'s launches")
    for r in rows:
        dev_a = r["pass"] + r["merge"]
        print(f"{r['nq']:4d}  {r['k']:2d}  {r['reps']:3d}  {r['a']:8.3f}  {r['sa']:6.1%}  {r['b']:8.3f}  {r['sb']:6.1%}  "
              f"{r['c']:8.3f}  {r['sc']:6.1%}  {r['a'] / r['b']:8.4f}  {r['a'] / r['c']:7.4f}  {r['pass']:9.3f}  "
              f"{r['merge']:9.3f}  {r['merge'] / dev_a:7.2%}  {r['db']:9.3f}  {dev_a / r['db']:11.4f}   {r['launches']}")
    slow = [(r["nq"], r["k"]) for r in rows if not r["a"] < r["c"] * (1 - r["sc"])]
    print("(a) faster than the nq single calls (c) by more than (c)'s own spread, every (nq, k): " +
          ("yes" if not slow else f"NO at (nq, k) = {slow}"))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    nqs = tuple(int(x) for x in sys.argv[3].split(",")) if len(sys.argv) > 3 else NQS
    ks = tuple(int(x) for x in sys.argv[4].split(",")) if len(sys.argv) > 4 else KS
    nqm = max(max(nqs), 64)
    dev = ih.Device(0)
    lib = ih.load_library()
    db = ih.Database(dev, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES)
    db.generate(n, 7)
    with ih.Database(dev, ih.KIND_TEMPLATES, nqm, ih.LAYOUT_TILES) as qdb:  # generated queries
        qdb.generate(nqm, 8)
        queries = qdb.read(0, nqm)
    for q in range(nqm):  # 1 + q % 8 near-copies of query q (rotation 0, 16 pattern bits flipped)
        rec = queries[q].copy()
        rec[9] ^= np.uint64(0x0F0F00000F0F)
        for j in range(1 + q % 8):
            db.write((q * 9973 + j * 1_000_003 + 17) % n, rec[None, :])
    singles = [ih.TemplateEngine(dev, q) for q in queries]
    batches = {nq: ih.TemplateBatchEngine(dev, queries[:nq]) for nq in set(nqs) | {16, 64}}
    calls = Calls(lib, db, batches, singles, nqm)

    if not check_results(calls, n, (16, 64)):
        return 1
    print(f"results: the batched lists and counts of 16 and of 64 queries equal the single-query calls' at n = {n}, k = 16")
    print(f"library: {lib.iris_version().decode()}")
    print(f"device: {dev.config()}")

    rows = []
    for nq in nqs:
        for k in ((K_WIDE,) if nq > 64 else ks):
            rows.append(measure(dev, calls, n, nq, k, reps))
    show(n, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
