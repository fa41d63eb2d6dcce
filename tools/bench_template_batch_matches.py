"""Measurement: template batch threshold matching (iris_template_batch_matches) against the batched
search it is the sibling of and against the single-query match calls it replaces.

On one device, in one process, on a generated TILES template database far past the Infinity Cache
(10M records by default), for nq in 4, 16, 64, 1024 generated queries:

  (a) one iris_template_batch_matches call of a TemplateBatchEngine of nq queries;
  (b) one iris_template_batch_search call on the same engine;
  (c) nq back-to-back iris_template_matches calls on nq prebuilt TemplateEngines.

All three are timed in the same run, interleaved with the order rotated every repetition (a b c,
b c a, c a b, ...) after a warm-up of each shape, with a host clock around the blocking C calls
(output buffers allocated once, outside the clock); the table gives medians and each call's own
spread ((max - min) / median of its repetitions).  Repetitions: `reps` (default 9) up to 16 queries,
5 at 64, 3 at 1024, where one call takes seconds; warm-up rounds 3, 2 and 1.  Two thresholds: 0.0
(every list empty) and 0.35 with 1 + q % 8 near-copies of query q written into the database at
scattered records (every list 1..8 records; generated templates lie near 0.47-0.49 from any query).
The device time of (a)'s and (b)'s launches comes from kernel_stats (HIP events, a pass of its own).

The yardstick is (b), code the match form leaves alone: (a)'s median should lie within (b)'s own
spread of (b)'s median.  (a) / (c) is reported for every nq.

threshold = +inf is timed once (16 queries, cap = 10: every list holds every record, all four
blocks run twice with their regions grown to the counts) and only reported, with its device share.

Before anything is timed the batched lists and counts at 0.35 are compared, byte for byte, with the
single-query calls' for 16 and for 64 queries; no number is printed if they differ.

usage: python tools/bench_template_batch_matches.py [n=10000000] [reps=9]"""
import ctypes
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402

NQS = (4, 16, 64, 1024)
CAP = 16
SPARSE = 0.35
INF = float("inf")


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
        self.out = (ih.Match * (nqmax * CAP))()
        self.one = (ih.Match * CAP)()
        self.best = (ih.Match * nqmax)()
        self.counts = (ctypes.c_uint64 * nqmax)()
        self.count = ctypes.c_uint64()

    def a(self, nq, n, t, cap=CAP):
        rc = self.lib.iris_template_batch_matches(self.batches[nq].handle, self.db.handle, 0, n, 0, t,
                                                  self.out if cap else None, cap, self.counts)
        assert rc == 0, (rc, self.lib.iris_last_error())

    def b(self, nq, n):
        rc = self.lib.iris_template_batch_search(self.batches[nq].handle, self.db.handle, 0, n, 0, self.best)
        assert rc == 0, (rc, self.lib.iris_last_error())

    def c(self, nq, n, t, keep=None):
        for q in range(nq):
            rc = self.lib.iris_template_matches(self.singles[q].handle, self.db.handle, 0, n, 0, t, self.one, CAP,
                                                ctypes.byref(self.count))
            assert rc == 0, (rc, self.lib.iris_last_error())
            if keep is not None:
                keep.append((self.count.value, bytes(self.one)[:32 * min(self.count.value, CAP)]))


def device_ms(dev, fn, names, reps):
    dev.reset_stats()
    dev.set_profiling(True)
    for _ in range(reps):
        fn()
    dev.set_profiling(False)
    stats = {k: dev.kernel_stats(k) for k in names}
    return sum(s[1] for s in stats.values()) / reps, {k: s[0] // reps for k, s in stats.items() if s[0]}


def check_results(calls, n, nqs):
    for nq in nqs:
        singles = []
        calls.c(nq, n, SPARSE, singles)
        calls.a(nq, n, SPARSE)
        raw = bytes(calls.out)
        for q, (count, recs) in enumerate(singles):
            if count != 1 + q % 8:
                print(f"query {q} has {count} matches under {SPARSE}, planted {1 + q % 8}: not the inputs this tool expects")
                return False
            if calls.counts[q] != count or raw[q * CAP * 32:q * CAP * 32 + len(recs)] != recs:
                print(f"batched list of query {q} of {nq} differs from the single-query call's: no numbers")
                return False
    return True


def measure(dev, calls, n, nqs, t, reps):
    rows = []
    for nq in nqs:
        fa, fb, fc = (lambda: calls.a(nq, n, t)), (lambda: calls.b(nq, n)), (lambda: calls.c(nq, n, t))
        warm, r = schedule(nq, reps)
        for _ in range(warm):
            fa(), fb(), fc()
        ts = ([], [], [])
        fs = (fa, fb, fc)
        for i in range(r):  # interleaved, the order rotated so that no call always follows the same other
            for j in range(3):
                k = (i + j) % 3
                ts[k].append(timed(fs[k]))
        ta, tb, tc = ts
        dreps = 3 if nq <= 64 else 1
        da, la = device_ms(dev, fa, ("template_batch_match", "template_match"), dreps)
        db_, _ = device_ms(dev, fb, ("template_batch",), dreps)
        ma, mb, mc = (float(np.median(x)) * 1e3 for x in (ta, tb, tc))
        rows.append({"nq": nq, "reps": r, "a": ma, "b": mb, "c": mc, "sa": spread(ta), "sb": spread(tb), "sc": spread(tc),
                     "da": da, "db": db_, "launches": la, "matches": sum(calls.counts[:nq])})
    return rows


def show(n, t, rows):
    print(f"\nn = {n} templates, threshold {t!r}")
    print("  nq reps  matches    (a) ms  spread    (b) ms  spread    (c) ms  spread   (a)/(b)  (a)/(c)   device (a)  device (b)"
          "   (a)'s launches")
    for r in rows:
        print(f"{r['nq']:4d}  {r['reps']:3d}  {r['matches']:7d}  {r['a']:8.3f}  {r['sa']:6.1%}  {r['b']:8.3f}  {r['sb']:6.1%}  "
              f"{r['c']:8.3f}  {r['sc']:6.1%}  {r['a'] / r['b']:8.4f}  {r['a'] / r['c']:7.4f}  {r['da']:10.3f}  "
              f"{r['db']:10.3f}   {r['launches']}")
    out = [(r["nq"], r["a"] / r["b"] - 1, r["sb"]) for r in rows if abs(r["a"] / r["b"] - 1) > r["sb"]]
    print("(a)'s median within (b)'s spread of (b)'s median, every nq: " +
          ("yes" if not out else "NO: " + ", ".join(f"nq = {q}: {d:+.1%} against a spread of {s:.1%}" for q, d, s in out)))
    slow = [r["nq"] for r in rows if r["a"] > r["c"]]
    print("(a) faster than the nq single calls (c), every nq: " + ("yes" if not slow else f"NO at nq = {slow}"))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    nqm = max(NQS)
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
    batches = {nq: ih.TemplateBatchEngine(dev, queries[:nq]) for nq in NQS}
    calls = Calls(lib, db, batches, singles, nqm)

    if not check_results(calls, n, (16, 64)):
        return 1
    print(f"results: the batched lists and counts of 16 and of 64 queries equal the single-query calls' at n = {n}")
    print(f"library: {lib.iris_version().decode()}")
    print(f"device: {dev.config()}")

    for t in (0.0, SPARSE):
        show(n, t, measure(dev, calls, n, NQS, t, reps))

    # +inf, once: reported only
    dev.reset_stats()
    dev.set_profiling(True)
    t0 = time.perf_counter()
    calls.a(16, n, INF, 10)
    wall = (time.perf_counter() - t0) * 1e3
    dev.set_profiling(False)
    launches, kms, _ = dev.kernel_stats("template_batch_match")
    print(f"\n+inf, 16 queries, cap = 10 (reported only): counts {sorted(set(calls.counts[:16]))}; {wall:.1f} ms per call, "
          f"{launches} launches of the batch kernel, device {kms:.3f} ms ({kms / wall:.1%}); the rest is the host's: the copy "
          f"back of 24 B per match and the partial sort by index")
    return 0


if __name__ == "__main__":
    sys.exit(main())
