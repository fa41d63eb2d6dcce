"""Measurement: one batched DistanceEngine call against the single-query calls it replaces.

On one device, on a generated TILES share database far past the 256 MiB Infinity Cache (2M records
= 51 GB by default), with the rows left in device memory, for nq in 1, 2, 4, 8, 16:

  (a) one iris_distance_batch_process_device call of a DistanceBatchEngine of nq queries;
  (b) nq back-to-back iris_engine_batch_process_device calls on nq prebuilt DistanceEngines
      (the single-query path, unchanged by the batch engine).

Both are timed in the same process, interleaved (a, b, a, b, ...), after a warm-up of each, with a
host clock around the blocking calls; the table gives medians.  The same at n = 20 000 (a
participant's chunk, src/main.rs:427-431).  Before anything is timed one batched result is compared
with the single-query results, and no number is printed if they differ.

Columns: records x queries / s of (a); (b)/(a); the spread of (b) in this run ((max - min) / median
of its repetitions: the margin of the "not slower" condition); the kernel ms of (a) from
kernel_stats("shares_batch") (HIP events, taken in a separate pass); the HBM fraction of (a),
n x 25 600 B / t over the 8 TB/s peak; and the fraction of the dense i8 MFMA peak (2 x 32 x 32 x
32 x 1200 ops per tile and query over 5.0e15 ops/s: tools/ubench_mfma.hip gives the bare rate).

usage: python tools/bench_shares_batch.py [n=2000000] [reps=11]"""
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402

HBM_PEAK = 8.0e12   # B/s (MI355X spec)
I8_PEAK = 5.0e15    # dense i8 ops/s (spec sheet)
NQS = (1, 2, 4, 8, 16)
ROT = 31


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def measure(dev, db, n, singles, batches, out_ptr, reps):
    rows = []
    for nq in NQS:
        eng = batches[nq]

        def a():
            eng.batch_process_device(db, out_ptr, first=0, n=n)

        def b():
            for q in range(nq):
                singles[q].batch_process_device(db, out_ptr + q * n * ROT * 2, first=0, n=n)

        for _ in range(2):  # warm-up of both
            a()
            b()
        ta, tb = [], []
        for _ in range(reps):  # interleaved
            ta.append(timed(a))
            tb.append(timed(b))
        dev.reset_stats()  # kernel time in a pass of its own
        dev.set_profiling(True)
        for _ in range(3):
            a()
        dev.set_profiling(False)
        launches, kms, _items = dev.kernel_stats("shares_batch")
        ma, mb = float(np.median(ta)), float(np.median(tb))
        rows.append({
            "nq": nq, "a_ms": ma * 1e3, "b_ms": mb * 1e3, "rate": n * nq / ma, "ratio": mb / ma,
            "b_spread": (max(tb) - min(tb)) / mb, "a_spread": (max(ta) - min(ta)) / ma,
            "kernel_ms": kms / max(1, launches), "hbm": n * 25600 / ma / HBM_PEAK,
            "mfma": (n / 32) * nq * 1200 * 2 * 32 * 32 * 32 / ma / I8_PEAK,
        })
    return rows


def show(title, n, rows):
    print(f"\n{title}: n = {n} shares ({n * 25600 / 1e9:.2f} GB), rows in device memory")
    print(" nq   batch ms  singles ms   rec*q/s    (b)/(a)  spread(b)  spread(a)  kernel ms   HBM frac  i8 frac")
    for r in rows:
        print(f"{r['nq']:3d}  {r['a_ms']:9.3f}  {r['b_ms']:10.3f}  {r['rate']:9.3e}  {r['ratio']:8.2f}  "
              f"{r['b_spread']:8.1%}  {r['a_spread']:9.1%}  {r['kernel_ms']:9.3f}  {r['hbm']:9.3f}  {r['mfma']:7.3f}")
    worst = min(r["ratio"] * (1 + r["b_spread"]) for r in rows)
    print(f"condition (batched not slower than the singles, within the spread of (b)): "
          f"{'holds' if worst >= 1.0 else 'FAILS'} (least (b)/(a) with the margin: {worst:.2f})")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
    small = 20_000
    dev = ih.Device(0)
    db = ih.Database(dev, ih.KIND_SHARES, n, ih.LAYOUT_TILES)
    db.generate(n, 7)
    queries = np.random.default_rng(3).integers(0, 1 << 16, (max(NQS), ih.BITS), dtype=np.uint16)
    singles = [ih.DistanceEngine(dev, q) for q in queries]
    batches = {nq: ih.DistanceBatchEngine(dev, queries[:nq]) for nq in NQS}
    out_ptr = dev.alloc(max(NQS) * n * ROT * 2)

    # results first: the batch of 16 against the 16 single-query engines, at both sizes
    for m in (small, min(n, 300_000)):
        got = np.empty((max(NQS), m, ROT), np.uint16)
        batches[max(NQS)].batch_process_device(db, out_ptr, first=0, n=m)
        dev.d2h(got, out_ptr)
        one = np.empty((m, ROT), np.uint16)
        for q, eng in enumerate(singles):
            eng.batch_process_device(db, out_ptr, first=0, n=m)
            dev.d2h(one, out_ptr)
            if not (got[q] == one).all():
                print(f"batched rows of query {q} differ from the single-query engine's at n = {m}: no numbers")
                return 1
    print(f"results: 16 batched slabs equal the single-query engines' rows at n = {small} and {min(n, 300_000)}")
    print(f"library: {ih.load_library().iris_version().decode()}")

    big = measure(dev, db, n, singles, batches, out_ptr, reps)
    show("large range", n, big)
    r1 = big[0]
    print(f"box check: one single-query pass {r1['b_ms']:.3f} ms for {n} shares = "
          f"{r1['b_ms'] * 1e7 / n:.2f} ms per 10M (VERDICT: 37.2-37.5)")
    show("participant chunk", small, measure(dev, db, small, singles, batches, out_ptr, max(reps, 101)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
