"""Measurement: one batched MasksEngine / resolver call against the single-query calls it replaces.

On one device, on a generated TILES masks database far past the 256 MiB Infinity Cache (10M records
= 16 GB by default), with the rows left in device memory, for nq in 2, 3, 4, 5, 8, 16 and two forms:

  rows     (a) one iris_masks_batch_process_device call of a MasksBatchEngine of nq queries;
           (b) nq back-to-back iris_engine_batch_process_device calls on nq prebuilt MasksEngines.
  resolve  (a) one iris_resolver_batch_search_masks call with 3 parts (query-major device arrays);
           (b) nq back-to-back iris_resolver_search_masks calls, each on its slab of every part.

(b) is the single-query path, unchanged by the batch engine.  Both are timed in the same process,
interleaved (a, b, a, b, ...), after a warm-up of each shape, with a host clock around the blocking
calls; the table gives medians.  The same at n = 20 000 (the resolver's chunk, src/main.rs:511-516).
Before anything is timed the batched rows and matches are compared with the single-query results
at both sizes, and no number is printed if they differ.  The share arrays hold random u16 values (a
32-MB block, repeated): the resolve kernels' time does not depend on them.

Columns: records x queries / s of (a); (b)/(a); the spread of each side in this run ((max - min) /
median of its repetitions: (b)'s is the margin of the "not slower" condition); the device time of (a)'s
launches from kernel_stats("masks_batch" / "masks_batch_resolve", plus the single-query names for
left-over queries and small ranges; HIP events, taken in a separate pass); the HBM fraction of (a):
the bytes the call has to move (1600 B per record and database pass -- ceil(nq / 4) passes, or nq
where the dispatch runs single-query launches -- plus 62 B per record and query written, or 3 x 62
read) over the 8 TB/s peak; and the fraction of the dense fp4 MFMA peak (200 MFMAs of 2 x 32 x 32 x 64
operations per tile and query over 10.0e15 ops/s).

usage: python tools/bench_masks_batch.py [n=10000000] [reps=9]"""
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402

HBM_PEAK = 8.0e12    # B/s (MI355X spec)
FP4_PEAK = 10.0e15   # dense fp4 ops/s (spec sheet)
NQS = (2, 3, 4, 5, 8, 16)
ROT = 31
PARTS = 3
SPLIT_TILES = 1024   # ranges of more tiles run the batch kernel (csrc/iris_masks_batch.hip)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def spread(ts):
    return (max(ts) - min(ts)) / float(np.median(ts))


def measure(dev, db, n, singles, batches, out_ptr, share_ptrs, form, reps):
    rows = []
    batch_runs = (n + 31) // 32 > SPLIT_TILES
    for nq in NQS:
        eng = batches[nq]
        slab = n * ROT * 2
        if form == "rows":
            def a():
                eng.batch_process_device(db, out_ptr, first=0, n=n)

            def b():
                for q in range(nq):
                    singles[q].batch_process_device(db, out_ptr + q * slab, first=0, n=n)
        else:
            def a():
                eng.resolve(db, share_ptrs, first=0, n=n)

            def b():
                for q in range(nq):
                    singles[q].resolve(db, [p + q * slab for p in share_ptrs], first=0, n=n)

        for _ in range(2):  # warm-up of both
            a()
            b()
        ta, tb = [], []
        for _ in range(reps):  # interleaved
            ta.append(timed(a))
            tb.append(timed(b))
        dev.reset_stats()  # device time in a pass of its own
        dev.set_profiling(True)
        for _ in range(3):
            a()
        dev.set_profiling(False)
        names = ("masks_batch", "masks") if form == "rows" else ("masks_batch_resolve", "masks_resolve", "reduce")
        stats = {k: dev.kernel_stats(k) for k in names}
        kms = sum(s[1] for s in stats.values()) / 3
        batch_launches = stats[names[0]][0] // 3
        ma, mb = float(np.median(ta)), float(np.median(tb))
        passes = (nq + 3) // 4 if batch_runs else nq
        moved = n * (1600 * passes + 62 * nq * (1 if form == "rows" else PARTS))
        rows.append({
            "nq": nq, "a_ms": ma * 1e3, "b_ms": mb * 1e3, "rate": n * nq / ma, "ratio": mb / ma,
            "b_spread": spread(tb), "a_spread": spread(ta), "kernel_ms": kms, "batch_launches": batch_launches,
            "hbm": moved / ma / HBM_PEAK, "mfma": (n / 32) * nq * 200 * 2 * 32 * 32 * 64 / ma / FP4_PEAK,
        })
    return rows


def show(title, n, rows):
    print(f"\n{title}: n = {n} masks ({n * 1600 / 1e9:.3f} GB)")
    print(" nq   batch ms  singles ms   rec*q/s    (b)/(a)  spread(b)  spread(a)  device ms  batch launches  HBM frac"
          "  fp4 frac")
    for r in rows:
        print(f"{r['nq']:3d}  {r['a_ms']:9.3f}  {r['b_ms']:10.3f}  {r['rate']:9.3e}  {r['ratio']:8.2f}  "
              f"{r['b_spread']:8.1%}  {r['a_spread']:9.1%}  {r['kernel_ms']:9.3f}  {r['batch_launches']:14d}  "
              f"{r['hbm']:8.3f}  {r['mfma']:8.3f}")
    worst = min(r["ratio"] * (1 + r["b_spread"]) for r in rows)
    print(f"condition (batched not slower than the singles, within the spread of (b)): "
          f"{'holds' if worst >= 1.0 else 'FAILS'} (least (b)/(a) with the margin: {worst:.2f})")


def check_results(dev, db, singles, batches, out_ptr, share_ptrs, sizes):
    nq = max(NQS)
    for m in sizes:
        got = np.empty((nq, m, ROT), np.uint16)
        batches[nq].batch_process_device(db, out_ptr, first=0, n=m)
        dev.d2h(got, out_ptr)
        matches = batches[nq].resolve(db, share_ptrs, first=0, n=m)
        one = np.empty((m, ROT), np.uint16)
        for q, eng in enumerate(singles):
            eng.batch_process_device(db, out_ptr, first=0, n=m)
            dev.d2h(one, out_ptr)
            if not (got[q] == one).all():
                print(f"batched rows of query {q} differ from the single-query engine's at n = {m}: no numbers")
                return False
            s = eng.resolve(db, [p + q * m * ROT * 2 for p in share_ptrs], first=0, n=m)
            b = matches[q]
            if (s.index, s.rotation, s.num, s.den) != (b.index, b.rotation, b.num, b.den):
                print(f"batched match of query {q} differs from the single-query call's at n = {m}: no numbers")
                return False
    return True


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    small = 20_000
    nqm = max(NQS)
    dev = ih.Device(0)
    db = ih.Database(dev, ih.KIND_MASKS, n, ih.LAYOUT_TILES)
    db.generate(n, 7)
    queries = np.random.default_rng(3).integers(0, 2**64, (nqm, ih.LIMBS), dtype=np.uint64)
    singles = [ih.MasksEngine(dev, q) for q in queries]
    batches = {nq: ih.MasksBatchEngine(dev, queries[:nq]) for nq in NQS}
    slab_bytes = nqm * n * ROT * 2
    out_ptr = dev.alloc(slab_bytes)
    # share arrays: one per part, filled with a repeated block of random u16
    share_ptrs = []
    for p in range(PARTS):
        ptr = dev.alloc(slab_bytes)
        rows = np.random.default_rng(p).integers(0, 2**16, 1 << 24, dtype=np.uint16)
        for off in range(0, slab_bytes, rows.nbytes):
            chunk = rows[:min(rows.size, (slab_bytes - off) // 2)]
            dev.h2d(ptr + off, chunk)
        share_ptrs.append(ptr)

    if not check_results(dev, db, singles, batches, out_ptr, share_ptrs, (small, min(n, 300_000))):
        return 1
    print(f"results: {nqm} batched slabs and matches equal the single-query calls' at n = {small} and "
          f"{min(n, 300_000)}")
    print(f"library: {ih.load_library().iris_version().decode()}")

    for form in ("rows", "resolve"):
        big = measure(dev, db, n, singles, batches, out_ptr, share_ptrs, form, reps)
        show(f"large range, {form}", n, big)
        r = big[0]
        print(f"box check: {r['nq']} single-query {form} calls {r['b_ms']:.3f} ms for {n} masks = "
              f"{r['b_ms'] / r['nq'] * 1e7 / n:.2f} ms per 10M and query")
    for form in ("rows", "resolve"):
        show(f"resolver chunk, {form}", small,
             measure(dev, db, small, singles, batches, out_ptr, share_ptrs, form, max(reps, 101)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
