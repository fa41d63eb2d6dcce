"""Measurement: the match list, the k closest records and the histogram of every probe of a query
stream, after tools/bench_topk_pipeline.py.

One loop per process over resident generated templates, 16 queries in turn, each a perturbed copy
of one record (entry 0 of its list, its one match), a new engine per step as bench.py builds one:

  blocking  TemplateEngine.report(): every call streams the database, merges, reduces and waits
  async     TemplateEngine.report_async(): step i + 1 is submitted before step i is waited for, so a
            running report pass may feed the next one's sinks (IRIS_TEST_HOOKS=1 IRIS_SEARCH_SHARE=0
            in the environment: the same pipeline, never shared, the blocking call's kernel)
  search    TemplateEngine.search_async(), pipelined the same way: the argmin only, for scale

parts: all (matches at a threshold of 0.3 with cap 16, top-k, 1024 bins), hist (1024 bins alone) or
mt (matches and top-k).  ~2 s of untimed loops, then `steps` timed steps: wall time per step, the
passes' device time per step (HIP events) and, for async, the share of passes that registered and
the tile groups carried per registration as a share of one pass.  Every result is checked: the
planted record heads the list and is the one match, the histogram adds up to n.
Prints one JSON line.

usage: python tools/bench_report_pipeline.py blocking|async|search [parts=all] [k=16] [n=10000000] [steps=200]"""
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else ""
assert mode in ("blocking", "async", "search"), __doc__
parts = sys.argv[2] if len(sys.argv) > 2 else "all"
assert parts in ("all", "hist", "mt"), __doc__
k = int(sys.argv[3]) if len(sys.argv) > 3 else 16
n = int(sys.argv[4]) if len(sys.argv) > 4 else 10_000_000
steps = int(sys.argv[5]) if len(sys.argv) > 5 else 200
args = dict(threshold=0.3 if parts != "hist" else None, cap=16 if parts != "hist" else None,
            k=k if parts != "hist" else None, nbins=1024 if parts != "mt" else None)
dev = ih.Device(0)
db = ih.Database(dev, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES)
db.generate(n, 42)
rng = np.random.default_rng(5)
sites = [int(x) for x in rng.choice(n, 16, replace=False)]
qs = []
for j, s in enumerate(sites):
    q = db.read(s, 1)[0].copy()
    q[1 + j] ^= np.uint64(0x00FF00FF00FF00FF)
    qs.append(q)
groups = -(-(-(-n // 32)) // 16)


def loop(count):
    got, pend = [], None
    for i in range(count):
        with ih.TemplateEngine(dev, qs[i % 16]) as e:
            if mode == "blocking":
                got.append(e.report(db, **args))
                continue
            p = e.report_async(db, **args) if mode == "async" else e.search_async(db)
        if pend is not None:
            got.append(pend.wait())
        pend = p
    if pend is not None:
        got.append(pend.wait())
    return got


t0 = time.perf_counter()
while time.perf_counter() - t0 < 2.0:
    loop(50)
dev.set_profiling(True)
dev.reset_stats()
t0 = time.perf_counter()
got = loop(steps)
dt = (time.perf_counter() - t0) * 1e3
for i, r in enumerate(got):
    if mode == "search":
        assert r.index == sites[i % 16]
        continue
    if parts != "hist":
        d = [m.distance for m in r.topk]
        assert len(r.topk) == k and r.topk[0].index == sites[i % 16] and d == sorted(d)
        assert r.matches_count == 1 and r.matches[0].index == sites[i % 16]
    if parts != "mt":
        assert int(r.bins.sum()) + r.invalid == n
names = ("template_search",) if mode == "search" else ("template_report", "template_match", "template_topk", "template_hist")
launches = sum(dev.kernel_stats(x)[0] for x in names)
total = sum(dev.kernel_stats(x)[1] for x in names)
after_ms = 0.0 if mode == "search" else dev.kernel_stats("topk_merge")[1] + dev.kernel_stats("hist_reduce")[1]
regs, _, carried = dev.kernel_stats("search_shared" if mode == "search" else "report_shared")
cfg = dev.config()
print(json.dumps({"mode": mode, "parts": parts, "k": k, "share": cfg.get("search_share", "1"), "n": n, "steps": steps,
                  "wall_ms_per_step": round(dt / steps, 4), "launches": launches,
                  "device_ms_per_step": round(total / steps, 4), "merge_reduce_ms_per_step": round(after_ms / steps, 4),
                  "registered": regs, "registered_share": round(regs / steps, 4),
                  "pass_share_per_registration": round(carried / (regs or 1) / groups, 4),
                  "library": ih.load_library().iris_version().decode()}))
db.close()
dev.close()
