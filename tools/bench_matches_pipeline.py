"""Measurement: threshold-match lists for a query stream, after
tools/bench_search_pipeline.py.

One loop per process over resident generated templates, 16 queries in turn, each a perturbed copy
of one record (its only record under threshold 0.3), a new engine per step as bench.py builds one:

  blocking  TemplateEngine.matches(): every call streams the database and waits
  async     TemplateEngine.matches_async(): step i + 1 is submitted before step i is waited for,
            so a running pass may compute the next one (IRIS_TEST_HOOKS=1 IRIS_SEARCH_SHARE=0 in
            the environment: the same pipeline, never shared)
  search    TemplateEngine.search_async(), pipelined the same way: the argmin only, for scale

~2 s of untimed loops, then `steps` timed steps: wall time per step, the passes' device time per
step (HIP events) and, for async, the tile groups carried per registration as a share of one pass.
Every list is checked against the planted record.  Prints one JSON line.

usage: python tools/bench_matches_pipeline.py blocking|async|search [n=10000000] [steps=200]"""
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
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
THRESHOLD = 0.3
dev = ih.Device(0)
db = ih.Database(dev, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES)
db.generate(n, 42)
rng = np.random.default_rng(5)
sites = [int(x) for x in rng.choice(n, 16, replace=False)]
qs = []
for k, s in enumerate(sites):
    q = db.read(s, 1)[0].copy()
    q[1 + k] ^= np.uint64(0x00FF00FF00FF00FF)
    qs.append(q)
groups = -(-(-(-n // 32)) // 16)


def loop(count):
    got, pend = [], None
    for i in range(count):
        with ih.TemplateEngine(dev, qs[i % 16]) as e:
            if mode == "blocking":
                got.append(e.matches(db, THRESHOLD))
                continue
            p = e.matches_async(db, THRESHOLD) if mode == "async" else e.search_async(db)
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
    else:
        assert ([m.index for m in r[0]], r[1]) == ([sites[i % 16]], 1)
kernel = "template_search" if mode == "search" else "template_match"
launches, total, _ = dev.kernel_stats(kernel)
regs, _, carried = dev.kernel_stats("search_shared" if mode == "search" else "match_shared")
cfg = dev.config()
print(json.dumps({"mode": mode, "share": cfg.get("search_share", "1"), "n": n, "steps": steps,
                  "wall_ms_per_step": round(dt / steps, 4), "launches": launches,
                  "device_ms_per_step": round(total / steps, 4), "registered": regs,
                  "pass_share_per_registration": round(carried / (regs or 1) / groups, 4),
                  "library": ih.load_library().iris_version().decode()}))
db.close()
dev.close()
