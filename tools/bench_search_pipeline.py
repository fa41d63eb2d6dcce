"""Measurement: the pipelined search loop in its steady state.

bench.py's pipelined workload -- the next search is submitted before the previous one is waited
for, so every other pass hosts the search after it -- over resident templates, but 200 steps per
repetition after ~3 s of untimed loops instead of 20 steps: the package sits at its power cap
throughout, which tools/bench_search_share.py's pairs (a 300-us spin and a wait between them) do
not reach.  Per repetition: wall time per step, the search launches' device time per step (HIP
events), and the tile groups carried for guests per registration as a share of one pass.  Every
result is checked against the planted record.

usage: python tools/bench_search_pipeline.py [n=10000000] [steps=200] [reps=3]"""
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "mpc-iris-code_amd"))
import numpy as np  # noqa: E402

import iris_hip as ih  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
dev = ih.Device(0)
print(f"library: {ih.load_library().iris_version().decode()}")
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
            p = e.search_async(db)
        if pend is not None:
            got.append(pend.wait())
        pend = p
    got.append(pend.wait())
    return got


t0 = time.perf_counter()
while time.perf_counter() - t0 < 3.0:
    loop(50)
dev.set_profiling(True)
for rep in range(reps):
    dev.reset_stats()
    t0 = time.perf_counter()
    got = loop(steps)
    dt = (time.perf_counter() - t0) * 1e3
    assert all(m.index == sites[i % 16] for i, m in enumerate(got))
    launches, total, _ = dev.kernel_stats("template_search")
    regs, _, carried = dev.kernel_stats("search_shared")
    print(f"rep {rep}: {dt / steps:.4f} ms/step wall, search launches {launches}, device {total / steps:.4f} ms/step, "
          f"registered {regs}, carried {carried} = {carried / (regs or 1) / groups:.4f} of a pass per registration")
db.close()
dev.close()
