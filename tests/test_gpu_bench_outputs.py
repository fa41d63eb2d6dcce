"""GPU: `bench.py --dump-outputs DIR` writes what the last timed step returned, and a plain
run (no --full) measures only its headline figure.  The dumped arrays are checked against the
CPU oracle over the bench's own seeded inputs, so two builds that both pass wrote the same files."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]
N = 70_001  # odd, and more than bench.DUMP_ROWS: the per-record dump is a sample


def _run(tmp_path, *extra):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--n-per-gpu",
           str(N), "--prewarm-s", "0", "--dump-outputs", str(tmp_path / "out"), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    (line,) = [l for l in r.stdout.splitlines() if l.startswith("{")]
    d = json.loads(line)
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["check"]["ok"]
    assert d["cpu_baseline"] is None and "ms_per_step_unprofiled" not in d  # those are --full's
    files = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    return d, files


def test_search_dump_is_the_oracle_argmin(tmp_path):
    import bench

    d, files = _run(tmp_path)
    assert set(files) == {"match"}
    query = oc.gen_templates(bench.SEED + 1, 0, 1)[0]
    db = oc.gen_templates(bench.SEED, 0, N)
    site = bench.plant_sites(N, 1)[0]
    db[site] = bench.planted_record(query, 9)
    dist, idx = oc.argmin(oc.template_distances(query, db))
    m = dict(zip(bench.MATCH_FIELDS, files["match"]))
    assert idx == site and m["index"] == idx and m["rotation"] == 9
    assert np.float64(m["distance"]).view(np.uint64) == np.float64(dist).view(np.uint64)
    assert d["check"]["found_index"] == idx and d["check"]["distance"] == dist


def test_masks_dump_is_a_seeded_sample_of_the_oracle_rows(tmp_path):
    import bench

    _, files = _run(tmp_path, "--workload", "masks")
    assert set(files) == {"rows", "row_indices"}
    rows = bench.dump_rows(N)
    assert len(rows) == bench.DUMP_ROWS and (np.diff(rows) > 0).all() and rows[-1] < N
    assert (rows == bench.dump_rows(N)).all()  # the same sample on every run
    assert (files["row_indices"] == rows).all()
    qmask = oc.gen_templates(bench.SEED + 1, 0, 1)[0][200:]
    want = oc.masks_batch(qmask, oc.gen_masks(bench.SEED, 0, N))
    assert files["rows"].shape == (bench.DUMP_ROWS, 31)
    assert (files["rows"] == want[rows]).all()
