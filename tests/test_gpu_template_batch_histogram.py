"""GPU: template batch histograms (iris_template_batch_histogram): every query's distance histogram
in one pass, against np.bincount of the CPU oracle's binned f64 distances (tests/hist_fixtures.py)
and, byte for byte, against the single-query iris_template_histogram calls it replaces.

Variants: engines of up to 3 queries run one single-query pass per query (TILES and LANES
databases); more run the batched GEMM's histogram form on a TILES database -- 5 queries leave a
ragged last query group and so padding queries, 17 run in the default shape (2 queries x 16 tiles per
workgroup) and under IRIS_BATCH_KERNEL=2 (4 queries x 8 tiles, staggered waves).  Queries 3 and 10
have zero masks: every record is invalid for them.  The larger database makes a workgroup walk
several N-groups and gives several workgroups per query group."""
import subprocess

import numpy as np
import pytest

import hist_fixtures as hf
import iris_hip as ih
from oracle import oracle_c as oc
from test_histogram_abi import build_cpp_program

pytestmark = pytest.mark.gpu
GUARD = 0xA5A5A5A5A5A5A5A5
VARIANTS = {"tiles": (None, ih.LAYOUT_TILES), "tiles-k2": ("2", ih.LAYOUT_TILES), "lanes": (None, ih.LAYOUT_LANES)}
CASES = [("tiles", 1), ("tiles", 2), ("tiles", 3), ("lanes", 1), ("lanes", 2), ("lanes", 3), ("tiles", 5), ("tiles", 17),
         ("tiles-k2", 5), ("tiles-k2", 17)]


def open_variant(variant, device, hooked_device):
    kernel, layout = VARIANTS[variant]
    return (hooked_device(IRIS_BATCH_KERNEL=kernel) if kernel else device), layout


def batch_call(eng, db, nbins, first, n):
    """The C entry point into pre-filled arrays with guard words behind them -> (bins [nq, nbins], invalid [nq])."""
    nq = eng.nq
    bins = np.full(nq * nbins + 3, GUARD, np.uint64)
    invalid = np.full(nq + 2, GUARD, np.uint64)
    rc = ih.load_library().iris_template_batch_histogram(eng.handle, db.handle, first, n, nbins, bins.ctypes.data,
                                                         invalid.ctypes.data)
    assert rc == 0, ih.load_library().iris_last_error()
    assert (bins[nq * nbins:] == np.uint64(GUARD)).all() and (invalid[nq:] == np.uint64(GUARD)).all()
    return bins[:nq * nbins].reshape(nq, nbins).copy(), invalid[:nq].copy()


def profiled(dev, f):
    dev.reset_stats()
    dev.set_profiling(True)
    try:
        res = f()
    finally:
        dev.set_profiling(False)
    return res


@pytest.fixture(scope="module")
def small():
    return hf.small_batch_case()


@pytest.fixture(scope="module")
def large():
    return hf.large_case()


@pytest.mark.parametrize("variant,nq", CASES, ids=[f"{v}-{nq}" for v, nq in CASES])
def test_small_database_against_oracle_and_single_calls(device, hooked_device, small, variant, nq):
    dev, layout = open_variant(variant, device, hooked_device)
    singles = [ih.TemplateEngine(dev, small.queries[q]) for q in range(nq)]
    try:
        with ih.Database(dev, ih.KIND_TEMPLATES, 300, layout) as db, ih.TemplateBatchEngine(dev, small.queries[:nq]) as eng:
            small.fill(db)
            for first, n in hf.RANGES:
                for nbins in (1, 1024):
                    bins, invalid = batch_call(eng, db, nbins, first, n)
                    for q in range(nq):
                        want, want_invalid = hf.expected(small.dist[q], nbins, first, n)
                        assert (bins[q] == want).all() and invalid[q] == want_invalid, (q, first, n, nbins)
                        assert int(bins[q].sum()) + int(invalid[q]) == n
                        one, one_invalid = singles[q].histogram(db, nbins, first=first, n=n)
                        assert one.tobytes() == bins[q].tobytes() and one_invalid == invalid[q], (q, first, n, nbins)
                        if q in hf.LargeCase.ZERO_MASK:
                            assert invalid[q] == n and not bins[q].any()
            # identical calls: identical bytes, nothing accumulated
            a = batch_call(eng, db, 64, 0, 257)
            b = batch_call(eng, db, 64, 0, 257)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            # the kernels that ran, and the Python mirror
            bins, invalid = profiled(dev, lambda: eng.histogram(db, 64, first=5, n=200))
            assert bins.shape == (nq, 64) and invalid.shape == (nq,) and bins.dtype == invalid.dtype == np.uint64
            for q in range(nq):
                want, want_invalid = hf.expected(small.dist[q], 64, 5, 200)
                assert (bins[q] == want).all() and invalid[q] == want_invalid
            if nq <= 3:
                assert dev.kernel_stats("template_hist")[0] == nq and dev.kernel_stats("template_batch_hist")[0] == 0
            else:
                assert dev.kernel_stats("template_batch_hist")[0] == 1 and dev.kernel_stats("template_hist")[0] == 0
    finally:
        for s in singles:
            s.close()


LARGE_CASES = [("tiles", 3), ("tiles", 5), ("tiles", 17), ("tiles-k2", 17)]


@pytest.mark.parametrize("variant,nq", LARGE_CASES, ids=[f"{v}-{nq}" for v, nq in LARGE_CASES])
def test_large_database_against_oracle(device, hooked_device, large, variant, nq):
    dev, layout = open_variant(variant, device, hooked_device)
    with ih.Database(dev, ih.KIND_TEMPLATES, hf.LARGE_N, layout) as db, ih.TemplateBatchEngine(dev, large.queries[:nq]) as eng:
        large.fill(db)
        for nbins, first, n in [(1024, 0, hf.LARGE_N), (1, 0, hf.LARGE_N), (1024, 4090 * 32 + 5, 250), (64, 37, 100000)]:
            bins, invalid = batch_call(eng, db, nbins, first, n)
            for q in range(nq):
                want, want_invalid = hf.expected(large.dist(q), nbins, first, n)
                assert (bins[q] == want).all() and invalid[q] == want_invalid, (q, nbins, first, n)
                assert int(bins[q].sum()) + int(invalid[q]) == n
        # byte for byte the single-query call, for a generated query and a zero-mask one
        bins, invalid = batch_call(eng, db, 1024, 0, hf.LARGE_N)
        for q in sorted({0, min(3, nq - 1), nq - 1}):
            with ih.TemplateEngine(dev, large.queries[q]) as single:
                one, one_invalid = single.histogram(db, 1024)
            assert one.tobytes() == bins[q].tobytes() and one_invalid == invalid[q], q


def test_refusals(device, small):
    lib = ih.load_library()
    bins = np.full(5 * 64, GUARD, np.uint64)
    invalid = np.full(5, GUARD, np.uint64)
    with ih.Database(device, ih.KIND_TEMPLATES, 300, ih.LAYOUT_LANES) as lanes, \
            ih.TemplateBatchEngine(device, small.queries[:5]) as eng:
        small.fill(lanes)
        f = lib.iris_template_batch_histogram
        assert f(eng.handle, lanes.handle, 0, 257, 64, bins.ctypes.data, invalid.ctypes.data) == -1
        assert "TILES" in lib.iris_last_error().decode()
        assert f(eng.handle, lanes.handle, 0, 257, 96, bins.ctypes.data, invalid.ctypes.data) == -1
        assert "IRIS_HIST_MAX_BINS" in lib.iris_last_error().decode()
    assert (bins == np.uint64(GUARD)).all() and (invalid == np.uint64(GUARD)).all()


def test_cpp_program_against_oracle(device, tmp_path):
    """One C++ program through iris_hip.hpp: a single-query and a batch histogram of a generated
    database, compared in the program with the oracle's values passed in a file."""
    n, seed, nbins, nq = 1000, 21, 64, 5
    templates = oc.gen_templates(seed, 0, n)
    queries = oc.gen_templates(seed + 1, 0, nq)
    per_query = [hf.expected(oc.template_distances(queries[q], templates), nbins, 1, n - 1) for q in range(nq)]
    expected = np.concatenate([per_query[0][0], [per_query[0][1]]] + [b for b, _ in per_query] +
                              [[i for _, i in per_query]]).astype(np.uint64)
    assert len(expected) == (nbins + 1) * (1 + nq) and int(expected[:nbins].sum()) == n - 1
    path = tmp_path / "expected.bin"
    path.write_bytes(expected.tobytes())
    exe = build_cpp_program(tmp_path)
    r = subprocess.run([str(exe), str(path), str(n), str(seed), str(ih.LAYOUT_TILES), str(nbins), str(nq)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    # the program notices a wrong expectation
    expected[3] += np.uint64(1)
    path.write_bytes(expected.tobytes())
    r = subprocess.run([str(exe), str(path), str(n), str(seed), str(ih.LAYOUT_TILES), str(nbins), str(nq)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 5, (r.returncode, r.stderr[-2000:])
