"""GPU: distance histograms of one query (iris_template_histogram): the distribution of a range's
best-rotation distances in one database pass, against np.bincount of the CPU oracle's f64 distances
binned by the header's rule (tests/hist_fixtures.py) -- never against the library's own search.

Variants as in test_gpu_matches.py: a TILES database under the library's own dispatch (on the small
database the K-split template kernel), TILES with IRIS_TILES_PER_WAVE=1 and =4 and a LANES database
(the VALU template kernel, the independent cross-check).  A database of 4098 * 32 + 27 records runs
the library's own choice past the K-split form."""
import ctypes

import numpy as np
import pytest

import hist_fixtures as hf
import iris_hip as ih
from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu
E_ARG, E_RANGE = -1, -5
GUARD = 0xA5A5A5A5A5A5A5A5
VARIANTS = ["tiles", "tiles-tpw1", "tiles-tpw4", "lanes"]


@pytest.fixture(params=VARIANTS)
def ctx(request, device, hooked_device):
    v = request.param
    if v == "tiles-tpw1":
        return hooked_device(IRIS_TILES_PER_WAVE=1), ih.LAYOUT_TILES
    if v == "tiles-tpw4":
        return hooked_device(IRIS_TILES_PER_WAVE=4), ih.LAYOUT_TILES
    return device, ih.LAYOUT_TILES if v == "tiles" else ih.LAYOUT_LANES


@pytest.fixture(scope="module")
def case():
    return hf.single_case()


def small_db(case, dev, layout):
    db = ih.Database(dev, ih.KIND_TEMPLATES, 300, layout)
    case.fill(db)
    return db


def raw_call(eng, db, nbins, first, n, fill=GUARD):
    """The C entry point into pre-filled arrays with guard words behind them -> (bins, invalid)."""
    bins = np.full(nbins + 3, fill, np.uint64)
    invalid = np.full(2, fill, np.uint64)
    rc = ih.load_library().iris_template_histogram(eng.handle, db.handle, first, n, nbins, bins.ctypes.data,
                                                   invalid.ctypes.data)
    assert rc == 0, ih.load_library().iris_last_error()
    assert (bins[nbins:] == np.uint64(fill)).all() and invalid[1] == np.uint64(fill), "words past the outputs were written"
    return bins[:nbins].copy(), int(invalid[0])


def test_against_oracle(ctx, case):
    device, layout = ctx
    with small_db(case, device, layout) as db:
        for key, query in case.queries.items():
            with ih.TemplateEngine(device, query) as eng:
                for first, n in hf.RANGES:
                    for nbins in hf.NBINS:
                        bins, invalid = raw_call(eng, db, nbins, first, n)
                        want, want_invalid = hf.expected(case.dist[key], nbins, first, n)
                        assert (bins == want).all() and invalid == want_invalid, (key, first, n, nbins)
                        assert int(bins.sum()) + invalid == n
                # the Python mirror returns the same arrays
                bins, invalid = eng.histogram(db, 1024)
                want, want_invalid = hf.expected(case.dist[key], 1024)
                assert bins.dtype == np.uint64 and bins.shape == (1024,) and (bins == want).all() and invalid == want_invalid
                assert isinstance(invalid, int)
                bins, invalid = eng.histogram(db, 64, first=5, n=200)
                assert (bins == hf.expected(case.dist[key], 64, 5, 200)[0]).all()


def test_prefix_sums_equal_match_totals(ctx, case):
    """bins[0] + ... + bins[j - 1] is the total matches(threshold = j / nbins, cap = 0) reports, at
    the planted edge (distance 0.25 = 256 / 1024 exactly: excluded by the threshold, in bin 256) too."""
    device, layout = ctx
    edges = {2: [0, 1], 64: [0, 15, 16, 17, 30, 31, 32, 63], 1024: [0, 1, 255, 256, 257, 480, 492, 500, 512, 1023]}
    with small_db(case, device, layout) as db:
        for key, query in case.queries.items():
            with ih.TemplateEngine(device, query) as eng:
                for first, n in [(0, 257), (5, 200)]:
                    for nbins, js in edges.items():
                        bins, _ = raw_call(eng, db, nbins, first, n)
                        for j in js:
                            _, total = eng.matches(db, j / nbins, first=first, n=n, cap=0)
                            assert int(bins[:j].sum()) == total, (key, first, n, nbins, j)
        with ih.TemplateEngine(device, case.edge_query) as eng:
            bins, _ = raw_call(eng, db, 1024, 0, 257)
            assert int(bins[:256].sum()) == 2 and int(bins[:257].sum()) == 3  # records 0 and 32, then 31 on the edge


def test_identical_calls_and_no_accumulation(ctx, case):
    device, layout = ctx
    with small_db(case, device, layout) as db, ih.TemplateEngine(device, case.gen_query) as eng:
        a = raw_call(eng, db, 1024, 0, 257)
        b = raw_call(eng, db, 1024, 0, 257, fill=7)  # other bytes in the arrays: overwritten, not added to
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
        assert int(b[0].sum()) + b[1] == 257
        # n == 0 writes zeros
        bins, invalid = raw_call(eng, db, 64, 10, 0)
        assert not bins.any() and invalid == 0
        # a smaller histogram after a larger one reads no stale counter
        bins, invalid = raw_call(eng, db, 2, 0, 257)
        want, want_invalid = hf.expected(case.dist["gen"], 2)
        assert (bins == want).all() and invalid == want_invalid


def test_other_calls_after_a_histogram(ctx, case):
    """search, matches and topk after a histogram call on the same device equal their oracle results:
    the histogram leaves the shared buffers in no state that disturbs them."""
    device, layout = ctx
    d = case.dist["gen"]
    order = np.lexsort((np.arange(len(d)), d))
    below = np.flatnonzero(d < 0.48)
    assert 5 < len(below) < 250
    with small_db(case, device, layout) as db, ih.TemplateEngine(device, case.gen_query) as eng:
        for nbins in (1024, 1):
            raw_call(eng, db, nbins, 0, 257)
            m = eng.search(db)
            best, idx = oc.argmin(d)
            assert (m.index, m.distance) == (idx, best)
            got, count = eng.matches(db, 0.48)
            assert count == len(below) and [g.index for g in got] == list(below)
            top = eng.topk(db, 5)
            assert [t.index for t in top] == list(order[:5]) and [t.distance for t in top] == list(d[order[:5]])
            bins, invalid = raw_call(eng, db, nbins, 0, 257)
            assert (bins == hf.expected(d, nbins)[0]).all() and invalid == 1


def test_one_launch_per_call(ctx, case):
    device, layout = ctx
    with small_db(case, device, layout) as db, ih.TemplateEngine(device, case.gen_query) as eng:
        device.reset_stats()
        device.set_profiling(True)
        try:
            for _ in range(3):
                raw_call(eng, db, 64, 0, 257)
            raw_call(eng, db, 64, 0, 0)  # an empty range launches nothing
        finally:
            device.set_profiling(False)
        assert device.kernel_stats("template_hist")[0] == 3
        assert device.kernel_stats("hist_reduce")[0] == 3


def test_refusals_leave_the_outputs_alone(device, case):
    lib = ih.load_library()
    bins = np.full(1024, GUARD, np.uint64)
    invalid = np.full(1, GUARD, np.uint64)
    queries = np.stack([case.gen_query] * 5)
    with small_db(case, device, ih.LAYOUT_TILES) as db, ih.TemplateEngine(device, case.gen_query) as eng, \
            ih.TemplateBatchEngine(device, queries) as batch, ih.Database(device, ih.KIND_MASKS, 64) as masks:
        f = lib.iris_template_histogram
        assert f(batch.handle, db.handle, 0, 257, 64, bins.ctypes.data, invalid.ctypes.data) == E_ARG
        assert "single-query" in lib.iris_last_error().decode()
        assert f(eng.handle, masks.handle, 0, 0, 64, bins.ctypes.data, invalid.ctypes.data) == E_ARG
        assert f(eng.handle, db.handle, 200, 58, 64, bins.ctypes.data, invalid.ctypes.data) == E_RANGE
        assert f(eng.handle, db.handle, 0, 257, 48, bins.ctypes.data, invalid.ctypes.data) == E_ARG
        assert lib.iris_template_batch_histogram(eng.handle, db.handle, 0, 257, 64, bins.ctypes.data,
                                                 invalid.ctypes.data) == E_ARG
        assert (bins == np.uint64(GUARD)).all() and invalid[0] == np.uint64(GUARD)
        with pytest.raises(ih.IrisError):
            eng.histogram(db, 1000)


@pytest.fixture(scope="module")
def large():
    return hf.large_case()


def test_large_range_own_dispatch(device, large):
    """4099 tiles under the library's own dispatch (one tile per wave, many workgroups per counter
    copy, the last tile partial), whole and from inside a tile to inside another."""
    with ih.Database(device, ih.KIND_TEMPLATES, hf.LARGE_N, ih.LAYOUT_TILES) as db:
        large.fill(db)
        for q in (0, 3):  # a generated query; one with a zero mask: every record invalid
            with ih.TemplateEngine(device, large.queries[q]) as eng:
                for nbins in (1024, 64):
                    for first, n in [(0, hf.LARGE_N), (4090 * 32 + 5, 250), (37, 100000)]:
                        bins, invalid = raw_call(eng, db, nbins, first, n)
                        want, want_invalid = hf.expected(large.dist(q), nbins, first, n)
                        assert (bins == want).all() and invalid == want_invalid, (q, nbins, first, n)
                device.reset_stats()
                device.set_profiling(True)
                try:
                    raw_call(eng, db, 1024, 0, hf.LARGE_N)
                finally:
                    device.set_profiling(False)
                assert device.kernel_stats("template_hist")[0] == 1
        assert hf.expected(large.dist(3), 64)[1] == hf.LARGE_N and np.count_nonzero(hf.expected(large.dist(0), 1024)[0]) > 20


@pytest.mark.parametrize("copies", [1, 2, 64])
def test_counter_copies_hook(hooked_device, case, large, copies):
    """IRIS_HIST_COPIES pins the number of counter copies a pass adds into (1: straight into the
    result, no reduce launch): the histogram does not depend on it."""
    dev = hooked_device(IRIS_HIST_COPIES=copies)
    assert dev.config()["hist_copies"] == str(copies)
    with small_db(case, dev, ih.LAYOUT_TILES) as db, ih.TemplateEngine(dev, case.edge_query) as eng:
        for nbins in (1, 1024):
            bins, invalid = raw_call(eng, db, nbins, 5, 252)
            want, want_invalid = hf.expected(case.dist["edge"], nbins, 5, 252)
            assert (bins == want).all() and invalid == want_invalid
    with ih.Database(dev, ih.KIND_TEMPLATES, hf.LARGE_N, ih.LAYOUT_TILES) as db, \
            ih.TemplateEngine(dev, large.queries[0]) as eng:
        large.fill(db)
        dev.reset_stats()
        dev.set_profiling(True)
        try:
            bins, invalid = raw_call(eng, db, 1024, 0, hf.LARGE_N)
        finally:
            dev.set_profiling(False)
        want, want_invalid = hf.expected(large.dist(0), 1024)
        assert (bins == want).all() and invalid == want_invalid
        assert dev.kernel_stats("template_hist")[0] == 1
        assert dev.kernel_stats("hist_reduce")[0] == (0 if copies == 1 else 1)
