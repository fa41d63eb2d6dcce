"""GPU: combined passes (iris_template_report) -- the match list, the k closest records and the
distance histogram of one probe from one read of the range.  Every expectation comes from the CPU
oracle (report_fixtures.py: matches, order and histogram of the oracle's counts and f64 distances),
never from the library's own sibling calls; the one exception is the test whose subject is that the
parts equal the siblings' outputs byte for byte.

Variants as in test_gpu_histogram.py: a TILES database under the library's own dispatch (on the 257
records of the small case the K-split template kernel), TILES with IRIS_TILES_PER_WAVE=1 and =4 and a
LANES database (the VALU template kernel, the independent cross-check): 9 tiles with a one-record
last tile in every TILES form.  A database of 4098 * 32 + 27 records runs the library's own choice
past the K-split form.  The C entry point is called raw (report_fixtures.raw_report): guard bytes
fill the fields of unselected parts and stand behind every output array."""
import ctypes
import subprocess

import numpy as np
import pytest

import hist_fixtures as hf
import iris_hip as ih
import order_fixtures as of
import report_fixtures as rf
from oracle import oracle_c as oc
from report_fixtures import ALL, HIST, MATCHES, TOPK
from test_gpu_matches import Expected
from test_report_abi import build_cpp_program

pytestmark = pytest.mark.gpu
E_ARG, E_RANGE = -1, -5
VARIANTS = ["tiles", "tiles-tpw1", "tiles-tpw4", "lanes"]
BASE = 2**40 + 7
ABOVE_HALF = float(np.nextafter(0.5, np.inf))
LARGE_RANGES = [(0, hf.LARGE_N), (4090 * 32 + 5, 250), (37, 100000)]
PASSES = ("template_report", "template_match", "template_topk", "template_hist", "topk_merge", "hist_reduce")


@pytest.fixture(params=VARIANTS)
def ctx(request, device, hooked_device):
    v = request.param
    if v == "tiles-tpw1":
        return hooked_device(IRIS_TILES_PER_WAVE=1), ih.LAYOUT_TILES
    if v == "tiles-tpw4":
        return hooked_device(IRIS_TILES_PER_WAVE=4), ih.LAYOUT_TILES
    return device, ih.LAYOUT_TILES if v == "tiles" else ih.LAYOUT_LANES


class SmallCase:
    """hist_fixtures.single_case() with the oracle's Expected of both queries."""

    def __init__(self):
        self.case = hf.single_case()
        self.queries = self.case.queries
        self.exp = {}
        for key, q in self.queries.items():
            self.exp[key] = Expected(*oc.template_counts(q, self.case.templates))
            assert (rf.bits_of(self.exp[key].dist) == rf.bits_of(self.case.dist[key])).all()

    def db(self, dev, layout):
        db = ih.Database(dev, ih.KIND_TEMPLATES, 300, layout)
        self.case.fill(db)
        return db


class LargeCase:
    def __init__(self):
        self.case = hf.large_case()
        self.queries = self.case.queries
        self.exp = {q: rf.SparseExpected(self.queries[q], self.case.templates, self.case.dist(q)) for q in (0, 3)}

    def db(self, dev):
        db = ih.Database(dev, ih.KIND_TEMPLATES, hf.LARGE_N, ih.LAYOUT_TILES)
        self.case.fill(db)
        return db


@pytest.fixture(scope="module")
def small():
    return SmallCase()


@pytest.fixture(scope="module")
def large():
    return LargeCase()


def profiled(device, call):
    """call() under profiling -> (its result, {pass name: launches})."""
    device.reset_stats()
    device.set_profiling(True)
    try:
        res = call()
    finally:
        device.set_profiling(False)
    return res, {name: device.kernel_stats(name)[0] for name in PASSES}


def run(eng, db, e, parts, first, n, threshold=None, cap=None, k=None, nbins=None, base=0, fill=rf.GUARD_BYTE):
    """One raw call, checked against the oracle -> its result."""
    res = rf.raw_report(eng, db, first, n, parts, threshold, cap, k, nbins, index_base=base, fill=fill)
    rf.check(e, res, parts, first, n, threshold, cap, k, nbins, base)
    return res


# ---------------------------------------------------------------- 1. against the oracle, small


def test_against_oracle(ctx, small):
    device, layout = ctx
    with small.db(device, layout) as db:
        for key, query in small.queries.items():
            e = small.exp[key]
            with ih.TemplateEngine(device, query) as eng:
                for first, n in hf.RANGES:
                    for parts in rf.SUBSETS:
                        run(eng, db, e, parts, first, n, 0.48, None, 5, 64)
                    for threshold, k, nbins in [(0.5, 64, 1024), (2.0, 1, 1), (0.0, 64, 2)]:
                        run(eng, db, e, ALL, first, n, threshold, None, k, nbins)
                    for cap in (0, 3, None):
                        run(eng, db, e, ALL, first, n, 0.48, cap, 5, 64, base=BASE)


# ---------------------------------------------------------------- 2. equal to the siblings, byte for byte


def sibling_bytes(eng, db, first, n, threshold, cap, k, nbins, base):
    lib = ih.load_library()
    cap = n if cap is None else cap
    marr, tarr = rf.match_array(cap), rf.match_array(k)
    count, tcount, invalid = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint64()
    bins = np.zeros(nbins, np.uint64)
    assert lib.iris_template_matches(eng.handle, db.handle, first, n, base, threshold, marr if cap else None, cap,
                                     ctypes.byref(count)) == 0
    assert lib.iris_template_topk(eng.handle, db.handle, first, n, base, k, tarr, ctypes.byref(tcount)) == 0
    assert lib.iris_template_histogram(eng.handle, db.handle, first, n, nbins, bins.ctypes.data,
                                       ctypes.byref(invalid)) == 0
    size = ctypes.sizeof(ih.Match)
    return (bytes(marr)[:min(count.value, cap) * size], count.value, bytes(tarr)[:tcount.value * size], tcount.value,
            bins.tobytes(), invalid.value)


def test_equal_to_the_siblings_byte_for_byte(ctx, small):
    device, layout = ctx
    with small.db(device, layout) as db:
        for key, query in small.queries.items():
            with ih.TemplateEngine(device, query) as eng:
                for first, n in hf.RANGES:
                    for threshold, cap, k, nbins in [(0.48, None, 5, 64), (0.5, 3, 64, 1024), (2.0, 0, 1, 1)]:
                        want = sibling_bytes(eng, db, first, n, threshold, cap, k, nbins, BASE)
                        for parts in rf.SUBSETS:
                            r = rf.raw_report(eng, db, first, n, parts, threshold, cap, k, nbins, index_base=BASE)
                            if parts & MATCHES:
                                assert (r.matches_bytes, r.matches_count) == want[0:2], (key, first, n, parts)
                            if parts & TOPK:
                                assert (r.topk_bytes, r.topk_count) == want[2:4], (key, first, n, parts)
                            if parts & HIST:
                                assert (r.bins.tobytes(), r.invalid) == want[4:6], (key, first, n, parts)


# ---------------------------------------------------------------- 3. ties


def test_ties(ctx):
    """Rotation ties and equal fractions in different terms (order_fixtures.py): the top-k part at
    k = 64 and the matches part at a quarter and at the next f64 after a half return the order and
    the rotations the oracle's exact rule gives -- what test_gpu_order.py pins for the sibling calls."""
    device, layout = ctx
    recs = of.crafted_db()
    with ih.Database(device, ih.KIND_TEMPLATES, of.N, layout) as db:
        db.append(recs)
        for query in (of.crafted_query(), of.periodic_query(5)):
            e = Expected(*oc.template_counts(query, recs))
            with ih.TemplateEngine(device, query) as eng:
                for first, n in [(0, of.N), (41, 1000)]:
                    for threshold in (of.QUARTER, ABOVE_HALF):
                        run(eng, db, e, ALL, first, n, threshold, None, 64, 64, base=BASE)
                        run(eng, db, e, MATCHES | TOPK, first, n, threshold, None, 64)
    # the crafted query's list at the half holds the tied records, in both terms
    e = Expected(*oc.template_counts(of.crafted_query(), recs))
    assert set(of.TIED) <= set(e.hits(ABOVE_HALF)) and len(e.hits(0.5)) == 1
    assert {(int(e.num[i]), int(e.den[i])) for i in of.TIED} == {(32, 64), (64, 128)}


# ---------------------------------------------------------------- 4. large, the library's own dispatch


def test_large_range_own_dispatch(device, large):
    with large.db(device) as db:
        for q in (0, 3):
            e = large.exp[q]
            with ih.TemplateEngine(device, large.queries[q]) as eng:
                for first, n in LARGE_RANGES:
                    res = run(eng, db, e, ALL, first, n, 0.46, None, 64, 1024)
                    if q == 3:
                        assert res.matches == [] and res.matches_count == 0 and res.topk_count == 0 and res.invalid == n
                res, launches = profiled(device, lambda: run(eng, db, e, ALL, 0, hf.LARGE_N, 0.46, None, 64, 1024))
                assert launches == {"template_report": 1, "topk_merge": 1, "hist_reduce": 1, "template_match": 0,
                                    "template_topk": 0, "template_hist": 0}
        assert large.exp[0].hits(0.46).size == 12


# ---------------------------------------------------------------- 5. the overflow rerun


def test_overflowing_match_list_runs_the_matches_part_again(hooked_device, large):
    device = hooked_device()  # a fresh device: its match buffer has not grown
    e = large.exp[0]
    with large.db(device) as db, ih.TemplateEngine(device, large.queries[0]) as eng:
        res, launches = profiled(device, lambda: run(eng, db, e, ALL, 0, hf.LARGE_N, 0.47, 1100, 64, 1024))
        assert res.matches_count == 1373 and len(res.matches) == 1100
        assert [m.index for m in res.matches] == list(e.hits(0.47)[:1100])
        assert launches["template_report"] == 1 and launches["template_match"] == 1
        assert launches["template_topk"] == 0 and launches["template_hist"] == 0 and launches["topk_merge"] == 1
    device = hooked_device()
    with large.db(device) as db, ih.TemplateEngine(device, large.queries[0]) as eng:
        res, launches = profiled(device, lambda: run(eng, db, e, ALL, 0, hf.LARGE_N, 0.47, 0, 64, 1024))
        assert res.matches_count == 1373 and res.matches == []
        assert launches["template_report"] == 1 and launches["template_match"] == 0


# ---------------------------------------------------------------- 6. one part runs the sibling's pass


def test_one_part_runs_the_siblings_pass(ctx, small):
    device, layout = ctx
    e = small.exp["gen"]
    with small.db(device, layout) as db, ih.TemplateEngine(device, small.queries["gen"]) as eng:
        for parts, name in ((MATCHES, "template_match"), (TOPK, "template_topk"), (HIST, "template_hist")):
            _, launches = profiled(device, lambda: run(eng, db, e, parts, 0, 257, 0.48, None, 5, 64))
            assert launches["template_report"] == 0 and launches[name] == 1, (parts, launches)
            assert sum(launches[p] for p in ("template_match", "template_topk", "template_hist")) == 1
        _, launches = profiled(device, lambda: run(eng, db, e, ALL, 0, 257, 0.48, None, 5, 64))
        assert launches["template_report"] == 1
        assert sum(launches[p] for p in ("template_match", "template_topk", "template_hist")) == 0
        _, launches = profiled(device, lambda: run(eng, db, e, ALL, 10, 0, 0.48, None, 5, 64))  # n == 0: no launch
        assert not any(launches.values())


# ---------------------------------------------------------------- 7. neighbours undisturbed


def test_neighbours_undisturbed(ctx, small):
    """The report shares the device's match, counter and result buffers with its siblings by region:
    each sibling after a report and a report after each sibling equal the oracle."""
    device, layout = ctx
    e = small.exp["gen"]
    d = e.dist
    below = e.hits(0.48)
    top = rf.order(e, 0, 257)[:5]

    def siblings(eng, db):
        m = eng.search(db)
        best, idx = oc.argmin(d)
        assert (m.index, m.distance) == (idx, best)
        yield "search"
        got, count = eng.matches(db, 0.48)
        assert count == len(below) and [g.index for g in got] == list(below)
        yield "matches"
        t = eng.topk(db, 5)
        assert [x.index for x in t] == list(top) and [x.distance for x in t] == list(d[top])
        yield "topk"
        bins, invalid = eng.histogram(db, 1024)
        want, want_invalid = hf.expected(d, 1024)
        assert (bins == want).all() and invalid == want_invalid
        yield "histogram"

    with small.db(device, layout) as db, ih.TemplateEngine(device, small.queries["gen"]) as eng:
        for _ in siblings(eng, db):
            run(eng, db, e, ALL, 0, 257, 0.48, None, 5, 1024)  # a report after each sibling
        for step in range(4):  # each sibling straight after a report
            run(eng, db, e, ALL, 0, 257, 0.5, None, 64, 64)
            it = siblings(eng, db)
            for _ in range(step + 1):
                next(it)
        # outputs are overwritten, not accumulated: identical calls into differently filled arrays
        a = run(eng, db, e, ALL, 5, 200, 0.48, None, 5, 1024)
        b = run(eng, db, e, ALL, 5, 200, 0.48, None, 5, 1024, fill=0x07)
        assert (a.matches_bytes, a.matches_count, a.topk_bytes, a.topk_count, a.bins.tobytes(), a.invalid) == \
               (b.matches_bytes, b.matches_count, b.topk_bytes, b.topk_count, b.bins.tobytes(), b.invalid)
        # a smaller histogram after a larger one reads no stale counter
        run(eng, db, e, ALL, 0, 257, 0.48, None, 5, 2)
        run(eng, db, e, TOPK | HIST, 0, 257, None, None, 64, 1)


# ---------------------------------------------------------------- 8. IRIS_HIST_COPIES


@pytest.mark.parametrize("copies", [1, 2, 64])
def test_counter_copies_hook(hooked_device, small, large, copies):
    dev = hooked_device(IRIS_HIST_COPIES=copies)
    assert dev.config()["hist_copies"] == str(copies)
    with small.db(dev, ih.LAYOUT_TILES) as db, ih.TemplateEngine(dev, small.queries["edge"]) as eng:
        for nbins in (1, 1024):
            run(eng, db, small.exp["edge"], ALL, 5, 252, 0.3, None, 5, nbins)
    with large.db(dev) as db, ih.TemplateEngine(dev, large.queries[0]) as eng:
        _, launches = profiled(dev, lambda: run(eng, db, large.exp[0], ALL, 0, hf.LARGE_N, 0.46, None, 64, 1024))
        assert launches["template_report"] == 1 and launches["hist_reduce"] == (0 if copies == 1 else 1)
        assert launches["template_hist"] == 0


# ---------------------------------------------------------------- 9. refusals on the device


def test_refusals_leave_everything_alone(device, small):
    queries = np.stack([small.queries["gen"]] * 5)
    with small.db(device, ih.LAYOUT_TILES) as db, ih.TemplateEngine(device, small.queries["gen"]) as eng, \
            ih.TemplateBatchEngine(device, queries) as batch, ih.Database(device, ih.KIND_MASKS, 64) as masks:
        for parts in (ALL, MATCHES | HIST, TOPK):
            r = rf.raw_report(batch, db, 0, 257, parts, 0.48, 4, 5, 64, expect_rc=E_ARG)
            assert "single-query" in r.error
            rf.raw_report(eng, masks, 0, 0, parts, 0.48, 4, 5, 64, expect_rc=E_ARG)
            rf.raw_report(eng, db, 200, 58, parts, 0.48, 4, 5, 64, expect_rc=E_RANGE)
            rf.raw_report(eng, db, 0, 257, parts, 0.48, 4, 5 if parts != TOPK else 65, 48 if parts != TOPK else 64,
                          expect_rc=E_ARG)
        # and the device is as usable as before
        run(eng, db, small.exp["gen"], ALL, 0, 257, 0.48, None, 5, 64)
        with pytest.raises(ih.IrisError):
            eng.report(db, nbins=1000)
        with pytest.raises(ih.IrisError):
            eng.report(db)


# ---------------------------------------------------------------- 10. the mirrors and index_base


def test_python_mirror_and_index_base(ctx, small):
    device, layout = ctx
    e = small.exp["gen"]
    with small.db(device, layout) as db, ih.TemplateEngine(device, small.queries["gen"]) as eng:
        r = eng.report(db, threshold=0.48, k=5, nbins=64, first=5, n=200, index_base=BASE)
        hits = e.hits(0.48, 5, 200)
        assert r.matches_count == len(hits)
        rf.check_list(e, r.matches, hits, BASE)
        rf.check_list(e, r.topk, rf.order(e, 5, 200)[:5], BASE)
        want, want_invalid = hf.expected(e.dist, 64, 5, 200)
        assert r.bins.dtype == np.uint64 and (r.bins == want).all() and r.invalid == want_invalid
        assert r.matches[0].index == BASE + 5 + (int(hits[0]) - 5)
        # unselected parts are None; a cap keeps the lowest indices and the exact total
        r = eng.report(db, threshold=0.5, cap=3, k=1)
        assert r.bins is None and r.invalid is None and r.matches_count == 253 and len(r.matches) == 3
        rf.check_list(e, r.matches, e.hits(0.5)[:3], 0)
        rf.check_list(e, r.topk, rf.order(e, 0, 257)[:1], 0)
        r = eng.report(db, nbins=1024)
        assert r.matches is None and r.matches_count is None and r.topk is None
        assert (r.bins == hf.expected(e.dist, 1024)[0]).all() and r.invalid == 1
        r = eng.report(db, threshold=0.48, cap=0, nbins=2)
        assert r.matches == [] and r.matches_count == 84 and r.topk is None


def test_python_mirror_fetches_a_long_list(device, large):
    """cap=None past the combined pass's first 1024 records: the rest comes through matches()."""
    e = large.exp[0]
    with large.db(device) as db, ih.TemplateEngine(device, large.queries[0]) as eng:
        r = eng.report(db, threshold=0.47, k=64)
        assert r.matches_count == 1373 and [m.index for m in r.matches] == list(e.hits(0.47))
        rf.check_list(e, r.topk, rf.order(e, 0, hf.LARGE_N)[:64], 0)


@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES])
def test_cpp_report(layout, tmp_path):
    """tests/cpp/report.cpp through iris_hip.hpp on generated templates, against the oracle."""
    n, seed, threshold, k, nbins = 700, 21, 0.475, 7, 64
    exe = build_cpp_program(tmp_path)
    out = subprocess.run([str(exe), str(n), str(seed), str(layout), repr(threshold), "-1", str(k), str(nbins)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    recs = oc.gen_templates(seed, 0, n)
    query = oc.gen_templates(seed + 1, 0, 1)[0]
    e = Expected(*oc.template_counts(query, recs))
    lines = [ln.split() for ln in out.stdout.strip().split("\n")]
    hits, top = e.hits(threshold, 1, n - 1), rf.order(e, 1, n - 1)[:k]
    assert 3 < len(hits) < n // 2
    want = [["count", str(len(hits))]]
    want += [["m", str(1000 + int(i)), str(e.num[i]), str(e.den[i]), str(e.rot[i])] for i in hits]
    want += [["t", str(1000 + int(i)), str(e.num[i]), str(e.den[i]), str(e.rot[i])] for i in top]
    bins, invalid = hf.expected(e.dist, nbins, 1, n - 1)
    want += [["b"] + [str(int(b)) for b in bins], ["invalid", str(invalid)], ["only"] + [str(1000 + int(i)) for i in top]]
    assert lines == want
