"""GPU: the template batch report (iris_template_batch_report): for every query of a template batch
engine any of its match list, its k closest records and its distance histogram from one GEMM pass.

Expectations come from the CPU oracle alone (per query an Expected of
test_gpu_template_batch_matches on the 257 records of hist_fixtures.small_batch_case(), a
report_fixtures.SparseExpected on the 4098 * 32 + 27 records of hist_fixtures.large_case()), except
in the byte-equality test, which compares with the three sibling batch calls and with the
single-query iris_template_report.  The C entry point is called raw (batch_report_fixtures): guard
bytes fill the fields and arrays of unselected parts and stand behind every output array.

Variants: engines of 1..3 queries run one single-query report per query (TILES and LANES); 5 queries
(a ragged last group with padding queries) and 17 (queries 3 and 10 with zero masks) run the GEMM's
report form in its default shape and under IRIS_BATCH_KERNEL=2.  The 257 records are 9 tiles with a
one-record last tile: the single N-group has clamped tiles and waves whose tiles are all clamped,
which must still store empty lists and reach both histogram barriers.  The large case gives several
workgroups per query group and several N-groups per workgroup."""
import ctypes
import subprocess

import numpy as np
import pytest

import batch_report_fixtures as bf
import hist_fixtures as hf
import iris_hip as ih
import report_fixtures as rf
from batch_report_fixtures import ALL, HIST, MATCHES, MULTI, TOPK
from test_gpu_template_batch_matches import Expected
from test_template_batch_report_abi import build_cpp_program

pytestmark = pytest.mark.gpu
E_ARG, E_RANGE = -1, -5
BASE = 2**40 + 7
LARGE_RANGES = [(0, hf.LARGE_N), (4090 * 32 + 5, 250), (37, 100000)]
PASSES = ("template_batch_report", "template_batch_match", "template_batch_topk", "template_batch_hist",
          "template_report", "template_match", "template_topk", "template_hist")
# kMatchFirstRoom (csrc/iris_api_select.hip): records a query's first pass has room for when the cap
# asks for fewer; RERUN_BLOCK is batch_query_group() (csrc/iris_batch.hip, kBatchBQ): the aligned
# block of queries that runs again.  Neither is exported: a change there is made here too.
MATCH_FIRST_ROOM = 1024
RERUN_BLOCK = 4
VARIANTS = [("tiles", 1), ("tiles", 2), ("tiles", 3), ("lanes", 1), ("lanes", 2), ("lanes", 3), ("tiles", 5), ("tiles", 17),
            ("tiles-k2", 5), ("tiles-k2", 17)]
GEMM = [v for v in VARIANTS if v[1] > 3]


def open_variant(variant, device, hooked_device):
    if variant == "tiles-k2":
        return hooked_device(IRIS_BATCH_KERNEL="2"), ih.LAYOUT_TILES
    return device, ih.LAYOUT_TILES if variant == "tiles" else ih.LAYOUT_LANES


class SmallCase:
    """hist_fixtures.small_batch_case() with the oracle's Expected of every query."""

    N = hf.SMALL_N

    def __init__(self):
        self.case = hf.small_batch_case()
        self.queries = self.case.queries
        self.exp = [Expected(q, self.case.templates) for q in self.queries]
        for e, d in zip(self.exp, self.case.dist):
            assert (rf.bits_of(e.dist) == rf.bits_of(d)).all()

    def db(self, dev, layout):
        db = ih.Database(dev, ih.KIND_TEMPLATES, 300, layout)
        self.case.fill(db)
        return db


class LargeCase:
    def __init__(self):
        self.case = hf.large_case()
        self.queries = self.case.queries
        self.exp = [rf.SparseExpected(self.queries[q], self.case.templates, self.case.dist(q)) for q in range(self.case.NQ)]

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


@pytest.fixture
def own_device():
    """A device handle of the test's own: its match buffer starts empty, so launch counts do not
    depend on what ran before, and the buffer the test grows is not the session device's."""
    with ih.Device(0) as dev:
        yield dev


def profiled(device, call):
    """call() under profiling -> (its result, {pass name: launches})."""
    device.reset_stats()
    device.set_profiling(True)
    try:
        res = call()
    finally:
        device.set_profiling(False)
    return res, {name: device.kernel_stats(name)[0] for name in PASSES}


def run(eng, db, exps, parts, first, n, threshold=None, cap=None, k=None, nbins=None, base=0):
    """One raw call, every selected part of every query checked against the oracle -> its result."""
    res = bf.raw_report(eng, db, first, n, parts, threshold=threshold, cap=cap, k=k, nbins=nbins, index_base=base)
    bf.check(exps[:eng.nq], res, parts, first, n, threshold, cap, k, nbins, base)
    return res


def same(a, b, parts):
    if parts & MATCHES:
        assert a.matches_counts == b.matches_counts and a.matches_bytes == b.matches_bytes
    if parts & TOPK:
        assert a.topk_counts == b.topk_counts and a.topk_bytes == b.topk_bytes
    if parts & HIST:
        assert a.bins.tobytes() == b.bins.tobytes() and a.invalid == b.invalid


def siblings(eng, db, first, n, base, threshold, cap, k, nbins):
    """The three sibling batch calls, raw -> (counts, per-query list bytes, top-k counts, per-query
    list bytes, bins [nq, nbins], invalid)."""
    lib = ih.load_library()
    nq = eng.nq
    marr = (ih.Match * max(nq * cap, 1))()
    mcounts = (ctypes.c_uint64 * nq)()
    assert lib.iris_template_batch_matches(eng.handle, db.handle, first, n, base, threshold, marr if cap else None, cap,
                                           mcounts) == 0
    tarr = (ih.Match * (nq * k))()
    tcounts = (ctypes.c_uint32 * nq)()
    assert lib.iris_template_batch_topk(eng.handle, db.handle, first, n, base, k, tarr, tcounts) == 0
    bins = np.zeros((nq, nbins), np.uint64)
    invalid = np.zeros(nq, np.uint64)
    assert lib.iris_template_batch_histogram(eng.handle, db.handle, first, n, nbins, bins.ctypes.data_as(ctypes.c_void_p),
                                             invalid.ctypes.data_as(ctypes.c_void_p)) == 0
    mraw, traw, size = bytes(marr), bytes(tarr), bf.SIZE
    return ([int(c) for c in mcounts],
            [mraw[q * cap * size:(q * cap + min(int(mcounts[q]), cap)) * size] for q in range(nq)],
            [int(c) for c in tcounts],
            [traw[q * k * size:(q * k + int(tcounts[q])) * size] for q in range(nq)], bins, [int(v) for v in invalid])


def equal_to_siblings_and_singles(device, eng, db, queries, ranges, threshold, cap, k, nbins):
    singles = [ih.TemplateEngine(device, queries[q]) for q in range(eng.nq)]
    try:
        for first, n in ranges:
            res = bf.raw_report(eng, db, first, n, ALL, threshold=threshold, cap=cap, k=k, nbins=nbins, index_base=BASE)
            mc, mb, tc, tb, bins, invalid = siblings(eng, db, first, n, BASE, threshold, cap, k, nbins)
            assert (res.matches_counts, res.matches_bytes, res.topk_counts, res.topk_bytes, res.invalid) == \
                   (mc, mb, tc, tb, invalid), (first, n)
            assert res.bins.tobytes() == bins.tobytes(), (first, n)
            for parts in (MATCHES | TOPK, TOPK | HIST, MATCHES | HIST):
                same(bf.raw_report(eng, db, first, n, parts, threshold=threshold, cap=cap, k=k, nbins=nbins, index_base=BASE),
                     res, parts)
            for q, one in enumerate(singles):
                r1 = rf.raw_report(one, db, first, n, ALL, threshold, cap, k, nbins, index_base=BASE)
                assert (r1.matches_count, r1.matches_bytes, r1.topk_count, r1.topk_bytes, r1.invalid) == \
                       (res.matches_counts[q], res.matches_bytes[q], res.topk_counts[q], res.topk_bytes[q], res.invalid[q]), \
                       (q, first, n)
                assert r1.bins.tobytes() == res.bins[q].tobytes(), (q, first, n)
    finally:
        for s in singles:
            s.close()


# ---------------------------------------------------------------- 1. against the oracle, small


@pytest.mark.parametrize("variant,nq", VARIANTS, ids=[f"{v}-{nq}" for v, nq in VARIANTS])
def test_against_oracle(device, hooked_device, small, variant, nq):
    dev, layout = open_variant(variant, device, hooked_device)
    with small.db(dev, layout) as db, ih.TemplateBatchEngine(dev, small.queries[:nq]) as eng:
        for first, n in hf.RANGES:
            for parts in MULTI:
                for cap in sorted({0, 3, n}) if parts & MATCHES else [None]:
                    run(eng, db, small.exp, parts, first, n, 0.48, cap, 5, 64, BASE)
            for threshold, k, nbins in ((0.5, 64, 1024), (2.0, 1, 1), (0.0, 64, 2)):
                run(eng, db, small.exp, ALL, first, n, threshold, n, k, nbins, BASE)
        if nq == 17:  # queries 3 and 10 have zero masks: every record invalid, the lists empty
            res = run(eng, db, small.exp, ALL, 0, small.N, 2.0, small.N, 64, 64)
            for q in hf.LargeCase.ZERO_MASK:
                assert (res.matches_counts[q], res.topk_counts[q], res.invalid[q]) == (0, 0, small.N)
                assert not res.bins[q].any()
            assert res.matches_counts[0] == small.N - 1 and res.invalid[0] == 1  # the zero-mask record


# ---------------------------------------------------------------- 2. byte for byte against the siblings


@pytest.mark.parametrize("variant,nq", VARIANTS, ids=[f"{v}-{nq}" for v, nq in VARIANTS])
def test_equal_to_the_siblings_and_the_single_reports_small(device, hooked_device, small, variant, nq):
    dev, layout = open_variant(variant, device, hooked_device)
    with small.db(dev, layout) as db, ih.TemplateBatchEngine(dev, small.queries[:nq]) as eng:
        equal_to_siblings_and_singles(dev, eng, db, small.queries, hf.RANGES, 0.48, 7, 5, 64)
        equal_to_siblings_and_singles(dev, eng, db, small.queries, [(0, small.N)], 0.5, small.N, 64, 1024)


@pytest.mark.parametrize("variant", ["tiles", "tiles-k2"])
def test_large_ranges_against_the_oracle_and_the_siblings(device, hooked_device, large, variant):
    dev, _ = open_variant(variant, device, hooked_device)
    with large.db(dev) as db, ih.TemplateBatchEngine(dev, large.queries) as eng:
        for first, n in LARGE_RANGES:
            res = run(eng, db, large.exp, ALL, first, n, 0.46, 40, 16, 1024, BASE)
            for q in hf.LargeCase.ZERO_MASK:
                assert (res.matches_counts[q], res.topk_counts[q], res.invalid[q]) == (0, 0, n)
        equal_to_siblings_and_singles(dev, eng, db, large.queries, LARGE_RANGES, 0.46, 40, 64, 1024)


# ---------------------------------------------------------------- 3. the overflow rerun


def overflowing_blocks(exps, threshold, n):
    return {q // RERUN_BLOCK for q, e in enumerate(exps) if len(e.hits(threshold, 0, n)) > MATCH_FIRST_ROOM}


@pytest.mark.parametrize("threshold", [2.0, 0.47])
def test_overflow_reruns_the_overflowing_blocks_once(own_device, large, threshold):
    """cap = 3: the first pass has room for 1024 records a query.  Under 2.0 every valid record
    matches, so every block of four queries holds an overflowing one; under 0.47 the oracle says
    which do.  The top-k lists and the histograms are what a call without a rerun (cap = 0) gives, and
    an identical second call finds room for every list behind the lists: one pass."""
    dev, n = own_device, hf.LARGE_N
    blocks = overflowing_blocks(large.exp, threshold, n)
    assert blocks and (threshold != 2.0 or len(blocks) == 5)
    with large.db(dev) as db, ih.TemplateBatchEngine(dev, large.queries) as eng:
        quiet, launches = profiled(dev, lambda: run(eng, db, large.exp, ALL, 0, n, threshold, 0, 64, 1024, BASE))
        assert launches["template_batch_report"] == 1 and launches["template_batch_match"] == 0
        res, launches = profiled(dev, lambda: run(eng, db, large.exp, ALL, 0, n, threshold, 3, 64, 1024, BASE))
        assert launches["template_batch_report"] == 1 and launches["template_batch_match"] == len(blocks)
        assert launches["template_batch_topk"] == launches["template_batch_hist"] == 0
        if threshold == 2.0:
            for q in range(eng.nq):
                zero = q in hf.LargeCase.ZERO_MASK
                assert res.matches_counts[q] == (0 if zero else n)
                assert [m.index - BASE for m in res.matches[q]] == ([] if zero else [0, 1, 2])
        same(res, quiet, TOPK | HIST)
        again, launches = profiled(dev, lambda: run(eng, db, large.exp, ALL, 0, n, threshold, 3, 64, 1024, BASE))
        assert launches["template_batch_report"] == 1 and launches["template_batch_match"] == 0
        same(again, res, ALL)


# ---------------------------------------------------------------- 4. launch counts


def test_launch_counts_in_the_default_shape(device, small):
    with small.db(device, ih.LAYOUT_TILES) as db, ih.TemplateBatchEngine(device, small.queries) as eng, \
            ih.TemplateBatchEngine(device, small.queries[:3]) as few:
        args = (0, small.N, 0.48, 5, 5, 64)
        for parts in MULTI:
            _, launches = profiled(device, lambda: run(eng, db, small.exp, parts, *args))
            assert launches["template_batch_report"] == 1, (parts, launches)
            assert sum(launches.values()) == 1, (parts, launches)
        for parts, name in ((MATCHES, "template_batch_match"), (TOPK, "template_batch_topk"), (HIST, "template_batch_hist")):
            _, launches = profiled(device, lambda: run(eng, db, small.exp, parts, *args))
            assert launches[name] == 1 and sum(launches.values()) == 1, (parts, launches)
        _, launches = profiled(device, lambda: run(few, db, small.exp, ALL, *args))
        assert launches["template_report"] == 3 and sum(launches.values()) == 3, launches
        _, launches = profiled(device, lambda: run(eng, db, small.exp, ALL, 10, 0, 0.48, 5, 5, 64))  # n == 0: no launch
        assert not any(launches.values())


# ---------------------------------------------------------------- 5. identical calls


@pytest.mark.parametrize("variant,nq", GEMM + [("lanes", 3)], ids=[f"{v}-{nq}" for v, nq in GEMM + [("lanes", 3)]])
def test_identical_calls_return_identical_bytes(device, hooked_device, small, variant, nq):
    dev, layout = open_variant(variant, device, hooked_device)
    with small.db(dev, layout) as db, ih.TemplateBatchEngine(dev, small.queries[:nq]) as eng:
        a = run(eng, db, small.exp, ALL, 5, 200, 0.48, 200, 64, 1024, BASE)
        b = run(eng, db, small.exp, ALL, 5, 200, 0.48, 200, 64, 1024, BASE)
        same(a, b, ALL)
        # a smaller histogram and a shorter list after larger ones read nothing stale
        run(eng, db, small.exp, ALL, 0, small.N, 0.48, 3, 1, 2)
        run(eng, db, small.exp, TOPK | HIST, 0, small.N, None, None, 64, 1)
        same(run(eng, db, small.exp, ALL, 5, 200, 0.48, 200, 64, 1024, BASE), a, ALL)


# ---------------------------------------------------------------- 6. refusals write nothing


def test_refusals_write_nothing_and_leave_the_device_usable(device, own_device, small):
    good = dict(threshold=0.48, cap=4, k=5, nbins=64)
    with small.db(device, ih.LAYOUT_TILES) as db, small.db(device, ih.LAYOUT_LANES) as ldb, \
            small.db(own_device, ih.LAYOUT_TILES) as other_db, \
            ih.TemplateBatchEngine(device, small.queries[:6]) as eng, \
            ih.TemplateBatchEngine(device, small.queries[:3]) as few, \
            ih.TemplateEngine(device, small.queries[0]) as single:

        def refused(code, word, e=eng, d=db, first=0, n=small.N, parts=ALL, nq=None, **kw):
            args = dict(good)
            args.update(kw)
            res = bf.raw_report(e, d, first, n, parts, nq=nq, expect_rc=code, **args)
            assert word in res.error, (res.error, word)
            run(eng, db, small.exp, ALL, 0, small.N, **good)  # and the device is as usable as before

        for parts in (0, 8, 15):
            refused(E_ARG, "parts must be one or more", parts=parts)
        refused(E_ARG, "reserved must be 0", reserved=1)
        refused(E_ARG, "threshold is NaN", threshold=float("nan"))
        for k in (0, 65):
            refused(E_ARG, "IRIS_TOPK_MAX", k=k)
        for nbins in (3, 2048):
            refused(E_ARG, "IRIS_HIST_MAX_BINS", nbins=nbins)
        for field in ("matches", "matches_counts", "topk", "topk_counts", "bins", "invalid"):
            refused(E_ARG, "NULL", null=(field,))
        refused(E_ARG, "not a batched template engine", e=single, nq=1)
        refused(E_ARG, "TILES", d=ldb)  # a LANES database with nq > 3
        refused(E_RANGE, "", first=200, n=100)
        refused(E_ARG, "different devices", d=other_db)
        for parts in MULTI:  # and with two parts
            refused(E_RANGE, "", first=258, n=1, parts=parts)
        # an engine of up to 3 queries takes either layout
        run(few, ldb, small.exp, ALL, 0, small.N, **good)


# ---------------------------------------------------------------- 7. the mirrors


def test_python_mirror(device, small):
    with small.db(device, ih.LAYOUT_TILES) as db, ih.TemplateBatchEngine(device, small.queries) as eng:
        res = eng.report(db, ALL, threshold=0.48, cap=4, k=5, nbins=64, first=5, n=200, index_base=BASE)
        raw = bf.raw_report(eng, db, 5, 200, ALL, threshold=0.48, cap=4, k=5, nbins=64, index_base=BASE)
        assert res.matches_counts == raw.matches_counts and list(res.invalid) == raw.invalid
        assert (res.bins == raw.bins).all()
        for q in range(eng.nq):
            assert b"".join(bytes(m) for m in res.matches[q]) == raw.matches_bytes[q]
            assert b"".join(bytes(m) for m in res.topk[q]) == raw.topk_bytes[q]
        two = eng.report(db, TOPK | HIST, k=5, nbins=64, first=5, n=200, index_base=BASE)
        assert two.matches is None and two.matches_counts is None and (two.bins == raw.bins).all()
        with pytest.raises(ih.IrisError):
            eng.report(db, ALL, threshold=0.48, cap=4, k=5, nbins=1000)


@pytest.mark.parametrize("nq,layout", [(3, ih.LAYOUT_LANES), (17, ih.LAYOUT_TILES)], ids=["3-lanes", "17-tiles"])
def test_cpp_program_equals_the_c_call(device, small, nq, layout, tmp_path):
    """tests/cpp/template_batch_report.cpp through iris_hip.hpp, as its own process, on the small
    case: the bytes of every part equal the raw C call's."""
    first, n, threshold, cap, k, nbins = 5, 250, 0.48, 6, 5, 64
    exe = build_cpp_program(tmp_path)
    (tmp_path / "templates.bin").write_bytes(np.ascontiguousarray(small.case.templates).tobytes())
    (tmp_path / "queries.bin").write_bytes(np.ascontiguousarray(small.queries[:nq]).tobytes())
    out = tmp_path / "report.bin"
    r = subprocess.run([str(exe), str(tmp_path / "templates.bin"), str(small.N), str(tmp_path / "queries.bin"), str(nq),
                        str(layout), str(first), str(n), str(BASE), repr(threshold), str(cap), str(k), str(nbins), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    with small.db(device, layout) as db, ih.TemplateBatchEngine(device, small.queries[:nq]) as eng:
        want = run(eng, db, small.exp, ALL, first, n, threshold, cap, k, nbins, BASE)
    raw, pos = out.read_bytes(), 0

    def word():
        nonlocal pos
        pos += 8
        return int(np.frombuffer(raw, np.uint64, 1, pos - 8)[0])

    def take(count):
        nonlocal pos
        pos += count
        return raw[pos - count:pos]

    for q in range(nq):
        assert word() == want.matches_counts[q]
        assert take(word() * bf.SIZE) == want.matches_bytes[q]
        assert take(word() * bf.SIZE) == want.topk_bytes[q]
        assert take(8 * nbins) == want.bins[q].tobytes()
        assert word() == want.invalid[q]
    assert pos == len(raw)
