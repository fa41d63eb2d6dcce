"""GPU: the resolver reports (iris_resolver_report, iris_resolver_report_masks) -- the match list, the
k closest records and the distance histogram of one probe from one read of the participants' share
rows.  Every expectation comes from the CPU oracle (resolver_report_fixtures.py over
resolver_hist_fixtures.py's cases: oc.masks_batch for the denominators, resolver_expected's decoded
best rotations, hist_fixtures.expected's binning), never from the library's own sibling calls; the
one exception is the test whose subject is that the parts equal the siblings' outputs byte for byte.

Variants as in test_gpu_resolver_histogram.py: a TILES database under the library's own dispatch,
TILES with IRIS_TILES_PER_WAVE=1 and =4 (the hook pins masks_mfma_kernel<MASKS_REPORT> at one tile
per wave and at its large form on ranges of any size) and a LANES database (the masks kernel into the
workspace, then resolver_kernel's report mode).  The C entry points are called raw
(resolver_report_fixtures.raw_report): guard bytes fill the fields of unselected parts and stand
behind every output array."""
import ctypes
import subprocess

import numpy as np
import pytest

import hist_fixtures as hf
import iris_hip as ih
import report_fixtures as tf
import resolver_hist_fixtures as rhf
import resolver_report_fixtures as rr
from oracle import oracle_c as oc
from resolver_report_fixtures import ALL, HIST, MATCHES, TOPK
from test_gpu_masks_batch_matches import background, planted_shares
from test_gpu_matches import DeviceArrays, resolver_expected
from test_resolver_report_abi import build_cpp_program

pytestmark = pytest.mark.gpu
ROT = 31
E_ARG, E_RANGE = -1, -5
INF = float("inf")
VARIANTS = ["tiles", "tiles-tpw1", "tiles-tpw4", "lanes"]
BASE = 2**40 + 7
ABOVE_QUARTER = float(np.nextafter(0.25, np.inf))
LARGE_RANGES = [(0, hf.LARGE_N), (4090 * 32 + 5, 250), (37, 100000)]
PASSES = ("masks_report", "masks_match", "masks_topk", "masks_resolve_hist", "resolver_report", "resolver_match",
          "resolver_topk", "resolver_hist", "masks", "topk_merge", "hist_reduce")
SIBLINGS = ("masks_match", "masks_topk", "masks_resolve_hist", "resolver_match", "resolver_topk", "resolver_hist")
# (threshold, k, nbins): the k and the bin counts of the issue; thresholds around the planted quarter
SETTINGS = [(0.25, 1, 1), (ABOVE_QUARTER, 16, 64), (0.5, 64, 1024)]


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
    return rhf.small_case()


@pytest.fixture(scope="module")
def large():
    return rhf.large_case()


def profiled(device, call):
    """call() under profiling -> (its result, {pass name: launches})."""
    device.reset_stats()
    device.set_profiling(True)
    try:
        res = call()
    finally:
        device.set_profiling(False)
    return res, {name: device.kernel_stats(name)[0] for name in PASSES}


def run(call, e, parts, first, n, threshold=None, cap=None, k=None, nbins=None, base=0, fill=rr.GUARD_BYTE):
    """One raw call, checked against the oracle -> its result."""
    res = rr.raw_report(call, n, parts, threshold, cap, k, nbins, fill=fill)
    rr.check(e, res, parts, first, n, threshold, cap, k, nbins, base)
    return res


def result_bytes(r):
    return (r.matches_bytes, r.matches_count, r.topk_bytes, r.topk_count, None if r.bins is None else r.bins.tobytes(),
            r.invalid)


# ---------------------------------------------------------------- 1. against the oracle, small


def test_masks_form_against_oracle(ctx, case):
    """Every subset, range, part count, alignment, k and bin count on 257 masks: 9 tiles with a
    one-record last tile, record 77 zero, query GARBAGE's slab with distances above 1."""
    device, layout = ctx
    with case.db(device, layout) as db:
        for q in (0, case.GARBAGE):
            with ih.MasksEngine(device, case.qmasks[q]) as eng:
                for parts in rhf.PARTS:
                    e = case.exp[parts][q]
                    for offset in (0, 2):
                        for first, n in rhf.RANGES:
                            with DeviceArrays(device, case.shares[parts][:, q, first:first + n], offset) as ptrs:
                                call = rr.masks_call(eng, db, first, n, ptrs)
                                for sub in rr.SUBSETS:
                                    run(call, e, sub, first, n, 0.405, None, 5, 64)
                                for threshold, k, nbins in SETTINGS:
                                    run(call, e, ALL, first, n, threshold, None, k, nbins)
                                based = rr.masks_call(eng, db, first, n, ptrs, index_base=BASE)
                                for cap in (0, 3, None):
                                    run(based, e, ALL, first, n, 0.405, cap, 16, 64, base=BASE)
                                run(based, e, MATCHES | HIST, first, n, INF, None, None, 2, base=BASE)


def test_denominators_given_against_oracle(device, case):
    """iris_resolver_report over the oracle's denominators of the same case: resolver_kernel's report
    mode, rows from 0, one workgroup of 256 rows and one of a single row."""
    for q in (0, case.GARBAGE):
        for parts in rhf.PARTS:
            e = case.exp[parts][q]
            for offset in (0, 2):
                with DeviceArrays(device, list(case.shares[parts][:, q]) + [case.den[q]], offset) as ptrs:
                    for n in (257, 256, 200, 65, 1, 0):
                        call = rr.plain_call(device, ptrs[:-1], ptrs[-1], n)
                        for sub in rr.SUBSETS:
                            run(call, e, sub, 0, n, 0.405, None, 5, 64)
                        for threshold, k, nbins in SETTINGS:
                            run(call, e, ALL, 0, n, threshold, None, k, nbins)
                        based = rr.plain_call(device, ptrs[:-1], ptrs[-1], n, index_base=BASE)
                        for cap in (0, 3, None):
                            run(based, e, ALL, 0, n, 0.405, cap, 16, 64, base=BASE)


@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "offset2"])
def test_arbitrary_denominators(device, offset):
    """Denominators anywhere in u16 that are no masks engine's (above 12800, zeros among them) and
    uniform shares; rows 10..19 decode to uneq above their denominators in every rotation, so their
    distances lie above 1: they are in the last bin, match only above 1 and rank last; rows of zeros
    are invalid; 1000 rows are four workgroups, the last one partial."""
    n = 1000
    rng = np.random.default_rng(11)
    den = rng.integers(0, 2**16, (n, ROT), dtype=np.uint16)
    den[::7, ::2] = 0
    den[5] = 0
    den[n - 1] = 0
    den[10:20] = rng.integers(12801, 25000, (10, ROT), dtype=np.uint16)
    for parts in rhf.PARTS:
        shares = rng.integers(0, 2**16, (parts, n, ROT), dtype=np.uint16)
        shares[:, 10:20] = planted_shares(rng, den[10:20], rng.integers(26000, 32768, (10, ROT)), parts)
        e = resolver_expected(shares, den)
        assert (e.den > 12800).any() and (e.num[10:20] > e.den[10:20]).all() and (e.den == 0).sum() == 2
        assert (e.dist[10:20] > 1.0).all() and hf.expected(e.dist, 1024, 10, 10)[0][1023] == 10
        with DeviceArrays(device, list(shares) + [den], offset) as ptrs:
            for m in (n, 257, 64, 1):
                call = rr.plain_call(device, ptrs[:-1], ptrs[-1], m, index_base=BASE)
                for threshold, k, nbins in [(0.01, 1, 1), (0.3, 16, 64), (1.5, 64, 1024), (INF, 64, 2)]:
                    for sub in (ALL, MATCHES | TOPK, TOPK | HIST):
                        run(call, e, sub, 0, m, threshold, None, k, nbins, base=BASE)


# ---------------------------------------------------------------- 2. equal to the siblings, byte for byte


def sibling_bytes(masks, eng, db, device, first, n, ptrs, den_ptr, threshold, cap, k, nbins, base):
    lib = ih.load_library()
    cap = n if cap is None else cap
    marr, tarr = tf.match_array(cap), tf.match_array(k)
    count, tcount, invalid = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint64()
    bins = np.zeros(nbins, np.uint64)
    arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    m = marr if cap else None
    if masks:
        assert lib.iris_resolver_matches_masks(eng.handle, db.handle, first, n, arr, len(ptrs), base, threshold, m, cap,
                                               ctypes.byref(count)) == 0
        assert lib.iris_resolver_topk_masks(eng.handle, db.handle, first, n, arr, len(ptrs), base, k, tarr,
                                            ctypes.byref(tcount)) == 0
        assert lib.iris_resolver_histogram_masks(eng.handle, db.handle, first, n, arr, len(ptrs), nbins, bins.ctypes.data,
                                                 ctypes.addressof(invalid)) == 0
    else:
        assert lib.iris_resolver_matches(device.handle, arr, len(ptrs), den_ptr, n, base, threshold, m, cap,
                                         ctypes.byref(count)) == 0
        assert lib.iris_resolver_topk(device.handle, arr, len(ptrs), den_ptr, n, base, k, tarr, ctypes.byref(tcount)) == 0
        assert lib.iris_resolver_histogram(device.handle, arr, len(ptrs), den_ptr, n, nbins, bins.ctypes.data,
                                           ctypes.addressof(invalid)) == 0
    size = ctypes.sizeof(ih.Match)
    return (bytes(marr)[:min(count.value, cap) * size], count.value, bytes(tarr)[:tcount.value * size], tcount.value,
            bins.tobytes(), invalid.value)


def test_equal_to_the_siblings_byte_for_byte(ctx, case):
    device, layout = ctx
    q = case.GARBAGE
    with case.db(device, layout) as db, ih.MasksEngine(device, case.qmasks[q]) as eng:
        for first, n in rhf.RANGES:
            with DeviceArrays(device, list(case.shares[3][:, q, first:first + n]) + [case.den[q][first:first + n]]) as ptrs:
                for masks in (True, False):
                    call = rr.masks_call(eng, db, first, n, ptrs[:3], BASE) if masks else \
                        rr.plain_call(device, ptrs[:3], ptrs[3], n, BASE)
                    small = None
                    for threshold, cap, k, nbins in [(0.405, None, 5, 64), (0.5, 3, 64, 1024), (2.0, 0, 1, 1)]:
                        want = sibling_bytes(masks, eng, db, device, first, n, ptrs[:3], ptrs[3], threshold, cap, k, nbins, BASE)
                        for sub in rr.SUBSETS:
                            r = rr.raw_report(call, n, sub, threshold, cap, k, nbins)
                            if sub & MATCHES:
                                assert (r.matches_bytes, r.matches_count) == want[0:2], (masks, first, n, sub)
                            if sub & TOPK:
                                assert (r.topk_bytes, r.topk_count) == want[2:4], (masks, first, n, sub)
                            if sub & HIST:
                                assert (r.bins.tobytes(), r.invalid) == want[4:6], (masks, first, n, sub)
                        if k == 5:
                            small = want[2]
                        if k == 64 and small is not None:  # a smaller k is a prefix
                            assert want[2][:len(small)] == small
                    # the prefix sum of j bins is the matches part's total at threshold j / nbins
                    bins = rr.raw_report(call, n, HIST, nbins=64).bins
                    prefix = np.concatenate([[0], np.cumsum(bins, dtype=np.uint64)])
                    for j in (0, 1, 16, 17, 29, 40, 63):
                        r = rr.raw_report(call, n, MATCHES | HIST, j / 64, 0, None, 64)
                        assert r.matches_count == int(prefix[j]) and r.bins.tobytes() == bins.tobytes(), (masks, first, n, j)


# ---------------------------------------------------------------- 3. ties


class TieCase:
    """The small case's masks under query 1, background uneq in [0.4 den, 0.6 den).  Exactly 1/4 --
    equal fractions in different terms -- is planted in two records of one tile (3, 4), in a second
    tile of the same four-tile group and of the same 64-row resolver wave (40), in a second group
    (130, 131) and in the one-record last tile, the first row of the resolver's second workgroup (256);
    records 40 and 131 hold it in TWO rotations, so the lower rotation is the record's."""

    Q = 1
    TIED = (3, 4, 40, 130, 131, 256)
    TWICE = (40, 131)

    def __init__(self):
        c = rhf.small_case()
        rng = np.random.default_rng(99)
        self.den = c.den[self.Q]
        d = self.den.astype(np.int64)
        uneq = background(rng, self.den, 0.4, 0.6)
        self.rot = {}
        for rec in self.TIED:
            ks = [k for k in range(ROT) if d[rec, k] % 4 == 0 and d[rec, k] >= 2048]
            assert len(ks) >= 2, rec
            for k in ks[:2] if rec in self.TWICE else ks[:1]:
                uneq[rec, k] = d[rec, k] // 4
            self.rot[rec] = ks[0] - 15
        self.shares = planted_shares(rng, self.den, uneq, 3)
        self.exp = resolver_expected(self.shares, self.den)


def test_ties(ctx, case):
    device, layout = ctx
    t = TieCase()
    e = t.exp
    assert all(e.dist[i] == 0.25 and e.rot[i] == t.rot[i] for i in t.TIED)
    assert len({int(e.den[i]) for i in t.TIED}) > 1  # different terms
    assert list(rr.order(e, 0, case.N)[:len(t.TIED)]) == list(t.TIED) and list(e.hits(ABOVE_QUARTER)) == list(t.TIED)
    with case.db(device, layout) as db, ih.MasksEngine(device, case.qmasks[t.Q]) as eng:
        for first, n in [(0, case.N), (4, 253), (5, 200)]:
            with DeviceArrays(device, list(t.shares[:, first:first + n]) + [t.den[first:first + n]]) as ptrs:
                for call in (rr.masks_call(eng, db, first, n, ptrs[:3], BASE), rr.plain_call(device, ptrs[:3], ptrs[3], n, BASE)):
                    for k in (1, 3, 64):
                        res = run(call, e, ALL, first, n, ABOVE_QUARTER, None, k, 1024, base=BASE)
                        run(call, e, MATCHES | TOPK, first, n, 0.25, None, k, base=BASE)
                    want = [BASE + i - first for i in t.TIED if first <= i < first + n]
                    assert [m.index for m in res.matches] == want and [m.index for m in res.topk[:len(want)]] == want
                    assert [m.rotation for m in res.matches] == [t.rot[i] for i in t.TIED if first <= i < first + n]


# ---------------------------------------------------------------- 4. large ranges


@pytest.mark.parametrize("tpw", [None, 1, 4], ids=["dispatch", "tpw1", "tpw4"])
def test_large_range(device, hooked_device, large, tpw):
    """4098 * 32 + 27 masks, 3 parts: waves walk several tile groups, the last tile is ragged, record
    ZERO is invalid; sub-ranges that start and end inside tiles.  Two or three parts launch one report
    pass and no sibling pass; one part launches the sibling's pass alone."""
    dev = device if tpw is None else hooked_device(IRIS_TILES_PER_WAVE=tpw)
    e = large.exp[0]
    with large.db(dev) as db, ih.MasksEngine(dev, large.qmasks[0]) as eng:
        for first, n in LARGE_RANGES:
            with DeviceArrays(dev, large.shares[:, 0, first:first + n]) as ptrs:
                call = rr.masks_call(eng, db, first, n, ptrs, BASE)
                res, launches = profiled(dev, lambda: run(call, e, ALL, first, n, 0.052, None, 64, 1024, base=BASE))
                assert launches["masks_report"] == 1 and launches["topk_merge"] == 1 and launches["hist_reduce"] == 1
                assert not any(launches[p] for p in SIBLINGS + ("resolver_report", "masks")), launches
                if n == hf.LARGE_N:
                    assert res.matches_count > 100 and res.invalid == 1
                    for sub in (MATCHES | TOPK, MATCHES | HIST, TOPK | HIST):
                        _, launches = profiled(dev, lambda: run(call, e, sub, first, n, 0.0505, None, 16, 64, base=BASE))
                        assert launches["masks_report"] == 1 and not any(launches[p] for p in SIBLINGS), (sub, launches)
                    for sub, name in ((MATCHES, "masks_match"), (TOPK, "masks_topk"), (HIST, "masks_resolve_hist")):
                        _, launches = profiled(dev, lambda: run(call, e, sub, first, n, 0.0505, None, 16, 64, base=BASE))
                        assert launches["masks_report"] == 0 and launches[name] == 1, (sub, launches)
                        assert sum(launches[p] for p in SIBLINGS) == 1
        g = large.exp[large.GARBAGE]
        with ih.MasksEngine(dev, large.qmasks[large.GARBAGE]) as geng, \
                DeviceArrays(dev, large.shares[:, large.GARBAGE]) as ptrs:
            res = run(rr.masks_call(geng, db, 0, hf.LARGE_N, ptrs), g, ALL, 0, hf.LARGE_N, 0.01, 100, 64, 1024)
            assert res.bins[1023] > 1000


def test_one_part_runs_the_siblings_pass_on_every_form(ctx, case):
    device, layout = ctx
    tiles = layout == ih.LAYOUT_TILES
    e = case.exp[3][0]
    names = ("masks_match", "masks_topk", "masks_resolve_hist") if tiles else ("resolver_match", "resolver_topk", "resolver_hist")
    report = "masks_report" if tiles else "resolver_report"
    with case.db(device, layout) as db, ih.MasksEngine(device, case.qmasks[0]) as eng, \
            DeviceArrays(device, list(case.shares[3][:, 0]) + [case.den[0]]) as ptrs:
        call = rr.masks_call(eng, db, 0, case.N, ptrs[:3])
        for sub, name in zip((MATCHES, TOPK, HIST), names):
            _, launches = profiled(device, lambda: run(call, e, sub, 0, case.N, 0.405, None, 5, 64))
            assert launches[report] == 0 and launches[name] == 1 and sum(launches[p] for p in SIBLINGS) == 1, (sub, launches)
        _, launches = profiled(device, lambda: run(call, e, ALL, 0, case.N, 0.405, None, 5, 64))
        assert launches[report] == 1 and not any(launches[p] for p in SIBLINGS)
        assert launches["masks"] == (0 if tiles else 1)
        _, launches = profiled(device, lambda: run(rr.masks_call(eng, db, 10, 0, ptrs[:3]), e, ALL, 10, 0, 0.405, None, 5, 64))
        assert not any(launches.values())  # n == 0: nothing is launched
        plain = rr.plain_call(device, ptrs[:3], ptrs[3], case.N)
        for sub, name in zip((MATCHES, TOPK, HIST), ("resolver_match", "resolver_topk", "resolver_hist")):
            _, launches = profiled(device, lambda: run(plain, e, sub, 0, case.N, 0.405, None, 5, 64))
            assert launches["resolver_report"] == 0 and launches[name] == 1 and sum(launches[p] for p in SIBLINGS) == 1
        _, launches = profiled(device, lambda: run(plain, e, TOPK | HIST, 0, case.N, None, None, 5, 64))
        assert launches["resolver_report"] == 1 and not any(launches[p] for p in SIBLINGS) and launches["masks"] == 0


# ---------------------------------------------------------------- 5. the overflow rerun


@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles", "lanes"])
def test_overflowing_match_list_runs_the_matches_part_again(hooked_device, large, layout):
    """Threshold 0.5 matches far more than the first pass's 1024 records of room; cap = 10.  The
    report pass runs once and the plain match pass once; on LANES the masks kernel runs once for both."""
    device = hooked_device()  # a fresh device: its match buffer has not grown
    e = large.exp[0]
    tiles = layout == ih.LAYOUT_TILES
    report, match = ("masks_report", "masks_match") if tiles else ("resolver_report", "resolver_match")
    with ih.Database(device, ih.KIND_MASKS, large.N, layout) as db, ih.MasksEngine(device, large.qmasks[0]) as eng, \
            DeviceArrays(device, large.shares[:, 0]) as ptrs:
        db.generate(large.N, large.SEED)
        db.write(large.ZERO, large.masks[large.ZERO][None, :])
        call = rr.masks_call(eng, db, 0, large.N, ptrs)
        res, launches = profiled(device, lambda: run(call, e, ALL, 0, large.N, 0.5, 10, 64, 1024))
        hits = e.hits(0.5)
        assert res.matches_count == len(hits) > rr.MATCH_FIRST_ROOM and [m.index for m in res.matches] == list(hits[:10])
        assert launches[report] == 1 and launches[match] == 1 and launches["masks"] == (0 if tiles else 1), launches
        assert launches["topk_merge"] == 1 and sum(launches[p] for p in SIBLINGS) == 1
        # the rerun grew the buffer past the top-k lists: the same call again finds room behind them and
        # is one pass, at every k -- a steady list length reruns once, not in every call
        for k in (64, 1, 16):
            res, launches = profiled(device, lambda: run(call, e, ALL, 0, large.N, 0.5, 10, k, 1024))
            assert res.matches_count == len(hits) and launches[report] == 1, (k, launches)
            assert not any(launches[p] for p in SIBLINGS) and launches["masks"] == (0 if tiles else 1), (k, launches)
    device = hooked_device()
    with large.db(device) as db, ih.MasksEngine(device, large.qmasks[0]) as eng, DeviceArrays(device, large.shares[:, 0]) as ptrs:
        call = rr.masks_call(eng, db, 0, large.N, ptrs)
        res, launches = profiled(device, lambda: run(call, e, ALL, 0, large.N, 0.5, 0, 64, 1024))
        assert res.matches == [] and launches["masks_report"] == 1 and launches["masks_match"] == 0  # cap 0 only counts


# ---------------------------------------------------------------- 6. IRIS_HIST_COPIES


@pytest.mark.parametrize("copies", [1, 2, 64])
def test_counter_copies_do_not_change_the_bytes(hooked_device, case, large, copies):
    dev = hooked_device(IRIS_HIST_COPIES=copies)
    assert dev.config()["hist_copies"] == str(copies)
    q = case.GARBAGE
    for layout in (ih.LAYOUT_TILES, ih.LAYOUT_LANES):
        with case.db(dev, layout) as db, ih.MasksEngine(dev, case.qmasks[q]) as eng, \
                DeviceArrays(dev, list(case.shares[3][:, q, 5:]) + [case.den[q][5:]]) as ptrs:
            for nbins in (1, 1024):
                run(rr.masks_call(eng, db, 5, 252, ptrs[:3]), case.exp[3][q], ALL, 5, 252, 0.3, None, 5, nbins)
                run(rr.plain_call(dev, ptrs[:3], ptrs[3], 252), case.exp[3][q], TOPK | HIST, 5, 252, None, None, 5, nbins)
    with large.db(dev) as db, ih.MasksEngine(dev, large.qmasks[0]) as eng, DeviceArrays(dev, large.shares[:, 0]) as ptrs:
        call = rr.masks_call(eng, db, 0, large.N, ptrs)
        _, launches = profiled(dev, lambda: run(call, large.exp[0], ALL, 0, large.N, 0.0505, None, 64, 1024))
        assert launches["masks_report"] == 1 and launches["hist_reduce"] == (0 if copies == 1 else 1)
        assert launches["masks_resolve_hist"] == 0


# ---------------------------------------------------------------- 7. refusals on the device


def test_refusals_leave_everything_alone(ctx, case):
    device, layout = ctx
    e = case.exp[3][0]
    with case.db(device, layout) as db, ih.MasksEngine(device, case.qmasks[0]) as eng, \
            ih.MasksBatchEngine(device, case.qmasks[:3]) as batch, \
            ih.TemplateEngine(device, oc.gen_templates(99, 0, 1)[0]) as te, \
            ih.Database(device, ih.KIND_TEMPLATES, 300, layout) as tdb, \
            DeviceArrays(device, list(case.shares[3][:, 0]) + [case.den[0]]) as ptrs:
        tdb.generate(257, 8)
        sh, null_part = ptrs[:3], [ptrs[0], None, ptrs[2]]
        for sub in (ALL, MATCHES | HIST, TOPK):
            args = (sub, 0.405, 4, 5, 64)
            r = rr.raw_report(rr.masks_call(batch, db, 0, 257, sh), 257, *args, expect_rc=E_ARG)
            assert "batch" in r.error
            rr.raw_report(rr.masks_call(te, db, 0, 257, sh), 257, *args, expect_rc=E_ARG)  # a template engine
            rr.raw_report(rr.masks_call(eng, tdb, 0, 257, sh), 257, *args, expect_rc=E_ARG)  # a templates database
            rr.raw_report(rr.masks_call(eng, db, 200, 58, sh), 58, *args, expect_rc=E_RANGE)
            rr.raw_report(rr.masks_call(eng, db, 257, 1, sh), 1, *args, expect_rc=E_RANGE)
            rr.raw_report(rr.masks_call(eng, db, 0, 257, null_part), 257, *args, expect_rc=E_ARG)
            rr.raw_report(rr.masks_call(eng, db, 0, 257, None, nparts=3), 257, *args, expect_rc=E_ARG)
            rr.raw_report(rr.masks_call(eng, db, 0, 257, sh + sh + sh, nparts=9), 257, *args, expect_rc=E_ARG)
            rr.raw_report(rr.plain_call(device, null_part, ptrs[3], 257), 257, *args, expect_rc=E_ARG)
            rr.raw_report(rr.plain_call(device, sh, 0, 257), 257, *args, expect_rc=E_ARG)  # no denominators
            rr.raw_report(rr.plain_call(device, sh, ptrs[3], 257, nparts=0), 257, *args, expect_rc=E_ARG)
            rr.raw_report(rr.plain_call(None, sh, ptrs[3], 257), 257, *args, expect_rc=E_ARG)
        # and the device is as usable as before
        run(rr.masks_call(eng, db, 0, 257, sh), e, ALL, 0, 257, 0.405, None, 5, 64)
        run(rr.plain_call(device, sh, ptrs[3], 257), e, ALL, 0, 257, 0.405, None, 5, 64)
        with pytest.raises(ih.IrisError):
            eng.report(db, sh, nbins=1000)
        with pytest.raises(ih.IrisError):
            eng.report(db, sh)


# ---------------------------------------------------------------- 8. neighbours undisturbed, outputs overwritten


def test_neighbours_undisturbed_and_outputs_overwritten(ctx, case):
    """The report shares the device's match, counter and result buffers with its siblings by region:
    a sibling straight after a report and a report after each sibling equal the oracle; identical
    calls into differently filled arrays return identical bytes."""
    device, layout = ctx
    e = case.exp[3][0]
    with case.db(device, layout) as db, ih.MasksEngine(device, case.qmasks[0]) as eng, \
            DeviceArrays(device, case.shares[3][:, 0]) as ptrs:
        call = rr.masks_call(eng, db, 0, 257, ptrs)
        for step in range(3):
            run(call, e, ALL, 0, 257, 0.5, None, 64, 1024)
            if step == 0:
                got, count = eng.matches(db, ptrs, 0.405)
                assert count == len(e.hits(0.405)) and [g.index for g in got] == list(e.hits(0.405))
            elif step == 1:
                assert [x.index for x in eng.topk(db, ptrs, 5)] == list(rr.order(e, 0, 257)[:5])
            else:
                bins, invalid = eng.histogram(db, ptrs, 1024)
                assert (bins == hf.expected(e.dist, 1024)[0]).all() and invalid == 1
            run(call, e, ALL, 0, 257, 0.405, None, 5, 64)
        a = run(call, e, ALL, 0, 257, 0.405, None, 5, 1024)
        b = run(call, e, ALL, 0, 257, 0.405, None, 5, 1024, fill=0x07)
        assert result_bytes(a) == result_bytes(b)
        run(call, e, ALL, 0, 257, 0.405, None, 5, 2)  # a smaller histogram after a larger one reads no stale counter
        run(call, e, TOPK | HIST, 0, 257, None, None, 64, 1)


# ---------------------------------------------------------------- 9. the mirrors


def test_python_mirrors(ctx, case):
    device, layout = ctx
    e = case.exp[3][0]
    with case.db(device, layout) as db, ih.MasksEngine(device, case.qmasks[0]) as eng, \
            DeviceArrays(device, list(case.shares[3][:, 0, 5:205]) + [case.den[0][5:205]]) as ptrs:
        for r in (eng.report(db, ptrs[:3], threshold=0.405, k=5, nbins=64, first=5, n=200, index_base=BASE),
                  ih.resolver_report(device, ptrs[:3], ptrs[3], 200, threshold=0.405, k=5, nbins=64, index_base=BASE)):
            hits = e.hits(0.405, 5, 200)
            assert r.matches_count == len(hits) > 0
            tf.check_list(e, r.matches, hits, BASE - 5)
            tf.check_list(e, r.topk, rr.order(e, 5, 200)[:5], BASE - 5)
            want, want_invalid = hf.expected(e.dist, 64, 5, 200)
            assert r.bins.dtype == np.uint64 and (r.bins == want).all() and r.invalid == want_invalid == 1
        # unselected parts are None; a cap keeps the lowest indices and the exact total
        r = eng.report(db, ptrs[:3], threshold=0.5, cap=3, k=1, first=5, n=200)
        assert r.bins is None and r.invalid is None and r.matches_count == len(e.hits(0.5, 5, 200)) and len(r.matches) == 3
        tf.check_list(e, r.matches, e.hits(0.5, 5, 200)[:3], -5)
        r = ih.resolver_report(device, ptrs[:3], ptrs[3], 200, nbins=1024)
        assert r.matches is None and r.matches_count is None and r.topk is None
        assert (r.bins == hf.expected(e.dist, 1024, 5, 200)[0]).all()


def test_python_mirror_fetches_a_long_list(device, large):
    """cap=None past the combined pass's first 1024 records: the rest comes through matches()."""
    e = large.exp[0]
    with large.db(device) as db, ih.MasksEngine(device, large.qmasks[0]) as eng, DeviceArrays(device, large.shares[:, 0]) as ptrs:
        r = eng.report(db, ptrs, threshold=0.052, k=64)
        hits = e.hits(0.052)
        assert r.matches_count == len(hits) > 1024 and [m.index for m in r.matches] == list(hits)
        tf.check_list(e, r.topk, rr.order(e, 0, large.N)[:64], 0)


@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles", "lanes"])
def test_cpp_resolver_report(layout, tmp_path):
    """tests/cpp/resolver_report.cpp through iris_hip.hpp on generated masks, against the oracle."""
    n, seed, threshold, k, nbins = 700, 41, 0.2, 7, 64
    exe = build_cpp_program(tmp_path)
    out = subprocess.run([str(exe), str(n), str(seed), str(layout), repr(threshold), "-1", str(k), str(nbins)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    with np.errstate(over="ignore"):
        qm = (np.arange(ih.LIMBS, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    rows = n - 1
    el = np.arange(rows * ROT, dtype=np.uint64)
    shares = np.stack([(((el * 2654435761) & 0xFFFFFFFF) >> 7) + 12345 * p for p in range(2)]).astype(np.uint16)
    shares = shares.reshape(2, rows, ROT)
    e = resolver_expected(shares, oc.masks_batch(qm, oc.gen_masks(seed, 0, n))[1:])
    hits, top = e.hits(threshold), rr.order(e, 0, rows)[:k]
    assert 3 < len(hits) < rows
    bins, invalid = hf.expected(e.dist, nbins)
    part = [["count", str(len(hits))]]
    part += [["m", str(1000 + int(i)), str(e.num[i]), str(e.den[i]), str(e.rot[i])] for i in hits]
    part += [["t", str(1000 + int(i)), str(e.num[i]), str(e.den[i]), str(e.rot[i])] for i in top]
    part += [["b"] + [str(int(b)) for b in bins], ["invalid", str(invalid)]]
    want = [["form", "masks"]] + part + [["form", "plain"]] + part + [["only"] + [str(1000 + int(i)) for i in top]]
    assert [ln.split() for ln in out.stdout.strip().split("\n")] == want


def test_three_party_flow(ctx):
    """257 planted templates shared among three parties, each party's rows from the oracle's
    DistanceEngine, summed and resolved in the report call: every part is iris_template_report's over
    the plaintext database for the same probe, threshold, k and nbins."""
    device, layout = ctx
    c = hf.single_case()
    shares, masks = oc.prepare_shares(c.templates, bytes(range(32)))
    with ih.Database(device, ih.KIND_TEMPLATES, 300, layout) as tdb, ih.Database(device, ih.KIND_MASKS, 300, layout) as mdb:
        tdb.append(c.templates)
        mdb.append(masks)
        for key, query in c.queries.items():
            rows = [oc.distance_batch(oc.encode(query), shares[p]) for p in range(3)]
            with ih.TemplateEngine(device, query) as te, ih.MasksEngine(device, query[200:]) as me, \
                    DeviceArrays(device, rows) as ptrs:
                for threshold, k, nbins in [(0.48, 5, 64), (0.5, 64, 1024), (0.26, 1, 1)]:
                    plain = tf.raw_report(te, tdb, 0, 257, ALL, threshold, None, k, nbins, index_base=BASE)
                    want, want_invalid = hf.expected(c.dist[key], nbins)
                    assert (plain.bins == want).all() and plain.invalid == want_invalid == 1
                    for sub in (ALL, MATCHES | TOPK, TOPK | HIST):
                        got = rr.raw_report(rr.masks_call(me, mdb, 0, 257, ptrs, BASE), 257, sub, threshold, None, k, nbins)
                        if sub & MATCHES:
                            assert (got.matches_bytes, got.matches_count) == (plain.matches_bytes, plain.matches_count)
                        if sub & TOPK:
                            assert (got.topk_bytes, got.topk_count) == (plain.topk_bytes, plain.topk_count)
                        if sub & HIST:
                            assert got.bins.tobytes() == plain.bins.tobytes() and got.invalid == plain.invalid
