"""GPU: template batch top-k (iris_template_batch_topk): for every query of a template batch
engine, the k closest records of a range, best first -- against lists built here from the CPU oracle
(oc.template_counts per query: the best rotation in the exact fraction order, lowest rotation on
ties; records by exact fraction, then by index; records without a valid rotation excluded), byte for
byte against the single-query iris_template_topk calls it replaces, and against
iris_template_batch_search for the first entry.

Variants: engines of up to 3 queries run one single-query pass per query (TILES and LANES
databases); more than 3 run the batched GEMM's top-k form on a TILES database, in its default shape
(2 queries x 16 tiles per workgroup) and under IRIS_BATCH_KERNEL=2 (4 queries x 8 tiles, staggered
waves).  The fixtures of tests/test_gpu_template_batch_matches.py are used unchanged."""
import ctypes
import fractions
import subprocess

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_gpu_template_batch_matches import Expected, SmallCase, WideCase, open_variant
from test_template_batch_topk_abi import build_cpp_program

gpu = pytest.mark.gpu
E_ARG, E_RANGE = -1, -5
RANGES = [(0, 257), (5, 200), (33, 1), (256, 1), (0, 0)]
KS = [1, 2, 16, 63, 64]
BASE = 2**40 + 3
MATCH_DT = np.dtype([("distance", "<f8"), ("index", "<u8"), ("num", "<u4"), ("den", "<u4"), ("rotation", "<i4"),
                     ("reserved", "<u4")])
assert MATCH_DT.itemsize == ctypes.sizeof(ih.Match) == 32
FILL = 0x5A
UNTOUCHED = np.frombuffer(bytes([FILL]) * 32, MATCH_DT)[0]
GUARD = 0xA5A5A5A5


# ---------------------------------------------------------------- the oracle


def order(e, first=0, n=None):
    """Record indices of [first, first + n) with a valid rotation, in the search order: the exact
    fraction num / den of the best rotation, then the index.  Integers only: two different fractions
    with num, den <= 12800 < 2^14 differ by at least 1 / 12800^2 > 2^-28, so floor(num * 2^40 / den)
    orders them as the fractions themselves and is equal exactly for equal fractions (num * 2^40
    < 2^54 fits an int64).  test_order_key_is_the_exact_fraction_order ties it to
    fractions.Fraction."""
    n = len(e.den) - first if n is None else n
    idx = np.arange(first, first + n)
    idx = idx[e.den[idx] != 0]
    key = (e.num[idx] << 40) // e.den[idx]
    return idx[np.lexsort((idx, key))]


def batch_call(eng, db, k, first, n, base, guards=2):
    """One call of the C entry point into a 0x5A-filled buffer and a counts array with guard words
    after nq -> (records [nq, k], counts)."""
    out = (ih.Match * (eng.nq * k))()
    ctypes.memset(out, FILL, ctypes.sizeof(out))
    counts = (ctypes.c_uint32 * (eng.nq + guards))(*([GUARD] * (eng.nq + guards)))
    rc = ih.load_library().iris_template_batch_topk(eng.handle, db.handle, first, n, base, k, out, counts)
    assert rc == 0, ih.load_library().iris_last_error()
    assert list(counts)[eng.nq:] == [GUARD] * guards, "the words after counts[nq - 1] were written"
    recs = np.frombuffer(bytes(out), MATCH_DT).reshape(eng.nq, k)
    return recs, list(counts)[:eng.nq]


def check_against_oracle(recs, counts, exps, k, first, n, base):
    """base: the call's index_base (a record's index is index_base + its place in the database)."""
    for q, e in enumerate(exps):
        idx = order(e, first, n)[:k]
        assert counts[q] == len(idx), (q, k, first, n, counts[q], len(idx))
        assert recs[q, :len(idx)].tobytes() == e.records(idx, base).tobytes(), (q, k, first, n)
        assert (recs[q, len(idx):] == UNTOUCHED).all(), (q, "entries past the count were written")


@pytest.fixture(scope="module")
def case():
    return SmallCase()


@pytest.fixture(params=["tiles", "tiles-k2"])
def gemm(request, device, hooked_device):
    """(device, layout) of the two shapes of the batched kernel."""
    return open_variant(request.param, device, hooked_device)


@pytest.fixture
def own_device():
    """A device handle of the test's own: its match buffer starts empty and the launch counts
    below do not depend on what ran before."""
    with ih.Device(0) as dev:
        yield dev


def test_small_fixture_facts(case):
    """CPU only, from the oracle alone: what the small case exercises."""
    assert case.N == 257 and (case.N + 31) // 32 == 9 and case.N % 32 == 1  # waves 5-7: clamped tiles only
    for q, e in enumerate(case.exp):
        o = order(e)
        if q in case.ZERO_MASK:
            assert len(o) == 0 and len(order(e, 5, 200)) == 0
        else:
            assert len(o) == case.N
            for rec in case.PLANTS.get(q, []):  # the planted records lead the list
                assert rec in o[:len(case.PLANTS[q])]
    e6 = case.exp[6]
    assert list(order(e6)[:2]) == [130, 200]  # two equal records: the lower index first
    assert e6.num[130] * e6.den[200] == e6.num[200] * e6.den[130]


# ---------------------------------------------------------------- 1. oracle and the single calls

CASES = ([("tiles", nq) for nq in (1, 2, 3, 4, 5, 6, 7, 8, 9, 17)] + [("lanes", nq) for nq in (1, 2, 3)] +
         [("tiles-k2", nq) for nq in (4, 5, 6, 7, 8, 9, 17)])


@gpu
@pytest.mark.parametrize("variant,nq", CASES, ids=[f"{v}-{nq}" for v, nq in CASES])
def test_against_oracle_single_calls_and_search(device, hooked_device, case, variant, nq):
    dev, layout = open_variant(variant, device, hooked_device)
    singles = [ih.TemplateEngine(dev, case.queries[q]) for q in range(nq)]
    try:
        with case.db(dev, layout) as db, ih.TemplateBatchEngine(dev, case.queries[:nq]) as eng:
            for first, n in RANGES:
                best = eng.search(db, first, n, BASE) if n else None
                by_k = {}
                for k in KS:
                    recs, counts = by_k[k] = batch_call(eng, db, k, first, n, BASE)
                    check_against_oracle(recs, counts, case.exp[:nq], k, first, n, BASE)
                    for q in range(nq):
                        one = singles[q].topk(db, k, first=first, n=n, index_base=BASE)
                        assert len(one) == counts[q], (q, k, first, n)
                        assert b"".join(bytes(m) for m in one) == recs[q, :counts[q]].tobytes(), (q, k, first, n)
                        if counts[q]:  # the first entry is the batched search's result
                            m, r0 = best[q], recs[q, 0]
                            assert np.float64(m.distance).view(np.uint64) == r0["distance"].view(np.uint64), (q, k)
                            assert (m.index, m.rotation) == (int(r0["index"]), int(r0["rotation"])), (q, k, first, n)
                    if n == 1:
                        assert max(counts) <= 1
                # a smaller k returns per-query prefixes
                (r16, c16), (r64, c64) = by_k[16], by_k[64]
                for q in range(nq):
                    assert c16[q] == min(c64[q], 16) and r16[q, :c16[q]].tobytes() == r64[q, :c16[q]].tobytes()
            # identical calls return identical bytes
            a = batch_call(eng, db, 64, 0, case.N, BASE)
            b = batch_call(eng, db, 64, 0, case.N, BASE)
            assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes()
    finally:
        for s in singles:
            s.close()


# ---------------------------------------------------------------- 2. the ramp


class RampCase:
    """12 queries over 4099 templates (129 tiles).  near(f) is query 5 with its pattern flipped at
    the first f set positions of its own mask: rotation 0 then gives f / 6460 exactly.  Tile 64
    (records 2048..2079) holds near(70 - i): the distance falls with the index, so every candidate
    of the tile enters its wave's list at position 0.  Tile 65 (records 2080..2111) holds
    near(1 + i): the distance rises with the index and all of it is closer than all of tile 64, so
    at a small k most of its voters find their place past the list's end.  Record 10 is a copy of
    record 2080: an equal fraction in another workgroup's list, ordered by index in the merge."""

    N, NQ, Q = 4099, 12, 5
    DEN = 6460

    def __init__(self):
        self.templates = oc.gen_templates(21, 0, self.N).copy()
        self.queries = oc.gen_templates(22, 0, self.NQ).copy()
        q = self.queries[self.Q]
        self.positions = np.flatnonzero(np.unpackbits(q[200:].copy().view(np.uint8), bitorder="little"))
        for i in range(32):
            self.templates[2048 + i] = self.near(70 - i)
            self.templates[2080 + i] = self.near(1 + i)
        self.templates[10] = self.templates[2080]
        self.exp = [Expected(qq, self.templates) for qq in self.queries]
        self.head = [10] + list(range(2080, 2112)) + list(range(2079, 2047, -1))  # query 5's first 65

    def near(self, f):
        rec = self.queries[self.Q].copy()
        for p in self.positions[:f]:
            rec[p // 64] ^= np.uint64(1) << np.uint64(p % 64)
        return rec


@pytest.fixture(scope="module")
def ramp():
    return RampCase()


def test_ramp_fixture_facts(ramp):
    """CPU only, from the oracle alone."""
    e = ramp.exp[ramp.Q]
    assert len(ramp.positions) == ramp.DEN
    for i in range(32):
        for rec, f in ((2048 + i, 70 - i), (2080 + i, 1 + i)):
            assert (e.num[rec], e.den[rec], e.rot[rec]) == (f, ramp.DEN, 0), rec
    assert (e.num[10], e.den[10], e.rot[10]) == (1, ramp.DEN, 0)
    o = order(e)
    assert len(ramp.head) == 65 and list(o[:65]) == ramp.head
    assert 0.46 < e.dist[o[65]] < 0.47  # the next best record is an ordinary one
    # ties: records whose best fraction equals an earlier record's (ordered by index alone) -- 991 of
    # query 5's 4099, about a thousand for every query
    repeats = [ramp.N - len(np.unique((x.num << 40) // x.den)) for x in ramp.exp]
    assert all((x.den != 0).all() for x in ramp.exp)
    assert repeats[ramp.Q] == 991 and all(900 < t < 1100 for t in repeats), repeats


def test_order_key_is_the_exact_fraction_order(ramp):
    """order()'s integer key against fractions.Fraction, on two queries of the ramp case."""
    for q in (ramp.Q, 0):
        e = ramp.exp[q]
        idx = [i for i in range(ramp.N) if e.den[i] != 0]
        want = sorted(idx, key=lambda i: (fractions.Fraction(int(e.num[i]), int(e.den[i])), i))
        assert list(order(e)) == want


@gpu
def test_ramp_insertion_order_drops_and_two_merge_levels(gemm, ramp):
    dev, layout = gemm
    with ih.Database(dev, ih.KIND_TEMPLATES, ramp.N, layout) as db, ih.TemplateBatchEngine(dev, ramp.queries) as eng:
        db.append(ramp.templates)
        for k in (1, 4, 16, 64):
            recs, counts = batch_call(eng, db, k, 0, ramp.N, 7)
            check_against_oracle(recs, counts, ramp.exp, k, 0, ramp.N, 7)
            assert [int(i) - 7 for i in recs[ramp.Q]["index"]] == ramp.head[:k]
            assert counts == [k] * ramp.NQ


@gpu
def test_ramp_launches(own_device, ramp):
    """72 lists a query (9 workgroups of 8 waves per query group): one pass and two merge levels."""
    dev = own_device
    with ih.Database(dev, ih.KIND_TEMPLATES, ramp.N, ih.LAYOUT_TILES) as db, ih.TemplateBatchEngine(dev, ramp.queries) as eng:
        db.append(ramp.templates)
        dev.reset_stats()
        dev.set_profiling(True)
        try:
            recs, counts = batch_call(eng, db, 16, 0, ramp.N, 7)
        finally:
            dev.set_profiling(False)
        check_against_oracle(recs, counts, ramp.exp, 16, 0, ramp.N, 7)
        assert dev.kernel_stats("template_batch_topk")[0] == 1
        assert dev.kernel_stats("template_batch_topk")[2] == ramp.N * ramp.NQ
        assert dev.kernel_stats("topk_merge")[0] == 2
        assert dev.kernel_stats("template_topk")[0] == 0


# ---------------------------------------------------------------- 3. 1024 queries, resident lists


@pytest.fixture(scope="module")
def wide():
    return WideCase()


@gpu
def test_1024_queries_keep_their_lists_across_groups(gemm, wide):
    """33 tiles: one workgroup per query group (G = 1) walks all 3 (or 5) N-groups with its lists
    resident; 8 lists a query, one merge level with 1024 slots."""
    dev, layout = gemm
    with ih.Database(dev, ih.KIND_TEMPLATES, wide.N, layout) as db, ih.TemplateBatchEngine(dev, wide.queries) as eng:
        db.append(wide.templates)
        for first, n in ((0, wide.N), (5, 517)):
            for k in (4, 64):
                recs, counts = batch_call(eng, db, k, first, n, 11)
                check_against_oracle(recs, counts, wide.exp, k, first, n, 11)
                for q in wide.ZERO_MASK:
                    assert counts[q] == 0


# ---------------------------------------------------------------- 4. output hygiene


@gpu
def test_output_hygiene(gemm, case):
    dev, layout = gemm
    with case.db(dev, layout) as db, ih.TemplateBatchEngine(dev, case.queries) as eng:
        # a range of 3 records: every list ends after 3 (or 0) entries, the rest stays 0x5A
        recs, counts = batch_call(eng, db, 8, 30, 3, 9)
        check_against_oracle(recs, counts, case.exp, 8, 30, 3, 9)
        assert sorted(set(counts)) == [0, 3]
        # n == 0 zeroes every count and touches nothing else
        recs, counts = batch_call(eng, db, 8, 10, 0, 0)
        assert counts == [0] * case.NQ and (recs == UNTOUCHED).all()
        # the mirror returns the same lists
        lists = eng.topk(db, 8, first=30, n=3, index_base=9)
        want, _ = batch_call(eng, db, 8, 30, 3, 9)
        assert [b"".join(bytes(m) for m in x) for x in lists] == [want[q, :len(lists[q])].tobytes()
                                                                 for q in range(case.NQ)]
        assert [len(x) for x in lists] == [0 if q in case.ZERO_MASK else 3 for q in range(case.NQ)]


# ---------------------------------------------------------------- 5. refusals with live handles


@gpu
def test_refusals_leave_the_device_usable(device, own_device, case):
    lib = ih.load_library()
    f = lib.iris_template_batch_topk
    nq, k = 6, 4
    out = (ih.Match * (nq * k))()
    ctypes.memset(out, FILL, ctypes.sizeof(out))
    counts = (ctypes.c_uint32 * nq)(*([99] * nq))
    with case.db(device, ih.LAYOUT_TILES) as db, case.db(device, ih.LAYOUT_LANES) as ldb, \
            case.db(own_device, ih.LAYOUT_TILES) as other_db, \
            ih.TemplateBatchEngine(device, case.queries[:nq]) as eng, \
            ih.TemplateBatchEngine(device, case.queries[:3]) as small, \
            ih.TemplateEngine(device, case.queries[0]) as single, \
            ih.MasksBatchEngine(device, case.queries[:2, 200:]) as mbe, \
            ih.Database(device, ih.KIND_MASKS, 300, ih.LAYOUT_TILES) as mdb:
        mdb.generate(257, 8)

        def good():
            recs, got = batch_call(eng, db, k, 0, case.N, 0)
            check_against_oracle(recs, got, case.exp[:nq], k, 0, case.N, 0)

        refusals = [
            ((eng.handle, ldb.handle, 0, 257, 0, k, out, counts), E_ARG, b"TILES"),  # LANES with nq > 3
            ((single.handle, db.handle, 0, 257, 0, k, out, counts), E_ARG, b"not a batched template engine"),
            ((mbe.handle, db.handle, 0, 257, 0, k, out, counts), E_ARG, b"not a batched template engine"),
            ((eng.handle, mdb.handle, 0, 257, 0, k, out, counts), E_ARG, b"does not hold templates"),
            ((eng.handle, db.handle, 200, 100, 0, k, out, counts), E_RANGE, b""),
            ((eng.handle, other_db.handle, 0, 257, 0, k, out, counts), E_ARG, b"different devices"),
            ((eng.handle, db.handle, 0, 257, 0, 0, out, counts), E_ARG, b"k must be"),
            ((eng.handle, db.handle, 0, 257, 0, 65, out, counts), E_ARG, b"k must be"),
            ((eng.handle, db.handle, 0, 257, 0, k, None, counts), E_ARG, b"out is NULL"),
            ((eng.handle, db.handle, 0, 257, 0, k, out, None), E_ARG, b"counts"),
        ]
        for args, code, word in refusals:
            assert f(*args) == code, args[2:6]
            assert word in lib.iris_last_error(), (args[2:6], lib.iris_last_error())
            assert list(counts) == [99] * nq and bytes(out) == bytes([FILL]) * ctypes.sizeof(out)
            good()
        # the single-query call still refuses a batch engine
        one = ctypes.c_uint32(99)
        assert lib.iris_template_topk(eng.handle, db.handle, 0, 257, 0, k, out, ctypes.byref(one)) == E_ARG
        assert one.value == 99 and bytes(out) == bytes([FILL]) * ctypes.sizeof(out)
        good()


@gpu
def test_three_queries_take_a_lanes_database(own_device, case):
    """An engine of up to 3 queries runs one single-query top-k pass per query, on any layout."""
    dev = own_device
    with case.db(dev, ih.LAYOUT_LANES) as ldb, ih.TemplateBatchEngine(dev, case.queries[:3]) as small:
        dev.reset_stats()
        dev.set_profiling(True)
        try:
            recs, counts = batch_call(small, ldb, 4, 0, case.N, 0)
        finally:
            dev.set_profiling(False)
        check_against_oracle(recs, counts, case.exp[:3], 4, 0, case.N, 0)
        assert dev.kernel_stats("template_topk")[0] == 3 and dev.kernel_stats("template_batch_topk")[0] == 0


# ---------------------------------------------------------------- 6. the C++ program


@gpu
@pytest.mark.parametrize("nq,layout", [(3, ih.LAYOUT_TILES), (3, ih.LAYOUT_LANES), (6, ih.LAYOUT_TILES)],
                         ids=["3-tiles", "3-lanes", "6-tiles"])
def test_cpp_template_batch_topk(nq, layout, tmp_path):
    """iris_hip.hpp's TemplateBatchEngine::topk, run as its own process: every query's 2 and 64
    closest records against the oracle."""
    n, seed = 300, 41
    exe = build_cpp_program(tmp_path)
    path = tmp_path / "lists.bin"
    r = subprocess.run([str(exe), str(path), str(nq), str(n), str(seed), str(layout)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = path.read_bytes()
    i = np.arange(ih.LIMBS, dtype=np.uint64)
    with np.errstate(over="ignore"):
        queries = np.stack([np.concatenate([
            ((i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) * np.uint64(2 * j + 1)) ^ np.uint64(j << 7),
            ((i + np.uint64(3)) * np.uint64(0xD1B54A32D192ED03) * np.uint64(2 * j + 5)) | np.uint64(0x8000000000000001)])
            for j in range(nq)])
    exps = [Expected(q, oc.gen_templates(seed, 0, n)) for q in queries]
    pos = 0
    for k in (2, 64):
        for q in range(nq):
            idx = order(exps[q])[:k]
            count = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
            assert count == len(idx) == k, (k, q)
            got = np.frombuffer(raw, MATCH_DT, count, pos + 8)
            pos += 8 + 32 * count
            assert got.tobytes() == exps[q].records(idx, 7).tobytes(), (k, q)
    assert pos == len(raw)
