"""GPU: template batch threshold matching (iris_template_batch_matches): for every query of a
template batch engine, every record whose best-rotation distance is below one threshold, in
ascending index order with the exact total -- against lists built here from the CPU oracle
(oc.template_counts per query: the best fraction in the exact order, lowest rotation on ties, tied
to oc.template_distances bit for bit) and, byte for byte, against the single-query
iris_template_matches calls it replaces.

Variants: engines of up to 3 queries run one single-query pass per query (TILES and LANES
databases); more than 3 run the batched GEMM's match form on a TILES database, in its default shape
(2 queries x 16 tiles per workgroup) and under IRIS_BATCH_KERNEL=2 (4 queries x 8 tiles, staggered
waves).

The lists under 0.35 are known by construction: generated templates lie near 0.5 from every query,
and near-copies of chosen queries (rotated by -15 / 0 / +15, a few pattern bits flipped) are planted
at chosen records -- the first tile, the tile edges, the ragged tail, two equal records."""
import ctypes
import subprocess

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_template_batch_matches_abi import build_cpp_program

gpu = pytest.mark.gpu
ROT = 31
E_ARG, E_RANGE = -1, -5
INF = float("inf")
MIXED = 0.482  # about half of the generated records (their best rotation lies at 0.47-0.49)
THRESHOLDS = [-1.0, 0.0, 0.35, MIXED, 0.5, 2.0, INF]
RANGES = [(0, 257), (5, 200), (33, 1), (256, 1), (0, 0)]
BASE = 2**40 + 3
MATCH_DT = np.dtype([("distance", "<f8"), ("index", "<u8"), ("num", "<u4"), ("den", "<u4"), ("rotation", "<i4"),
                     ("reserved", "<u4")])
assert MATCH_DT.itemsize == ctypes.sizeof(ih.Match) == 32
FILL = 0x5A
UNTOUCHED = np.frombuffer(bytes([FILL]) * 32, MATCH_DT)[0]


# ---------------------------------------------------------------- the oracle


def bits_of(x):
    return np.asarray(x, np.float64).view(np.uint64)


class Expected:
    """One query against `templates`: per record the best rotation's (num, den, k) in the exact
    fraction order with the lowest k on ties (den = 0: none) and the f64 distance (+inf when none)."""

    def __init__(self, query, templates):
        num, den = (np.asarray(a, np.int64) for a in oc.template_counts(query, templates))
        n = num.shape[0]
        bn, bd, bk = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        for k in range(ROT):
            better = (den[:, k] != 0) & ((bd == 0) | (num[:, k] * bd < bn * den[:, k]))
            bn[better], bd[better], bk[better] = num[better, k], den[better, k], k
        self.num, self.den, self.rot = bn, bd, bk - 15
        with np.errstate(divide="ignore", invalid="ignore"):
            self.dist = np.where(bd != 0, bn.astype(np.float64) / bd.astype(np.float64), np.inf)

    def hits(self, threshold, first=0, n=None):
        """Record indices of [first, first + n) below the threshold (no valid rotation: never)."""
        n = len(self.dist) - first if n is None else n
        idx = np.arange(first, first + n)
        return idx[(self.den[idx] != 0) & (self.dist[idx] < threshold)]

    def records(self, idx, base):
        """The iris_match_t records of record indices idx; index = base + record."""
        w = np.zeros(len(idx), MATCH_DT)
        w["distance"], w["num"], w["den"], w["rotation"] = self.dist[idx], self.num[idx], self.den[idx], self.rot[idx]
        w["index"] = np.asarray(idx, np.uint64) + np.uint64(base)
        return w


def planted(q, rotation, flip_limb=9, flips=0x0F0F00000F0F):
    """The query rotated, a few pattern bits flipped (as test_gpu_scale.planted)."""
    rec = np.concatenate([oc.bits_rotated(q[:200], rotation), oc.bits_rotated(q[200:], rotation)])
    rec[flip_limb] ^= np.uint64(flips)
    return rec


class SmallCase:
    """257 templates (9 tiles, the last one record), 17 queries; PLANTS[q] = the records under 0.35."""

    N, NQ = 257, 17
    ZERO_MASK = (3, 10)  # queries that never match
    PLANTS = {1: [0], 5: [31, 32, 256], 6: [130, 200], 8: [64], 16: [224, 255]}

    def __init__(self):
        self.templates = oc.gen_templates(8, 0, self.N).copy()
        self.queries = oc.gen_templates(99, 0, self.NQ).copy()
        for q in self.ZERO_MASK:
            self.queries[q, 200:] = 0
        q = self.queries
        self.templates[0] = planted(q[1], -15)
        self.templates[31] = planted(q[5], 0, 11)
        self.templates[32] = planted(q[5], 15, 12, 0xFFFFFFFFFF)
        self.templates[256] = planted(q[5], -15, 13, 0xF)
        self.templates[130] = planted(q[6], 0)
        self.templates[200] = self.templates[130]  # two equal records
        self.templates[64] = planted(q[8], 15)
        self.templates[224] = planted(q[16], -15)
        self.templates[255] = planted(q[16], 0, 20)
        self.exp = [Expected(qq, self.templates) for qq in q]
        for qq, e in zip(q, self.exp):
            assert (bits_of(e.dist) == bits_of(oc.template_distances(qq, self.templates))).all()

    def db(self, dev, layout):
        db = ih.Database(dev, ih.KIND_TEMPLATES, 300, layout)
        db.append(self.templates)
        return db


@pytest.fixture(scope="module")
def case():
    return SmallCase()


def test_fixture_lists_are_known_by_construction(case):
    """CPU only, from the oracle alone: the lists under 0.35 are the planted records."""
    for q, e in enumerate(case.exp):
        assert list(e.hits(0.35)) == case.PLANTS.get(q, []), q
        if q in case.ZERO_MASK:
            assert (e.den == 0).all() and len(e.hits(INF)) == 0
        else:
            assert len(e.hits(INF)) == case.N and 0.25 * case.N < len(e.hits(MIXED)) < 0.75 * case.N
    e5, e6 = case.exp[5], case.exp[6]
    assert [int(e5.rot[i]) for i in case.PLANTS[5]] == [0, 15, -15]
    assert len({float(e5.dist[i]) for i in case.PLANTS[5]}) == 3  # distinct distances: a boundary per record
    assert bits_of(e6.dist[130]) == bits_of(e6.dist[200]) and e6.rot[130] == e6.rot[200] == 0


# ---------------------------------------------------------------- helpers


def batch_call(eng, db, t, first, n, base, cap, guards=2):
    """One call of the C entry point into a 0x5A-filled buffer and a counts array with guard words
    after nq -> (records [nq, cap], counts)."""
    out = (ih.Match * max(eng.nq * cap, 1))()
    ctypes.memset(out, FILL, ctypes.sizeof(out))
    counts = (ctypes.c_uint64 * (eng.nq + guards))(*([0xA5A5A5A5] * (eng.nq + guards)))
    rc = ih.load_library().iris_template_batch_matches(eng.handle, db.handle, first, n, base, t, out if cap else None, cap,
                                                       counts)
    assert rc == 0, ih.load_library().iris_last_error()
    assert list(counts)[eng.nq:] == [0xA5A5A5A5] * guards, "the words after counts[nq - 1] were written"
    raw = bytes(out)
    recs = np.frombuffer(raw, MATCH_DT)[:eng.nq * cap].reshape(eng.nq, cap)
    if cap == 0:
        assert raw == bytes([FILL]) * len(raw)
    return recs, list(counts)[:eng.nq]


def check_against_oracle(recs, counts, exps, t, first, n, base, cap):
    """base: the call's index_base (a match's index is index_base + record)."""
    for q, e in enumerate(exps):
        idx = e.hits(t, first, n)
        assert counts[q] == len(idx), (q, t, first, n, counts[q], len(idx))
        k = min(len(idx), cap)
        assert recs[q, :k].tobytes() == e.records(idx[:k], base).tobytes(), (q, t, first, n)
        assert (recs[q, k:] == UNTOUCHED).all(), (q, "entries past the list were written")


VARIANTS = {"tiles": (None, ih.LAYOUT_TILES), "tiles-k2": ("2", ih.LAYOUT_TILES), "lanes": (None, ih.LAYOUT_LANES)}


def open_variant(variant, device, hooked_device):
    kernel, layout = VARIANTS[variant]
    return (hooked_device(IRIS_BATCH_KERNEL=kernel) if kernel else device), layout


@pytest.fixture(params=["tiles", "tiles-k2"])
def gemm(request, device, hooked_device):
    """(device, layout) of the two shapes of the batched kernel."""
    return open_variant(request.param, device, hooked_device)


# ---------------------------------------------------------------- 1. oracle and the single calls

CASES = ([("tiles", nq) for nq in (1, 2, 3, 4, 5, 6, 7, 8, 9, 17)] + [("lanes", nq) for nq in (1, 2, 3)] +
         [("tiles-k2", nq) for nq in (4, 5, 6, 7, 8, 9, 17)])


@gpu
@pytest.mark.parametrize("variant,nq", CASES, ids=[f"{v}-{nq}" for v, nq in CASES])
def test_against_oracle_and_single_calls(device, hooked_device, case, variant, nq):
    dev, layout = open_variant(variant, device, hooked_device)
    singles = [ih.TemplateEngine(dev, case.queries[q]) for q in range(nq)]
    try:
        with case.db(dev, layout) as db, ih.TemplateBatchEngine(dev, case.queries[:nq]) as eng:
            for first, n in RANGES:
                cap = max(n, 1)
                one = (ih.Match * cap)()
                for t in THRESHOLDS:
                    recs, counts = batch_call(eng, db, t, first, n, BASE, cap)
                    check_against_oracle(recs, counts, case.exp[:nq], t, first, n, BASE, cap)
                    for q in range(nq):
                        _, c1 = singles[q].matches(db, t, first=first, n=n, index_base=BASE, out=one)
                        assert c1 == counts[q], (q, t, first, n)
                        assert bytes(one)[:32 * c1] == recs[q, :c1].tobytes(), (q, t, first, n)
            # identical calls return identical bytes
            a = batch_call(eng, db, MIXED, 0, case.N, BASE, case.N)
            b = batch_call(eng, db, MIXED, 0, case.N, BASE, case.N)
            assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes()
    finally:
        for s in singles:
            s.close()


# ---------------------------------------------------------------- 2. the boundary


@gpu
def test_threshold_boundary_in_a_later_group(gemm, case):
    """Query 5 (default shape: slot 1 of the third group; 4-query shape: slot 1 of the second):
    a planted record's exact distance excludes it, the next f64 includes it."""
    dev, layout = gemm
    e = case.exp[5]
    with case.db(dev, layout) as db, ih.TemplateBatchEngine(dev, case.queries) as eng:
        for rec in case.PLANTS[5]:
            edge = float(e.dist[rec])
            lists, counts = eng.matches(db, edge)
            assert rec not in {m.index for m in lists[5]} and counts[5] == len(e.hits(edge))
            lists, counts = eng.matches(db, float(np.nextafter(edge, np.inf)))
            assert rec in {m.index for m in lists[5]} and counts[5] == len(e.hits(edge)) + 1
            assert counts == [len(x.hits(np.nextafter(edge, np.inf))) for x in case.exp]


# ---------------------------------------------------------------- 3. output hygiene


@gpu
def test_output_hygiene_short_cap_and_counts_only(gemm, case):
    dev, layout = gemm
    with case.db(dev, layout) as db, ih.TemplateBatchEngine(dev, case.queries) as eng:
        for t in (0.35, MIXED, INF):
            for cap in (300, 2):  # longer than any list; shorter than most
                recs, counts = batch_call(eng, db, t, 0, case.N, 9, cap)
                check_against_oracle(recs, counts, case.exp, t, 0, case.N, 9, cap)
            recs, counts0 = batch_call(eng, db, t, 0, case.N, 9, 0)
            assert counts0 == [len(e.hits(t)) for e in case.exp]
            lists, counts1 = eng.matches(db, t, cap=0)
            assert lists == [[]] * case.NQ and counts1 == counts0
        # n == 0 zeroes every count and touches nothing else
        recs, counts = batch_call(eng, db, INF, 10, 0, 0, 2)
        assert counts == [0] * case.NQ and (recs == UNTOUCHED).all()
        # cap=None of the mirror: every list in full
        lists, counts = eng.matches(db, INF)
        assert [len(x) for x in lists] == counts == [len(e.hits(INF)) for e in case.exp]


# ---------------------------------------------------------------- 4. 1024 queries, many N-groups


class WideCase:
    """1024 queries over 1027 templates (33 tiles): one workgroup per query group walks every N-group
    (3 in the default shape, 5 in the 4-query shape).  Near-copies spread over the query groups."""

    N, NQ = 1027, 1024
    PLANTS = {0: (0, -15), 3: (100, 0), 255: (1000, 15), 511: (512, -15), 514: (513, 7), 1020: (7, 4), 1023: (1026, -1)}
    ZERO_MASK = (600, 1001)

    def __init__(self):
        self.templates = oc.gen_templates(811, 0, self.N).copy()
        self.queries = oc.gen_templates(812, 0, self.NQ).copy()
        for q in self.ZERO_MASK:
            self.queries[q, 200:] = 0
        for q, (rec, rot) in self.PLANTS.items():
            self.templates[rec] = planted(self.queries[q], rot)
        self.templates[300] = self.templates[100]  # a second record for query 3
        self.exp = [Expected(q, self.templates) for q in self.queries]


@pytest.fixture(scope="module")
def wide():
    return WideCase()


@gpu
def test_1024_queries_walk_many_groups(gemm, wide):
    dev, layout = gemm
    with ih.Database(dev, ih.KIND_TEMPLATES, wide.N, layout) as db, ih.TemplateBatchEngine(dev, wide.queries) as eng:
        db.append(wide.templates)
        for first, n in ((0, wide.N), (5, 517)):
            recs, counts = batch_call(eng, db, 0.35, first, n, 11, 4)
            check_against_oracle(recs, counts, wide.exp, 0.35, first, n, 11, 4)
            recs, counts = batch_call(eng, db, INF, first, n, 11, 4)
            check_against_oracle(recs, counts, wide.exp, INF, first, n, 11, 4)
        sizes = [len(e.hits(0.35)) for e in wide.exp]
        assert sizes[3] == 2 and sum(sizes) == len(wide.PLANTS) + 1
        assert all(sizes[q] >= 1 for q in wide.PLANTS)


# ---------------------------------------------------------------- 5. the overflow rule


class DenseCase:
    """12 queries over 4099 templates; 1500 near-copies of query 5 at every index = 1 mod 2 from 301."""

    N, NQ, DENSE_Q = 4099, 12, 5

    def __init__(self):
        rng = np.random.default_rng(5)
        self.templates = oc.gen_templates(21, 0, self.N).copy()
        self.queries = oc.gen_templates(22, 0, self.NQ).copy()
        self.dense = np.arange(301, 301 + 2 * 1500, 2)
        for i, rec in enumerate(self.dense):
            self.templates[rec] = planted(self.queries[self.DENSE_Q], int(rng.integers(-15, 16)), 5 + i % 150,
                                          int(rng.integers(1, 2**40)))
        self.templates[4098] = planted(self.queries[11], 3)
        self.exp = [Expected(q, self.templates) for q in self.queries]


@pytest.fixture(scope="module")
def dense():
    return DenseCase()


@pytest.fixture
def own_device():
    """A device handle of the test's own: its match buffer starts empty, so the launch counts below
    do not depend on what ran before, and the buffer these tests grow is not the session device's,
    on which other tests assert launch counts."""
    with ih.Device(0) as dev:
        yield dev


def _profiled(device, f):
    device.reset_stats()
    device.set_profiling(True)
    try:
        res = f()
    finally:
        device.set_profiling(False)
    return res, device.kernel_stats("template_batch_match")[0]


@gpu
def test_overflow_reruns_only_the_overflowing_block(own_device, dense):
    dev, n = own_device, dense.N
    sizes = [len(e.hits(0.35)) for e in dense.exp]
    assert sizes[dense.DENSE_Q] == 1500 and sizes[11] == 1 and sum(sizes) == 1501, sizes
    with ih.Database(dev, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES) as db, ih.TemplateBatchEngine(dev, dense.queries) as eng:
        db.append(dense.templates)
        # cap 8: the first pass has room for 1024 records a query, query 5 has 1500 -- its block
        # of four (queries 4-7) runs once more, the other two blocks do not
        (recs, counts), launches = _profiled(dev, lambda: batch_call(eng, db, 0.35, 0, n, 7, 8))
        check_against_oracle(recs, counts, dense.exp, 0.35, 0, n, 7, 8)
        assert counts == sizes and launches == 2


@gpu
def test_overflow_of_every_block(own_device, dense):
    dev, n = own_device, dense.N
    with ih.Database(dev, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES) as db, ih.TemplateBatchEngine(dev, dense.queries) as eng:
        db.append(dense.templates)
        # +inf, cap 2000: room for 2000 a query, every list holds all 4099 -- 1 + 3 launches
        (recs, counts), launches = _profiled(dev, lambda: batch_call(eng, db, INF, 0, n, 7, 2000))
        check_against_oracle(recs, counts, dense.exp, INF, 0, n, 7, 2000)
        assert counts == [n] * dense.NQ and launches == 4


# ---------------------------------------------------------------- 6. refusals with live handles


@gpu
def test_refusals_leave_the_device_usable(device, own_device, case):
    lib = ih.load_library()
    f = lib.iris_template_batch_matches
    nq = 6
    out = (ih.Match * (nq * 4))()
    ctypes.memset(out, FILL, ctypes.sizeof(out))
    counts = (ctypes.c_uint64 * nq)(*([99] * nq))
    with case.db(device, ih.LAYOUT_TILES) as db, case.db(device, ih.LAYOUT_LANES) as ldb, \
            case.db(own_device, ih.LAYOUT_TILES) as other_db, \
            ih.TemplateBatchEngine(device, case.queries[:nq]) as eng, \
            ih.TemplateBatchEngine(device, case.queries[:3]) as small, \
            ih.TemplateEngine(device, case.queries[0]) as single, \
            ih.MasksBatchEngine(device, case.queries[:2, 200:]) as mbe, \
            ih.Database(device, ih.KIND_MASKS, 300, ih.LAYOUT_TILES) as mdb:
        mdb.generate(257, 8)

        def good():
            recs, got = batch_call(eng, db, 0.35, 0, case.N, 0, 4)
            check_against_oracle(recs, got, case.exp[:nq], 0.35, 0, case.N, 0, 4)

        refusals = [
            ((eng.handle, ldb.handle, 0, 257, 0, 0.5, out, 4, counts), E_ARG, b"TILES"),  # LANES with nq > 3
            ((single.handle, db.handle, 0, 257, 0, 0.5, out, 4, counts), E_ARG, b"not a batched template engine"),
            ((mbe.handle, db.handle, 0, 257, 0, 0.5, out, 4, counts), E_ARG, b"not a batched template engine"),
            ((eng.handle, mdb.handle, 0, 257, 0, 0.5, out, 4, counts), E_ARG, b"does not hold templates"),
            ((eng.handle, db.handle, 200, 100, 0, 0.5, out, 4, counts), E_RANGE, b""),
            ((eng.handle, other_db.handle, 0, 257, 0, 0.5, out, 4, counts), E_ARG, b"different devices"),
            ((eng.handle, db.handle, 0, 257, 0, float("nan"), out, 4, counts), E_ARG, b"NaN"),
            ((eng.handle, db.handle, 0, 257, 0, 0.5, None, 4, counts), E_ARG, b"out is NULL"),
            ((eng.handle, db.handle, 0, 257, 0, 0.5, out, 4, None), E_ARG, b"count"),
        ]
        for args, code, word in refusals:
            assert f(*args) == code, args[2:6]
            assert word in lib.iris_last_error(), (args[2:6], lib.iris_last_error())
            assert list(counts) == [99] * nq and bytes(out) == bytes([FILL]) * ctypes.sizeof(out)
            good()
        # the single-query call still refuses a batch engine
        one = ctypes.c_uint64()
        assert lib.iris_template_matches(eng.handle, db.handle, 0, 257, 0, 0.5, out, 4, ctypes.byref(one)) == E_ARG
        good()
        # an engine of up to 3 queries takes any layout
        recs, got = batch_call(small, ldb, 0.35, 0, case.N, 0, 4)
        check_against_oracle(recs, got, case.exp[:3], 0.35, 0, case.N, 0, 4)


# ---------------------------------------------------------------- 7. the C++ program


@gpu
@pytest.mark.parametrize("nq,layout", [(3, ih.LAYOUT_TILES), (3, ih.LAYOUT_LANES), (6, ih.LAYOUT_TILES)],
                         ids=["3-tiles", "3-lanes", "6-tiles"])
def test_cpp_template_batch_matches(nq, layout, tmp_path):
    """iris_hip.hpp's TemplateBatchEngine::matches, run as its own process: every list, the two
    lowest of every list, and the counts alone, against the oracle."""
    n, seed, threshold = 300, 41, MIXED
    exe = build_cpp_program(tmp_path)
    path = tmp_path / "lists.bin"
    r = subprocess.run([str(exe), str(path), str(nq), str(n), str(seed), str(layout), repr(threshold)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = path.read_bytes()
    i = np.arange(ih.LIMBS, dtype=np.uint64)
    with np.errstate(over="ignore"):
        queries = np.stack([np.concatenate([
            ((i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) * np.uint64(2 * j + 1)) ^ np.uint64(j << 7),
            ((i + np.uint64(3)) * np.uint64(0xD1B54A32D192ED03) * np.uint64(2 * j + 5)) | np.uint64(0x8000000000000001)])
            for j in range(nq)])
    exps = [Expected(q, oc.gen_templates(seed, 0, n)) for q in queries]
    hits = [e.hits(threshold) for e in exps]
    assert any(0 < len(h) < n for h in hits), [len(h) for h in hits]
    pos = 0
    for cap in (None, 2):
        for q in range(nq):
            count = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
            k = count if cap is None else min(count, cap)
            got = np.frombuffer(raw, MATCH_DT, k, pos + 8)
            pos += 8 + 32 * k
            assert count == len(hits[q]), (cap, q)
            assert got.tobytes() == exps[q].records(hits[q][:k], 7).tobytes(), (cap, q)
    assert list(np.frombuffer(raw, np.uint64, nq, pos)) == [len(h) for h in hits]
    assert pos + 8 * nq == len(raw)
