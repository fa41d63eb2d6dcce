"""GPU: batched threshold matching (iris_resolver_batch_matches_masks): for every query of a masks
batch engine, every record of the resolver step whose decoded distance is below one threshold, in
ascending index order with the exact total -- against lists built from the CPU oracle
(oc.masks_batch for the denominators, the integer best-rotation restatement of test_gpu_matches.py)
and, byte for byte, against the single-query iris_resolver_matches_masks calls it replaces.

Variants as in test_gpu_matches.py: a TILES database under the library's own dispatch (on the small
fixture one fused single-query launch per query), TILES with IRIS_TILES_PER_WAVE=1 and =4 (the hook
pins masks_batch_kernel<G, T, BATCH_MATCH> at one tile per wave and at its large form on ranges of
any size: groups of four queries, a left-over three in the four-slot kernel, a left-over two in the
two-slot kernel, a left-over one in the single-query kernel) and a LANES database (the masks kernel
into a workspace, then the resolver match kernel, per query).

The share slabs are built so that the lists are known by construction: for every (query, record,
rotation) a target uneq is chosen, parts 0 and 1 are uniform random and part 2 is
den - 2 uneq - part0 - part1 (mod 2^16), which decode_distance (src/lib.rs:97-107) turns back into
uneq / den."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_gpu_matches import DeviceArrays, Expected, resolver_expected
from test_masks_batch_matches_abi import build_cpp_program

gpu = pytest.mark.gpu
ROT = 31
E_ARG, E_RANGE = -1, -5
INF = float("inf")
PERSIST_N = 4098 * 32 + 27  # the masks-batch tests' size: some waves walk two tile groups
VARIANTS = ["tiles", "tiles-tpw1", "tiles-tpw4", "lanes"]
THRESHOLDS = [0.0, -1.0, 0.35, 0.5, 2.0, INF]
RANGES = [(0, 257), (5, 200), (33, 1), (256, 1), (0, 0)]
MATCH_DT = np.dtype([("distance", "<f8"), ("index", "<u8"), ("num", "<u4"), ("den", "<u4"), ("rotation", "<i4"),
                     ("reserved", "<u4")])
assert MATCH_DT.itemsize == ctypes.sizeof(ih.Match) == 32
FILL = 0x5A


@pytest.fixture(params=VARIANTS)
def ctx(request, device, hooked_device):
    v = request.param
    if v == "tiles-tpw1":
        return hooked_device(IRIS_TILES_PER_WAVE=1), ih.LAYOUT_TILES
    if v == "tiles-tpw4":
        return hooked_device(IRIS_TILES_PER_WAVE=4), ih.LAYOUT_TILES
    return device, ih.LAYOUT_TILES if v == "tiles" else ih.LAYOUT_LANES


# ---------------------------------------------------------------- expected lists from the oracle


def planted_shares(rng, den, uneq, parts=3):
    """[parts, ...] u16 shares whose wrapping sum decodes to uneq against den (same shapes)."""
    shares = rng.integers(0, 2**16, (parts,) + den.shape, dtype=np.uint16)
    rest = shares[:-1].astype(np.int64).sum(axis=0)
    shares[-1] = ((den.astype(np.int64) - 2 * uneq.astype(np.int64) - rest) % 2**16).astype(np.uint16)
    return shares


def background(rng, den, lo, hi):
    """uneq in [lo den, hi den) per element (den = 0 gives 0)."""
    return (den.astype(np.float64) * (lo + (hi - lo) * rng.random(den.shape))).astype(np.int64)


def want_records(e, idx, first, base):
    """The iris_match_t records of record indices idx (ascending) of a range starting at first."""
    w = np.zeros(len(idx), MATCH_DT)
    w["distance"], w["num"], w["den"], w["rotation"] = e.dist[idx], e.num[idx], e.den[idx], e.rot[idx]
    w["index"] = (np.asarray(idx, np.uint64) - np.uint64(first)) + np.uint64(base)
    return w


class SmallCase:
    """257 masks (record ZERO written as zero), 7 query masks, 3 parts; see the module docstring."""

    N, NQ, ZERO = 257, 7, 77
    EDGES = (31, 32, 256)  # query 2's hits: the tile edges
    TIE = (64, 130)  # query 5: two records with the same distance at different rotations

    def __init__(self):
        rng = np.random.default_rng(2024)
        self.masks = oc.gen_masks(8, 0, self.N).copy()
        self.masks[self.ZERO] = 0
        self.qmasks = rng.integers(0, 2**64, (self.NQ, ih.LIMBS), dtype=np.uint64)
        self.den = np.stack([oc.masks_batch(q, self.masks) for q in self.qmasks])
        d = self.den.astype(np.int64)
        uneq = background(rng, self.den, 0.4, 0.6)

        def plant(q, rec, k, frac):
            uneq[q, rec, k] = int(d[q, rec, k] * frac)

        plant(1, 0, 3, 0.1)
        for rec, k, frac in zip(self.EDGES, (0, 30, 15), (0.05, 0.15, 0.25)):
            plant(2, rec, k, frac)
        free = np.setdiff1d(np.arange(self.N), [self.ZERO])
        self.many = np.sort(rng.choice(free, 40, replace=False))
        for rec in self.many:
            plant(3, rec, int(rng.integers(0, ROT)), 0.3 * rng.random())
        plant(4, 100, 7, 0.2)
        plant(4, 200, 22, 0.2)
        # query 5: p / g at record a, rotation ka, and at record b, rotation kb != ka, g a common divisor
        a, b = self.TIE
        pair = next((ka, kb) for ka in range(ROT) for kb in range(ROT)
                    if ka != kb and math.gcd(int(d[5, a, ka]), int(d[5, b, kb])) >= 10)
        g = math.gcd(int(d[5, a, pair[0]]), int(d[5, b, pair[1]]))
        uneq[5, a, pair[0]] = (g // 5) * (d[5, a, pair[0]] // g)
        uneq[5, b, pair[1]] = (g // 5) * (d[5, b, pair[1]] // g)
        self.tie_rot = (pair[0] - 15, pair[1] - 15)
        plant(5, 10, 1, 0.25)
        self.shares = planted_shares(rng, self.den, uneq)  # [3, 7, 257, 31]
        self.shares[2, 6] = rng.integers(0, 2**16, (self.N, ROT), dtype=np.uint16)  # slab 6: uniform garbage
        self.exp = [resolver_expected(self.shares[:, q], self.den[q]) for q in range(self.NQ)]

    def db(self, dev, layout):
        db = ih.Database(dev, ih.KIND_MASKS, 300, layout)
        db.generate(self.N, 8)
        db.write(self.ZERO, self.masks[self.ZERO][None, :])
        return db


@pytest.fixture(scope="module")
def case():
    return SmallCase()


def test_fixture_lists_are_known_by_construction(case):
    """CPU only, from the oracle alone: the list sizes at 0.35 and the planted records."""
    sizes = [len(e.hits(0.35)) for e in case.exp]
    assert sizes[:3] == [0, 1, 3] and sizes[3] >= 30, sizes
    assert list(case.exp[1].hits(0.35)) == [0] and list(case.exp[2].hits(0.35)) == list(case.EDGES)
    assert set(case.exp[3].hits(0.35)) == set(case.many) and sizes[4] == 2
    a, b = case.TIE
    e5 = case.exp[5]
    assert e5.dist[a].view(np.uint64) == e5.dist[b].view(np.uint64) and 0 < e5.dist[a] < 0.3
    assert (e5.rot[a], e5.rot[b]) == case.tie_rot and e5.rot[a] != e5.rot[b]
    assert list(e5.hits(0.35)) == [10, a, b]
    e6 = case.exp[6]  # the garbage slab: uneq > den and wrapped values occur, some records match
    assert (e6.num > e6.den).any() and 0 < sizes[6] < case.N
    for e in case.exp:  # the zero-mask record has no valid rotation
        assert e.den[case.ZERO] == 0 and case.ZERO not in e.hits(INF) and len(e.hits(INF)) == case.N - 1


# ---------------------------------------------------------------- helpers


def slab_ptrs(ptrs, q, n):
    """Device pointers of slab q of query-major arrays of n rows per query."""
    return [p + q * n * ROT * 2 for p in ptrs]


def batch_call(eng, db, ptrs, t, first, n, base, cap):
    """One batched call into a 0x5A-filled buffer -> (records [nq, cap], counts, the raw bytes)."""
    out = (ih.Match * max(eng.nq * cap, 1))()
    ctypes.memset(out, FILL, ctypes.sizeof(out))
    _, counts = eng.matches(db, ptrs, t, first=first, n=n, index_base=base, cap=cap, out=out)
    raw = bytes(out)
    return np.frombuffer(raw, MATCH_DT)[:eng.nq * cap].reshape(eng.nq, cap), counts, raw


def check_against_oracle(recs, counts, exps, t, first, n, base, cap):
    untouched = np.frombuffer(bytes([FILL]) * 32, MATCH_DT)[0]
    for q, e in enumerate(exps):
        idx = e.hits(t, first, n)
        assert counts[q] == len(idx), (q, t, first, n)
        k = min(len(idx), cap)
        assert recs[q, :k].tobytes() == want_records(e, idx[:k], first, base).tobytes(), (q, t, first, n)
        assert (recs[q, k:] == untouched).all(), (q, "entries past the list were written")


# ---------------------------------------------------------------- 1. oracle and the single call


@gpu
@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 6, 7])
def test_against_oracle_and_single_calls(ctx, case, nq):
    device, layout = ctx
    singles = [ih.MasksEngine(device, case.qmasks[q]) for q in range(nq)]
    try:
        with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[:nq]) as eng:
            for offset in (0, 2):
                for first, n in RANGES:
                    cap = max(n, 1)
                    one = (ih.Match * cap)()
                    with DeviceArrays(device, case.shares[:, :nq, first:first + n], offset) as ptrs:
                        for t in THRESHOLDS:
                            for base in (0, 2**40):
                                recs, counts, _ = batch_call(eng, db, ptrs, t, first, n, base, cap)
                                check_against_oracle(recs, counts, case.exp[:nq], t, first, n, base, cap)
                                if first == 0:  # the zero-mask record never appears
                                    assert all(case.ZERO + base not in recs[q, :counts[q]]["index"] for q in range(nq))
                                for q in range(nq):
                                    _, c1 = singles[q].matches(db, slab_ptrs(ptrs, q, n), t, first=first, n=n,
                                                               index_base=base, out=one)
                                    assert c1 == counts[q], (q, t, first, n)
                                    assert bytes(one)[:32 * c1] == recs[q, :c1].tobytes(), (q, t, first, n)
    finally:
        for s in singles:
            s.close()


# ---------------------------------------------------------------- 2. the boundary


@gpu
def test_threshold_boundary_in_later_slots(ctx, case):
    """A planted record's exact distance excludes it, the next f64 includes it: query 2 (slot 2 of the
    first group) and query 5 (slot 1 of the second), whose two tied records cross together."""
    device, layout = ctx
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks) as eng, \
            DeviceArrays(device, case.shares) as ptrs:
        for q, recs in ((2, [32]), (5, list(case.TIE))):
            e = case.exp[q]
            edge = float(e.dist[recs[0]])
            lists, counts = eng.matches(db, ptrs, edge)
            assert not set(recs) & {m.index for m in lists[q]}
            assert counts[q] == len(e.hits(edge))
            lists, counts = eng.matches(db, ptrs, float(np.nextafter(edge, np.inf)))
            assert set(recs) <= {m.index for m in lists[q]}
            assert counts[q] == len(e.hits(edge)) + len(recs)


# ---------------------------------------------------------------- 3. slot isolation, untouched output


@gpu
def test_slot_isolation_and_untouched_output(ctx, case):
    device, layout = ctx
    cap = 300  # larger than any list
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks) as eng, \
            DeviceArrays(device, case.shares) as ptrs:
        recs, counts, raw = batch_call(eng, db, ptrs, 0.35, 0, case.N, 0, cap)
        check_against_oracle(recs, counts, case.exp, 0.35, 0, case.N, 0, cap)
        assert counts[0] == 0 and raw[:cap * 32] == bytes([FILL]) * (cap * 32)
        for q in range(case.NQ):  # each region: its own list, then untouched bytes
            region = raw[q * cap * 32:(q + 1) * cap * 32]
            assert region[counts[q] * 32:] == bytes([FILL]) * ((cap - counts[q]) * 32), q
        _, counts2, raw2 = batch_call(eng, db, ptrs, 0.35, 0, case.N, 0, cap)
        assert counts2 == counts and raw2 == raw


# ---------------------------------------------------------------- 4. short cap


@gpu
def test_short_cap_and_counts_only(ctx, case):
    device, layout = ctx
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks) as eng, \
            DeviceArrays(device, case.shares) as ptrs:
        for t in (0.35, INF):
            recs, counts, _ = batch_call(eng, db, ptrs, t, 0, case.N, 9, 2)
            check_against_oracle(recs, counts, case.exp, t, 0, case.N, 9, 2)
            lists, counts0 = eng.matches(db, ptrs, t, cap=0)
            assert lists == [[]] * case.NQ and counts0 == [len(e.hits(t)) for e in case.exp]
            c = (ctypes.c_uint64 * case.NQ)(*([99] * case.NQ))
            arr = (ctypes.c_void_p * 3)(*ptrs)
            assert ih.load_library().iris_resolver_batch_matches_masks(eng.handle, db.handle, 0, case.N, arr, 3, 0, t,
                                                                       None, 0, c) == 0
            assert list(c) == counts0
        # n == 0 sets every count to 0 and touches nothing
        recs, counts, raw = batch_call(eng, db, ptrs, INF, 10, 0, 0, 2)
        assert counts == [0] * case.NQ and raw == bytes([FILL]) * len(raw)


# ---------------------------------------------------------------- 5. nq = 64


@gpu
def test_sixty_four_queries(ctx, case):
    """The 7 queries cycled: every slab repeats its source's list."""
    device, layout = ctx
    src = np.arange(64) % case.NQ
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[src]) as eng, \
            DeviceArrays(device, case.shares[:, src]) as ptrs:
        for t in (0.35, INF):
            recs, counts, _ = batch_call(eng, db, ptrs, t, 0, case.N, 0, case.N)
            check_against_oracle(recs, counts, [case.exp[s] for s in src], t, 0, case.N, 0, case.N)


# ---------------------------------------------------------------- 6. large range, the rerun rule


class LargeCase:
    """8 queries over PERSIST_N generated masks (every record has valid rotations).  Slabs 0-3 are
    dense (background uneq under 0.3 den), slabs 4-7 sparse with a handful of planted records."""

    N, NQ, SEED = PERSIST_N, 8, 21
    SPOTS = [0, 37, 4095 * 32 + 31, 4096 * 32, 4097 * 32 + 1, PERSIST_N - 51, PERSIST_N - 1]

    def __init__(self):
        rng = np.random.default_rng(6)
        masks = oc.gen_masks(self.SEED, 0, self.N)
        self.qmasks = rng.integers(0, 2**64, (self.NQ, ih.LIMBS), dtype=np.uint64)
        self.den = np.stack([oc.masks_batch(q, masks) for q in self.qmasks])
        assert (self.den != 0).all()
        uneq = np.empty(self.den.shape, np.int64)
        uneq[:4] = background(rng, self.den[:4], 0.0, 0.3)
        uneq[4:] = background(rng, self.den[4:], 0.4, 0.6)
        for q in range(4, 8):
            for j, s in enumerate(self.SPOTS[:q]):  # 4, 5, 6 and 7 spots
                uneq[q, s, (5 * q + j) % ROT] = int(self.den[q, s, (5 * q + j) % ROT]) // (5 + j)
        self.shares = planted_shares(rng, self.den, uneq)  # [3, 8, N, 31]
        self.exp = [resolver_expected(self.shares[:, q], self.den[q]) for q in range(self.NQ)]


@pytest.fixture(scope="module")
def large():
    return LargeCase()


def _profiled(device, f):
    device.reset_stats()
    device.set_profiling(True)
    try:
        res = f()
    finally:
        device.set_profiling(False)
    return res, device.kernel_stats("masks_batch_match")[0]


@pytest.fixture
def own_device():
    """A device handle of the test's own: its match buffer starts empty, so the launch counts below do
    not depend on what ran before, and the buffer this test grows (a group's 4 n records) is not the
    session device's -- a later single-query call there would otherwise find room in its first pass."""
    with ih.Device(0) as dev:
        yield dev


@gpu
def test_large_range_reruns_only_the_overflowing_group(own_device, large):
    device, n = own_device, large.N
    sizes = [len(e.hits(0.35)) for e in large.exp]
    assert sizes[:4] == [n] * 4 and sizes[4:] == [4, 5, 6, 7], sizes
    with ih.Database(device, ih.KIND_MASKS, n, ih.LAYOUT_TILES) as db, ih.MasksBatchEngine(device, large.qmasks) as eng:
        db.generate(n, large.SEED)
        with DeviceArrays(device, large.shares) as ptrs:
            # +inf: every list is dense and past the 1024-record first room, so both groups run twice
            (recs, counts, _), launches = _profiled(device, lambda: batch_call(eng, db, ptrs, INF, 0, n, 2**40, 10))
            check_against_oracle(recs, counts, large.exp, INF, 0, n, 2**40, 10)
            assert counts == [n] * 8 and launches == 4
            # 0.35: only the group of the dense slabs 0-3 overflows and runs twice
            (recs, counts, _), launches = _profiled(device, lambda: batch_call(eng, db, ptrs, 0.35, 0, n, 0, 10))
            check_against_oracle(recs, counts, large.exp, 0.35, 0, n, 0, 10)
            assert counts == sizes and launches == 3
            # the same lists from the single-query call on slab q of every part
            one = (ih.Match * 10)()
            for q in (1, 6):
                with ih.MasksEngine(device, large.qmasks[q]) as single:
                    _, c1 = single.matches(db, slab_ptrs(ptrs, q, n), 0.35, out=one)
                assert c1 == counts[q] and bytes(one)[:32 * min(c1, 10)] == recs[q, :min(c1, 10)].tobytes()
        # a sub-range that starts and ends inside tiles (its first record no multiple of 8)
        first, m = 37, n - 37 - 50
        with DeviceArrays(device, large.shares[:, :, first:first + m]) as ptrs:
            (recs, counts, _), launches = _profiled(device, lambda: batch_call(eng, db, ptrs, 0.35, first, m, 5, 10))
            check_against_oracle(recs, counts, large.exp, 0.35, first, m, 5, 10)
            assert launches == 3 and counts[4:] == [3, 4, 5, 5]  # spots 0 and N - 1 lie outside


# ---------------------------------------------------------------- 7. three-party flow


@gpu
def test_three_party_flow(ctx):
    """Plaintext templates shared among three parties, each party's rows from its batched
    DistanceEngine for 5 queries, summed and decided in the batched call: the matches at 0.48 are
    those of iris_template_matches over the plaintext database, per query."""
    device, layout = ctx
    n, nq = 257, 5
    templates = oc.gen_templates(8, 0, n)
    queries = oc.gen_templates(99, 0, nq)
    shares, masks = oc.prepare_shares(templates, bytes(range(32)))
    enc = np.stack([oc.encode(q) for q in queries])
    ptrs = []
    sdbs = [ih.Database(device, ih.KIND_SHARES, n) for _ in range(3)]
    try:
        with ih.DistanceBatchEngine(device, enc) as de:
            for p, sdb in enumerate(sdbs):
                sdb.append(shares[p])
                ptrs.append(device.alloc(nq * n * ROT * 2))
                de.batch_process_device(sdb, ptrs[-1])
        with ih.Database(device, ih.KIND_TEMPLATES, n, layout) as tdb, ih.Database(device, ih.KIND_MASKS, n, layout) as mdb, \
                ih.MasksBatchEngine(device, queries[:, 200:]) as me:
            tdb.append(templates)
            mdb.append(masks)
            lists, counts = me.matches(mdb, ptrs, 0.48)
            sizes = []
            for q in range(nq):
                with ih.TemplateEngine(device, queries[q]) as te:
                    plain, pcount = te.matches(tdb, 0.48)
                e = Expected(*oc.template_counts(queries[q], templates))
                e.check(plain, pcount, e.hits(0.48), 0)
                assert counts[q] == pcount and [bytes(m) for m in lists[q]] == [bytes(m) for m in plain], q
                sizes.append(pcount)
            assert any(0 < s < n for s in sizes), sizes
    finally:
        for p in ptrs:
            device.free(p)
        for db in sdbs:
            db.close()


# ---------------------------------------------------------------- 8. refusals with live handles


@gpu
def test_refusals_leave_the_device_usable(ctx, case):
    device, layout = ctx
    lib = ih.load_library()
    f = lib.iris_resolver_batch_matches_masks
    nq = 3
    out = (ih.Match * (nq * 4))()
    ctypes.memset(out, FILL, ctypes.sizeof(out))
    counts = (ctypes.c_uint64 * nq)(*([99] * nq))
    enc = np.zeros((2, ih.BITS), np.uint16)
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[:nq]) as eng, \
            ih.MasksEngine(device, case.qmasks[0]) as single, ih.DistanceBatchEngine(device, enc) as dbe, \
            ih.TemplateEngine(device, oc.gen_templates(99, 0, 1)[0]) as te, \
            ih.Database(device, ih.KIND_TEMPLATES, 300, layout) as tdb, \
            DeviceArrays(device, case.shares[:, :nq]) as ptrs:
        tdb.generate(257, 8)
        arr = (ctypes.c_void_p * 3)(*ptrs)
        null_part = (ctypes.c_void_p * 3)(ptrs[0], None, ptrs[2])
        cases = [
            ((single.handle, db.handle, 0, 257, arr, 3, 0, 0.5, out, 4, counts), E_ARG),  # a single-query masks engine
            ((dbe.handle, db.handle, 0, 257, arr, 3, 0, 0.5, out, 4, counts), E_ARG),  # a distance batch engine
            ((te.handle, db.handle, 0, 257, arr, 3, 0, 0.5, out, 4, counts), E_ARG),  # a template engine
            ((eng.handle, tdb.handle, 0, 257, arr, 3, 0, 0.5, out, 4, counts), E_ARG),  # a templates database
            ((eng.handle, db.handle, 200, 100, arr, 3, 0, 0.5, out, 4, counts), E_RANGE),
            ((eng.handle, db.handle, 0, 257, arr, 9, 0, 0.5, out, 4, counts), E_ARG),
            ((eng.handle, db.handle, 0, 257, null_part, 3, 0, 0.5, out, 4, counts), E_ARG),
            ((eng.handle, db.handle, 0, 257, None, 3, 0, 0.5, out, 4, counts), E_ARG),
            ((eng.handle, db.handle, 0, 257, arr, 3, 0, 0.5, out, 4, None), E_ARG),
            ((eng.handle, db.handle, 0, 257, arr, 3, 0, float("nan"), out, 4, counts), E_ARG),
            ((eng.handle, db.handle, 0, 257, arr, 3, 0, 0.5, None, 4, counts), E_ARG),
        ]
        for args, code in cases:
            assert f(*args) == code, args[2:7]
            assert lib.iris_last_error(), args[2:7]
        assert list(counts) == [99] * nq and bytes(out) == bytes([FILL]) * ctypes.sizeof(out)
        # the single-query call still refuses the batch engine, and names this call
        one = ctypes.c_uint64()
        assert lib.iris_resolver_matches_masks(eng.handle, db.handle, 0, 257, arr, 3, 0, 0.5, out, 4,
                                               ctypes.byref(one)) == E_ARG
        assert b"iris_resolver_batch_matches_masks" in lib.iris_last_error()
        # afterwards a valid call returns the right answer
        recs, got, _ = batch_call(eng, db, ptrs, 0.35, 0, case.N, 0, case.N)
        check_against_oracle(recs, got, case.exp[:nq], 0.35, 0, case.N, 0, case.N)


# ---------------------------------------------------------------- 9. the C++ program


@gpu
@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles-mfma", "lanes-valu"])
def test_cpp_masks_batch_matches(layout, tmp_path):
    """iris_hip.hpp's MasksBatchEngine::matches, run as its own process: every list, the two lowest
    of every list, and the counts alone, against the oracle."""
    nq, n, seed, threshold = 5, 300, 41, 0.125
    exe = build_cpp_program(tmp_path)
    path = tmp_path / "lists.bin"
    r = subprocess.run([str(exe), str(path), str(nq), str(n), str(seed), str(layout), repr(threshold)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = path.read_bytes()
    i = np.arange(ih.LIMBS, dtype=np.uint64)
    with np.errstate(over="ignore"):
        qm = np.stack([((i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) * np.uint64(2 * j + 1)) ^ np.uint64(j << 7)
                       for j in range(nq)])
    el = np.arange(nq * n * ROT, dtype=np.uint64)
    shares = np.stack([(((el * 2654435761) & 0xFFFFFFFF) >> 7) + 12345 * p for p in range(2)]).astype(np.uint16)
    shares = shares.reshape(2, nq, n, ROT)
    masks = oc.gen_masks(seed, 0, n)
    exps = [resolver_expected(shares[:, q], oc.masks_batch(qm[q], masks)) for q in range(nq)]
    hits = [e.hits(threshold) for e in exps]
    assert all(0 < len(h) < n for h in hits) and any(len(h) > 2 for h in hits)
    pos = 0
    for cap in (None, 2):
        for q in range(nq):
            count = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
            k = count if cap is None else min(count, cap)
            got = np.frombuffer(raw, MATCH_DT, k, pos + 8)
            pos += 8 + 32 * k
            assert count == len(hits[q]), (cap, q)
            assert got.tobytes() == want_records(exps[q], hits[q][:k], 0, 7).tobytes(), (cap, q)
    assert list(np.frombuffer(raw, np.uint64, nq, pos)) == [len(h) for h in hits]
    assert pos + 8 * nq == len(raw)
