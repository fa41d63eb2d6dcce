"""GPU: top-k (iris_template_topk, iris_resolver_topk, iris_resolver_topk_masks): the k closest
records of a range, best first -- against lists built from the CPU oracle's counts (the best rotation
recomputed in integer arithmetic as test_gpu_matches.Expected does, then ordered by the exact fraction
and the index), never from the library's own search.

Variants as in test_gpu_matches.py: a TILES database under the library's own dispatch (on these small
ranges the K-split template kernel), TILES with IRIS_TILES_PER_WAVE=1 and =4 and a LANES database.

Merge levels: a merge workgroup folds 64 lists (kTopkFanIn) and every wave that holds sums writes one
list.  257 records give 3..9 lists (one level); 1100 records up to 36 (one level); the 4098*32+27
records of test_large_range_runs_three_merge_levels give 4099 lists under the library's dispatch (one
tile per wave): 4099 -> 65 -> 2 -> 1, three levels -- the depth a 10M-record call reaches
(78125 -> 1221 -> 20 -> 1)."""
import ctypes
import subprocess

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_gpu_matches import (PERSIST_N, RANGES, ROT, VARIANTS, DeviceArrays, Expected, ResolverCase, TemplateCase,
                              _near_copy, bits_of, resolver_expected)
from test_topk_abi import build_topk_program

pytestmark = pytest.mark.gpu
E_ARG, E_RANGE = -1, -5
INF = float("inf")
KS = [1, 2, 5, 16, 31, 32, 33, 64]
BASE = 2**40 + 7
BIG_N = 1100  # three workgroups of the four-tiles-per-wave form (512 records each), the last partial


@pytest.fixture(params=VARIANTS)
def ctx(request, device, hooked_device):
    v = request.param
    if v == "tiles-tpw1":
        return hooked_device(IRIS_TILES_PER_WAVE=1), ih.LAYOUT_TILES
    if v == "tiles-tpw4":
        return hooked_device(IRIS_TILES_PER_WAVE=4), ih.LAYOUT_TILES
    return device, ih.LAYOUT_TILES if v == "tiles" else ih.LAYOUT_LANES


def order(e, first=0, n=None):
    """Record indices of [first, first + n) with a valid rotation in the search order: exact fraction,
    then index.  Sorted by the f64 quotient first (distinct fractions of counts below 2^16 differ by
    more than 2^-32, equal ones divide to the same f64), then PROVEN in integers: every neighbour
    pair is in strictly ascending (cross-product, index) order."""
    n = len(e.dist) - first if n is None else n
    idx = np.arange(first, first + n)
    idx = idx[e.den[idx] != 0]
    idx = idx[np.lexsort((idx, e.dist[idx]))]
    a, b = idx[:-1], idx[1:]
    l, r = e.num[a] * e.den[b], e.num[b] * e.den[a]
    assert ((l < r) | ((l == r) & (a < b))).all()
    return idx


def check(e, got, want, base):
    """got (list of Match) against the record indices `want`, in order; Match.index = base + record."""
    assert len(got) == len(want), (len(got), len(want))
    for m, i in zip(got, want):
        assert m.index == base + int(i), (m.index - base, i)
        assert (m.num, m.den, m.rotation, m.reserved) == (e.num[i], e.den[i], e.rot[i], 0), (m, i)
        assert bits_of(m.distance) == bits_of(e.dist[i]), (m, i)


def raw_topk(call, k, room=None):
    """call(out, count_ref) on a sentinel-filled array -> (count, the array's bytes)."""
    out = (ih.Match * (room or k))()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    cnt = ctypes.c_uint32(99)
    assert call(out, ctypes.byref(cnt)) == 0, ih.load_library().iris_last_error()
    return cnt.value, bytes(out)


def untied(e, want, j):
    """Entry j of the list `want` is the last of its fraction (not inside a tie)."""
    if j + 1 >= len(want):
        return True
    a, b = want[j], want[j + 1]
    return e.num[a] * e.den[b] != e.num[b] * e.den[a]


@pytest.fixture(scope="module")
def tcase():
    return TemplateCase()


@pytest.fixture(scope="module")
def rcase():
    return ResolverCase()


class BigCase:
    """1100 generated templates with planted near-copies of the query: the four best in records 3, 35,
    67 and 99 (one lane of a four-tiles-per-wave wave), the next eight inside one tile (72..79), one
    more per further workgroup (600, 1090), and exact copies at different rotations (distance 0 ties)
    spread over waves and workgroups in `ties`, a second database."""

    lane = [3, 35, 67, 99]
    tile = list(range(72, 80))
    groups = [600, 1090]
    tie_spots = [2, 40, 130, 131, 300, 513, 700, 1000]

    def __init__(self):
        rng = np.random.default_rng(21)
        self.query = oc.gen_templates(99, 0, 1)[0]
        base = oc.gen_templates(8, 0, BIG_N).copy()
        self.random = Expected(*oc.template_counts(self.query, base))
        self.planted = {}
        for j, i in enumerate(self.lane):
            self.planted[i] = _near_copy(self.query, 2 * j - 3, 10 + 10 * j, rng)
        for j, i in enumerate(self.tile):
            self.planted[i] = _near_copy(self.query, 0, 300 - 20 * j, rng)  # better towards the tile's end
        for j, i in enumerate(self.groups):
            self.planted[i] = _near_copy(self.query, 15 - 30 * j, 500 + 100 * j, rng)
        self.templates = base.copy()
        for i, rec in self.planted.items():
            self.templates[i] = rec
        self.exp = Expected(*oc.template_counts(self.query, self.templates))
        self.tie_planted = {i: _near_copy(self.query, (5 * j) % 31 - 15, 0, rng) for j, i in enumerate(self.tie_spots)}
        self.tie_templates = base.copy()
        for i, rec in self.tie_planted.items():
            self.tie_templates[i] = rec
        self.tie_exp = Expected(*oc.template_counts(self.query, self.tie_templates))

    def db(self, dev, layout, planted):
        db = ih.Database(dev, ih.KIND_TEMPLATES, BIG_N, layout)
        db.generate(BIG_N, 8)
        for i, rec in planted.items():
            db.write(i, rec[None, :])
        return db


@pytest.fixture(scope="module")
def big():
    return BigCase()


def test_fixture_is_not_vacuous(tcase, rcase, big):
    """The fixtures hold what the tests are about: a tie at a cut, a range with fewer than k valid
    records, winners that share a lane, a tile and that sit in different workgroups."""
    e = tcase.exp
    assert e.den[100] == 0 and len(order(e)) == 256  # k = 257 would come back short; (100, 1) is empty
    assert len(order(e, 100, 1)) == 0 and len(order(e, 33, 1)) == 1
    assert list(order(e)[:4]) == [0, 31, 32, 256]
    b = big.exp
    top = list(order(b)[:14])
    assert sorted(top[:4]) == big.lane and sorted(top[4:12]) == big.tile and sorted(top[12:]) == big.groups
    assert top[4:12] == big.tile[::-1]  # the tile's winners arrive worst first: every one inserts at the front
    assert all(i % 32 == 3 and i // 128 == 0 for i in big.lane)  # one lane of wave 0 at 4 tiles per wave
    assert b.dist[big.groups[-1]] < big.random.dist.min()
    t = big.tie_exp
    assert (t.num[big.tie_spots] == 0).all() and len(set(t.rot[big.tie_spots])) > 4
    assert list(order(t)[:8]) == big.tie_spots  # a cut at k = 5 falls inside the tie of eight
    r = rcase.exp_zero
    assert r.den[rcase.zero] == 0 and len(order(r)) == 256


# ---------------------------------------------------------------- 1. templates


def test_template_topk_against_oracle(ctx, tcase):
    device, layout = ctx
    e = tcase.exp
    lib = ih.load_library()
    with tcase.db(device, layout) as db, ih.TemplateEngine(device, tcase.query) as eng:
        for first, n in RANGES:
            want_all = order(e, first, n)
            best = eng.search(db, first=first, n=n, index_base=BASE)
            full = eng.topk(db, 64, first=first, n=n, index_base=BASE)
            for k in KS:
                want = want_all[:k]
                call = lambda o, c: lib.iris_template_topk(eng.handle, db.handle, first, n, BASE, k, o, c)
                count, raw = raw_topk(call, k, room=k + 2)
                got = [ih.Match.from_buffer_copy(raw, 32 * i) for i in range(count)]
                check(e, got, want, BASE)
                assert raw[32 * count:] == b"\xa5" * (32 * (k + 2 - count))  # entries past count: untouched
                assert raw_topk(call, k, room=k + 2) == (count, raw)  # identical calls, identical bytes
                assert [bytes(m) for m in full[:k]] == [bytes(m) for m in got]  # a prefix of the k = 64 list
                if count:
                    assert bytes(got[0]) == bytes(best)
                else:
                    assert best.distance == INF
            # the matches below the next f64 after entry j are the entries up to j, by index
            for j in (0, 4, len(full) - 1):
                if 0 <= j < len(full) and untied(e, want_all, j):
                    lst, cnt = eng.matches(db, float(np.nextafter(full[j].distance, INF)), first=first, n=n,
                                           index_base=BASE)
                    assert cnt == j + 1
                    assert [bytes(m) for m in lst] == [bytes(m) for m in sorted(full[:j + 1], key=lambda m: m.index)]
        assert len(eng.topk(db, 64, first=99, n=3)) == 2  # n < k, one of the three without a valid rotation
        assert eng.topk(db, 3, first=100, n=1) == []


def test_winners_sharing_a_lane_a_tile_and_workgroups(ctx, big):
    device, layout = ctx
    e = big.exp
    want = order(e)
    with big.db(device, layout, big.planted) as db, ih.TemplateEngine(device, big.query) as eng:
        device.reset_stats()
        device.set_profiling(True)
        try:
            for k in (1, 4, 5, 12, 14, 33, 64):
                check(e, eng.topk(db, k, index_base=BASE), want[:k], BASE + 0)
        finally:
            device.set_profiling(False)
        assert device.kernel_stats("template_topk")[0] == 7 and device.kernel_stats("topk_merge")[0] == 7
        assert device.kernel_stats("template_search")[0] == 0 and device.kernel_stats("reduce")[0] == 0
        # a sub-range that cuts the lane's winners and starts inside a tile
        check(e, eng.topk(db, 16, first=35, n=1000, index_base=5), order(e, 35, 1000)[:16], 5)
        assert bytes(eng.topk(db, 1)[0]) == bytes(eng.search(db))


def test_ties_through_the_cut(ctx, big):
    device, layout = ctx
    e = big.tie_exp
    want = order(e)
    with big.db(device, layout, big.tie_planted) as db, ih.TemplateEngine(device, big.query) as eng:
        for k in (1, 5, 8, 11):
            got = eng.topk(db, k)
            check(e, got, want[:k], 0)
        assert [m.index for m in eng.topk(db, 5)] == big.tie_spots[:5]  # the lowest indices win
        assert len({m.rotation for m in eng.topk(db, 8)}) > 4
        assert bytes(eng.topk(db, 5)[0]) == bytes(eng.search(db))


def test_fewer_than_k_valid(ctx):
    """A range whose records all have zero masks but three."""
    device, layout = ctx
    query = oc.gen_templates(99, 0, 1)[0]
    templates = oc.gen_templates(8, 0, 200).copy()
    keep = [7, 64, 199]
    zero = templates.copy()
    zero[:, 200:] = 0
    for i in keep:
        zero[i] = templates[i]
    e = Expected(*oc.template_counts(query, zero))
    assert len(order(e)) == 3
    with ih.Database(device, ih.KIND_TEMPLATES, 200, layout) as db, ih.TemplateEngine(device, query) as eng:
        db.append(zero)
        for k in (1, 3, 4, 64):
            check(e, eng.topk(db, k), order(e)[:k], 0)
        assert eng.topk(db, 64, first=8, n=50) == []
        assert eng.search(db, first=8, n=50).distance == INF


def test_large_range_runs_three_merge_levels(device):
    """The library's own dispatch past the K-split form (4099 tiles, one per wave: 4099 lists, merged
    64 at a time in three levels, see the module docstring) against the oracle over all records."""
    n, seed = PERSIST_N, 77
    rng = np.random.default_rng(3)
    query = oc.gen_templates(99, 0, 1)[0]
    templates = oc.gen_templates(seed, 0, n)
    spots = [0, 127, 128, 64 * 32 + 5, 64 * 64 * 32 + 1, 4095 * 32, n - 1]  # in different first- and second-level groups
    with ih.Database(device, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES) as db, ih.TemplateEngine(device, query) as eng:
        db.generate(n, seed)
        for j, s in enumerate(spots):
            templates[s] = _near_copy(query, 3 * j - 9, 100 + 150 * (len(spots) - j), rng)
            db.write(s, templates[s][None, :])
        e = Expected(*oc.template_counts(query, templates))
        want = order(e)
        assert list(want[:7]) == spots[::-1]
        device.reset_stats()
        device.set_profiling(True)
        try:
            got = eng.topk(db, 64, index_base=BASE)
        finally:
            device.set_profiling(False)
        check(e, got, want[:64], BASE)
        assert device.kernel_stats("template_topk")[0] == 1 and device.kernel_stats("topk_merge")[0] == 1
        for k in (1, 7, 16):
            assert [bytes(m) for m in eng.topk(db, k, index_base=BASE)] == [bytes(m) for m in got[:k]]
        assert bytes(got[0]) == bytes(eng.search(db, index_base=BASE))
        first, m = 4090 * 32 + 5, 250  # starts and ends inside tiles
        check(e, eng.topk(db, 33, first=first, n=m), order(e, first, m)[:33], 0)


# ---------------------------------------------------------------- 2. resolver


@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "offset2"])
def test_resolver_topk_device_arrays(device, rcase, offset):
    e = rcase.exp
    with DeviceArrays(device, list(rcase.shares) + [rcase.den], offset) as ptrs:
        for n, base in [(257, 0), (200, BASE), (1, 5), (0, 0)]:
            want = order(e, 0, n)
            for k in KS:
                got = ih.resolver_topk(device, ptrs[:3], ptrs[3], n, k, index_base=base)
                check(e, got, want[:k], base)
            if n:
                best = ih.resolver_search_device(device, ptrs[:3], ptrs[3], n, index_base=base)
                assert bytes(ih.resolver_topk(device, ptrs[:3], ptrs[3], n, 3, index_base=base)[0]) == bytes(best)
        full = ih.resolver_topk(device, ptrs[:3], ptrs[3], 257, 64)
        want = order(e)
        for j in (0, 9, 63):
            if untied(e, want, j):
                lst, cnt = ih.resolver_matches(device, ptrs[:3], ptrs[3], 257, float(np.nextafter(full[j].distance, INF)))
                assert cnt == j + 1
                assert [bytes(m) for m in lst] == [bytes(m) for m in sorted(full[:j + 1], key=lambda m: m.index)]


def test_resolver_crafted_rows(device):
    """Rows of equal fraction but different (num, den) on both sides of the cut, and garbage rows
    (den = 0 everywhere; uneq > den) ordered as the sibling search orders them."""
    n = 70
    den = np.zeros((n, ROT), np.uint16)
    uneq = np.zeros((n, ROT), np.int64)
    # rows 0..9: 1/4 as (k, 4k) at rotation 3, worse elsewhere; rows 10..19: 1/8; row 20: den = 0 everywhere;
    # row 21: uneq > den (a fraction above 1, listed last); the rest: 1/2 as (m, 2m)
    for i in range(n):
        den[i, :] = 1000
        uneq[i, :] = 900
        if i < 10:
            den[i, 3], uneq[i, 3] = 4 * (i + 1), i + 1
        elif i < 20:
            den[i, 3], uneq[i, 3] = 8 * (30 - i), 30 - i
        elif i == 20:
            den[i, :] = 0
        elif i == 21:
            den[i, :], uneq[i, :] = 10, 30
        else:
            den[i, 7], uneq[i, 7] = 2 * (i + 1), i + 1
    total = (den.astype(np.int64) - 2 * uneq) & 0xFFFF
    shares = np.random.default_rng(9).integers(0, 2**16, (3, n, ROT), dtype=np.uint16)
    shares[2] = (total - shares[0].astype(np.int64) - shares[1].astype(np.int64)) & 0xFFFF
    e = resolver_expected(shares, den)
    want = order(e)
    assert list(want[:20]) == list(range(10, 20)) + list(range(0, 10)) and want[-1] == 21 and 20 not in want
    assert e.num[21] > e.den[21]
    with DeviceArrays(device, list(shares) + [den]) as ptrs:
        for k in (1, 5, 10, 15, 20, 25, 64):  # cuts inside the 1/8 tie, between the ties, inside 1/4 and 1/2
            check(e, ih.resolver_topk(device, ptrs[:3], ptrs[3], n, k), want[:k], 0)
        assert len(ih.resolver_topk(device, ptrs[:3], ptrs[3], n, 64)) == 64
        assert len(ih.resolver_topk(device, ptrs[:3], ptrs[3], 22, 64)) == 21  # n < k, one row without a rotation
        best = ih.resolver_search_device(device, ptrs[:3], ptrs[3], n)
        assert bytes(ih.resolver_topk(device, ptrs[:3], ptrs[3], n, 1)[0]) == bytes(best)


@pytest.mark.parametrize("descending", [True, False], ids=["every-record-inserts", "ascending"])
def test_every_record_inserts(ctx, descending):
    """4096 rows whose distance strictly decreases with the index -- every row beats all before it, an
    insertion per record -- and the same rows in ascending order, through both resolver forms (all-ones
    masks and query mask: den = 12800 at every rotation)."""
    device, layout = ctx
    n = 4096
    u = 2 * (n - np.arange(n)) if descending else 2 * (1 + np.arange(n))
    den = np.full((n, ROT), 12800, np.uint16)
    total = (12800 - 2 * np.repeat(u[:, None], ROT, axis=1)) & 0xFFFF
    shares = np.random.default_rng(4).integers(0, 2**16, (2, n, ROT), dtype=np.uint16)
    shares[1] = (total - shares[0].astype(np.int64)) & 0xFFFF
    e = resolver_expected(shares, den)
    want = order(e)
    assert list(want[:3]) == ([n - 1, n - 2, n - 3] if descending else [0, 1, 2]) and (e.rot == -15).all()
    ones = np.full(200, ~np.uint64(0))
    with DeviceArrays(device, list(shares) + [den]) as ptrs, ih.MasksEngine(device, ones) as eng, \
            ih.Database(device, ih.KIND_MASKS, n, layout) as db:
        db.append(np.tile(ones, (n, 1)))
        for k in (1, 16, 64):
            plain = ih.resolver_topk(device, ptrs[:2], ptrs[2], n, k, index_base=BASE)
            check(e, plain, want[:k], BASE)
            fused = eng.topk(db, ptrs[:2], k, index_base=BASE)
            assert [bytes(m) for m in fused] == [bytes(m) for m in plain]
        first, m = 1000, 2077
        with DeviceArrays(device, shares[:, first:first + m]) as sub:
            check(e, eng.topk(db, sub, 33, first=first, n=m, index_base=first), order(e, first, m)[:33], 0)


def test_resolver_topk_masks_fused(ctx, rcase):
    device, layout = ctx
    e = rcase.exp_zero
    with ih.Database(device, ih.KIND_MASKS, 300, layout) as db, ih.MasksEngine(device, rcase.qmask) as eng:
        db.generate(257, 8)
        db.write(rcase.zero, rcase.masks[rcase.zero][None, :])
        for offset in (0, 2):
            for first, n in RANGES:
                with DeviceArrays(device, rcase.shares[:, first:first + n], offset) as ptrs:
                    want = order(e, first, n)
                    best = eng.resolve(db, ptrs, first=first, n=n, index_base=BASE) if n else None
                    for k in KS:
                        got = eng.topk(db, ptrs, k, first=first, n=n, index_base=BASE)
                        check(e, got, want[:k], BASE - first)  # indices are index_base + the row within the range
                        if got:
                            assert bytes(got[0]) == bytes(best)
        with DeviceArrays(device, list(rcase.shares)) as ptrs:
            a = eng.topk(db, ptrs, 64)
            assert rcase.zero not in [m.index for m in a]
            assert [bytes(m) for m in eng.topk(db, ptrs, 64)] == [bytes(m) for m in a]
            want = order(e)
            for j in (0, 20):
                if untied(e, want, j):
                    lst, cnt = eng.matches(db, ptrs, float(np.nextafter(a[j].distance, INF)))
                    assert cnt == j + 1
                    assert [bytes(m) for m in lst] == [bytes(m) for m in sorted(a[:j + 1], key=lambda m: m.index)]


def test_large_resolver_step(device):
    """The persistent fused kernel past the small-range forms (4098*32+27 rows: every wave of the grid
    walks several tile groups with its list resident) and the resolver kernel over the engine's own
    rows agree with the oracle's order."""
    n = PERSIST_N
    qmask = oc.gen_templates(99, 0, 1)[0][200:]
    den = oc.masks_batch(qmask, oc.gen_masks(8, 0, n))
    shares = np.random.default_rng(6).integers(0, 2**16, (3, n, ROT), dtype=np.uint16)
    e = resolver_expected(shares, den)
    want = order(e)
    with ih.Database(device, ih.KIND_MASKS, n, ih.LAYOUT_TILES) as db, ih.MasksEngine(device, qmask) as eng, \
            DeviceArrays(device, list(shares) + [den]) as ptrs:
        db.generate(n, 8)
        device.reset_stats()
        device.set_profiling(True)
        try:
            fused = eng.topk(db, ptrs[:3], 64, index_base=BASE)
        finally:
            device.set_profiling(False)
        assert device.kernel_stats("masks_topk")[0] == 1 and device.kernel_stats("topk_merge")[0] == 1
        check(e, fused, want[:64], BASE)
        plain = ih.resolver_topk(device, ptrs[:3], ptrs[3], n, 64, index_base=BASE)
        assert [bytes(m) for m in plain] == [bytes(m) for m in fused]
        assert bytes(fused[0]) == bytes(eng.resolve(db, ptrs[:3], index_base=BASE))


# ---------------------------------------------------------------- 3. refusals with live handles


def test_refusals_leave_the_device_usable(ctx, tcase, rcase):
    device, layout = ctx
    lib = ih.load_library()
    out = (ih.Match * 4)()
    cnt = ctypes.c_uint32()
    c = ctypes.byref(cnt)
    tq = np.stack([tcase.query] * 4)
    with tcase.db(device, layout) as tdb, ih.TemplateEngine(device, tcase.query) as te, \
            ih.TemplateBatchEngine(device, tq) as tbe, ih.MasksEngine(device, rcase.qmask) as me, \
            ih.MasksBatchEngine(device, np.stack([rcase.qmask] * 2)) as mbe, \
            ih.Database(device, ih.KIND_MASKS, 300, layout) as mdb, \
            DeviceArrays(device, list(rcase.shares) + [rcase.den]) as ptrs:
        mdb.generate(257, 8)
        arr = (ctypes.c_void_p * 3)(*ptrs[:3])
        null_part = (ctypes.c_void_p * 3)(ptrs[0], None, ptrs[2])
        tk, rk, fk = lib.iris_template_topk, lib.iris_resolver_topk, lib.iris_resolver_topk_masks
        cases = [
            (tk, (tbe.handle, tdb.handle, 0, 257, 0, 4, out, c), E_ARG),  # a batch engine
            (tk, (me.handle, tdb.handle, 0, 257, 0, 4, out, c), E_ARG),  # an engine of another kind
            (tk, (te.handle, mdb.handle, 0, 257, 0, 4, out, c), E_ARG),  # a database of another kind
            (tk, (te.handle, tdb.handle, 200, 100, 0, 4, out, c), E_RANGE),
            (tk, (te.handle, tdb.handle, 0, 257, 0, 0, out, c), E_ARG),
            (tk, (te.handle, tdb.handle, 0, 257, 0, 65, out, c), E_ARG),
            (tk, (te.handle, tdb.handle, 0, 257, 0, 4, None, c), E_ARG),
            (tk, (te.handle, tdb.handle, 0, 257, 0, 4, out, None), E_ARG),
            (fk, (mbe.handle, mdb.handle, 0, 257, arr, 3, 0, 4, out, c), E_ARG),  # a masks batch engine
            (fk, (te.handle, mdb.handle, 0, 257, arr, 3, 0, 4, out, c), E_ARG),
            (fk, (me.handle, tdb.handle, 0, 257, arr, 3, 0, 4, out, c), E_ARG),
            (fk, (me.handle, mdb.handle, 200, 100, arr, 3, 0, 4, out, c), E_RANGE),
            (fk, (me.handle, mdb.handle, 0, 257, arr, 9, 0, 4, out, c), E_ARG),
            (fk, (me.handle, mdb.handle, 0, 257, null_part, 3, 0, 4, out, c), E_ARG),
            (fk, (me.handle, mdb.handle, 0, 257, None, 3, 0, 4, out, c), E_ARG),
            (rk, (device.handle, null_part, 3, ptrs[3], 257, 0, 4, out, c), E_ARG),
            (rk, (device.handle, arr, 3, None, 257, 0, 4, out, c), E_ARG),
            (rk, (device.handle, arr, 0, ptrs[3], 257, 0, 4, out, c), E_ARG),
        ]
        for f, args, code in cases:
            assert f(*args) == code, (f.__name__, args[2:6])
            assert lib.iris_last_error(), f.__name__
        check(tcase.exp, te.topk(tdb, 5), order(tcase.exp)[:5], 0)


# ---------------------------------------------------------------- 4. the C++ program


@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles-mfma", "lanes-valu"])
def test_cpp_topk(layout, device, tmp_path):
    """iris_hip.hpp's TemplateEngine::topk, MasksEngine::topk, resolver_topk and topk_merge, run as their
    own process on 257-record databases, against the Python mirror on the same seeded inputs."""
    n, seed, k = 257, 41, 33
    exe = build_topk_program(tmp_path)
    path = tmp_path / "topk.bin"
    r = subprocess.run([str(exe), str(path), str(n), str(seed), str(layout), str(k)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = path.read_bytes()

    def take(pos):
        count = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
        return [raw[pos + 8 + 32 * i:pos + 40 + 32 * i] for i in range(count)], pos + 8 + 32 * count

    query = oc.gen_templates(seed + 1, 3, 1)[0].copy()
    query[0] = ~query[0]
    tlist, pos = take(0)
    rlist, pos = take(pos)
    assert pos == len(raw) and len(tlist) == k and len(rlist) == k
    e = np.arange(n * ROT, dtype=np.uint64)
    shares = np.stack([(((e * 2654435761) & 0xFFFFFFFF) >> 7) + 12345 * p for p in range(2)]).astype(np.uint16)
    shares = shares.reshape(2, n, ROT)
    ones = np.full(200, ~np.uint64(0))
    with ih.Database(device, ih.KIND_TEMPLATES, n, layout) as tdb, ih.TemplateEngine(device, query) as te, \
            ih.Database(device, ih.KIND_MASKS, n, layout) as mdb, ih.MasksEngine(device, ones) as me, \
            DeviceArrays(device, list(shares)) as ptrs:
        tdb.generate(n, seed)
        mdb.generate(n, seed)
        assert [bytes(m) for m in te.topk(tdb, k, first=1, n=n - 1, index_base=1000)] == tlist
        assert [bytes(m) for m in me.topk(mdb, ptrs, k, index_base=7)] == rlist
    # and the oracle on the template list
    te_exp = Expected(*oc.template_counts(query, oc.gen_templates(seed, 0, n)))
    check(te_exp, [ih.Match.from_buffer_copy(b) for b in tlist], order(te_exp, 1, n - 1)[:k], 1000)
