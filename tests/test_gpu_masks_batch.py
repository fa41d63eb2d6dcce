"""GPU: the batched MasksEngine and resolver step (iris_masks_batch_*, iris_resolver_batch_search_masks):
every query's slab equals what a MasksEngine of that query writes, and every out[q] what
iris_resolver_search_masks gives for that query -- against the CPU oracle on small databases, and
against the single-query engine (itself checked against the oracle by test_gpu_parity.py) plus sampled
oracle rows at the sizes that reach the other kernel forms.

Dispatch on a TILES database (csrc/iris_masks_batch.hip): ranges of more than 1024 tiles of 32 records
run groups of 4 queries per pass of masks_batch_kernel (timed as "masks_batch" / "masks_batch_resolve"),
2 or 3 left-over queries a pass of their own and a single one the single-query kernel; smaller ranges
and LANES databases run one single-query pass per query.  IRIS_TILES_PER_WAVE (a test hook) pins the
batch kernel, at 1 tile per wave or at its large form, on ranges of any size: the small databases
below run that way too ("tiles-batch1", "tiles-batch4")."""
import subprocess

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_masks_batch_abi import build_cpp_program

pytestmark = pytest.mark.gpu
ROT = 31
E_ARG, E_RANGE = -1, -5
SPLIT_TILES = 1024  # kMasksSplitTiles
NONE = 2**64 - 1
# Persistent grid of the batch kernel: min(ceil(ceil(ntiles / T) / 4), 2 x CUs) workgroups of 4 waves, T = 2
# tiles per wave for passes of 3 or 4 queries (nq = 5 and 7 run no pass of 2).  On 256 CUs that
# is 512 workgroups = 2048 waves = 4096 tiles per sweep at T = 2, so 4099 tiles are 2050 groups: waves
# 0 and 1 walk two groups and the last group holds one tile of its two, whose last record is the
# range's 27th of that tile.
PERSIST_N = 4098 * 32 + 27

VARIANTS = ["tiles", "tiles-batch1", "tiles-batch4", "lanes"]


def bits_eq(a, b):
    return (np.asarray(a, np.float64).view(np.uint64) == np.asarray(b, np.float64).view(np.uint64)).all()


@pytest.fixture(params=VARIANTS)
def ctx(request, device, hooked_device):
    """(device, layout): the session device, or one opened with the batch kernel pinned."""
    v = request.param
    if v == "tiles-batch1":
        return hooked_device(IRIS_TILES_PER_WAVE=1), ih.LAYOUT_TILES
    if v == "tiles-batch4":
        return hooked_device(IRIS_TILES_PER_WAVE=4), ih.LAYOUT_TILES
    return device, ih.LAYOUT_TILES if v == "tiles" else ih.LAYOUT_LANES


@pytest.fixture(scope="module")
def qmasks():
    """64 distinct random query masks, except q[1] = 0, q[2] = all ones, q[3] = q[0]."""
    q = np.random.default_rng(78).integers(0, 2**64, (64, ih.LIMBS), dtype=np.uint64)
    q[1] = 0
    q[2] = ~np.uint64(0)
    q[3] = q[0]
    return q


@pytest.fixture(scope="module")
def masks257():
    return oc.gen_masks(8, 0, 257)


@pytest.fixture(scope="module")
def want257(qmasks, masks257):
    """The oracle's [64, 257, 31] rows, computed once."""
    return np.stack([oc.masks_batch(q, masks257) for q in qmasks])


def _db257(dev, layout):
    db = ih.Database(dev, ih.KIND_MASKS, 300, layout)
    db.generate(257, 8)
    return db


def _device_rows(device, eng, db, first, n, nq=None):
    """The engine's device-output rows of [first, first + n), copied back."""
    shape = (n, ROT) if nq is None else (nq, n, ROT)
    out = np.empty(shape, np.uint16)
    ptr = device.alloc(max(out.nbytes, 16))
    try:
        eng.batch_process_device(db, ptr, first=first, n=n)
        if out.nbytes:
            device.d2h(out, ptr)
    finally:
        device.free(ptr)
    return out


class DeviceShares:
    """parts query-major [nq, n, 31] u16 arrays in device memory, each `offset` bytes past a 16-B
    aligned allocation."""

    def __init__(self, device, shares, offset=0):
        self.device, self.raw, self.ptrs = device, [], []
        for s in shares:
            s = np.ascontiguousarray(s, np.uint16)
            p = device.alloc(s.nbytes + 32)
            self.raw.append(p)
            assert p % 16 == 0
            device.h2d(p + offset, s)
            self.ptrs.append(p + offset)

    def __enter__(self):
        return self.ptrs

    def __exit__(self, *exc):
        for p in self.raw:
            self.device.free(p)


def _expect(shares_q, den):
    """(index or NONE, rotation, num, den, distance, dist[n]) of one query from the oracle:
    shares_q [parts, n, 31], den [n, 31]."""
    dist = oc.resolver_combine(shares_q, den)
    best, idx = oc.argmin(dist)
    if idx == NONE:
        return NONE, 0, 0, 0, np.inf, dist
    total = shares_q[:, idx].astype(np.int64).sum(axis=0) & 0xFFFF
    d = den[idx].astype(np.int64)
    u = ((d - total) & 0xFFFF) >> 1  # decode_distance (src/lib.rs:97-107)
    k = None
    for j in range(ROT):  # exact order, the lowest rotation on ties
        if d[j] and (k is None or u[j] * d[k] < u[k] * d[j]):
            k = j
    assert bits_eq(u[k] / d[k], best)
    return int(idx), k - 15, int(u[k]), int(d[k]), best, dist


def _realistic_shares(rng, den, parts):
    """[parts, nq, n, 31] shares of encoded dots den - 2 uneq with uneq in [3/8, 1/2] of den (the
    distances of unrelated templates), so that a planted near-copy is the only small distance."""
    d = den.astype(np.int64)
    uneq = d // 2 - ((d // 8) * rng.random(d.shape)).astype(np.int64)
    shares = rng.integers(0, 2**16, (parts,) + den.shape, dtype=np.uint16)
    rest = shares[:-1].astype(np.int64).sum(axis=0)
    shares[-1] = ((d - 2 * uneq - rest) % 2**16).astype(np.uint16)
    return shares


def _check_resolve(device, eng, db, shares, den, first, n, index_base=0, offset=0, with_dist=True):
    """eng.resolve over [first, first + n) with shares [parts, nq, n, 31] against the oracle
    (den [nq, n, 31]); returns the matches."""
    nq = eng.nq
    dist = device.alloc(max(nq * n * 8, 16)) if with_dist else None
    try:
        with DeviceShares(device, shares, offset) as ptrs:
            got = eng.resolve(db, ptrs, first=first, n=n, index_base=index_base, dist_out=dist)
        gd = np.empty((nq, n), np.float64)
        if with_dist:
            device.d2h(gd, dist)
    finally:
        if dist:
            device.free(dist)
    assert len(got) == nq
    for q in range(nq):
        idx, rot, num, dn, best, want = _expect(shares[:, q], den[q])
        m = got[q]
        assert m.index == (idx if idx == NONE else idx + index_base), (q, m, idx)
        assert (m.rotation, m.num, m.den) == (rot, num, dn), (q, m)
        assert bits_eq(m.distance, best), (q, m)
        if with_dist:
            assert bits_eq(gd[q], want), q
    return got


# ---------------------------------------------------------------- 1. slot identity, group edges


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 64])
def test_slot_identity_and_group_edges(ctx, qmasks, want257, nq):
    device, layout = ctx
    with _db257(device, layout) as db, ih.MasksBatchEngine(device, qmasks[:nq]) as eng:
        assert eng.nq == nq
        out = np.zeros((nq, 257, ROT), np.uint16)
        eng.batch_process(out, db)
    for q in range(nq):
        assert (out[q] == want257[q]).all(), f"slab {q} of {nq}"


# ---------------------------------------------------------------- 2. range edges


def test_range_edges(ctx, qmasks, want257):
    device, layout = ctx
    nq = 5
    with _db257(device, layout) as db, ih.MasksBatchEngine(device, qmasks[:nq]) as eng:
        for first, n in [(157, 100), (31, 34), (256, 1), (0, 32), (32, 0)]:
            out = np.full((nq, n, ROT), 0xABCD, np.uint16)
            eng.batch_process(out, db, first=first, n=n)
            assert (out == want257[:nq, first:first + n]).all(), (first, n)
        with pytest.raises(ih.IrisError) as ei:
            eng.batch_process(np.zeros((nq, 100, ROT), np.uint16), db, first=200, n=100)
        assert ei.value.code == E_RANGE and str(ei.value)
        with pytest.raises(ih.IrisError, match=r"out\.len\(\) == db\.len\(\)"):
            eng.batch_process(np.zeros((nq, 99, ROT), np.uint16), db, first=157, n=100)
        # device form into a larger pre-filled buffer: only the nq * n rows from its start change
        first, n, pad = 31, 34, 3 * ROT
        buf = np.full(nq * n * ROT + pad, 0x5A5A, np.uint16)
        ptr = device.alloc(buf.nbytes)
        try:
            device.h2d(ptr, buf)
            eng.batch_process_device(db, ptr, first=first, n=n)
            got = np.empty_like(buf)
            device.d2h(got, ptr)
            # n = 0 writes nothing at all
            eng.batch_process_device(db, ptr, first=32, n=0)
            again = np.empty_like(buf)
            device.d2h(again, ptr)
        finally:
            device.free(ptr)
        assert (got[:nq * n * ROT].reshape(nq, n, ROT) == want257[:nq, first:first + n]).all()
        assert (got[nq * n * ROT:] == 0x5A5A).all()
        assert (again == got).all()


# ---------------------------------------------------------------- 3. count extremes


def test_count_extremes(ctx):
    """Counts at both ends of the range (12 800 and 0), a single bit, and a single column that the
    31 rotations move in and out of the query's window; neighbouring slots differ."""
    device, layout = ctx
    rng = np.random.default_rng(6)
    ones = np.full(ih.LIMBS, ~np.uint64(0))
    one_bit = np.zeros(ih.LIMBS, np.uint64)
    one_bit[97] = np.uint64(1) << np.uint64(41)
    column = np.zeros(ih.LIMBS, np.uint64)
    column[3] = ~np.uint64(0)  # one column of 64 bits
    edge = np.zeros(ih.LIMBS, np.uint64)
    edge[0] = edge[199] = ~np.uint64(0)  # the first and the last column
    special = [ones, np.zeros(ih.LIMBS, np.uint64), one_bit, column, edge]
    masks = rng.integers(0, 2**64, (70, ih.LIMBS), dtype=np.uint64)
    for i, s in enumerate(special):
        masks[2 + 13 * i] = s
        masks[33 + i] = s  # neighbours in the second tile
    q = np.stack([ones, rng.integers(0, 2**64, ih.LIMBS, dtype=np.uint64), np.zeros(ih.LIMBS, np.uint64), column,
                  one_bit, ones, edge])
    with ih.Database(device, ih.KIND_MASKS, 70, layout) as db, ih.MasksBatchEngine(device, q) as eng:
        db.append(masks)
        out = np.zeros((len(q), 70, ROT), np.uint16)
        eng.batch_process(out, db)
    for i in range(len(q)):
        assert (out[i] == oc.masks_batch(q[i], masks)).all(), i
    assert out[0, 2].max() == 12800 and out[5, 33].min() == 12800 and (out[2] == 0).all()


# ---------------------------------------------------------------- 4. every dispatch form (TILES)


@pytest.fixture(scope="module")
def big_dbs(device):
    """Generated TILES masks databases of the sizes of test 4, made once."""
    dbs = {}
    for n in (20000, SPLIT_TILES * 32 + 27, PERSIST_N):
        db = ih.Database(device, ih.KIND_MASKS, n, ih.LAYOUT_TILES)
        db.generate(n, 21)
        dbs[n] = db
    yield dbs
    for db in dbs.values():
        db.close()


def _batch_dispatched(n):
    return (n + 31) // 32 > SPLIT_TILES


@pytest.mark.parametrize("nq", [5, 7])
@pytest.mark.parametrize("n", [20000, SPLIT_TILES * 32 + 27, PERSIST_N])
def test_every_dispatch_form(device, big_dbs, qmasks, n, nq):
    db = big_dbs[n]
    with ih.MasksBatchEngine(device, qmasks[:nq]) as eng:
        device.reset_stats()
        device.set_profiling(True)
        try:
            got = _device_rows(device, eng, db, 0, n, nq)
        finally:
            device.set_profiling(False)
        batch_launches = device.kernel_stats("masks_batch")[0]
        single_launches = device.kernel_stats("masks")[0]
    if _batch_dispatched(n):  # 5 = 4 + 1 single; 7 = 4 + a pass of 3
        assert (batch_launches, single_launches) == ((1, 1) if nq == 5 else (2, 0))
    else:
        assert (batch_launches, single_launches) == (0, nq)
    for q in range(nq):
        with ih.MasksEngine(device, qmasks[q]) as single:
            assert (got[q] == _device_rows(device, single, db, 0, n)).all(), f"slab {q}"
    edges = [0, 31, 32, 63, 64, 8 * 32 - 1, 8 * 32, n - 60, n - 33, n - 32, n - 28, n - 27, n - 1]
    if n == PERSIST_N:  # the second sweep's first tiles
        edges += [4096 * 32 - 1, 4096 * 32, 4097 * 32, 4098 * 32 - 1, 4098 * 32]
    rows = np.unique(np.concatenate([edges, np.random.default_rng(9).integers(0, n, 64 - len(edges))]))  # 64 at most
    ref = np.concatenate([oc.gen_masks(21, int(i), 1) for i in rows])
    for q in range(nq):
        assert (got[q][rows] == oc.masks_batch(qmasks[q], ref)).all(), f"slab {q} against the oracle"


# ---------------------------------------------------------------- 5. batched resolve against the oracle


@pytest.mark.parametrize("nq", [1, 2, 4, 5, 7, 9])  # 2: the two-slot kernel, 7: a pass with an unused slot
@pytest.mark.parametrize("parts", [1, 3, 8])
def test_resolve_against_oracle(ctx, qmasks, want257, parts, nq):
    device, layout = ctx
    rng = np.random.default_rng(100 * parts + nq)
    # (first, n, index_base, byte offset of the share arrays): n = 256 puts every slab on a 16-B
    # boundary, n = 257 only slabs 0 and 8; first = 5 is no multiple of 8, 40 none of 32; the offset
    # takes the unaligned path for every slab
    cases = [(0, 256, 0, 0), (0, 257, 2**32 + 5, 0), (5, 200, 2**33 + 7, 0), (40, 150, 11, 2), (64, 64, 0, 2)]
    with _db257(device, layout) as db, ih.MasksBatchEngine(device, qmasks[:nq]) as eng:
        for first, n, base, off in cases:
            shares = rng.integers(0, 2**16, (parts, nq, n, ROT), dtype=np.uint16)
            _check_resolve(device, eng, db, shares, want257[:nq, first:first + n], first, n, base, off)
        # no distances output
        _check_resolve(device, eng, db, shares, want257[:nq, 64:128], 64, 64, 3, 0, with_dist=False)
        # an empty range: no candidate for any query
        got = eng.resolve(db, [16] * parts, first=10, n=0)
        assert [m.index for m in got] == [NONE] * nq and all(np.isinf(m.distance) for m in got)


@pytest.mark.parametrize("n", [20000, PERSIST_N])
def test_resolve_large_ranges(device, big_dbs, qmasks, n):
    """nq = 5, parts = 3 at the resolver's chunk size and at the size whose waves walk two tile groups,
    from a first record that is no multiple of 8 (element-wise share reads) and from 0; the
    denominators are the single-query engine's rows (test 4 ties those to the oracle)."""
    nq, parts = 5, 3
    db = big_dbs[n]
    rng = np.random.default_rng(n)
    den = np.empty((nq, n, ROT), np.uint16)
    for q in range(nq):
        with ih.MasksEngine(device, qmasks[q]) as single:
            den[q] = _device_rows(device, single, db, 0, n)
    with ih.MasksBatchEngine(device, qmasks[:nq]) as eng:
        for first in (0, 37):
            m = n - first
            shares = _realistic_shares(rng, den[:, first:], parts)
            # a planted near-copy per query (in different tiles), so the minimum is not left to chance
            for q in (0, 3, 4):
                i = (m // 5) * q + 17
                shares[2, q, i] = den[q, first + i] - 20 - shares[0, q, i] - shares[1, q, i]
            device.reset_stats()
            device.set_profiling(True)
            try:
                got = _check_resolve(device, eng, db, shares, den[:, first:], first, m, 2**40, 0)
            finally:
                device.set_profiling(False)
            launches = device.kernel_stats("masks_batch_resolve")[0]
            assert launches == (1 if _batch_dispatched(n) else 0)
            assert got[4].index == 2**40 + (m // 5) * 4 + 17
            # the single-query call on slab q of every part gives the same match
            for q in (0, 4):
                with ih.MasksEngine(device, qmasks[q]) as single, DeviceShares(device, shares[:, q]) as ptrs:
                    one = single.resolve(db, ptrs, first=first, n=m, index_base=2**40)
                assert (one.index, one.rotation, one.num, one.den) == \
                    (got[q].index, got[q].rotation, got[q].num, got[q].den)


# ---------------------------------------------------------------- 6. ties, empty denominators


def _ties_case(device, layout, n, spots, qmasks):
    """Records `spots` are identical (masks and share rows) and decode to the least distance of
    every query but the zero one; some records are zero masks; query 1 is the zero mask."""
    nq, parts = 6, 3
    rng = np.random.default_rng(n)
    masks = oc.gen_masks(31, 0, n)
    for s in spots:
        masks[s] = masks[spots[0]]
    for z in (0, 33, n - 1):
        masks[z] = 0
    q = qmasks[:nq]
    den = np.stack([oc.masks_batch(x, masks) for x in q])
    shares = _realistic_shares(rng, den, parts)
    for j in range(nq):
        row = (den[j, spots[0]] - 6 - shares[0, j, spots[0]] - shares[1, j, spots[0]]).astype(np.uint16)
        for s in spots:
            shares[0, j, s], shares[1, j, s], shares[2, j, s] = shares[0, j, spots[0]], shares[1, j, spots[0]], row
    with ih.Database(device, ih.KIND_MASKS, n, layout) as db, ih.MasksBatchEngine(device, q) as eng:
        db.append(masks)
        got = _check_resolve(device, eng, db, shares, den, 0, n, 1000, 0)
        for j in range(nq):
            with ih.MasksEngine(device, q[j]) as single, DeviceShares(device, shares[:, j]) as ptrs:
                one = single.resolve(db, ptrs, index_base=1000)
            assert (one.index, one.rotation, one.num, one.den, one.distance) == \
                (got[j].index, got[j].rotation, got[j].num, got[j].den, got[j].distance), j
        # from the second spot on: the lowest index of the range wins
        sub = _check_resolve(device, eng, db, shares[:, :, spots[0] + 1:], den[:, spots[0] + 1:], spots[0] + 1,
                             n - spots[0] - 1, 0, 0)
    low = min(spots)
    assert [m.index for m in got] == [1000 + low, NONE, 1000 + low, 1000 + low, 1000 + low, 1000 + low]
    assert np.isinf(got[1].distance) and got[1].den == 0
    assert sub[0].index == min(s for s in spots if s > spots[0]) - spots[0] - 1


def test_ties_and_empty_denominators(ctx, qmasks):
    device, layout = ctx
    # tiles 0, 1 (waves of one workgroup at 1 tile per wave), 6 and 21 (other workgroups), listed out of order
    _ties_case(device, layout, 800, [5, 700, 40, 200], qmasks)


def test_ties_large_range(device, qmasks):
    """The same through the dispatch's own choice of the batch kernel: 1025 tiles, the last of 27 records."""
    n = SPLIT_TILES * 32 + 27
    _ties_case(device, ih.LAYOUT_TILES, n, [4001, n - 3, 4040, 20000, 129], qmasks)


def test_all_denominators_zero(ctx, qmasks):
    """Zero record masks only: no query has a candidate; equal to the single-query call."""
    device, layout = ctx
    n, nq = 100, 5
    shares = np.random.default_rng(2).integers(0, 2**16, (2, nq, n, ROT), dtype=np.uint16)
    with ih.Database(device, ih.KIND_MASKS, n, layout) as db, ih.MasksBatchEngine(device, qmasks[:nq]) as eng:
        db.append(np.zeros((n, ih.LIMBS), np.uint64))
        got = _check_resolve(device, eng, db, shares, np.zeros((nq, n, ROT), np.uint16), 0, n, 77, 0)
        with ih.MasksEngine(device, qmasks[0]) as single, DeviceShares(device, shares[:, 0]) as ptrs:
            one = single.resolve(db, ptrs, index_base=77)
    assert all(m.index == NONE and m.den == 0 and np.isinf(m.distance) for m in got)
    assert (one.index, one.num, one.den, one.rotation) == (got[0].index, got[0].num, got[0].den, got[0].rotation)


# ---------------------------------------------------------------- 7. three-party flow


def test_three_party_flow(device):
    n, nq = 2050, 6
    templates = oc.gen_templates(57, 0, n)
    picks = [999, 0, 2049, 1024, 31, 32]
    queries = templates[picks].copy()
    for j in range(nq):
        queries[j, :200] ^= np.uint64(0x10 << j)  # a near-copy of template picks[j]
    enc = np.stack([oc.encode(q) for q in queries])
    ptrs = []
    with ih.Database(device, ih.KIND_TEMPLATES, n) as tdb:
        tdb.append(templates)
        sdbs = [ih.Database(device, ih.KIND_SHARES, n) for _ in range(3)]
        mdb = ih.Database(device, ih.KIND_MASKS, n)
        try:
            ih.prepare_shares(tdb, sdbs, mdb, key=bytes(range(32)))
            with ih.DistanceBatchEngine(device, enc) as de:
                for sdb in sdbs:
                    ptrs.append(device.alloc(nq * n * ROT * 2))
                    de.batch_process_device(sdb, ptrs[-1])
            with ih.MasksBatchEngine(device, queries[:, 200:]) as me:
                got = me.resolve(mdb, ptrs)
            for j in range(nq):
                with ih.TemplateEngine(device, queries[j]) as te:
                    ref = te.search(tdb)
                best, idx = oc.argmin(oc.template_distances(queries[j], templates))
                assert got[j].index == ref.index == idx == picks[j], j
                assert bits_eq(got[j].distance, best) and bits_eq(ref.distance, best), j
        finally:
            for p in ptrs:
                device.free(p)
            for db in sdbs + [mdb]:
                db.close()


# ---------------------------------------------------------------- 8. host and device forms


def test_host_and_device_forms_agree_and_engines_share_nothing(ctx, qmasks, want257):
    device, layout = ctx
    with _db257(device, layout) as db:
        a = ih.MasksBatchEngine(device, qmasks[:6])
        host_a = np.zeros((6, 257, ROT), np.uint16)
        a.batch_process(host_a, db)
        b = ih.MasksBatchEngine(device, qmasks[10:13])
        dev_a = _device_rows(device, a, db, 0, 257, 6)
        dev_b = _device_rows(device, b, db, 0, 257, 3)
        a.close()
        a2 = ih.MasksBatchEngine(device, qmasks[20:26])  # reuses a's pooled query buffers
        host_b = np.zeros((3, 257, ROT), np.uint16)
        b.batch_process(host_b, db)
        dev_a2 = _device_rows(device, a2, db, 0, 257, 6)
        b.close()
        a2.close()
    assert host_a.tobytes() == dev_a.tobytes() and (host_a == want257[:6]).all()
    assert host_b.tobytes() == dev_b.tobytes() and (host_b == want257[10:13]).all()
    assert (dev_a2 == want257[20:26]).all()


# ---------------------------------------------------------------- 9. error paths


def test_error_paths_leave_the_device_usable(ctx, qmasks, want257):
    device, layout = ctx
    lib = ih.load_library()
    nq = 3

    def err():
        return lib.iris_last_error().decode(errors="replace")

    out = np.zeros((nq, 257, ROT), np.uint16)
    shares = np.random.default_rng(4).integers(0, 2**16, (2, nq, 257, ROT), dtype=np.uint16)
    enc = np.zeros((2, ih.BITS), np.uint16)
    with _db257(device, layout) as db, ih.MasksBatchEngine(device, qmasks[:nq]) as eng, \
            ih.MasksEngine(device, qmasks[0]) as single, ih.DistanceBatchEngine(device, enc) as dbe, \
            ih.Database(device, ih.KIND_SHARES, 64, layout) as sdb, DeviceShares(device, shares) as ptrs:
        sdb.generate(64, 3)
        for bad in (np.zeros((0, ih.LIMBS), np.uint64), np.zeros((65, ih.LIMBS), np.uint64)):
            with pytest.raises(ih.IrisError) as ei:
                ih.MasksBatchEngine(device, bad)
            assert ei.value.code == E_ARG and "IRIS_MASKS_BATCH_MAX" in str(ei.value)
        m = (ih.Match * nq)()
        arr = (ih.ctypes.c_void_p * 8)(*(ptrs + [ptrs[0]] * 6))
        null_part = (ih.ctypes.c_void_p * 2)(ptrs[0], None)
        process, process_dev, resolve = lib.iris_masks_batch_process, lib.iris_masks_batch_process_device, \
            lib.iris_resolver_batch_search_masks
        cases = [
            (process, (None, db.handle, 0, 1, ih._ptr(out)), E_ARG),
            (process, (eng.handle, None, 0, 1, ih._ptr(out)), E_ARG),
            (process, (eng.handle, db.handle, 0, 1, None), E_ARG),
            (process_dev, (eng.handle, db.handle, 0, 1, None), E_ARG),
            (process, (eng.handle, sdb.handle, 0, 1, ih._ptr(out)), E_ARG),  # a database of the wrong kind
            (process, (eng.handle, db.handle, 200, 100, ih._ptr(out)), E_RANGE),
            (process_dev, (eng.handle, db.handle, 258, 0, ih._ptr(out)), E_RANGE),
            # a masks batch engine handed to the single-query calls
            (lib.iris_engine_batch_process, (eng.handle, db.handle, 0, 1, ih._ptr(out)), E_ARG),
            (lib.iris_engine_batch_process_device, (eng.handle, db.handle, 0, 1, ih._ptr(out)), E_ARG),
            (lib.iris_engine_batch_process_host, (eng.handle, ih._ptr(qmasks), 1, ih._ptr(out)), E_ARG),
            (lib.iris_resolver_search_masks, (eng.handle, db.handle, 0, 257, arr, 2, 0, None, m), E_ARG),
            (lib.iris_resolver_search_masks_host, (eng.handle, db.handle, 0, 257, arr, 2, 0, m), E_ARG),
            # a single-query engine and a distance batch engine handed to the batch calls
            (process, (single.handle, db.handle, 0, 1, ih._ptr(out)), E_ARG),
            (process_dev, (single.handle, db.handle, 0, 1, ih._ptr(out)), E_ARG),
            (resolve, (single.handle, db.handle, 0, 257, arr, 2, 0, None, m), E_ARG),
            (process, (dbe.handle, db.handle, 0, 1, ih._ptr(out)), E_ARG),
            (process, (dbe.handle, sdb.handle, 0, 1, ih._ptr(out)), E_ARG),
            (resolve, (dbe.handle, db.handle, 0, 257, arr, 2, 0, None, m), E_ARG),
            # the resolver step's own arguments
            (resolve, (eng.handle, sdb.handle, 0, 64, arr, 2, 0, None, m), E_ARG),
            (resolve, (eng.handle, db.handle, 0, 257, arr, 0, 0, None, m), E_ARG),
            (resolve, (eng.handle, db.handle, 0, 257, arr, 9, 0, None, m), E_ARG),
            (resolve, (eng.handle, db.handle, 0, 257, null_part, 2, 0, None, m), E_ARG),
            (resolve, (eng.handle, db.handle, 0, 257, None, 2, 0, None, m), E_ARG),
            (resolve, (eng.handle, db.handle, 0, 257, arr, 2, 0, None, None), E_ARG),
            (resolve, (eng.handle, db.handle, 200, 100, arr, 2, 0, None, m), E_RANGE),
        ]
        for f, args, code in cases:
            assert f(*args) == code, (f.__name__, args[2:4])
            assert err(), f.__name__
        assert (out == 0).all()
        # n == 0 is fine and writes nothing, even with a NULL output
        assert process(eng.handle, db.handle, 32, 0, None) == 0
        # the device and the engines still work
        eng.batch_process(out, db)
        assert (out == want257[:nq]).all()
        one = np.zeros((257, ROT), np.uint16)
        single.batch_process(one, db)
        assert (one == want257[0]).all()
        _check_resolve(device, eng, db, shares, want257[:nq], 0, 257, 5, 0)


# ---------------------------------------------------------------- 10. the C++ program


@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles-mfma", "lanes-valu"])
def test_cpp_masks_batch_engine(device, layout, tmp_path):
    """iris_hip.hpp's MasksBatchEngine, run as its own process at nq = 3, n = 100."""
    nq, n, seed = 3, 100, 33
    exe = build_cpp_program(tmp_path)
    rows = tmp_path / "rows.bin"
    r = subprocess.run([str(exe), str(rows), str(nq), str(n), str(seed), str(layout)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.fromfile(rows, np.uint16).reshape(nq, n, ROT)
    i = np.arange(ih.LIMBS, dtype=np.uint64)
    with np.errstate(over="ignore"):
        q = np.stack([((i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) * np.uint64(2 * j + 1)) ^ np.uint64(j << 7)
                      for j in range(nq)])
    with ih.Database(device, ih.KIND_MASKS, n + 57, layout) as db, ih.MasksBatchEngine(device, q) as eng:
        db.generate(n + 57, seed)
        want = np.zeros((nq, n, ROT), np.uint16)
        eng.batch_process(want, db, first=57, n=n)
    assert (got == want).all()
    assert (want[1] == oc.masks_batch(q[1], oc.gen_masks(seed, 57, n))).all()
