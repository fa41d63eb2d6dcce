"""GPU: the batched DistanceEngine (iris_distance_batch_*): every query's slab equals what a
DistanceEngine of that query writes -- against the CPU oracle on small databases, and against the
single-query engine (itself checked against the oracle by test_gpu_parity.py) plus sampled oracle
rows at the sizes that reach the other kernel forms.

Dispatch on a TILES database (csrc/iris_shares_batch.hip): ranges of up to 4096 tiles of 32 records
(131 072 records) run full groups of 4 queries in the K-split batch form and left-over queries as
single-query passes; larger ranges run groups of 4 queries in the form with one tile per wave and 4
waves per workgroup (no persistent grid: one workgroup per 4 tiles), 2 or 3 left-over queries in
the same form with unused slots, a single one in the single-query kernel.  IRIS_TILES_PER_WAVE (a
test hook) pins the large form on ranges of any size: the small databases below run that way too
("tiles-batch").  While profiling, a call counts its passes by form in the stats
"shares_batch_large" / "shares_batch_split" / "shares_batch_single": the tests read there which
kernel ran (the results are bit-identical by design)."""
import subprocess

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_distance_batch_abi import build_cpp_program

pytestmark = pytest.mark.gpu
ROT = 31
E_ARG, E_RANGE = -1, -5
SPLIT_TILES = 4096  # kSharesSplitTiles
BIG_N = SPLIT_TILES * 32 + 27
FILL = 0x5A5A

VARIANTS = ["tiles-mfma", "tiles-batch", "lanes-valu"]


@pytest.fixture(params=VARIANTS)
def ctx(request, device, hooked_device):
    """(device, layout, variant): the session device, or one opened with the large batch form pinned."""
    v = request.param
    if v == "tiles-batch":
        return hooked_device(IRIS_TILES_PER_WAVE=1), ih.LAYOUT_TILES, v
    return device, ih.LAYOUT_TILES if v == "tiles-mfma" else ih.LAYOUT_LANES, v


@pytest.fixture(scope="module")
def queries():
    """64 distinct uniform u16 queries, except q[1] = 0, q[2] = 0xFFFF.., q[3] = q[0]."""
    q = np.random.default_rng(77).integers(0, 1 << 16, (64, ih.BITS), dtype=np.uint16)
    q[1] = 0
    q[2] = 0xFFFF
    q[3] = q[0]
    return q


@pytest.fixture(scope="module")
def shares257():
    return oc.gen_shares(8, 0, 257)


@pytest.fixture(scope="module")
def want257(queries, shares257):
    """The oracle's [64, 257, 31] rows, computed once."""
    return np.stack([oc.distance_batch(q, shares257) for q in queries])


def _db257(dev, layout):
    """The 257-record database on the device of the test's engine."""
    db = ih.Database(dev, ih.KIND_SHARES, 300, layout)
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


def _counted(device, call):
    """call()'s result and the (large, split, single) passes its distance batch calls ran."""
    device.reset_stats()
    device.set_profiling(True)
    try:
        res = call()
    finally:
        device.set_profiling(False)
    return res, tuple(device.kernel_stats("shares_batch_" + f)[0] for f in ("large", "split", "single"))


def _want_forms(variant, nq, large_by_size=False):
    """(large, split, single) passes of one call with nq queries."""
    if variant == "lanes-valu":
        return 0, 0, 0
    if variant == "tiles-batch" or large_by_size:  # groups of 4, a pass of 2 or 3 left-over queries, a single one alone
        return nq // 4 + (nq % 4 >= 2), 0, int(nq % 4 == 1)
    return 0, nq // 4, nq % 4  # up to SPLIT_TILES tiles: full groups in the K-split form, the rest single passes


def _guarded_device_rows(device, eng, db, first, n, nq, slabs=None, guard=64):
    """The device-output form into the middle of a pre-filled buffer whose start is `guard` u16
    (a multiple of 16 B, so the vector path stays in play) past the allocation: -> (words before,
    rows [slabs, n, 31], words after); slabs >= nq, the slabs from nq on must stay untouched."""
    slabs = nq if slabs is None else slabs
    body = slabs * n * ROT
    buf = np.full(guard + body + guard, FILL, np.uint16)
    ptr = device.alloc(buf.nbytes)
    try:
        assert ptr % 16 == 0 and (2 * guard) % 16 == 0
        device.h2d(ptr, buf)
        eng.batch_process_device(db, ptr + 2 * guard, first=first, n=n)
        got = np.empty_like(buf)
        device.d2h(got, ptr)
    finally:
        device.free(ptr)
    return got[:guard], got[guard:guard + body].reshape(slabs, n, ROT), got[guard + body:]


# ---------------------------------------------------------------- 1. slot identity, group edges


# 6: a group of 4 and a pass of two, whose slabs 4 and 5 sit after a full group
@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 64])
def test_slot_identity_and_group_edges(ctx, queries, want257, nq):
    device, layout, variant = ctx
    with _db257(device, layout) as db, ih.DistanceBatchEngine(device, queries[:nq]) as eng:
        assert eng.nq == nq
        out = np.zeros((nq, 257, ROT), np.uint16)
        _, forms = _counted(device, lambda: eng.batch_process(out, db))
    for q in range(nq):
        assert (out[q] == want257[q]).all(), f"slab {q} of {nq}"
    assert forms == _want_forms(variant, nq), (variant, nq)


# ---------------------------------------------------------------- 2. range edges


def test_range_edges(ctx, queries, want257):
    device, layout, _ = ctx
    nq = 5
    with _db257(device, layout) as db257, ih.DistanceBatchEngine(device, queries[:nq]) as eng:
        for first, n in [(157, 100), (31, 34), (256, 1), (0, 32), (32, 0)]:
            out = np.full((nq, n, ROT), 0xABCD, np.uint16)
            eng.batch_process(out, db257, first=first, n=n)
            assert (out == want257[:nq, first:first + n]).all(), (first, n)
        with pytest.raises(ih.IrisError) as ei:
            eng.batch_process(np.zeros((nq, 100, ROT), np.uint16), db257, first=200, n=100)
        assert ei.value.code == E_RANGE and str(ei.value)
        with pytest.raises(ih.IrisError, match=r"out\.len\(\) == db\.len\(\)"):
            eng.batch_process(np.zeros((nq, 99, ROT), np.uint16), db257, first=157, n=100)
        # device form into a larger pre-filled buffer: only the nq * n rows from its start change
        first, n, pad = 31, 34, 3 * ROT
        buf = np.full(nq * n * ROT + pad, 0x5A5A, np.uint16)
        ptr = device.alloc(buf.nbytes)
        try:
            device.h2d(ptr, buf)
            eng.batch_process_device(db257, ptr, first=first, n=n)
            got = np.empty_like(buf)
            device.d2h(got, ptr)
            # n = 0 writes nothing at all
            eng.batch_process_device(db257, ptr, first=32, n=0)
            again = np.empty_like(buf)
            device.d2h(again, ptr)
        finally:
            device.free(ptr)
        assert (got[:nq * n * ROT].reshape(nq, n, ROT) == want257[:nq, first:first + n]).all()
        assert (got[nq * n * ROT:] == 0x5A5A).all()
        assert (again == got).all()


# Ranges chosen for the large form's grid (one workgroup of 4 waves per 4 tiles, waves past the range
# clamped to the last tile) ...
GRID_RANGES = [
    (33, 60),    # 2 tiles (1..2), both partial: waves 2 and 3 past the range
    (5, 123),    # 4 tiles (0..3), the first partial: one whole workgroup
    (64, 192),   # 6 tiles (2..7), aligned: the second workgroup with two waves past the range
    (0, 257),    # 9 tiles, the last of one record: the third workgroup with three waves past the range
]
# ... and for the store paths.  A tile is written with 16-B vector stores when its slab starts on a
# 16-B boundary and the tile lies whole in the range at (tile_t0 - first) % 8 == 0, else record by
# record.  Slab q starts q * n * 62 B into the (16-B aligned) output.
STORE_RANGES = [
    (0, 256),    # n * 62 = 16 * 992: every slab aligned, every tile vectorised
    (8, 240),    # n * 62 = 16 * 930: every slab aligned; the first tile (records 8..31) element-wise, the
                 # other 7 vectorised at (tile_t0 - first) % 8 == 0
    (4, 252),    # n * 62 = 16 * 976 + 8: even slabs aligned, odd ones 8 B off, but (tile_t0 - first) % 8
                 # == 4 for every tile: all element-wise
    (32, 224),   # n * 62 = 16 * 868: every slab aligned, every tile vectorised, from tile 1 on
]


@pytest.mark.parametrize("nq", [5, 8])  # 8: a second full group
def test_range_edges_of_the_grid_and_the_store_paths(ctx, queries, want257, nq):
    device, layout, variant = ctx
    with _db257(device, layout) as db, ih.DistanceBatchEngine(device, queries[:nq]) as eng:
        for first, n in GRID_RANGES + STORE_RANGES:
            want = want257[:nq, first:first + n]
            out = np.full((nq, n, ROT), 0xABCD, np.uint16)
            _, forms = _counted(device, lambda: eng.batch_process(out, db, first=first, n=n))
            bad = np.argwhere((out != want).any(axis=2))
            assert bad.size == 0, f"host form {(first, n)}: (slab, record) {bad[:8].tolist()}"
            assert forms == _want_forms(variant, nq), (variant, first, n)
            got = _device_rows(device, eng, db, first, n, nq)
            bad = np.argwhere((got != want).any(axis=2))
            assert bad.size == 0, f"device form {(first, n)}: (slab, record) {bad[:8].tolist()}"


@pytest.mark.parametrize("first,n", [(8, 240), (31, 34)])
def test_device_form_writes_its_rows_only(ctx, queries, want257, first, n):
    """The nq * n rows in the middle of a pre-filled buffer: the words before and after stay."""
    device, layout, _ = ctx
    nq = 5
    with _db257(device, layout) as db, ih.DistanceBatchEngine(device, queries[:nq]) as eng:
        before, rows, after = _guarded_device_rows(device, eng, db, first, n, nq)
    assert (rows == want257[:nq, first:first + n]).all()
    assert (before == FILL).all(), "words before the output"
    assert (after == FILL).all(), "words after the output"


# The single-query kernels share their K-loop and epilogue with each other and the epilogue with the
# batch kernels: each of their forms on the tile span, the clamp of the last tile and both store paths.
@pytest.mark.parametrize("tpw", [None, 1, 4], ids=["split", "one-tile", "two-tiles"])
def test_single_query_forms_at_the_range_edges(device, hooked_device, queries, want257, tpw):
    """shares_split_kernel (no hook on a small range), shares_mfma_kernel<1> (IRIS_TILES_PER_WAVE=1) and
    shares_mfma_kernel<2> (=4: the big variant is two tiles per wave) over one record inside a tile, a
    range across two tile boundaries, whole aligned tiles and an aligned start with a ragged end (9
    tiles: the last wave's second tile is past the range)."""
    dev = device if tpw is None else hooked_device(IRIS_TILES_PER_WAVE=tpw)
    with _db257(dev, ih.LAYOUT_TILES) as db, ih.DistanceEngine(dev, queries[0]) as eng:
        for first, n in [(5, 1), (31, 34), (64, 64), (8, 240), (0, 257)]:
            out = np.full((n, ROT), 0xABCD, np.uint16)
            eng.batch_process(out, db, first=first, n=n)
            assert (out == want257[0, first:first + n]).all(), (first, n)
            assert (_device_rows(dev, eng, db, first, n) == want257[0, first:first + n]).all(), (first, n)


# ---------------------------------------------------------------- 3. byte-bias extremes

CONSTS = [0x0000, 0xFFFF, 0x8000, 0x7FFF, 0x00FF, 0xFF00, 0x0080, 0x8080]


def _extreme_queries(rng):
    q = rng.integers(0, 1 << 16, (8, ih.BITS), dtype=np.uint16)
    for i, c in enumerate(CONSTS):
        q[i] = c
    q[5, ::3] = 0x1234  # not every query constant
    return q


def test_byte_bias_extremes(ctx):
    """Rows whose bytes sit at the ends of the XOR-0x80 bias, where the 128 * sum corrections of a
    multi-query epilogue go wrong first."""
    device, layout, _ = ctx
    rng = np.random.default_rng(5)
    shares = rng.integers(0, 1 << 16, (70, ih.BITS), dtype=np.uint16)
    q = _extreme_queries(rng)
    for i, c in enumerate(CONSTS):
        shares[3 + 7 * i] = c
    with ih.Database(device, ih.KIND_SHARES, 70, layout) as db, ih.DistanceBatchEngine(device, q) as eng:
        db.append(shares)
        out = np.zeros((8, 70, ROT), np.uint16)
        eng.batch_process(out, db)
    for i in range(8):
        assert (out[i] == oc.distance_batch(q[i], shares)).all(), i


def test_byte_bias_extremes_whole_tiles(ctx):
    """4 tiles in which every record is one of the eight constants, so the row-31 byte sums
    sum e'_lo / sum e'_hi sit at their ends (12800 * -128, 12800 * 127) for every record of a tile:
    tile 0 all 0x0000, tile 1 all 0xFFFF, tile 2 0x00FF / 0xFF00 in turn, tile 3 all eight in turn."""
    device, layout, variant = ctx
    q = _extreme_queries(np.random.default_rng(5))
    shares = np.empty((128, ih.BITS), np.uint16)
    shares[0:32] = 0x0000
    shares[32:64] = 0xFFFF
    shares[64:96:2], shares[65:96:2] = 0x00FF, 0xFF00
    for i in range(32):
        shares[96 + i] = CONSTS[i % 8]
    with ih.Database(device, ih.KIND_SHARES, 128, layout) as db, ih.DistanceBatchEngine(device, q) as eng:
        db.append(shares)
        out = np.zeros((8, 128, ROT), np.uint16)
        _, forms = _counted(device, lambda: eng.batch_process(out, db))
    for i in range(8):
        want = oc.distance_batch(q[i], shares)
        bad = np.argwhere((out[i] != want).any(axis=1))
        assert bad.size == 0, f"query {i}: records {bad[:8].ravel().tolist()}"
    assert forms == _want_forms(variant, 8)


# ---------------------------------------------------------------- 4. duplicate and unused slots


@pytest.mark.parametrize("picks", [(0, 0), (0, 5, 0)], ids=["a-a", "a-b-a"])
def test_duplicate_queries_and_unused_slots(ctx, queries, want257, picks):
    """Passes of 2 and 3 queries whose last equals the first: the large form's slots valid..3 repeat
    slot 0's fragments and output pointer and store nothing, so equal queries give equal slabs and
    exactly nq slabs of a pre-filled device output are written."""
    device, layout, variant = ctx
    nq = len(picks)
    with _db257(device, layout) as db, ih.DistanceBatchEngine(device, queries[list(picks)]) as eng:
        for first, n in [(0, 257), (8, 240)]:
            (before, rows, after), forms = _counted(
                device, lambda: _guarded_device_rows(device, eng, db, first, n, nq, slabs=4))
            for s, p in enumerate(picks):
                assert (rows[s] == want257[p, first:first + n]).all(), (first, n, s)
            assert rows[0].tobytes() == rows[nq - 1].tobytes()
            assert (rows[nq:] == FILL).all(), f"slabs past the {nq} queries were written"
            assert (before == FILL).all() and (after == FILL).all()
            assert forms == _want_forms(variant, nq), (variant, first, n)


# ---------------------------------------------------------------- 5. K positions

# Chunk and step edges of the first steps (a step is 2 chunks of 32 = 64 positions; even steps read
# ring slot 0, odd ones slot 1), the K-split form's slice boundary (6400), the last block of 6
# steps (12 352 .. 12 671) and the two tail steps (12 672 .. 12 735, 12 736 .. 12 799).
K_POSITIONS = [0, 31, 32, 63, 64, 127, 128, 6399, 6400, 12671, 12672, 12735, 12736, 12799]


def test_k_positions(ctx):
    """Share records that are zero except e[i] = 1: out[q][t][k] = rot_k(query_q)[i] (from the
    oracle), so a step that is skipped or doubled shows at its own i.  Record 3 j holds position
    K_POSITIONS[j]: two tiles.  The MFMA forms multiply the bytes XOR 0x80, where a zero share is
    -128 at every position, so a step paired with another step's query fragments spoils every such
    record; record 3 j + 1 is therefore the same probe on a background of 0x8080 (zero after the XOR,
    0x8081 at i), which only a fault at i's own step changes: those name the step in the message.
    Records 3 j + 2 are zero."""
    device, layout, variant = ctx
    nq, n = 4, 3 * len(K_POSITIONS)
    q = np.random.default_rng(11).integers(0, 1 << 16, (nq, ih.BITS), dtype=np.uint16)
    shares = np.zeros((n, ih.BITS), np.uint16)
    for j, i in enumerate(K_POSITIONS):
        shares[3 * j, i] = 1
        shares[3 * j + 1] = 0x8080
        shares[3 * j + 1, i] = 0x8081
    want = np.stack([oc.distance_batch(x, shares) for x in q])
    with ih.Database(device, ih.KIND_SHARES, n, layout) as db, ih.DistanceBatchEngine(device, q) as eng:
        db.append(shares)
        out = np.zeros((nq, n, ROT), np.uint16)
        _, forms = _counted(device, lambda: eng.batch_process(out, db))
    assert forms == _want_forms(variant, nq)
    wrong = (out != want).any(axis=(0, 2))  # per record
    plain = [i for j, i in enumerate(K_POSITIONS) if wrong[3 * j]]
    biased = [i for j, i in enumerate(K_POSITIONS) if wrong[3 * j + 1]]
    assert not plain and not biased, (
        f"first wrong at i = {(plain or biased)[0]}; on the 0x8080 background wrong at i = {biased}; "
        f"(query, record, rotation) {np.argwhere(out != want)[:8].tolist()}")
    assert (out == want).all(), "the zero records"


# ---------------------------------------------------------------- 6. every dispatch form (TILES)


@pytest.fixture(scope="module")
def big_dbs(device):
    """Generated TILES share databases of the sizes of test 6, made once (BIG_N: 3.36 GB)."""
    dbs = {}
    for n in (20000, BIG_N):
        db = ih.Database(device, ih.KIND_SHARES, n, ih.LAYOUT_TILES)
        db.generate(n, 21)
        dbs[n] = db
    yield dbs
    for db in dbs.values():
        db.close()


def _check_large(device, db, queries, nq, first, n, edges, large_by_size):
    """The batch over [first, first + n) of a seed-21 database: the pass counts, every slab against
    the single-query engine, and at most 64 rows (`edges`, relative to first, and random ones)
    against the oracle."""
    assert len(edges) <= 64
    with ih.DistanceBatchEngine(device, queries[:nq]) as eng:
        got, forms = _counted(device, lambda: _device_rows(device, eng, db, first, n, nq))
    assert forms == _want_forms("tiles-mfma", nq, large_by_size), (n, nq)
    for q in range(nq):
        with ih.DistanceEngine(device, queries[q]) as single:
            assert (got[q] == _device_rows(device, single, db, first, n)).all(), f"slab {q}"
    rows = np.unique(np.concatenate([edges, np.random.default_rng(9).integers(0, n, 64 - len(edges))]))  # 64 at most
    ref = np.concatenate([oc.gen_shares(21, first + int(i), 1) for i in rows])
    for q in range(nq):
        assert (got[q][rows] == oc.distance_batch(queries[q], ref)).all(), f"slab {q} against the oracle"


# 20 000 records = 625 tiles: the K-split form (a participant's chunk).  131 099 records = 4097
# tiles, one past SPLIT_TILES: the large form, 1025 workgroups of 4 waves, the last with three
# waves past the range and a last tile of 27 records.
# nq = 5 is a group of 4 and a single query; nq = 7 at the large size adds the pass with an unused slot.
@pytest.mark.parametrize("n,nq", [(20000, 5), (BIG_N, 5), (BIG_N, 7)])
def test_every_dispatch_form(device, big_dbs, queries, n, nq):
    _check_large(device, big_dbs[n], queries, nq, 0, n, [0, 31, 32, 63, 64, n - 33, n - 32, n - 28, n - 27, n - 1],
                 n == BIG_N)


def test_large_form_by_size_from_an_odd_first_record(device, big_dbs, queries):
    """first = 5 and 3 records short of the end: still 4097 tiles, so the large form runs by size,
    with a first tile of 27 records (element-wise stores, then tiles at (tile_t0 - first) % 8 == 3),
    a last tile of 24 and, at nq = 6, a pass of two behind the full group."""
    first, n = 5, BIG_N - 5 - 3
    assert (first + n + 31) // 32 - first // 32 == SPLIT_TILES + 1
    last_tile = SPLIT_TILES * 32 - first  # the last tile's first record, relative to first
    _check_large(device, big_dbs[BIG_N], queries, 6, first, n,
                 [0, 26, 27, 58, 59, last_tile - 32, last_tile - 1, last_tile, n - 2, n - 1], True)


# ---------------------------------------------------------------- 7. host and device forms


def test_host_and_device_forms_agree_and_engines_share_nothing(ctx, queries, want257):
    device, layout, _ = ctx
    qa, qb = queries[:6], queries[10:13]
    with _db257(device, layout) as db257:
        a = ih.DistanceBatchEngine(device, qa)
        host_a = np.zeros((6, 257, ROT), np.uint16)
        a.batch_process(host_a, db257)
        b = ih.DistanceBatchEngine(device, qb)
        dev_a = _device_rows(device, a, db257, 0, 257, 6)
        dev_b = _device_rows(device, b, db257, 0, 257, 3)
        a.close()
        a2 = ih.DistanceBatchEngine(device, queries[20:26])  # reuses a's pooled query buffers
        host_b = np.zeros((3, 257, ROT), np.uint16)
        b.batch_process(host_b, db257)
        dev_a2 = _device_rows(device, a2, db257, 0, 257, 6)
        b.close()
        a2.close()
    assert host_a.tobytes() == dev_a.tobytes() and (host_a == want257[:6]).all()
    assert host_b.tobytes() == dev_b.tobytes() and (host_b == want257[10:13]).all()
    assert (dev_a2 == want257[20:26]).all()


# ---------------------------------------------------------------- 8. error paths


def test_error_paths_leave_the_device_usable(ctx, queries, want257):
    device, layout, _ = ctx
    lib = ih.load_library()
    nq = 3

    def err():
        return lib.iris_last_error().decode(errors="replace")

    out = np.zeros((nq, 257, ROT), np.uint16)
    with _db257(device, layout) as db257, ih.DistanceBatchEngine(device, queries[:nq]) as eng, \
            ih.DistanceEngine(device, queries[0]) as single, \
            ih.Database(device, ih.KIND_MASKS, 64, ih.LAYOUT_TILES) as masks:
        masks.generate(64, 3)
        for bad in (np.zeros((0, ih.BITS), np.uint16), np.zeros((65, ih.BITS), np.uint16)):
            with pytest.raises(ih.IrisError) as ei:
                ih.DistanceBatchEngine(device, bad)
            assert ei.value.code == E_ARG and str(ei.value)
        cases = [
            (lib.iris_distance_batch_process, (None, db257.handle, 0, 1, ih._ptr(out)), E_ARG),
            (lib.iris_distance_batch_process, (eng.handle, None, 0, 1, ih._ptr(out)), E_ARG),
            (lib.iris_distance_batch_process, (eng.handle, db257.handle, 0, 1, None), E_ARG),
            (lib.iris_distance_batch_process_device, (eng.handle, db257.handle, 0, 1, None), E_ARG),
            (lib.iris_distance_batch_process, (eng.handle, masks.handle, 0, 1, ih._ptr(out)), E_ARG),
            (lib.iris_distance_batch_process, (eng.handle, db257.handle, 200, 100, ih._ptr(out)), E_RANGE),
            (lib.iris_distance_batch_process_device, (eng.handle, db257.handle, 258, 0, ih._ptr(out)), E_RANGE),
            # a batch engine handed to the single-query calls, and the reverse
            (lib.iris_engine_batch_process, (eng.handle, db257.handle, 0, 1, ih._ptr(out)), E_ARG),
            (lib.iris_engine_batch_process_device, (eng.handle, db257.handle, 0, 1, ih._ptr(out)), E_ARG),
            (lib.iris_engine_batch_process_host, (eng.handle, ih._ptr(queries), 1, ih._ptr(out)), E_ARG),
            (lib.iris_distance_batch_process, (single.handle, db257.handle, 0, 1, ih._ptr(out)), E_ARG),
            (lib.iris_distance_batch_process_device, (single.handle, db257.handle, 0, 1, ih._ptr(out)), E_ARG),
        ]
        for f, args, code in cases:
            assert f(*args) == code, (f.__name__, args[2:4])
            assert err(), f.__name__
        assert (out == 0).all()
        # n == 0 is fine and writes nothing, even with a NULL output
        assert lib.iris_distance_batch_process(eng.handle, db257.handle, 32, 0, None) == 0
        # the device still works: a correct call of each engine
        eng.batch_process(out, db257)
        assert (out == want257[:nq]).all()
        one = np.zeros((257, ROT), np.uint16)
        single.batch_process(one, db257)
        assert (one == want257[0]).all()


# ---------------------------------------------------------------- 9. the C++ program


@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles-mfma", "lanes-valu"])
def test_cpp_distance_batch_engine(device, layout, tmp_path):
    """iris_hip.hpp's DistanceBatchEngine, run as its own process at nq = 3, n = 100."""
    nq, n, seed = 3, 100, 33
    exe = build_cpp_program(tmp_path)
    rows = tmp_path / "rows.bin"
    r = subprocess.run([str(exe), str(rows), str(nq), str(n), str(seed), str(layout)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.fromfile(rows, np.uint16).reshape(nq, n, ROT)
    i = np.arange(ih.BITS, dtype=np.uint64)
    q = np.stack([((i * (2 * j + 3) + 7 * j + (i >> np.uint64(3))) & np.uint64(0xFFFF)).astype(np.uint16)
                  for j in range(nq)])
    with ih.Database(device, ih.KIND_SHARES, n + 57, layout) as db, ih.DistanceBatchEngine(device, q) as eng:
        db.generate(n + 57, seed)
        want = np.zeros((nq, n, ROT), np.uint16)
        eng.batch_process(want, db, first=57, n=n)
    assert (got == want).all()
    assert (want[1] == oc.distance_batch(q[1], oc.gen_shares(seed, 57, n))).all()
