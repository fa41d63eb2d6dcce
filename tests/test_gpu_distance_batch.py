"""GPU: the batched DistanceEngine (iris_distance_batch_*): every query's slab equals what a
DistanceEngine of that query writes -- against the CPU oracle on small databases, and against the
single-query engine (itself checked against the oracle by test_gpu_parity.py) plus sampled oracle
rows at the sizes that reach the other kernel forms.

Dispatch on a TILES database (csrc/iris_shares_batch.hip): ranges of up to 4096 tiles of 32 records
(131 072 records) run full groups of 4 queries in the K-split batch form and left-over queries as
single-query passes; larger ranges run groups of 4 queries in the form with one tile per wave and 4
waves per workgroup (no persistent grid: one workgroup per 4 tiles), 2 or 3 left-over queries in
the same form with unused slots, a single one in the single-query kernel."""
import subprocess

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_distance_batch_abi import build_cpp_program

pytestmark = pytest.mark.gpu
ROT = 31
E_ARG, E_RANGE = -1, -5
SPLIT_TILES = 4096  # kSharesBatchSplitTiles


@pytest.fixture(scope="module", params=[ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles-mfma", "lanes-valu"])
def layout(request):
    return request.param


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


@pytest.fixture(scope="module")
def db257(device, layout):
    db = ih.Database(device, ih.KIND_SHARES, 300, layout)
    db.generate(257, 8)
    yield db
    db.close()


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


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 64])
def test_slot_identity_and_group_edges(device, db257, queries, want257, nq):
    with ih.DistanceBatchEngine(device, queries[:nq]) as eng:
        assert eng.nq == nq
        out = np.zeros((nq, 257, ROT), np.uint16)
        eng.batch_process(out, db257)
    for q in range(nq):
        assert (out[q] == want257[q]).all(), f"slab {q} of {nq}"


def test_range_edges(device, db257, queries, want257):
    nq = 5
    with ih.DistanceBatchEngine(device, queries[:nq]) as eng:
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


def test_byte_bias_extremes(device, layout):
    """Rows whose bytes sit at the ends of the XOR-0x80 bias, where the 128 * sum corrections of a
    multi-query epilogue go wrong first."""
    consts = [0x0000, 0xFFFF, 0x8000, 0x7FFF, 0x00FF, 0xFF00, 0x0080, 0x8080]
    rng = np.random.default_rng(5)
    shares = rng.integers(0, 1 << 16, (70, ih.BITS), dtype=np.uint16)
    q = rng.integers(0, 1 << 16, (8, ih.BITS), dtype=np.uint16)
    for i, c in enumerate(consts):
        shares[3 + 7 * i] = c
        q[i] = c
    q[5, ::3] = 0x1234  # not every query constant
    with ih.Database(device, ih.KIND_SHARES, 70, layout) as db, ih.DistanceBatchEngine(device, q) as eng:
        db.append(shares)
        out = np.zeros((8, 70, ROT), np.uint16)
        eng.batch_process(out, db)
    for i in range(8):
        assert (out[i] == oc.distance_batch(q[i], shares)).all(), i


# 20 000 records = 625 tiles: the K-split form (a participant's chunk).  131 099 records = 4097
# tiles, one past SPLIT_TILES: the large form, 1025 workgroups of 4 waves, the last with three
# waves past the range and a last tile of 27 records.
# nq = 5 is a group of 4 and a single query; nq = 7 at the large size adds the pass with an unused slot.
@pytest.mark.parametrize("n,nq", [(20000, 5), (SPLIT_TILES * 32 + 27, 5), (SPLIT_TILES * 32 + 27, 7)])
def test_every_dispatch_form(device, queries, n, nq):
    seed = 21
    with ih.Database(device, ih.KIND_SHARES, n, ih.LAYOUT_TILES) as db:
        db.generate(n, seed)
        with ih.DistanceBatchEngine(device, queries[:nq]) as eng:
            got = _device_rows(device, eng, db, 0, n, nq)
        for q in range(nq):
            with ih.DistanceEngine(device, queries[q]) as single:
                assert (got[q] == _device_rows(device, single, db, 0, n)).all(), f"slab {q}"
        rows = np.unique(np.concatenate([[0, 31, 32, 63, 64, n - 33, n - 32, n - 28, n - 27, n - 1],
                                         np.random.default_rng(9).integers(0, n, 54)]))  # 64 at most
        ref = np.concatenate([oc.gen_shares(seed, int(i), 1) for i in rows])
        for q in range(nq):
            assert (got[q][rows] == oc.distance_batch(queries[q], ref)).all(), f"slab {q} against the oracle"


def test_host_and_device_forms_agree_and_engines_share_nothing(device, db257, queries, want257):
    qa, qb = queries[:6], queries[10:13]
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


def test_error_paths_leave_the_device_usable(device, db257, queries, want257):
    lib = ih.load_library()
    nq = 3

    def err():
        return lib.iris_last_error().decode(errors="replace")

    out = np.zeros((nq, 257, ROT), np.uint16)
    with ih.DistanceBatchEngine(device, queries[:nq]) as eng, ih.DistanceEngine(device, queries[0]) as single, \
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
