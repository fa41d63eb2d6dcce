"""GPU: record I/O in full -- the code that fills a device database and reads it back computes
nothing, and every row, match and winner the library reports is read from what it stored.  The pack /
unpack / generate kernels of both layouts and the host loops that cut a transfer into chunks and
double-buffer them (db_write_pinned, db_write_runtime, iris_db_read, iris_db_generate of
iris_api.hip; iris_db_load_file's three paths and iris_db_save_file of iris_io.hip) are compared
here record for record, over every record moved, at every chunk seam.

Rules every test keeps: records are uniformly random over the dtype's whole range (a dropped or
doubled record never compares equal); every transfer starts at an index that is no multiple of 64
(after 3 or 37 records, or first = 13), so every seam lies inside a TILES tile and a LANES block, and
ends ragged; every seam position is derived from the constants of the sources (Consts, read from
csrc/) and the page size, and the test asserts that the transfer crosses the seams it is there for
-- by those positions and by the "pack" / "unpack" / "generate" launches the library counted -- so a
change of a constant fails loudly instead of testing nothing.

What the suite did not look at before, and the test that now does:
1. a pinned write's slot seams (masks never, one layout only)   test_pinned_write_slots, and
   test_gpu_parity.py::test_large_write_paths now reads in full
2. db_write_runtime's second chunk (256 MB staging)              test_runtime_write_crosses_staging_chunk
3. iris_db_read's pinned slots: shares, LANES, first != 0        test_pinned_read_slots,
                                                                 test_pinned_read_three_slots
4. iris_db_save_file beyond one chunk (chunks start mid-tile)    test_save_file_chunks
5. iris_db_load_file in several chunks: shares, LANES, the       test_load_file_paths,
   window path's lead chunk, after an unaligned len              test_load_file_share_leads,
                                                                 test_load_file_count_mid_chunk
6. iris_db_write into the middle of a populated database         test_overwrite_in_place
7. iris_db_generate's grid-stride tail, global_index0 != 0       test_generate_grid_stride
8. a layout that pack and unpack agree on but the engines do     check_engine_rows, on every database of
   not read: engine rows against the oracle around every seam    items 1, 2 and 5
9. the packed masks rows at the packing boundary                 test_gpu_resident.py::test_packed_rows_boundary,
                                                                 test_packed_boundary.py (CPU: the fixture's facts)

Sizes: items 1, 6 use the smallest writes of the pinned path (just over kUploadTuneMin, slots of
kUploadPieceMin: three or four slots, the third reuses pinned buffer 0, the last is short); item 2
one chunk_records() chunk and a rest; item 3 one kUploadSlot slot and a rest (one seam), and once
three slots; items 4 and 5 two kIoChunkBytes chunks and a rest, so that the third chunk reuses the
first buffer on every path.

Out of scope: iris_prepare_shares' chunking (test_gpu_prepare.py), device groups' load_file,
attach_host, transfers past 2^32 bytes (test_gpu_seams.py), and any assertion on time.

The file's 74 tests take 8 s together on an MI355X, of the 90 s the seams file set as a budget; the
slowest, 0.3 s, is the first to open a hooked device (profiles/r20_db_io.txt has every test's time,
and a library with three of these loops and kernels made subtly wrong failing the tests that cover
them)."""
import contextlib
import ctypes
import functools
import math
import os
import pathlib
import re

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_gpu_io import KINDS, LOAD_PATHS, _records, open_load_path

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "mpc-iris-code_amd" / "csrc"
ROT, TILE = 31, 32
REC_BYTES = {ih.KIND_TEMPLATES: 3200, ih.KIND_MASKS: 1600, ih.KIND_SHARES: 25600}
LAYOUTS = [ih.LAYOUT_TILES, ih.LAYOUT_LANES]
LAYOUT_IDS = ["tiles", "lanes"]
KIND_IDS = ["masks", "shares", "templates"]
DTYPE = {kind: (dtype, width) for kind, dtype, width in KINDS}
E_RANGE = -5
BASE = 2**40 + 3  # generator index of the generated records
PAGE = os.sysconf("SC_PAGESIZE")

kinds = pytest.mark.parametrize("kind,dtype,width", KINDS, ids=KIND_IDS)
layouts = pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)


# ---------------------------------------------------------------- the sources' constants and loops


@functools.lru_cache(None)
def const(file, name):
    """`constexpr T name = A << B;` (or `= A;`) of a source file."""
    m = re.search(rf"constexpr \w+ {name} = (\d+)(?:ull)?(?: << (\d+))?;", (CSRC / file).read_text())
    assert m, (file, name)
    return int(m.group(1)) << int(m.group(2) or 0)


class Consts:
    upload_slot = const("iris_handles.hpp", "kUploadSlot")          # 64 MB: a pinned upload slot
    upload_ring = const("iris_handles.hpp", "kUploadRing")          # 2 pinned slots per device
    upload_tune_min = const("iris_handles.hpp", "kUploadTuneMin")   # 8 MB: from here the pinned paths
    staging = const("iris_handles.hpp", "kStagingBytes")            # 256 MB: chunk_records()
    piece_min = const("iris_api.hip", "kUploadPieceMin")            # 4 MB: a pinned write's smallest slot
    io_chunk = const("iris_io.hip", "kIoChunkBytes")                # 64 MB: a file chunk
    lanes = const("iris_internal.hpp", "kLanes")                    # 64: a LANES block


def pinned_write_slot(kind, n):
    """Records per slot of db_write_pinned for a write of n records."""
    rb = REC_BYTES[kind]
    piece = min(Consts.upload_slot, max(Consts.piece_min, n * rb // 4))
    return max(64, piece // rb // 64 * 64)


def runtime_chunk(kind):
    """chunk_records(): db_write_runtime's chunk (and the small reads')."""
    return max(64, Consts.staging // REC_BYTES[kind] // 64 * 64)


def read_slot(kind):
    """Records per slot of iris_db_read's pinned path."""
    return max(64, Consts.upload_slot // REC_BYTES[kind] // 64 * 64)


def io_chunk(kind):
    """Records per chunk of iris_db_save_file and of iris_db_load_file's pread path."""
    return max(1, Consts.io_chunk // REC_BYTES[kind])


def chunks(n, ch, lead=0):
    """Sizes of the pieces a loop cuts n records into: `lead` first (if any), then `ch` each."""
    sizes = [min(lead, n)] if lead and n else []
    done = sum(sizes)
    while done < n:
        sizes.append(min(ch, n - done))
        done += sizes[-1]
    return sizes


def seams(sizes, start=0):
    """Database indices at which a piece after the first starts."""
    return [start + int(s) for s in np.cumsum(sizes)[:-1]]


def load_chunks(path, kind, first, n):
    """The pieces of iris_db_load_file(first, n) on one of its paths."""
    rb, ch = REC_BYTES[kind], io_chunk(kind)
    if path == "slots":  # db_write_pinned, filled by pread
        return chunks(n, pinned_write_slot(kind, n))
    if path == "pread":
        return chunks(n, ch)
    unit = PAGE // math.gcd(PAGE, rb)  # registered windows end on page-aligned record boundaries
    return chunks(n, max(unit, ch // unit * unit), -first % unit)


def assert_seams_inside_blocks(where):
    """Every seam lies inside a TILES tile and inside a LANES block."""
    assert where and all(s % TILE and s % Consts.lanes for s in where), where


@contextlib.contextmanager
def counting(dev):
    """The launches the library counts between here and the block's end: name -> (launches, records)."""
    got = {}
    dev.synchronize()
    dev.reset_stats()
    dev.set_profiling(True)
    try:
        yield got
        dev.synchronize()
        for name in ("pack", "unpack", "generate"):
            launches, _, items = dev.kernel_stats(name)
            got[name] = (launches, items)
    finally:
        dev.set_profiling(False)


def equal_records(got, want):
    """Every record equal; names the first ones that are not."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} records differ, the first at {bad[:8].tolist()}"
    return True


# ---------------------------------------------------------------- A.7: the layout is the engines' own

HALF = 40  # records on either side of a seam


@functools.lru_cache(None)
def query_template():
    return oc.gen_templates(4242, 0, 1)[0]


def seam_windows(n, where):
    """[lo, hi) ranges of 40 records on either side of every seam and of the first and last record,
    overlapping ones merged."""
    out = []
    for s in sorted({0, n} | set(where)):
        lo, hi = max(0, s - HALF), min(n, s + HALF)
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(lo, hi) for lo, hi in out]


def check_engine_rows(dev, db, kind, want, where):
    """The kind's single-query engine over the windows of seam_windows(len(db), where) -- the one
    place that does not compare in full, for the oracle's cost: its rows equal the oracle's on
    `want`, the records the database was just shown to hold.  A write and a read that agree on a
    wrong index formula pass every round trip; the engine kernels read the layout themselves."""
    n = len(db)
    assert want.shape[0] == n
    wins = seam_windows(n, where)
    qt = query_template()
    if kind == ih.KIND_TEMPLATES:
        with ih.TemplateEngine(dev, qt) as eng:
            for lo, hi in wins:
                num, den = eng.counts(db, first=lo, n=hi - lo)
                wnum, wden = oc.template_counts(qt, want[lo:hi])
                assert (num == wnum).all() and (den == wden).all(), (lo, hi, wins)
        return
    if kind == ih.KIND_MASKS:
        q, eng, ref = qt[200:], ih.MasksEngine, oc.masks_batch
    else:
        q, eng, ref = oc.encode(qt), ih.DistanceEngine, oc.distance_batch
    with eng(dev, q) as e:
        for lo, hi in wins:
            out = np.empty((hi - lo, ROT), np.uint16)
            e.batch_process(out, db, first=lo, n=hi - lo)
            assert (out == ref(q, want[lo:hi])).all(), (lo, hi, wins)


# ---------------------------------------------------------------- A.1, A.2: the write paths


def smallest_pinned_write(kind):
    """Just over kUploadTuneMin: 5 300 masks, 2 679 templates, 385 shares."""
    return -(-Consts.upload_tune_min // REC_BYTES[kind]) + 57


@layouts
@kinds
def test_pinned_write_slots(hooked_device, kind, dtype, width, layout):
    """IRIS_UPLOAD=pinned, the smallest write that takes the path (just over 8 MB), appended after 3
    records: slots of 4 MB (2 560 masks, 1 280 templates, 128 shares), so three or four of them, the
    third into pinned buffer 0 again, the last one short.  Read back in full; engine rows at every
    seam."""
    dev = hooked_device(IRIS_UPLOAD="pinned")
    n = smallest_pinned_write(kind)
    recs = _records(kind, dtype, width, 3 + n, 100 + kind)
    sizes = chunks(n, pinned_write_slot(kind, n))
    assert n * REC_BYTES[kind] >= Consts.upload_tune_min
    assert len(sizes) > Consts.upload_ring and sizes[-1] < sizes[0], sizes  # a buffer reused, a short slot
    where = seams(sizes, 3)
    assert_seams_inside_blocks(where)
    with ih.Database(dev, kind, 3 + n, layout) as db:
        db.append(recs[:3])
        with counting(dev) as got:
            db.append(recs[3:])
        assert got["pack"] == (len(sizes), n), (got, sizes)
        assert len(db) == 3 + n
        assert equal_records(db.read(0, 3 + n), recs)
        check_engine_rows(dev, db, kind, recs, [3] + where)


@pytest.mark.parametrize("kind,layout", [(ih.KIND_SHARES, ih.LAYOUT_LANES), (ih.KIND_TEMPLATES, ih.LAYOUT_TILES)],
                         ids=["shares-lanes", "templates-tiles"])
def test_runtime_write_crosses_staging_chunk(hooked_device, kind, layout):
    """IRIS_UPLOAD=runtime, one chunk_records() chunk (256 MB: 10 432 shares, 83 840 templates) and
    101 records, appended after 37: the loop's second iteration, which reuses the staging buffer.  The
    loop does not depend on the kind, so one kind per layout.  Read back in full (through five slots
    of the pinned read path); engine rows at the seam."""
    dev = hooked_device(IRIS_UPLOAD="runtime")
    dtype, width = DTYPE[kind]
    ch = runtime_chunk(kind)
    n = ch + 101
    recs = _records(kind, dtype, width, 37 + n, 200 + kind)
    sizes = chunks(n, ch)
    assert len(sizes) == 2 and sizes[-1] < sizes[0]
    where = seams(sizes, 37)
    assert_seams_inside_blocks(where)
    with ih.Database(dev, kind, 37 + n, layout) as db:
        db.append(recs[:37])
        with counting(dev) as got:
            db.append(recs[37:])
        assert got["pack"] == (2, n), got
        assert len(db) == 37 + n
        with counting(dev) as got:
            full = db.read(0, 37 + n)
        assert got["unpack"] == (len(chunks(37 + n, read_slot(kind))), 37 + n), got
        assert equal_records(full, recs)
        check_engine_rows(dev, db, kind, recs, [37] + where)


# ---------------------------------------------------------------- A.3: overwrite in place


@pytest.mark.parametrize("path", ["pinned", "runtime"])
@layouts
@pytest.mark.parametrize("kind,dtype,width", KINDS[:2], ids=KIND_IDS[:2])
def test_overwrite_in_place(hooked_device, kind, dtype, width, layout, path):
    """iris_db_write of 8 MB into a database of three or four slots, at an index that is unaligned
    and no seam of the write that filled it: wholly inside, then running past len.  The whole
    database equals the expected array and len is right after each; a write that starts beyond len,
    or runs past the capacity, is refused and changes nothing."""
    dev = hooked_device(IRIS_UPLOAD=path)
    n0 = 3 + smallest_pinned_write(kind)
    m = -(-Consts.upload_tune_min // REC_BYTES[kind]) + 5
    expected = _records(kind, dtype, width, n0, 300 + kind)
    first_seams = [3] + seams(chunks(n0 - 3, pinned_write_slot(kind, n0 - 3)), 3)
    inside, past = 37, n0 - 150
    for at in (inside, past):
        assert at % 64 and at % TILE and at not in first_seams and 0 < at < n0
    assert inside + m < n0 < past + m
    launches = len(chunks(m, pinned_write_slot(kind, m))) if path == "pinned" else 1
    assert m * REC_BYTES[kind] >= Consts.upload_tune_min and (path != "pinned" or launches > Consts.upload_ring)
    with ih.Database(dev, kind, past + m + 10, layout) as db:
        db.append(expected[:3])
        db.append(expected[3:])
        for i, at in enumerate((inside, past)):
            w = _records(kind, dtype, width, m, 310 + 10 * i + kind)
            with counting(dev) as got:
                db.write(at, w)
            assert got["pack"] == (launches, m), got
            expected = np.concatenate([expected[:at], w, expected[at + m:]])
            assert len(db) == expected.shape[0] == max(n0, at + m)
            assert equal_records(db.read(0, len(db)), expected)
        n1, cap = len(db), db.capacity
        assert m > cap - n1
        for at in (n1 + 1, n1, n1 - 3):  # beyond len; past the capacity, from len and from inside
            with pytest.raises(ih.IrisError) as ei:
                db.write(at, w)
            assert ei.value.code == E_RANGE, ei.value
            assert len(db) == n1
        assert equal_records(db.read(0, n1), expected)


# ---------------------------------------------------------------- A.4: the pinned read path


def read_into(db, first, n, dest_address):
    ih._check(ih.load_library().iris_db_read(db.handle, int(first), int(n), ctypes.c_void_p(dest_address)))


def check_pinned_read(device, kind, dtype, width, layout, slots, seed):
    """read(13, n) of `slots` full slots and 83 records, from a database that goes on for 5 more:
    into a fresh array, and into one that starts 2 bytes after a 64-byte boundary (parallel_copy's
    destination; the bytes around it stay as they were)."""
    ch, rb = read_slot(kind), REC_BYTES[kind]
    n = slots * ch + 83
    sizes = chunks(n, ch)
    assert n * rb >= Consts.upload_tune_min and len(sizes) == slots + 1 and sizes[-1] < ch
    assert_seams_inside_blocks(seams(sizes, 13))
    recs = _records(kind, dtype, width, 13 + n + 5, seed)
    want = recs[13:13 + n]
    with ih.Database(device, kind, 13 + n + 5, layout) as db:
        db.append(recs)
        with counting(device) as got:
            fresh = db.read(13, n)
        assert got["unpack"] == (len(sizes), n), (got, sizes)
        assert equal_records(fresh, want)
        del fresh
        buf = np.full(n * rb + 256, 0x5A, np.uint8)
        at = (2 - buf.ctypes.data) % 64 + 64
        assert (buf.ctypes.data + at) % 64 == 2
        with counting(device) as got:
            read_into(db, 13, n, buf.ctypes.data + at)
        assert got["unpack"] == (len(sizes), n), (got, sizes)
        assert (buf[:at] == 0x5A).all() and (buf[at + n * rb:] == 0x5A).all()
        assert equal_records(buf[at:at + n * rb].reshape(n, rb), want.view(np.uint8).reshape(n, rb))


@layouts
@kinds
def test_pinned_read_slots(device, kind, dtype, width, layout):
    """One 64-MB slot (41 920 masks, 20 928 templates, 2 560 shares) and a ragged rest, from
    first = 13: the seam that only TILES masks and templates crossed, and only from record 0."""
    check_pinned_read(device, kind, dtype, width, layout, 1, 400 + kind)


def test_pinned_read_three_slots(device):
    """Two full slots and a rest: slot 2 is copied into pinned buffer 0 after slot 0 has left it."""
    kind, dtype, width = KINDS[0]
    assert 3 > Consts.upload_ring
    check_pinned_read(device, kind, dtype, width, ih.LAYOUT_LANES, 2, 410)


# ---------------------------------------------------------------- A.5, A.6: record files


def file_records(kind):
    """13 records to skip, two file chunks, a ragged rest of an eighth of a chunk."""
    ch = io_chunk(kind)
    return 13 + 2 * ch + (ch // 8 | 1)


@pytest.fixture(scope="module")
def record_files(tmp_path_factory):
    """One file of uniformly random records per kind, written once: kind -> (path, records)."""
    made = {}

    def get(kind):
        if kind not in made:
            dtype, width = DTYPE[kind]
            recs = _records(kind, dtype, width, file_records(kind), 500 + kind)
            path = tmp_path_factory.mktemp("db_io") / f"kind{kind}.records"
            recs.astype(np.dtype(dtype).newbyteorder("<"), copy=False).tofile(path)
            made[kind] = (path, recs)
        return made[kind]

    return get


def check_load(dev, path_name, kind, layout, file, recs, first, count=None):
    """load_file(first, count) into a database that holds 3 records (37 where a seam would otherwise
    fall on a tile boundary: the pread path's share chunk of 2 621 records ends at 3 + 2 621 = 82
    tiles): loaded and len, the pieces the path cuts it into, every record, and the engine's rows
    around every seam."""
    dtype, width = DTYPE[kind]
    n = recs.shape[0] - first if count is None else count
    sizes = load_chunks(path_name, kind, first, n)
    assert len(sizes) >= 3, sizes  # two seams: the third piece reuses the first buffer
    h = next(h for h in (3, 37) if all(s % TILE and s % Consts.lanes for s in seams(sizes, h)))
    where = seams(sizes, h)
    assert_seams_inside_blocks(where)
    head = _records(kind, dtype, width, h, 600 + kind)
    with ih.Database(dev, kind, h + n, layout) as db:
        db.append(head)
        with counting(dev) as got:
            loaded = db.load_file(file, first=first, count=count)
        assert loaded == n and len(db) == h + n
        assert got["pack"] == (len(sizes), n), (got, sizes)
        full = db.read(0, h + n)
        assert equal_records(full[:h], head) and equal_records(full[h:], recs[first:first + n])
        check_engine_rows(dev, db, kind, full, [h] + where)
    return sizes


@pytest.mark.parametrize("path", LOAD_PATHS)
@layouts
@kinds
def test_load_file_paths(device, hooked_device, record_files, kind, dtype, width, layout, path):
    """Two 64-MB chunks and a rest from first = 13, on each of the loader's paths: the pinned
    upload slots (pieces of a quarter of the load), the registered windows (a lead chunk up to the
    first page-aligned record boundary, then chunks of whole pages) and pread into two buffers."""
    file, recs = record_files(kind)
    check_load(open_load_path(path, device, hooked_device), path, kind, layout, file, recs, 13)


@pytest.mark.parametrize("path", LOAD_PATHS)
@layouts
@pytest.mark.parametrize("first", [1, 2, 3])
def test_load_file_share_leads(device, hooked_device, record_files, first, layout, path):
    """Shares (25 600 B: 4 records are 25 pages) from first = 1, 2 and 3: the window path's lead
    chunk of 3, 2 and 1 records; the other two paths start their pieces there."""
    kind = ih.KIND_SHARES
    file, recs = record_files(kind)
    sizes = check_load(open_load_path(path, device, hooked_device), path, kind, layout, file, recs, first)
    if path == "windows":
        assert sizes[0] == 4 - first and PAGE // math.gcd(PAGE, REC_BYTES[kind]) == 4


@pytest.mark.parametrize("path", LOAD_PATHS)
def test_load_file_count_mid_chunk(device, hooked_device, record_files, path):
    """`count` ends in the middle of the file's last piece: nothing behind it is loaded."""
    kind, layout = ih.KIND_SHARES, ih.LAYOUT_LANES
    file, recs = record_files(kind)
    count = 2 * io_chunk(kind) + io_chunk(kind) // 16
    sizes = check_load(open_load_path(path, device, hooked_device), path, kind, layout, file, recs, 13, count)
    assert 13 + count + 50 < recs.shape[0] and sizes[-1] < max(sizes)


@layouts
@kinds
def test_save_file_chunks(device, record_files, tmp_path, kind, dtype, width, layout):
    """save_file(13, n) of two 64-MB chunks (41 943 masks, 20 971 templates, 2 621 shares: no multiple
    of the tile, so every later chunk's unpack starts inside one) and a rest: the file's bytes are the
    records'.  The file then loads into a database of the other layout and reads back equal, which a
    round trip within one layout cannot show."""
    _, recs = record_files(kind)
    n = recs.shape[0] - 13 - 5
    sizes = chunks(n, io_chunk(kind))
    assert len(sizes) >= 3 and sizes[-1] < sizes[0], sizes
    assert_seams_inside_blocks(seams(sizes, 13))
    out = tmp_path / "saved.records"
    other = ih.LAYOUT_LANES if layout == ih.LAYOUT_TILES else ih.LAYOUT_TILES
    with ih.Database(device, kind, recs.shape[0], layout) as db:
        db.append(recs)
        with counting(device) as got:
            db.save_file(out, first=13, n=n)
        assert got["unpack"] == (len(sizes), n), (got, sizes)
    assert out.stat().st_size == n * REC_BYTES[kind]
    saved = np.fromfile(out, np.dtype(dtype).newbyteorder("<")).reshape(n, width)
    assert equal_records(saved.astype(dtype, copy=False), recs[13:13 + n])
    del saved
    with ih.Database(device, kind, n, other) as db:
        assert db.layout == other and db.load_file(out) == n
        assert equal_records(db.read(0, n), recs[13:13 + n])


# ---------------------------------------------------------------- A.8: generate

GRID_THREADS = 256 * 64 * 256  # the generate kernels' grid cap: 16 384 workgroups of 256 threads
# threads per record: generate_tiles_kernel 2 * kPlaneGroups, generate_masks_tiles 2 * (kMaskChunks / 4),
# generate_shares_tiles 2 * kShareChunks; generate_kernel (LANES) one per 16-byte group of the record
GEN_THREADS = {(ih.KIND_TEMPLATES, ih.LAYOUT_TILES): 200, (ih.KIND_TEMPLATES, ih.LAYOUT_LANES): 200,
               (ih.KIND_MASKS, ih.LAYOUT_TILES): 100, (ih.KIND_MASKS, ih.LAYOUT_LANES): 100,
               (ih.KIND_SHARES, ih.LAYOUT_TILES): 800, (ih.KIND_SHARES, ih.LAYOUT_LANES): 1600}
ORACLE_GEN = {ih.KIND_TEMPLATES: oc.gen_templates, ih.KIND_MASKS: oc.gen_masks, ih.KIND_SHARES: oc.gen_shares}


@layouts
@kinds
def test_generate_grid_stride(device, kind, dtype, width, layout):
    """iris_db_generate past one pass of its grid: n is a tenth more than the 4 194 304 threads of
    the capped grid cover (above 20 971 templates, 41 943 masks, 5 242 TILES / 2 621 LANES shares), so
    the grid-stride loop runs its second, partial pass.  Appended after 37 records, which stay as
    they were, with global_index0 = 2^40 + 3; a second generate behind it continues the index.
    Every record equals the oracle's generator."""
    per = GEN_THREADS[kind, layout]
    n, n2, seed = GRID_THREADS // per * 11 // 10 + 3, 777, 700 + kind
    assert GRID_THREADS < n * per < 2 * GRID_THREADS and n % 64 and (37 + n) % 64
    head = _records(kind, dtype, width, 37, 710 + kind)
    with ih.Database(device, kind, 37 + n + n2, layout) as db:
        db.append(head)
        with counting(device) as got:
            db.generate(n, seed, BASE)
        assert got["generate"] == (1, n), got
        db.generate(n2, seed, BASE + n)
        assert len(db) == 37 + n + n2
        full = db.read(0, len(db))
    assert equal_records(full[:37], head)
    assert equal_records(full[37:], ORACLE_GEN[kind](seed, BASE, n + n2))
