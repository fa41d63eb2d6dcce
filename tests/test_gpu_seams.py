"""GPU: the batched and select kernels where their address arithmetic can go wrong without the small
fixtures of their own test files noticing: records whose device offset lies past 2^31, 2^32 and 2^36
bytes, row arrays of more than 2^32 bytes, and more than 65535 queries in one top-k merge level.

A. A generated database of seam tile + 65 tiles (2.2 / 4.3 GB for the 2^31 and 2^32 seams together,
   68.8 GB for 2^36) and, per seam, a range of 17 tiles (the seam tile is tile 8) and one of 83 tiles
   (tile 40: more than one workgroup of every form).  Winners, matches and top-k entries are planted
   at the last record before the seam block, the block's first and last record and the first record
   after it -- for the TILES tile of 32 records and the LANES block (kLanes of iris_internal.hpp)
   alike: both hold the seam byte and lie inside one 64-record block, so one fixture serves both
   layouts -- with an equal-distance pair on both sides of the seam (the lower index wins) and exact
   copies of the queries just outside the range, which must never be found.
B. nq = 64, first = 5, n = 1 090 027: [64][n][31] u16 is 4 325 227 136 B > 2^32; element 2^31 is row
   601 965 of slab 63.
C. 65535 + 9 queries in one TemplateBatchEngine: the merge level's launch seam (blockIdx.y).

Everything is compared bit for bit with lists built from the CPU oracle (rows as u16; Match records
byte for byte, the distance as its f64 bits), with the helpers of the sibling files.  A database
belongs to one device handle: every variant generates its own and closes it.

Every form sees every seam: the whole file takes 30 to 38 s on an MI355X, under its budget of 90 s,
so no 2^36 form was cut (profiles/r19_seams.txt has the timings; the slowest tests, 5 to 6 s, are
those that allocate right after a 68.8-GB database was released).
The forms are those the kernels' own files pin: templates on
a TILES database under the library's dispatch, IRIS_TILES_PER_WAVE=1 and =4 and on a LANES database;
the template batch in its default shape and under IRIS_BATCH_KERNEL=2; the shared search passes under
FORCED and with IRIS_SEARCH_SHARE_EVEN=1; the masks batch and the fused single-query masks select as
"tiles", "tiles-batch1", "tiles-batch4" and "lanes"; the distance batch as "tiles-mfma", "tiles-batch"
and "lanes-valu".

Out of scope here: iris_resolver_matches / iris_resolver_topk on device arrays past 2^32 bytes (that
needs 69M-row arrays built on the host), device groups, and ranges of more than 2^32 records.

For masks and shares there is nothing to find outside a range (the participants' rows exist for the
range only); a wrong record shows as a wrong denominator or row."""
import contextlib
import ctypes
import functools
import pathlib
import re

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_gpu_distance_batch import FILL as ROW_FILL
from test_gpu_distance_batch import _guarded_device_rows
from test_gpu_masks_batch_matches import background, planted_shares, slab_ptrs, want_records
from test_gpu_masks_batch_matches import batch_call as masks_batch_matches_call
from test_gpu_masks_batch_matches import check_against_oracle as masks_batch_matches_check
from test_gpu_masks_batch_topk import batch_call as masks_batch_topk_call
from test_gpu_masks_batch_topk import check_against_oracle as masks_batch_topk_check
from test_gpu_matches import DeviceArrays, _near_copy, resolver_expected
from test_gpu_search_share import FORCED, blocking, fields, grid_of, submit
from test_gpu_template_batch_matches import Expected, open_variant
from test_gpu_template_batch_matches import batch_call as template_batch_matches_call
from test_gpu_template_batch_matches import check_against_oracle as template_batch_matches_check
from test_gpu_template_batch_topk import batch_call as template_batch_topk_call
from test_gpu_template_batch_topk import check_against_oracle as template_batch_topk_check
from test_gpu_topk import order

gpu = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]
ROT, TILE = 31, 32
INF = float("inf")
BASE = 2**40 + 3
FILL = 0x5A
UNTOUCHED = bytes([FILL]) * 32
REC_BYTES = {ih.KIND_TEMPLATES: 3200, ih.KIND_MASKS: 1600, ih.KIND_SHARES: 25600}
# the issue's table: the TILES seam tile of every kind at 2^31, 2^32 and 2^36 bytes
SEAM_TILES = {ih.KIND_TEMPLATES: {31: 20_971, 32: 41_943, 36: 671_088},
              ih.KIND_MASKS: {31: 41_943, 32: 83_886, 36: 1_342_177},
              ih.KIND_SHARES: {31: 2_621, 32: 5_242, 36: 83_886}}
SPANS = [(31, 17), (31, 83), (32, 17), (32, 83)]
SPANS36 = [(36, 17), (36, 83)]
T_SEED, Q_SEED, M_SEED, S_SEED = 3101, 3102, 3201, 3301
NQ_T, NQ_M, NQ_S = 12, 7, 7
T_LIST = 0.2  # the planted templates lie below 0.1, generated ones at 0.45 and above
T_MIXED = 0.482  # about half of the generated templates
KS = (1, 5, 64)


# ---------------------------------------------------------------- geometry


@functools.lru_cache(None)
def lanes_block():
    """Records of a LANES block, from the layout's own header."""
    text = (ROOT / "mpc-iris-code_amd" / "csrc" / "iris_internal.hpp").read_text()
    return int(re.search(r"constexpr int kLanes = (\d+);", text).group(1))


def seam_block(kind, layout, log2):
    """(first record, records) of the layout's block that holds byte 2^log2 of the database."""
    blk = TILE if layout == ih.LAYOUT_TILES else lanes_block()
    return (1 << log2) // (blk * REC_BYTES[kind]) * blk, blk


def db_records(kind, log2):
    """Seam tile + 65 tiles."""
    return (seam_block(kind, ih.LAYOUT_TILES, log2)[0] // TILE + 65) * TILE


class Span:
    """One range around a seam: `ntiles` tiles, from 5 records into a tile to 7 before a tile's end
    (as span() of the share tests), the TILES seam tile being tile 8 of 17 or tile 40 of 83."""

    def __init__(self, kind, log2, ntiles):
        sb_t, _ = seam_block(kind, ih.LAYOUT_TILES, log2)
        sb_l, blk_l = seam_block(kind, ih.LAYOUT_LANES, log2)
        self.kind, self.log2, self.ntiles = kind, log2, ntiles
        self.seam_tile = sb_t // TILE
        self.first = (self.seam_tile - {17: 8, 83: 40}[ntiles]) * TILE + 5
        self.n = ntiles * TILE - 5 - 7
        self.lo, self.hi = min(sb_t, sb_l), max(sb_t + TILE, sb_l + blk_l)  # both layouts' seam blocks
        # last record before a seam block, its first and last record, the first record after it
        self.spots = sorted({sb_t - 1, sb_t, sb_t + TILE - 1, sb_t + TILE, sb_l - 1, sb_l, sb_l + blk_l - 1, sb_l + blk_l})
        self.tie = (self.lo - 2, self.hi + 1)  # an equal pair on both sides of either layout's seam block
        self.outside = (self.first - 1, self.first + self.n)
        # the window the oracle sees: the range's tiles and one more at either end
        self.w0, self.wn = self.first - 5 - TILE, (ntiles + 2) * TILE
        self.lf = self.first - self.w0  # the range's first record within the window

    def others(self, count):
        """`count` more records around the seam, none of them a spot or of the tie: alternately
        before and after the seam blocks, two of them inside the TILES seam tile."""
        inside = [self.seam_tile * TILE + 7, self.seam_tile * TILE + 20]
        out = [self.hi + 2 + j // 2 if j % 2 == 0 else self.lo - 3 - j // 2 for j in range(count - 2)]
        return (out[:4] + inside + out[4:])[:count]


# ---------------------------------------------------------------- fixtures from the oracle


class TemplateSeam:
    """12 queries over the window of one span.  Query 0: near-copies at every spot, at distances
    out of index order, and the equal pair, which is closer than all of them; queries 1..11 one
    near-copy each around the seam; exact copies of query 0 (and of query 1, one record further
    out) just outside the range."""

    def __init__(self, log2, ntiles):
        s = self.span = Span(ih.KIND_TEMPLATES, log2, ntiles)
        rng = np.random.default_rng(100 * log2 + ntiles)
        self.queries = oc.gen_templates(Q_SEED, 0, NQ_T).copy()
        q0 = self.queries[0]
        self.writes = {}
        for j, rec in enumerate(s.spots):
            self.writes[rec] = _near_copy(q0, (9 * j) % 31 - 15, 100 + 60 * ((5 * j) % 7), rng)
        self.writes[s.tie[0]] = _near_copy(q0, -3, 50, rng)
        self.writes[s.tie[1]] = self.writes[s.tie[0]].copy()
        self.plant = dict(zip(range(1, NQ_T), s.others(NQ_T - 1)))  # query -> its record
        for q, rec in self.plant.items():
            self.writes[rec] = _near_copy(self.queries[q], (7 * q) % 31 - 15, 60 + 20 * q, rng)
        for rec in s.outside:
            self.writes[rec] = q0.copy()
        self.writes[s.outside[0] - 1] = self.queries[1].copy()
        self.writes[s.outside[1] + 1] = self.queries[1].copy()
        assert len(self.writes) == len(s.spots) + 2 + NQ_T - 1 + 4
        self.recs = oc.gen_templates(T_SEED, s.w0, s.wn).copy()
        for rec, r in self.writes.items():
            self.recs[rec - s.w0] = r
        self.exp = [Expected(q, self.recs) for q in self.queries]

    def original(self, rec):
        return oc.gen_templates(T_SEED, rec, 1)


class MasksSeam:
    """7 query masks over the masks of one span's range and three participants' rows [3, 7, n, 31]
    with a known list per query (planted_shares): query 0 at every spot and an equal pair (the
    database holds the same mask at both records), queries 1..6 one record each around the seam.
    Record hi + 12 is written as zero: no valid rotation, never listed."""

    def __init__(self, log2, ntiles):
        s = self.span = Span(ih.KIND_MASKS, log2, ntiles)
        rng = np.random.default_rng(200 * log2 + ntiles)
        self.qmasks = rng.integers(0, 2**64, (NQ_M, ih.LIMBS), dtype=np.uint64)
        masks = oc.gen_masks(M_SEED, s.first, s.n).copy()
        self.zero = s.hi + 12
        self.writes = {s.tie[1]: masks[s.tie[0] - s.first].copy(), self.zero: np.zeros(ih.LIMBS, np.uint64)}
        for rec, r in self.writes.items():
            masks[rec - s.first] = r
        self.den = np.stack([oc.masks_batch(q, masks) for q in self.qmasks])  # [7, n, 31], rows of the range
        d = self.den.astype(np.int64)
        uneq = background(rng, self.den, 0.4, 0.6)
        for j, rec in enumerate(s.spots):
            k = (11 * j) % ROT
            uneq[0, rec - s.first, k] = int(d[0, rec - s.first, k] * (0.02 + 0.01 * ((5 * j) % 7)))
        a, b = s.tie[0] - s.first, s.tie[1] - s.first
        uneq[0, a, 5] = int(d[0, a, 5] * 0.01)
        uneq[0, b] = uneq[0, a]  # equal masks, equal rows: equal fractions at every rotation
        self.plant = dict(zip(range(1, NQ_M), s.others(NQ_M - 1)))
        for q, rec in self.plant.items():
            uneq[q, rec - s.first, (7 * q) % ROT] = int(d[q, rec - s.first, (7 * q) % ROT] * 0.01 * q)
        self.shares = planted_shares(rng, self.den, uneq)  # [3, 7, n, 31]
        self.exp = [resolver_expected(self.shares[:, q], self.den[q]) for q in range(NQ_M)]  # by row of the range

    def original(self, rec):
        return oc.gen_masks(M_SEED, rec, 1)


class SharesSeam:
    """7 uniform u16 queries over the shares of one span's range; three records at the seam written
    with extreme values.  want: the oracle's [7, n, 31] rows."""

    def __init__(self, log2, ntiles):
        s = self.span = Span(ih.KIND_SHARES, log2, ntiles)
        rng = np.random.default_rng(300 * log2 + ntiles)
        self.queries = rng.integers(0, 1 << 16, (NQ_S, ih.BITS), dtype=np.uint16)
        shares = oc.gen_shares(S_SEED, s.first, s.n).copy()
        self.writes = {s.spots[0]: np.full(ih.BITS, 0xFFFF, np.uint16), s.spots[1]: np.full(ih.BITS, 0x8000, np.uint16),
                       s.spots[-1]: self.queries[0].copy()}
        for rec, r in self.writes.items():
            shares[rec - s.first] = r
        self.want = np.stack([oc.distance_batch(q, shares) for q in self.queries])

    def original(self, rec):
        return oc.gen_shares(S_SEED, rec, 1)


@functools.lru_cache(None)
def tcase(log2, ntiles):
    return TemplateSeam(log2, ntiles)


@functools.lru_cache(None)
def mcase(log2, ntiles):
    return MasksSeam(log2, ntiles)


@functools.lru_cache(None)
def scase(log2, ntiles):
    return SharesSeam(log2, ntiles)


# part B
B_NQ, B_FIRST, B_N = 64, 5, 1_090_027
B_SEAM_SLAB, B_SEAM_ROW = 63, 601_965  # element 2^31 of [64][n][31]
B_WINDOWS = [(0, 0), (0, B_N - 100), (31, B_N - 100), (32, 0), (63, 0), (63, B_SEAM_ROW - 50), (63, B_N - 100)]
B_PLANTS = {0: [3, 601_000, B_N - 2], 31: [0, 17, B_N - 1], 63: [601_964, 601_965, 601_966, B_N - 1]}
B_LIST = 0.1


@functools.lru_cache(None)
def b_qmasks():
    return np.random.default_rng(64).integers(0, 2**64, (B_NQ, ih.LIMBS), dtype=np.uint64)


class RowPlants:
    """The planted rows of one query of part B's one-part array: total = den_row - 2 u with small u,
    so the row decodes to u / den.  Every other row of the zeroed array decodes to (den >> 1) / den:
    the masks are uniform random bits, den is a sum of 12 800 bits that are set with probability 1/4
    (3200 +- 49), so den >= 3 and the distance is at least 1/3 for all of them."""

    def __init__(self, slab):
        self.rows = B_PLANTS[slab]
        q = b_qmasks()[slab]
        self.den = np.concatenate([oc.masks_batch(q, oc.gen_masks(M_SEED, B_FIRST + r, 1)) for r in self.rows])
        u = np.stack([3 + 4 * j + np.abs(np.arange(ROT) - (7 * j + slab) % ROT) for j in range(len(self.rows))])
        self.total = ((self.den.astype(np.int64) - 2 * u) & 0xFFFF).astype(np.uint16)  # [plants, 31]
        self.exp = resolver_expected(self.total[None], self.den)  # by plant

    def records(self, idx, base):
        """Match records of the plants idx (places in rows), index = base + row."""
        w = want_records(self.exp, np.asarray(idx, np.int64), 0, 0)
        w["index"] = np.asarray([self.rows[i] for i in idx], np.uint64) + np.uint64(base)
        return w


@functools.lru_cache(None)
def row_plants(slab):
    return RowPlants(slab)


# part C
C_NQ, C_DISTINCT, C_NDB, C_FIRST, C_N = 65535 + 9, 7, 70, 3, 60
C_SEED = 3401


class ManyQueries:
    """7 distinct queries over 70 templates; query d has d % 4 near-copies in the range [3, 63) --
    lists of 0..3 under T_LIST -- and queries 1 and 2 an exact copy outside it."""

    def __init__(self):
        rng = np.random.default_rng(65544)
        self.distinct = oc.gen_templates(C_SEED + 1, 0, C_DISTINCT).copy()
        self.templates = oc.gen_templates(C_SEED, 0, C_NDB).copy()
        self.plants = {d: [5 + 8 * d + 3 * j for j in range(d % 4)] for d in range(C_DISTINCT)}
        for d, recs in self.plants.items():
            for j, rec in enumerate(recs):
                self.templates[rec] = _near_copy(self.distinct[d], (5 * d + j) % 31 - 15, 300 - 100 * j + 10 * d, rng)
        self.templates[1], self.templates[65] = self.distinct[1], self.distinct[2]
        self.exp = [Expected(q, self.templates) for q in self.distinct]


@functools.lru_cache(None)
def ccase():
    return ManyQueries()


# ---------------------------------------------------------------- D. the fixtures' facts, on the CPU


def test_seam_fixture_facts():
    """CPU only, from the oracle alone."""
    assert lanes_block() == 64
    for kind, rb in REC_BYTES.items():
        for log2 in (31, 32, 36):
            seam = 1 << log2
            assert seam_block(kind, ih.LAYOUT_TILES, log2)[0] == SEAM_TILES[kind][log2] * TILE
            for ntiles in (17, 83):
                s = Span(kind, log2, ntiles)
                assert s.first % TILE == 5 and (s.first + s.n) % TILE == TILE - 7
                assert (s.first + s.n - 1) // TILE - s.first // TILE + 1 == ntiles
                assert s.seam_tile - s.first // TILE == {17: 8, 83: 40}[ntiles]
                assert s.first + s.n + TILE <= db_records(kind, log2)
                for layout in (ih.LAYOUT_TILES, ih.LAYOUT_LANES):
                    sb, blk = seam_block(kind, layout, log2)
                    assert sb * rb <= seam < (sb + blk) * rb and s.lo <= sb and sb + blk <= s.hi
                    # the range's first and last block lie on opposite sides of the seam
                    assert (s.first // blk + 1) * blk * rb <= seam < (s.first + s.n - 1) // blk * blk * rb
                    assert {sb - 1, sb, sb + blk - 1, sb + blk} <= set(s.spots)
                assert s.first < s.tie[0] < s.lo and s.hi < s.tie[1] < s.first + s.n
                assert s.outside[0] == s.first - 1 and s.outside[1] == s.first + s.n
    # no written record's byte offset equals another written record's modulo 2^31 or 2^32: a load at a
    # wrapped address reads something else, and the comparison fails
    for case_of, kind, groups in ((tcase, ih.KIND_TEMPLATES, (SPANS, SPANS36)), (mcase, ih.KIND_MASKS, (SPANS, SPANS36)),
                                  (None, ih.KIND_SHARES, (SPANS, SPANS36))):
        for group in groups:  # the spans that share one database
            written = set()
            for log2, ntiles in group:
                written |= set(case_of(log2, ntiles).writes) if case_of else set(Span(kind, log2, ntiles).spots)
            for modulus in (1 << 31, 1 << 32):
                assert len({r * REC_BYTES[kind] % modulus for r in written}) == len(written), (kind, modulus)
                for blk in (TILE, lanes_block()):  # nor do two of them share a place in blocks that wrap onto each other
                    size = blk * REC_BYTES[kind]
                    assert len({(r // blk * size % modulus, r % blk) for r in written}) == len(written), (kind, modulus, blk)
    # templates: the lists the GPU tests expect are the planted records
    for log2, ntiles in SPANS + SPANS36:
        c = tcase(log2, ntiles)
        s, e0 = c.span, c.exp[0]
        own = sorted(s.spots + list(s.tie))
        assert [int(i) + s.w0 for i in e0.hits(T_LIST, s.lf, s.n)] == own
        first = [int(i) + s.w0 for i in order(e0, s.lf, s.n)[:len(own)]]
        assert first[:2] == list(s.tie) and sorted(first) == own and first[2:] != sorted(first[2:])
        a, b = s.tie[0] - s.w0, s.tie[1] - s.w0
        assert (e0.num[a], e0.den[a], e0.rot[a]) == (e0.num[b], e0.den[b], e0.rot[b]) == (50, e0.den[a], -3)
        assert len({int(e0.num[r - s.w0]) for r in s.spots}) > 3 and len({int(e0.rot[r - s.w0]) for r in s.spots}) > 3
        assert min(s.spots) < s.seam_tile * TILE <= max(s.spots)
        for q, rec in c.plant.items():
            assert [int(i) + s.w0 for i in c.exp[q].hits(T_LIST, s.lf, s.n)] == [rec], q
            assert int(order(c.exp[q], s.lf, s.n)[0]) + s.w0 == rec
        assert any(r < s.lo for r in c.plant.values()) and any(r >= s.hi for r in c.plant.values())
        for q, recs in ((0, s.outside), (1, (s.outside[0] - 1, s.outside[1] + 1))):  # exact copies, outside
            for rec in recs:
                assert c.exp[q].num[rec - s.w0] == 0 and c.exp[q].rot[rec - s.w0] == 0
                assert not s.first <= rec < s.first + s.n and s.w0 <= rec < s.w0 + s.wn
        half = len(e0.hits(T_MIXED, s.lf, s.n))
        assert 0.25 * s.n < half < 0.75 * s.n
    # masks: rows of the range
    for log2, ntiles in SPANS + SPANS36:
        c = mcase(log2, ntiles)
        s, e0 = c.span, c.exp[0]
        own = sorted(r - s.first for r in s.spots + list(s.tie))
        assert list(e0.hits(T_LIST)) == own
        top = list(order(e0)[:len(own)])
        assert top[:2] == [s.tie[0] - s.first, s.tie[1] - s.first] and sorted(top) == own
        a, b = top[:2]
        assert (e0.num[a], e0.den[a], e0.rot[a]) == (e0.num[b], e0.den[b], e0.rot[b]) and e0.rot[a] == 5 - 15
        for q, rec in c.plant.items():
            assert list(c.exp[q].hits(T_LIST)) == [rec - s.first] and order(c.exp[q])[0] == rec - s.first
        for e in c.exp:
            assert e.den[c.zero - s.first] == 0 and len(e.hits(INF)) == s.n - 1


def test_row_array_and_many_query_fixture_facts():
    """CPU only: parts B and C."""
    assert B_NQ * B_N * ROT * 2 == 4_325_227_136 > 1 << 32
    assert divmod((1 << 31) // ROT, B_N) == (B_SEAM_SLAB, B_SEAM_ROW)
    assert (B_SEAM_SLAB, B_SEAM_ROW) in [(sl, r) for sl, rows in B_PLANTS.items() for r in rows]
    for slab, rows in B_PLANTS.items():
        p = row_plants(slab)
        e = p.exp
        assert rows == sorted(rows) and len(rows) >= 3 and (p.den > 3000).all()
        assert (e.dist < 0.02).all() and len(set(e.dist)) == len(rows)  # all below B_LIST, a strict order
        assert list(e.hits(B_LIST)) == list(range(len(rows))) and len(order(e)) == len(rows)
        # an untouched row of the zeroed array: (den >> 1) / den >= 1/3 from den = 3 on
        assert all((d >> 1) * 3 >= d for d in range(3, 200)) and 1 / 3 > B_LIST
    c = ccase()
    assert C_NQ > 65535 and 65535 % C_DISTINCT != 0
    for d, e in enumerate(c.exp):
        assert [int(i) for i in e.hits(T_LIST, C_FIRST, C_N)] == c.plants[d] and len(c.plants[d]) == d % 4
        assert len(order(e, C_FIRST, C_N)) == C_N
        if c.plants[d]:
            assert sorted(int(i) for i in order(e, C_FIRST, C_N)[:len(c.plants[d])]) == c.plants[d]
    assert c.exp[1].num[1] == 0 and c.exp[2].num[65] == 0  # the copies outside [3, 63)


# ---------------------------------------------------------------- helpers of the GPU tests


def need(dev, nbytes, what):
    free, _ = dev.memory()
    assert free > nbytes + (2 << 30), f"{what} needs {nbytes / 1e9:.1f} GB, only {free / 1e9:.1f} GB free"


@contextlib.contextmanager
def database(dev, kind, layout, n, seed):
    need(dev, n * REC_BYTES[kind], f"a database of {n} records")
    free = dev.memory()[0]
    with ih.Database(dev, kind, n, layout) as db:
        db.generate(n, seed)
        print(f"database of {n} records of {REC_BYTES[kind]} B: {(free - dev.memory()[0]) / 1e9:.2f} GB of device memory")
        yield db


@contextlib.contextmanager
def planted(db, case):
    """The case's records written over the generated ones, and the generated ones put back."""
    for rec, r in case.writes.items():
        db.write(rec, r[None, :])
    try:
        yield
    finally:
        for rec in case.writes:
            db.write(rec, case.original(rec))


def raw_list(call, room, counter):
    """call(out, count_ref) on a 0x5A-filled array of `room` records -> (count, its bytes)."""
    out = (ih.Match * room)()
    ctypes.memset(out, FILL, ctypes.sizeof(out))
    cnt = counter(99)
    assert call(out, ctypes.byref(cnt)) == 0, ih.load_library().iris_last_error()
    return cnt.value, bytes(out)


def check_list(count, raw, want, room, total=None):
    """A call's count and bytes against the records `want` (all of them, or the first `room`)."""
    assert count == (len(want) if total is None else total), (count, len(want))
    k = min(len(want), room)
    assert raw[:32 * k] == want[:k].tobytes()
    assert raw[32 * k:] == UNTOUCHED * (room - k), "entries past the list were written"


def match_bytes(m):
    return bytes(m)


def check_template_single(dev, db, c):
    """TemplateEngine.search / matches / topk of query 0 over the case's range."""
    s, e, lib = c.span, c.exp[0], ih.load_library()
    base = BASE + s.w0  # a record of the window: index_base + w0 + its place
    ranked = order(e, s.lf, s.n)
    with ih.TemplateEngine(dev, c.queries[0]) as eng:
        best = eng.search(db, s.first, s.n, index_base=BASE)
        assert match_bytes(best) == e.records(ranked[:1], base).tobytes()
        assert best.index == BASE + s.tie[0]
        for k in KS:
            count, raw = raw_list(lambda o, cnt: lib.iris_template_topk(eng.handle, db.handle, s.first, s.n, BASE, k, o, cnt),
                                  k + 2, ctypes.c_uint32)
            check_list(count, raw, e.records(ranked[:k], base), k + 2)
        for t in (T_LIST, T_MIXED, INF):
            idx = e.hits(t, s.lf, s.n)
            count, raw = raw_list(lambda o, cnt: lib.iris_template_matches(eng.handle, db.handle, s.first, s.n, BASE, t, o,
                                                                           len(idx) + 2, cnt), len(idx) + 2, ctypes.c_uint64)
            check_list(count, raw, e.records(idx, base), len(idx) + 2)
        got, _ = eng.matches(db, T_LIST, first=s.first, n=s.n)
        assert [m.index for m in got] == sorted(s.spots + list(s.tie))


def check_pair_search(dev, db, c):
    """TemplateBatchEngine.search with 2 and 3 queries: the two-query pass and a single one."""
    s = c.span
    for nq in (2, 3):
        with ih.TemplateBatchEngine(dev, c.queries[:nq]) as eng:
            got = eng.search(db, s.first, s.n, BASE)
        for q in range(nq):
            assert match_bytes(got[q]) == c.exp[q].records(order(c.exp[q], s.lf, s.n)[:1], BASE + s.w0).tobytes(), (nq, q)
        assert got[0].index == BASE + s.tie[0] and got[1].index == BASE + c.plant[1]


def check_template_batch(dev, db, c, ks=KS):
    """TemplateBatchEngine.matches / topk / search with 5 and 12 queries."""
    s = c.span
    base = BASE + s.w0
    for nq in (5, NQ_T):
        exps = c.exp[:nq]
        with ih.TemplateBatchEngine(dev, c.queries[:nq]) as eng:
            for t in (T_LIST, T_MIXED):
                cap = max(len(e.hits(t, s.lf, s.n)) for e in exps) + 1
                recs, counts = template_batch_matches_call(eng, db, t, s.first, s.n, BASE, cap)
                template_batch_matches_check(recs, counts, exps, t, s.lf, s.n, base, cap)
            for k in ks:
                recs, counts = template_batch_topk_call(eng, db, k, s.first, s.n, BASE)
                template_batch_topk_check(recs, counts, exps, k, s.lf, s.n, base)
                if k == 1:
                    best = eng.search(db, s.first, s.n, BASE)
                    assert b"".join(match_bytes(m) for m in best) == recs.tobytes()
                    assert [m.index - BASE for m in best] == [s.tie[0]] + [c.plant[q] for q in range(1, nq)]


def check_shared_passes(dev, db, c, carried_want):
    """Two asynchronous searches back to back: the first pass carries the second."""
    s = c.span
    qa, qb = c.queries[0], c.queries[1]
    dev.reset_stats()
    pa, pb = submit(dev, db, [qa, qb], s.first, s.n)
    ma, mb = pa.wait(), pb.wait()
    regs, _, carried = dev.kernel_stats("search_shared")
    print(f"2^{s.log2} ntiles={s.ntiles} registered={regs} carried={carried}")
    assert (regs, carried) == (1, carried_want)
    for m, q in ((ma, 0), (mb, 1)):
        assert fields(m) == fields(blocking(dev, db, c.queries[q], s.first, s.n))
        assert match_bytes(m) == c.exp[q].records(order(c.exp[q], s.lf, s.n)[:1], 3 + s.w0).tobytes()
    assert (ma.index, mb.index) == (3 + s.tie[0], 3 + c.plant[1])


def check_masks(dev, db, c, ks=KS):
    """MasksBatchEngine rows / resolve / matches / topk with 7 queries (a group of four, a pair and a
    single) and MasksEngine.resolve / matches / topk of query 0, over the case's range."""
    s, lib = c.span, ih.load_library()
    with ih.MasksBatchEngine(dev, c.qmasks) as eng, DeviceArrays(dev, c.shares) as ptrs:
        out = np.full((NQ_M, s.n, ROT), ROW_FILL, np.uint16)
        eng.batch_process(out, db, first=s.first, n=s.n)
        assert (out == c.den).all()
        before, rows, after = _guarded_device_rows(dev, eng, db, s.first, s.n, NQ_M)
        assert (rows == c.den).all() and (before == ROW_FILL).all() and (after == ROW_FILL).all()
        best = eng.resolve(db, ptrs, first=s.first, n=s.n, index_base=BASE)
        for t in (T_LIST, 0.45):
            cap = max(len(e.hits(t)) for e in c.exp) + 1
            recs, counts, _ = masks_batch_matches_call(eng, db, ptrs, t, s.first, s.n, BASE, cap)
            masks_batch_matches_check(recs, counts, c.exp, t, 0, s.n, BASE, cap)
        for k in ks:
            counts, raw, tail = masks_batch_topk_call(eng, db, ptrs, k, s.first, s.n, BASE)
            masks_batch_topk_check(counts, raw, tail, c.exp, k, 0, s.n, BASE)
            if k == 1:
                assert b"".join(match_bytes(m) for m in best) == raw
        assert [m.index - BASE for m in best] == [s.tie[0] - s.first] + [c.plant[q] - s.first for q in range(1, NQ_M)]
        # the fused single-query select, on slab 0 of every part
        e = c.exp[0]
        arr = (ctypes.c_void_p * 3)(*slab_ptrs(ptrs, 0, s.n))
        with ih.MasksEngine(dev, c.qmasks[0]) as one:
            assert match_bytes(one.resolve(db, slab_ptrs(ptrs, 0, s.n), first=s.first, n=s.n, index_base=BASE)) == \
                match_bytes(best[0])
            for k in ks:
                count, raw = raw_list(lambda o, cnt: lib.iris_resolver_topk_masks(one.handle, db.handle, s.first, s.n, arr, 3,
                                                                                  BASE, k, o, cnt), k + 2, ctypes.c_uint32)
                check_list(count, raw, want_records(e, order(e)[:k], 0, BASE), k + 2)
            for t in (T_LIST, 0.45, INF):
                idx = e.hits(t)
                count, raw = raw_list(lambda o, cnt: lib.iris_resolver_matches_masks(one.handle, db.handle, s.first, s.n, arr,
                                                                                     3, BASE, t, o, len(idx) + 2, cnt),
                                      len(idx) + 2, ctypes.c_uint64)
                check_list(count, raw, want_records(e, idx, 0, BASE), len(idx) + 2)


def check_shares(dev, db, c):
    """DistanceBatchEngine.batch_process and batch_process_device with 4, 6 and 7 queries."""
    s = c.span
    for nq in (4, 6, NQ_S):
        with ih.DistanceBatchEngine(dev, c.queries[:nq]) as eng:
            out = np.full((nq, s.n, ROT), ROW_FILL, np.uint16)
            eng.batch_process(out, db, first=s.first, n=s.n)
            assert (out == c.want[:nq]).all(), (s.log2, s.ntiles, nq)
            before, rows, after = _guarded_device_rows(dev, eng, db, s.first, s.n, nq)
            assert (rows == c.want[:nq]).all(), (s.log2, s.ntiles, nq)
            assert (before == ROW_FILL).all() and (after == ROW_FILL).all()


def single_variant(variant, device, hooked_device):
    """(device, layout) of a variant of test_gpu_matches.VARIANTS / test_gpu_masks_batch.VARIANTS."""
    if variant.endswith("1"):
        return hooked_device(IRIS_TILES_PER_WAVE=1), ih.LAYOUT_TILES
    if variant.endswith("4"):
        return hooked_device(IRIS_TILES_PER_WAVE=4), ih.LAYOUT_TILES
    return device, ih.LAYOUT_LANES if variant == "lanes" else ih.LAYOUT_TILES


# ---------------------------------------------------------------- A. database offsets

# the spans that share one database: "4g" holds the 2^31 and the 2^32 seam (4.3 GB), "64g" the 2^36 seam (68.8 GB)
SEAMS = {"4g": (32, SPANS), "64g": (36, SPANS36)}
seams = pytest.mark.parametrize("seams", list(SEAMS))


@gpu
@seams
@pytest.mark.parametrize("variant", ["tiles", "tiles-tpw1", "tiles-tpw4", "lanes"])
def test_template_select_across_seams(device, hooked_device, variant, seams):
    dev, layout = single_variant(variant, device, hooked_device)
    log2max, spans = SEAMS[seams]
    with database(dev, ih.KIND_TEMPLATES, layout, db_records(ih.KIND_TEMPLATES, log2max), T_SEED) as db:
        for log2, ntiles in spans:
            c = tcase(log2, ntiles)
            with planted(db, c):
                check_template_single(dev, db, c)
                if variant in ("tiles", "lanes"):  # the pair pass knows no hook; LANES runs the two one by one
                    check_pair_search(dev, db, c)


@gpu
@seams
@pytest.mark.parametrize("variant", ["tiles", "tiles-k2"])
def test_template_batch_across_seams(device, hooked_device, variant, seams):
    dev, layout = open_variant(variant, device, hooked_device)
    log2max, spans = SEAMS[seams]
    with database(dev, ih.KIND_TEMPLATES, layout, db_records(ih.KIND_TEMPLATES, log2max), T_SEED) as db:
        for log2, ntiles in spans:
            c = tcase(log2, ntiles)
            with planted(db, c):
                check_template_batch(dev, db, c)
                check_pair_search(dev, db, c)


@gpu
@seams
@pytest.mark.parametrize("even", [0, 1], ids=["forced", "forced-even"])
def test_shared_passes_across_seams(hooked_device, even, seams):
    dev = hooked_device(**FORCED, IRIS_SEARCH_SHARE_EVEN=even)
    log2max, spans = SEAMS[seams]
    with database(dev, ih.KIND_TEMPLATES, ih.LAYOUT_TILES, db_records(ih.KIND_TEMPLATES, log2max), T_SEED) as db:
        for log2, ntiles in spans:
            c = tcase(log2, ntiles)
            with planted(db, c):
                # the even hook: the hosting pass carries its guest in the even tile groups only
                check_shared_passes(dev, db, c, (grid_of(ntiles) + 1) // 2 if even else grid_of(ntiles))


@gpu
@seams
@pytest.mark.parametrize("variant", ["tiles", "tiles-batch1", "tiles-batch4", "lanes"])
def test_masks_across_seams(device, hooked_device, variant, seams):
    dev, layout = single_variant(variant, device, hooked_device)
    log2max, spans = SEAMS[seams]
    with database(dev, ih.KIND_MASKS, layout, db_records(ih.KIND_MASKS, log2max), M_SEED) as db:
        for log2, ntiles in spans:
            c = mcase(log2, ntiles)
            with planted(db, c):
                check_masks(dev, db, c)


@gpu
@seams
@pytest.mark.parametrize("variant", ["tiles-mfma", "tiles-batch", "lanes-valu"])
def test_distance_batch_across_seams(device, hooked_device, variant, seams):
    dev = hooked_device(IRIS_TILES_PER_WAVE=1) if variant == "tiles-batch" else device
    layout = ih.LAYOUT_LANES if variant == "lanes-valu" else ih.LAYOUT_TILES
    log2max, spans = SEAMS[seams]
    with database(dev, ih.KIND_SHARES, layout, db_records(ih.KIND_SHARES, log2max), S_SEED) as db:
        for log2, ntiles in spans:
            c = scase(log2, ntiles)
            with planted(db, c):
                check_shares(dev, db, c)


# ---------------------------------------------------------------- B. row arrays past 2^32 bytes

B_BYTES = B_NQ * B_N * ROT * 2
B_GUARD = 4096  # bytes, filled before the call, before and after the array


def check_row_windows(dev, eng, db, oracle_rows):
    """eng.batch_process_device of [B_FIRST, B_FIRST + B_N) into one guarded device array; 100-row
    windows against oracle_rows(slab, first record, count)."""
    need(dev, B_BYTES, "the [64][n][31] output")
    guard = np.full(B_GUARD, FILL, np.uint8)
    ptr = dev.alloc(B_BYTES + 2 * B_GUARD)
    try:
        assert ptr % 16 == 0
        dev.h2d(ptr, guard)
        dev.h2d(ptr + B_GUARD + B_BYTES, guard)
        eng.batch_process_device(db, ptr + B_GUARD, first=B_FIRST, n=B_N)
        for slab, row in B_WINDOWS:
            got = np.empty((100, ROT), np.uint16)
            dev.d2h(got, ptr + B_GUARD + (slab * B_N + row) * ROT * 2)
            assert (got == oracle_rows(slab, B_FIRST + row, 100)).all(), (slab, row)
        for at in (ptr, ptr + B_GUARD + B_BYTES):
            got = np.empty(B_GUARD, np.uint8)
            dev.d2h(got, at)
            assert (got == FILL).all(), "the guard region was written"
    finally:
        dev.free(ptr)


@gpu
def test_masks_batch_rows_past_4g(device):
    q = b_qmasks()
    with database(device, ih.KIND_MASKS, ih.LAYOUT_TILES, B_FIRST + B_N, M_SEED) as db, ih.MasksBatchEngine(device, q) as eng:
        check_row_windows(device, eng, db, lambda slab, rec, cnt: oc.masks_batch(q[slab], oc.gen_masks(M_SEED, rec, cnt)))


@gpu
def test_distance_batch_rows_past_4g(device):
    q = np.random.default_rng(65).integers(0, 1 << 16, (B_NQ, ih.BITS), dtype=np.uint16)
    with database(device, ih.KIND_SHARES, ih.LAYOUT_TILES, B_FIRST + B_N, S_SEED) as db, \
            ih.DistanceBatchEngine(device, q) as eng:
        check_row_windows(device, eng, db, lambda slab, rec, cnt: oc.distance_batch(q[slab], oc.gen_shares(S_SEED, rec, cnt)))


@gpu
def test_participant_rows_past_4g(device):
    """resolve, matches and topk read one part of [64][n][31] u16: zero but for the planted rows."""
    dev, lib = device, ih.load_library()
    need(dev, B_BYTES, "the participant's [64][n][31] rows")
    with database(dev, ih.KIND_MASKS, ih.LAYOUT_TILES, B_FIRST + B_N, M_SEED) as db, \
            ih.MasksBatchEngine(dev, b_qmasks()) as eng:
        part = dev.alloc(B_BYTES)
        try:
            zeros = np.zeros(64 << 20, np.uint8)
            for off in range(0, B_BYTES, zeros.nbytes):
                dev.h2d(part + off, zeros[:min(zeros.nbytes, B_BYTES - off)])
            for slab in B_PLANTS:
                p = row_plants(slab)
                for j, row in enumerate(p.rows):
                    dev.h2d(part + (slab * B_N + row) * ROT * 2, p.total[j])
            best = eng.resolve(db, [part], first=B_FIRST, n=B_N, index_base=BASE)
            arr = (ctypes.c_void_p * 1)(part)
            cap, k = 8, 3
            out = (ih.Match * (B_NQ * cap))()
            ctypes.memset(out, FILL, ctypes.sizeof(out))
            counts = (ctypes.c_uint64 * B_NQ)()
            assert lib.iris_resolver_batch_matches_masks(eng.handle, db.handle, B_FIRST, B_N, arr, 1, BASE, B_LIST, out, cap,
                                                         counts) == 0, lib.iris_last_error()
            lists = bytes(out)
            top = (ih.Match * (B_NQ * k))()
            ctypes.memset(top, FILL, ctypes.sizeof(top))
            tcounts = (ctypes.c_uint32 * B_NQ)()
            assert lib.iris_resolver_batch_topk_masks(eng.handle, db.handle, B_FIRST, B_N, arr, 1, BASE, k, top,
                                                      tcounts) == 0, lib.iris_last_error()
            tops = bytes(top)
            for slab in B_PLANTS:
                p = row_plants(slab)
                ranked = [int(i) for i in order(p.exp)]
                assert match_bytes(best[slab]) == p.records(ranked[:1], BASE).tobytes(), slab
                m = len(p.rows)
                check_list(counts[slab], lists[slab * cap * 32:(slab + 1) * cap * 32], p.records(range(m), BASE), cap)
                check_list(tcounts[slab], tops[slab * k * 32:(slab + 1) * k * 32], p.records(ranked[:k], BASE), k)
        finally:
            dev.free(part)


# ---------------------------------------------------------------- C. more than 65535 queries


@gpu
def test_65544_queries_cross_the_merge_launch_seam(device):
    c, lib = ccase(), ih.load_library()
    src = np.arange(C_NQ) % C_DISTINCT
    queries = c.distinct[src]
    need(device, C_NQ * 16 * 200 * 32, "the query tiles")
    singles = [ih.TemplateEngine(device, q) for q in c.distinct]
    last = range(65533, C_NQ)
    try:
        with ih.Database(device, ih.KIND_TEMPLATES, C_NDB, ih.LAYOUT_TILES) as db, \
                ih.TemplateBatchEngine(device, queries) as eng:
            db.append(c.templates)
            del queries

            def same_as_source(recs, counts):
                rows = np.ascontiguousarray(recs).view(np.uint8).reshape(C_NQ, -1)
                cnt = np.asarray(counts)
                for d in range(C_DISTINCT):
                    assert (rows[d::C_DISTINCT] == rows[d]).all() and (cnt[d::C_DISTINCT] == cnt[d]).all(), d

            for k in (1, 3):
                recs, counts = template_batch_topk_call(eng, db, k, C_FIRST, C_N, BASE)
                same_as_source(recs, counts)
                template_batch_topk_check(recs[:C_DISTINCT], counts[:C_DISTINCT], c.exp, k, C_FIRST, C_N, BASE)
                one = [b"".join(match_bytes(m) for m in s.topk(db, k, first=C_FIRST, n=C_N, index_base=BASE)) for s in singles]
                for q in list(range(C_DISTINCT)) + list(last):
                    assert counts[q] == k and recs[q].tobytes() == one[src[q]], (k, q)
                    assert recs[q].tobytes() == c.exp[src[q]].records(order(c.exp[src[q]], C_FIRST, C_N)[:k], BASE).tobytes()
                if k == 1:
                    best = (ih.Match * C_NQ)()
                    assert lib.iris_template_batch_search(eng.handle, db.handle, C_FIRST, C_N, BASE, best) == 0
                    assert bytes(best) == recs.tobytes()
            cap = 4
            recs, counts = template_batch_matches_call(eng, db, T_LIST, C_FIRST, C_N, BASE, cap)
            same_as_source(recs, counts)
            template_batch_matches_check(recs[:C_DISTINCT], counts[:C_DISTINCT], c.exp, T_LIST, C_FIRST, C_N, BASE, cap)
            assert sorted(set(counts)) == [0, 1, 2, 3]
            for q in list(range(C_DISTINCT)) + list(last):
                got, cnt = singles[src[q]].matches(db, T_LIST, first=C_FIRST, n=C_N, index_base=BASE)
                assert cnt == counts[q] == len(c.plants[src[q]])
                assert b"".join(match_bytes(m) for m in got) == recs[q, :cnt].tobytes(), q
                assert [m.index - BASE for m in got] == c.plants[src[q]]
    finally:
        for s in singles:
            s.close()
