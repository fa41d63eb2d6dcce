"""Masks records on the boundary of the read-ahead's packed row form (store_tile_packed,
csrc/iris_device.hpp), for the CPU test of their facts (test_packed_boundary.py) and the GPU walk
(test_gpu_resident.py).  A row of 31 counts is packed when max - (min >> 6 << 6) <= 255 and is
stored in full (the escape rows) otherwise.

The query mask QUERY is every row of columns [15, 55); rotation k of the oracle's rows sees columns
[k, k + 40) of a record.  A record with S bits in columns 30..39 and e_j bits (0..64) in column
39 + j, j = 1..30, nothing elsewhere, therefore counts S + e_1 + ... + e_k at rotation k: the
minimum S at k = 0 and the maximum S + sum(e) at k = 30, which the 32x32 MFMA C layout holds in
different halves of the wave (rows 0..3 in lanes 0..31, rows 28..30 in lanes 32..63).  Its mirror
image (column c -> 69 - c) counts the same values in the opposite order, the maximum at k = 0."""
import numpy as np

ROWS, COLS = 64, 200
MARKER = 0xFF  # byte 31 of an escaped record


def from_bits(bits):
    """[64 rows, 200 columns] of 0/1 -> the 200 u64 limbs of a mask."""
    return np.packbits(np.asarray(bits, np.uint8).reshape(ROWS * COLS), bitorder="little").view(np.uint64).copy()


def block_query(c0=15, c1=55):
    bits = np.zeros((ROWS, COLS), np.uint8)
    bits[:, c0:c1] = 1
    return from_bits(bits)


QUERY = block_query()
ONES = from_bits(np.ones((ROWS, COLS), np.uint8))
EMPTY = from_bits(np.zeros((ROWS, COLS), np.uint8))


def steps(total, rng):
    """e_1..e_30, each 0..64, e_1 >= 1 and e_30 >= 1 (so the extremes are at k = 0 and k = 30 alone),
    summing to `total`."""
    e = np.zeros(30, np.int64)
    e[0] = e[29] = 1
    for _ in range(total - 2):
        j = int(rng.integers(30))
        while e[j] == ROWS:
            j = (j + 1) % 30
        e[j] += 1
    assert e.sum() == total and e.max() <= ROWS
    return e


def ramp(s, e, mirror=False):
    """The record of the module docstring: s bits over columns 30..39, e[j - 1] bits in column 39 + j."""
    assert 0 <= s <= 10 * ROWS
    bits = np.zeros((ROWS, COLS), np.uint8)
    cells = bits[:, 30:40].T.reshape(-1)  # column after column; a copy
    cells[:s] = 1
    bits[:, 30:40] = cells.reshape(10, ROWS).T
    for j, ej in enumerate(e, start=1):
        bits[:int(ej), 39 + j] = 1
    if mirror:
        bits[:, :70] = bits[:, 69::-1].copy()
    return from_bits(bits)


# (name, S, sum e, min, max, max - (min >> 6 << 6), packed?)  -- the issue's table
TABLE = [("s127-e192", 127, 192, 127, 319, 255, True),
         ("s127-e193", 127, 193, 127, 320, 256, False),
         ("s128-e255", 128, 255, 128, 383, 255, True),
         ("s128-e256", 128, 256, 128, 384, 256, False)]


def boundary_records(seed=17):
    """[(name, record, mirror?, table row)]: the four boundary records and their mirror images."""
    rng = np.random.default_rng(seed)
    out = []
    for row in TABLE:
        e = steps(row[2], rng)
        out.append((row[0], ramp(row[1], e), False, row))
        out.append((row[0] + "-mirror", ramp(row[1], e, mirror=True), True, row))
    return out


def specials():
    """The ten planted records: the boundary records, their mirrors, the all-ones and the empty mask."""
    return [rec for _, rec, _, _ in boundary_records()] + [ONES, EMPTY]


CHUNK = 96  # three tiles: a chunk's first and last tile differ and a random one lies between them
TAIL = 29   # the file's last, partial tile


def planted_file(seed=23):
    """(records, {record index: special index}): uniformly random masks with special c at records 0,
    13 and 31 (the first, a middle and the 32nd) of the first and of the last tile of chunk c, and
    every special once in the last, partial tile (its first and its last record among them)."""
    sp = specials()
    n = len(sp) * CHUNK + TAIL
    rng = np.random.default_rng(seed)
    recs = rng.integers(0, 2**64 - 1, (n, COLS), dtype=np.uint64, endpoint=True)
    where = {}
    for c in range(len(sp)):
        for tile0 in (c * CHUNK, (c + 1) * CHUNK - 32):
            for at in (0, 13, 31):
                where[tile0 + at] = c
    tail = list(range(0, 27, 3)) + [TAIL - 1]
    assert len(tail) == len(sp)
    for c, at in enumerate(tail):
        where[len(sp) * CHUNK + at] = c
    for i, c in where.items():
        recs[i] = sp[c]
    return recs, where


def span(rows):
    """max - (min >> 6 << 6) of each row of 31 counts: at most 255 in the packed form."""
    rows = np.asarray(rows, np.int64)
    return rows.max(axis=-1) - (rows.min(axis=-1) >> 6 << 6)
