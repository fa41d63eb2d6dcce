"""CPU: the facts of the packed-rows boundary fixture (packed_boundary.py), from the oracle alone.
The GPU walk of these records (test_gpu_resident.py::test_packed_rows_boundary) only means what it
says if every record really has the intended minimum, maximum and span under the block query."""
import numpy as np
import pytest

import packed_boundary as pb
from oracle import oracle_c as oc


@pytest.mark.parametrize("name,rec,mirror,row", pb.boundary_records(), ids=[b[0] for b in pb.boundary_records()])
def test_boundary_record_facts(name, rec, mirror, row):
    _, s, total, lo, hi, want_span, packed = row
    rows = oc.masks_batch(pb.QUERY, rec[None])[0].astype(int)
    assert rows.min() == lo == s and rows.max() == hi == s + total
    # the extremes are at the two ends of the row, each there alone: different halves of the C layout
    k_min, k_max = (30, 0) if mirror else (0, 30)
    assert list(np.flatnonzero(rows == lo)) == [k_min] and list(np.flatnonzero(rows == hi)) == [k_max]
    assert (np.diff(rows) <= 0).all() if mirror else (np.diff(rows) >= 0).all()
    assert pb.span(rows) == want_span == hi - (lo >> 6 << 6)
    assert (want_span <= 255) == packed
    assert lo % 64 == (63 if s == 127 else 0)
    if packed:  # the largest offset byte there is
        assert hi - (lo >> 6 << 6) == 255


def test_table_covers_both_sides_of_the_boundary():
    assert sorted({r[5] for r in pb.TABLE}) == [255, 256]
    assert sorted({r[3] % 64 for r in pb.TABLE}) == [0, 63]


def test_constant_rows():
    """All-ones under the all-ones query: every count 12 800, base byte B = 200, the largest there
    is, one below nothing but the escape marker's range; under the block query 40 columns x 64 rows.
    The empty mask: the all-zero row."""
    assert (oc.masks_batch(pb.ONES, pb.ONES[None]) == 12800).all() and 12800 >> 6 == 200 < pb.MARKER
    assert (oc.masks_batch(pb.QUERY, pb.ONES[None]) == 2560).all()
    assert (oc.masks_batch(pb.QUERY, pb.EMPTY[None]) == 0).all()
    assert (oc.masks_batch(pb.ONES, pb.EMPTY[None]) == 0).all()


def test_planted_file_placement():
    recs, where = pb.planted_file()
    sp = pb.specials()
    n = recs.shape[0]
    assert n % 32 == pb.TAIL and n // pb.CHUNK == len(sp)
    for c in range(len(sp)):
        at = sorted(i for i, s in where.items() if s == c)
        first_tile, last_tile = c * pb.CHUNK, (c + 1) * pb.CHUNK - 32
        assert at[:6] == [first_tile, first_tile + 13, first_tile + 31, last_tile, last_tile + 13, last_tile + 31]
        assert len(at) == 7 and at[6] >= n - pb.TAIL
        assert all((recs[i] == sp[c]).all() for i in at)
    assert where[n - pb.TAIL] == 0 and where[n - 1] == len(sp) - 1
    # both forms occur under the block query, and random masks never escape
    spans = pb.span(oc.masks_batch(pb.QUERY, recs))
    special = np.zeros(n, bool)
    special[list(where)] = True
    assert (spans[~special] <= 255).all()
    assert (spans[special] == 256).sum() == 4 * 7 and (spans[special] == 255).sum() == 4 * 7
