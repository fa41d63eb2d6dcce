"""The two-query round of a shared search pass stages both queries' operands in LDS once per
workgroup, with a barrier in every step of its streaming loop: every wave of a
two-query workgroup walks the whole loop and does its fetch duty whatever the range holds for
it.  These tests run the tile counts at which some wave of such a workgroup has no tile, or no
tile in its second round, plus ties, no-match, and a pass with solo and two-query workgroups side
by side.

Shapes, hooks and helpers are those of tests/test_gpu_search_share.py: the 4-tiles-per-wave,
separate-reduce form pinned on small ranges, every pass held back behind a 2-ms spin so that each
workgroup carries the guest (`search_shared` items == grid size).  Every result equals the
blocking search of the same query bit for bit (all Match fields, the distance as its f64 bit
pattern) and, once per tile count, the CPU oracle."""
import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc

gpu = pytest.mark.gpu
TILE = 32
FORCED = dict(IRIS_TILES_PER_WAVE=4, IRIS_FUSED_REDUCE=0, IRIS_SEARCH_SHARE_DELAY_US=2000)
MAXTILES = 35
NDB = MAXTILES * TILE + 3 * TILE  # the largest range plus a tile before and two after it
NONE = 2**64 - 1
# waves 1-3 without a tile (1, 2: and no second round at all; 3: one tile in wave 0's second
# round), waves 2-3 idle (4, 5, 7), the last wave partial or idle (13, 15), a full workgroup plus
# one with a single active wave (16..19), everything together (35)
NTILES = [1, 2, 3, 4, 5, 7, 13, 15, 16, 17, 18, 19, 35]


def grid_of(ntiles):
    """Workgroups of a range: 4 tiles per wave, 4 waves per workgroup."""
    return -(-(-(-ntiles // 4)) // 4)


def fields(m):
    return (int(np.float64(m.distance).view(np.uint64)), m.index, m.num, m.den, m.rotation)


def near(q, limb=3, flips=0x00FF00FF00FF00FF):
    """A record close to q: 32 pattern bits flipped."""
    r = q.copy()
    r[limb] ^= np.uint64(flips)
    return r


def span(ntiles):
    """(first, count) of a range that touches `ntiles` tiles, starting 5 records into a tile and
    ending 7 records before a tile's end (one tile: records 5..24 of it)."""
    first = TILE + 5
    return first, ntiles * TILE - 5 - 7


def in_tile(t, k):
    """Record k of the range's tile t (the range starts in tile 0 at record 5)."""
    return (1 + t) * TILE + k


def blocking(dev, db, q, first, cnt, base=3):
    with ih.TemplateEngine(dev, q) as e:
        return e.search(db, first, cnt, index_base=base)


def submit(dev, db, queries, first, cnt, base=3):
    """The queries' asynchronous searches back to back, every engine destroyed at once."""
    pend = []
    for q in queries:
        with ih.TemplateEngine(dev, q) as e:
            pend.append(e.search_async(db, first, cnt, index_base=base))
    return pend


def check_oracle(m, q, recs, first, cnt, base=3):
    want_d, want_i = oc.argmin(oc.template_distances(q, recs[first:first + cnt]))
    assert fields(m)[0] == int(np.float64(want_d).view(np.uint64)) and m.index == want_i + first + base


def shared_pair(dev, db, qa, qb, first, cnt, carried_want):
    """qa and qb back to back; the first pass carries qb in `carried_want` tile groups."""
    dev.reset_stats()
    pa, pb = submit(dev, db, [qa, qb], first, cnt)
    ma, mb = pa.wait(), pb.wait()
    regs, _, carried = dev.kernel_stats("search_shared")
    assert (regs, carried) == (1, carried_want)
    assert fields(ma) == fields(blocking(dev, db, qa, first, cnt))
    assert fields(mb) == fields(blocking(dev, db, qb, first, cnt))
    return ma, mb


@pytest.fixture(scope="module")
def recs():
    return oc.gen_templates(9191, 0, NDB)


@pytest.fixture(scope="module")
def queries():
    return oc.gen_templates(9192, 0, 4)


def planted(recs, queries, ntiles, site):
    """The range's records with the host's near match 11 records in and the guest's at `site`."""
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    cur = recs.copy()
    cur[first + min(cnt - 1, 11)] = near(qa)
    cur[site] = near(qb, limb=5)
    cur[first - 1] = qb  # exact copies just outside the range, before and after, are never found
    cur[first + cnt] = qb
    return cur


@gpu
@pytest.mark.parametrize("ntiles", NTILES)
def test_idle_waves_walk_the_staged_round(hooked_device, recs, queries, ntiles):
    """Two different queries back to back, the guest's near match in the first tile and then in
    the last (partial) one; the host's winner stays where it is."""
    dev = hooked_device(**FORCED)
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        for k, site in enumerate((first + 1, first + cnt - 1)):
            cur = planted(recs, queries, ntiles, site)
            db.truncate(0)
            db.append(cur)
            ma, mb = shared_pair(dev, db, qa, qb, first, cnt, grid_of(ntiles))
            assert mb.index == site + 3 and ma.index == first + min(cnt - 1, 11) + 3
            if k == 0:
                check_oracle(ma, qa, cur, first, cnt)
                check_oracle(mb, qb, cur, first, cnt)


@gpu
def test_tie_across_waves_and_rounds(hooked_device, recs, queries):
    """19 tiles.  The host's two equal records lie in tile 1 (wave 0, first round) and tile 14
    (wave 3, second round), the guest's in tile 6 (wave 1, second round) and tile 17 (the second
    workgroup's wave 0, first round): the lower index wins for both."""
    dev = hooked_device(**FORCED)
    first, cnt = span(19)
    qa, qb = queries[0], queries[1]
    data = recs.copy()
    lo_a, hi_a = in_tile(1, 30), in_tile(14, 2)
    lo_b, hi_b = in_tile(6, 17), in_tile(17, 0)
    data[lo_a] = data[hi_a] = near(qa)
    data[lo_b] = data[hi_b] = near(qb, limb=5)
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        ma, mb = shared_pair(dev, db, qa, qb, first, cnt, grid_of(19))
        assert (ma.index, mb.index) == (lo_a + 3, lo_b + 3)
        check_oracle(ma, qa, data, first, cnt)
        check_oracle(mb, qb, data, first, cnt)


@gpu
def test_no_match_for_both(hooked_device, recs, queries):
    """19 tiles, both queries with an all-zero mask: both report no match, as the blocking search."""
    dev = hooked_device(**FORCED)
    first, cnt = span(19)
    qa, qb = queries[0].copy(), queries[1].copy()
    qa[200:] = 0
    qb[200:] = 0
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(recs)
        ma, mb = shared_pair(dev, db, qa, qb, first, cnt, grid_of(19))
        for m in (ma, mb):
            assert (m.distance, m.index, m.num, m.den) == (np.inf, NONE, 0, 0)
        assert oc.argmin(oc.template_distances(qb, recs[first:first + cnt])) == (np.inf, NONE)


@gpu
def test_solo_and_two_query_workgroups_in_one_pass(hooked_device, recs, queries):
    """35 tiles, IRIS_SEARCH_SHARE_EVEN=1: tile groups 0 and 2 carry the guest, group 1 runs the
    registers-only single-query path with the ring allocated beside it; the guest's own launch
    computes group 1.  The guest's near match lies in the first tile (carried), then in group 1,
    then in the last, partial tile (carried, wave 0 of a workgroup whose other waves are idle)."""
    dev = hooked_device(**FORCED, IRIS_SEARCH_SHARE_EVEN=1)
    first, cnt = span(MAXTILES)
    qa, qb = queries[0], queries[1]
    even_groups = (grid_of(MAXTILES) + 1) // 2
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        for k, site in enumerate((first + 1, in_tile(21, 9), first + cnt - 1)):
            cur = planted(recs, queries, MAXTILES, site)
            db.truncate(0)
            db.append(cur)
            ma, mb = shared_pair(dev, db, qa, qb, first, cnt, even_groups)
            assert mb.index == site + 3 and ma.index == first + 11 + 3
            if k == 0:
                check_oracle(ma, qa, cur, first, cnt)
                check_oracle(mb, qb, cur, first, cnt)
