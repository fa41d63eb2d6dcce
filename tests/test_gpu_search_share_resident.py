"""Shared search passes whose tile groups are decided differently inside one pass (DESIGN.md
§4.1).  IRIS_SEARCH_SHARE_EVEN=1 makes a pass that is nobody's guest blind to its guest in odd
tile groups, so with three queries A, B, C submitted back to back over 6 tile groups (83 tiles,
the last one clamped and partial) every kind of group occurs: A's launch carries B in groups
0, 2, 4 and computes 1, 3, 5 alone; B's launch skips 0, 2, 4 and carries C in 1, 3, 5; C's
launch computes 0, 2, 4 alone and skips the rest.  A query's partials then come from two
launches, and its done words and the partials another launch wrote for it are published by the
end of that kernel alone (plain stores, relaxed loads; the resident grid these tests were first
written for measured slower and was left out).  Shapes, hooks and helpers are
those of tests/test_gpu_search_share.py: every result equals the blocking search of the same
query field for field (the distance as its f64 bits) and, once per test, the CPU oracle."""
import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc

gpu = pytest.mark.gpu
TILE = 32
GROUP = 16 * TILE  # records of a tile group
FORCED = dict(IRIS_TILES_PER_WAVE=4, IRIS_FUSED_REDUCE=0, IRIS_SEARCH_SHARE_DELAY_US=2000)
NTILES = 16 * 5 + 3  # 6 tile groups, the last one of 3 tiles
NDB = NTILES * TILE + 3 * TILE
NONE = 2**64 - 1


def fields(m):
    return (int(np.float64(m.distance).view(np.uint64)), m.index, m.num, m.den, m.rotation)


def near(q, limb=3, flips=0x00FF00FF00FF00FF):
    r = q.copy()
    r[limb] ^= np.uint64(flips)
    return r


def span(ntiles):
    """(first, count): `ntiles` tiles touched, from 5 records into a tile to 7 before a tile's end."""
    return TILE + 5, ntiles * TILE - 5 - 7


def in_group(g, off):
    """Record `off` of tile group g of a range that starts in tile 1."""
    return TILE + g * GROUP + off


def blocking(dev, db, q, first, cnt, base=3):
    with ih.TemplateEngine(dev, q) as e:
        return e.search(db, first, cnt, index_base=base)


def submit(dev, db, queries, first, cnt, base=3):
    pend = []
    for q in queries:
        with ih.TemplateEngine(dev, q) as e:
            pend.append(e.search_async(db, first, cnt, index_base=base))
    return pend


def check_oracle(m, q, recs, first, cnt, base=3):
    want_d, want_i = oc.argmin(oc.template_distances(q, recs[first:first + cnt]))
    assert fields(m)[0] == int(np.float64(want_d).view(np.uint64)) and m.index == want_i + first + base


@pytest.fixture(scope="module")
def recs():
    return oc.gen_templates(9191, 0, NDB)


@pytest.fixture(scope="module")
def queries():
    return oc.gen_templates(9192, 0, 4)


def test_even_hook_is_test_only(monkeypatch):
    """CPU: the hook takes effect, and shows in iris_config, only with IRIS_TEST_HOOKS=1."""
    for k in ("IRIS_TEST_HOOKS", "IRIS_SEARCH_SHARE_EVEN"):
        monkeypatch.delenv(k, raising=False)
    c = ih.config()
    assert "search_share_even" not in c and "ignored" not in c
    monkeypatch.setenv("IRIS_SEARCH_SHARE_EVEN", "1")
    c = ih.config()
    assert "search_share_even" not in c and c["ignored"] == ["IRIS_SEARCH_SHARE_EVEN"]
    monkeypatch.setenv("IRIS_TEST_HOOKS", "1")
    c = ih.config()
    assert "ignored" not in c and c["search_share_even"] == "1"
    monkeypatch.delenv("IRIS_SEARCH_SHARE_EVEN")
    assert ih.config()["search_share_even"] == "0"


@gpu
@pytest.mark.parametrize("run", ["computed-elsewhere", "computed-by-own-launch", "last-tile"])
def test_every_kind_of_group_in_one_pass(hooked_device, recs, queries, run):
    """A, B, C back to back: 3 groups carried by A's launch, 3 by B's (counter 6, 2
    registrations).  B's and C's winners lie in a group that another launch computed for them
    (B: group 4, by A's; C: group 3, by B's), then in one their own launch computed (B: 5, the
    clamped group; C: 4), then B's in the last, partial tile; A's groups are all its own
    launch's: a carrying group, then a solo one."""
    dev = hooked_device(**FORCED, IRIS_SEARCH_SHARE_EVEN=1)
    assert dev.config()["search_share_even"] == "1"
    first, cnt = span(NTILES)
    qa, qb, qc = queries[0], queries[1], queries[2]
    ga, gb, gc = (2, 4, 3) if run == "computed-elsewhere" else (3, 5, 4)
    sa, sc = in_group(ga, 33), in_group(gc, 15 * TILE + 31)
    sb = first + cnt - 1 if run == "last-tile" else in_group(gb, 2 * TILE + 1)
    data = recs.copy()
    data[sa], data[sb], data[sc] = near(qa), near(qb, limb=5), near(qc, limb=7)
    data[first - 1] = data[first + cnt] = qb  # exact copies just outside the range are never found
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pend = submit(dev, db, [qa, qb, qc], first, cnt)
        got = [p.wait() for p in pend]
        regs, _, carried = dev.kernel_stats("search_shared")
        print(f"run={run} registered={regs} carried={carried}")
        assert (regs, carried) == (2, 6)
        assert [m.index for m in got] == [sa + 3, sb + 3, sc + 3]
        for m, q in zip(got, (qa, qb, qc)):
            assert fields(m) == fields(blocking(dev, db, q, first, cnt))
        check_oracle(got[1], qb, data, first, cnt)
        check_oracle(got[2], qc, data, first, cnt)
        # A and B alone: A carries B in 0, 2, 4 only, B computes 1, 3, 5 with nobody to carry
        dev.reset_stats()
        pa, pb = submit(dev, db, [qa, qb], first, cnt)
        ma, mb = pa.wait(), pb.wait()
        assert dev.kernel_stats("search_shared")[::2] == (1, 3)
        assert (fields(ma), fields(mb)) == (fields(got[0]), fields(got[1]))


@gpu
@pytest.mark.parametrize("lower", ["carried", "own"])
def test_tie_rule_across_launches(hooked_device, recs, queries, lower):
    """Two equal-distance records of the guest, one in a group the hosting launch computed and
    one in a group its own launch computed, either one first: the lower index wins.  The
    host's two lie in a carrying group and a solo one."""
    dev = hooked_device(**FORCED, IRIS_SEARCH_SHARE_EVEN=1)
    first, cnt = span(NTILES)
    qa, qb = queries[0], queries[1]
    data = recs.copy()
    lo_a, hi_a = in_group(2, 4), in_group(3, 1)
    lo_b, hi_b = (in_group(2, 9 * TILE), in_group(5, 5)) if lower == "carried" else (in_group(1, 7), in_group(4, 300))
    data[lo_a] = data[hi_a] = near(qa)
    data[lo_b] = data[hi_b] = near(qb, limb=5)
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pa, pb = submit(dev, db, [qa, qb], first, cnt)
        ma, mb = pa.wait(), pb.wait()
        assert dev.kernel_stats("search_shared")[::2] == (1, 3)
        assert (ma.index, mb.index) == (lo_a + 3, lo_b + 3)
        assert fields(ma) == fields(blocking(dev, db, qa, first, cnt))
        assert fields(mb) == fields(blocking(dev, db, qb, first, cnt))
        check_oracle(mb, qb, data, first, cnt)


@gpu
def test_no_match_from_two_launches(hooked_device, recs, queries):
    """Zero masks for both queries: both report no match, the guest from three partials of the
    hosting launch and three of its own."""
    dev = hooked_device(**FORCED, IRIS_SEARCH_SHARE_EVEN=1)
    first, cnt = span(NTILES)
    qa, qb = queries[0].copy(), queries[1].copy()
    qa[200:] = 0
    qb[200:] = 0
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(recs)
        dev.reset_stats()
        pa, pb = submit(dev, db, [qa, qb], first, cnt)
        ma, mb = pa.wait(), pb.wait()
        assert dev.kernel_stats("search_shared")[::2] == (1, 3)
        for m, q in ((ma, qa), (mb, qb)):
            assert (m.distance, m.index, m.num, m.den) == (np.inf, NONE, 0, 0)
            assert fields(m) == fields(blocking(dev, db, q, first, cnt))
        assert oc.argmin(oc.template_distances(qb, recs[first:first + cnt])) == (np.inf, NONE)


@gpu
def test_write_after_a_mixed_pass(hooked_device, recs, queries):
    """A record written between two submissions keeps the second search from being carried,
    and it sees the record; the pair before it was shared group by group."""
    dev = hooked_device(**FORCED, IRIS_SEARCH_SHARE_EVEN=1)
    first, cnt = span(NTILES)
    qa, qb = queries[0], queries[1]
    data = recs.copy()
    data[in_group(2, 40)] = near(qa)
    data[in_group(1, 388)] = near(qb, limb=5, flips=0xFFFF00FFFFFF00FF)  # those 32 bits and 16 more
    site = in_group(4, 100)  # a group the hosting launch would have carried
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pa, pb = submit(dev, db, [qa, qb], first, cnt)
        assert (pa.wait().index, pb.wait().index) == (in_group(2, 40) + 3, in_group(1, 388) + 3)
        assert dev.kernel_stats("search_shared")[::2] == (1, 3)
        dev.reset_stats()
        with ih.TemplateEngine(dev, qa) as e:
            pa = e.search_async(db, first, cnt, index_base=3)
        data[site] = near(qb, limb=5)
        db.write(site, data[site][None, :])
        with ih.TemplateEngine(dev, qb) as e:
            pb = e.search_async(db, first, cnt, index_base=3)
        ma, mb = pa.wait(), pb.wait()
        assert dev.kernel_stats("search_shared")[::2] == (0, 0)
        assert (ma.index, mb.index) == (in_group(2, 40) + 3, site + 3)
        assert fields(ma) == fields(blocking(dev, db, qa, first, cnt))
        assert fields(mb) == fields(blocking(dev, db, qb, first, cnt))
        check_oracle(mb, qb, data, first, cnt)
