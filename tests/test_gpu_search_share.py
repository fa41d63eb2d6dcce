"""Shared search passes (iris_template_search_async): a pass that is still
streaming the database also computes the search submitted after it, workgroup by workgroup.
Whatever is shared, every result equals the blocking search of the same query bit for bit (all
Match fields, the distance as its f64 bit pattern) and, once per test, the CPU oracle.

The forced tests pin the 4-tiles-per-wave, separate-reduce form on small ranges and hold every
pass back behind a 2-ms spin (IRIS_SEARCH_SHARE_DELAY_US), so the next search's registration
lands before the pass starts and every workgroup carries the guest: the `search_shared`
counter (tile groups carried for guests) then equals the grid size."""
import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc

gpu = pytest.mark.gpu
TILE = 32
FORCED = dict(IRIS_TILES_PER_WAVE=4, IRIS_FUSED_REDUCE=0, IRIS_SEARCH_SHARE_DELAY_US=2000)
NDB = 83 * TILE + 3 * TILE  # the largest range plus a tile before and two after it
NONE = 2**64 - 1


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


@pytest.fixture(scope="module")
def recs():
    return oc.gen_templates(9191, 0, NDB)


@pytest.fixture(scope="module")
def queries():
    return oc.gen_templates(9192, 0, 4)


@gpu
@pytest.mark.parametrize("ntiles", [1, 17, 16 * 5 + 3])
def test_forced_full_sharing(hooked_device, recs, queries, ntiles):
    """Two different queries back to back: the first pass carries the second in every workgroup.
    The guest's winner lies in the first tile group, the last one, and the last (clamped,
    partial) tile in turn; the host's winner stays where it is."""
    dev = hooked_device(**FORCED)
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    last_tile = first // TILE + ntiles - 1
    sites = sorted({first + 1, min(first + cnt - 1, last_tile * TILE - 9) if ntiles > 1 else first + 2,
                    first + cnt - 1})
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        data = recs.copy()
        data[first + min(cnt - 1, 11)] = near(qa)
        for k, site in enumerate(sites):
            cur = data.copy()
            cur[site] = near(qb, limb=5)
            cur[first - 1] = qb  # exact copies just outside the range, before and after, are never found
            cur[first + cnt] = qb
            db.truncate(0)
            db.append(cur)
            dev.reset_stats()
            pa, pb = submit(dev, db, [qa, qb], first, cnt)
            ma, mb = pa.wait(), pb.wait()
            regs, _, carried = dev.kernel_stats("search_shared")
            print(f"ntiles={ntiles} site={site} registered={regs} carried={carried} grid={grid_of(ntiles)}")
            assert (regs, carried) == (1, grid_of(ntiles))
            assert mb.index == site + 3 and ma.index == first + min(cnt - 1, 11) + 3
            assert fields(ma) == fields(blocking(dev, db, qa, first, cnt))
            assert fields(mb) == fields(blocking(dev, db, qb, first, cnt))
            if k == 0:
                check_oracle(mb, qb, cur, first, cnt)


@gpu
def test_forced_sharing_no_match(hooked_device, recs, queries):
    """Every record has a zero joint mask with both queries: both report no match."""
    dev = hooked_device(**FORCED)
    first, cnt = span(17)
    qa, qb = queries[0].copy(), queries[1].copy()
    qa[200:] = 0
    qb[200:] = 0
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(recs)
        dev.reset_stats()
        pa, pb = submit(dev, db, [qa, qb], first, cnt)
        ma, mb = pa.wait(), pb.wait()
        assert dev.kernel_stats("search_shared")[2] == grid_of(17)
        for m, q in ((ma, qa), (mb, qb)):
            assert (m.distance, m.index, m.num, m.den) == (np.inf, NONE, 0, 0)
            assert fields(m) == fields(blocking(dev, db, q, first, cnt))


@gpu
@pytest.mark.parametrize("share", [1, 0], ids=["shared", "not-shared"])
def test_tie_rule(hooked_device, recs, queries, share):
    """Two equal-distance records in different workgroups: the lower index wins, for the
    hosting query and for the guest, shared or not."""
    dev = hooked_device(**FORCED, IRIS_SEARCH_SHARE=share)
    ntiles = 16 * 5 + 3
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    data = recs.copy()
    lo_a, hi_a = first + 16 * TILE + 4, first + 70 * TILE + 1  # workgroups 1 and 4
    lo_b, hi_b = first + 3, first + 81 * TILE  # workgroups 0 and 5
    data[lo_a] = data[hi_a] = near(qa)
    data[lo_b] = data[hi_b] = near(qb, limb=5)
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pa, pb = submit(dev, db, [qa, qb], first, cnt)
        ma, mb = pa.wait(), pb.wait()
        assert dev.kernel_stats("search_shared")[2] == (grid_of(ntiles) if share else 0)
        assert (ma.index, mb.index) == (lo_a + 3, lo_b + 3)
        assert fields(ma) == fields(blocking(dev, db, qa, first, cnt))
        assert fields(mb) == fields(blocking(dev, db, qb, first, cnt))
        check_oracle(ma, qa, data, first, cnt)


@gpu
@pytest.mark.parametrize("count", [3, 4])
def test_submissions_without_a_wait(hooked_device, recs, queries, count):
    """Three and four searches submitted before any wait, every engine destroyed before the
    first wait: each pass hosts at most one guest (the search after it), and every result
    equals the blocking search."""
    dev = hooked_device(**FORCED)
    ntiles = 16 * 5 + 3
    first, cnt = span(ntiles)
    data = recs.copy()
    for i in range(count):
        data[first + 7 + 600 * i] = near(queries[i], limb=2 + i)
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pend = submit(dev, db, list(queries[:count]), first, cnt)
        got = [p.wait() for p in pend]
        regs, _, carried = dev.kernel_stats("search_shared")
        print(f"count={count} registered={regs} carried={carried}")
        # every search but the first registers with the pass before it; a pass whose own tile groups
        # were all computed by its host exits at once and carries nothing: passes 1 and 3 carry
        assert (regs, carried) == (count - 1, count // 2 * grid_of(ntiles))
        for i, m in enumerate(got):
            assert m.index == first + 7 + 600 * i + 3
            assert fields(m) == fields(blocking(dev, db, queries[i], first, cnt))
        check_oracle(got[-1], queries[count - 1], data, first, cnt)


@gpu
@pytest.mark.parametrize("case", ["write", "other-first", "other-n", "lanes", "off"])
def test_no_sharing(hooked_device, recs, queries, case):
    """What must not share: a database written between the two submissions (search 2 sees the
    new record), another `first` or `n`, a LANES database, IRIS_SEARCH_SHARE=0."""
    env = dict(FORCED, IRIS_SEARCH_SHARE=0) if case == "off" else FORCED
    dev = hooked_device(**env)
    ntiles = 16 * 5 + 3
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    layout = ih.LAYOUT_LANES if case == "lanes" else ih.LAYOUT_TILES
    first2, cnt2 = (first + 1, cnt - 1) if case == "other-first" else (first, cnt - 1) if case == "other-n" else (first, cnt)
    data = recs.copy()
    data[first + 40] = near(qa)
    data[first + 900] = near(qb, limb=5, flips=0xFFFF00FFFFFF00FF)  # those 32 bits and 16 more
    site = first + 2000
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB, layout) as db:
        db.append(data)
        dev.reset_stats()
        with ih.TemplateEngine(dev, qa) as e:
            pa = e.search_async(db, first, cnt, index_base=3)
        if case == "write":  # becomes query 2's winner
            data[site] = near(qb, limb=5)
            db.write(site, data[site][None, :])
        with ih.TemplateEngine(dev, qb) as e:
            pb = e.search_async(db, first2, cnt2, index_base=3)
        ma, mb = pa.wait(), pb.wait()
        regs, _, carried = dev.kernel_stats("search_shared")
        assert (regs, carried) == (0, 0)
        assert ma.index == first + 40 + 3
        assert mb.index == (site if case == "write" else first + 900) + 3
        assert fields(ma) == fields(blocking(dev, db, qa, first, cnt))
        assert fields(mb) == fields(blocking(dev, db, qb, first2, cnt2))
        check_oracle(mb, qb, data, first2, cnt2)


@gpu
def test_unforced_pipeline_at_natural_size(device):
    """No hook: 2.2M templates (4297 workgroups, just above the fused limit of 4096), 12
    pipelined steps with 12 different queries, as bench.py runs them.  Whether a pass carries
    the next search depends on timing, so the counter is only printed."""
    n, steps = 2_200_000, 12
    rng = np.random.default_rng(5)
    with ih.Database(device, ih.KIND_TEMPLATES, n) as db:
        db.generate(n, 77)
        sites = [int(x) for x in rng.choice(n, steps, replace=False)]
        qs = [near(db.read(s, 1)[0], limb=1 + k) for k, s in enumerate(sites)]
        device.reset_stats()
        got, pend = [], None
        for q in qs:
            with ih.TemplateEngine(device, q) as e:
                p = e.search_async(db)
            if pend is not None:
                got.append(pend.wait())
            pend = p
        got.append(pend.wait())
        regs, _, carried = device.kernel_stats("search_shared")
        print(f"unforced: {steps} steps, registered={regs}, tile groups carried={carried} (grid 4297)")
        for q, s, m in zip(qs, sites, got):
            assert m.index == s
            assert fields(m) == fields(blocking(device, db, q, 0, n, base=0))


def test_share_hooks_are_test_only(monkeypatch):
    """CPU: the two hooks take effect, and show in iris_config, only with IRIS_TEST_HOOKS=1."""
    for k in ("IRIS_TEST_HOOKS", "IRIS_SEARCH_SHARE", "IRIS_SEARCH_SHARE_DELAY_US"):
        monkeypatch.delenv(k, raising=False)
    c = ih.config()
    assert "search_share" not in c and "search_share_delay_us" not in c and "ignored" not in c
    monkeypatch.setenv("IRIS_SEARCH_SHARE", "0")
    monkeypatch.setenv("IRIS_SEARCH_SHARE_DELAY_US", "2000")
    c = ih.config()
    assert "search_share" not in c and "search_share_delay_us" not in c
    assert c["ignored"] == ["IRIS_SEARCH_SHARE", "IRIS_SEARCH_SHARE_DELAY_US"]
    monkeypatch.setenv("IRIS_TEST_HOOKS", "1")
    c = ih.config()
    assert "ignored" not in c and (c["search_share"], c["search_share_delay_us"]) == ("0", "2000")
    monkeypatch.delenv("IRIS_SEARCH_SHARE")
    monkeypatch.delenv("IRIS_SEARCH_SHARE_DELAY_US")
    assert (ih.config()["search_share"], ih.config()["search_share_delay_us"]) == ("1", "0")
