"""Fixtures whose records reach their minimum at more than one rotation, or at equal fractions in
different terms, for the CPU test of their facts and the GPU walk of every ranking kernel
(test_gpu_order.py).  The rule under test: the exact fraction num/den, then the lowest record index,
and inside one record the lowest rotation k.

The 32x32 MFMA C tile holds rotation k of a record in half (k >> 2) & 1 of the wave (half 0: k in
0-3, 8-11, 16-19, 24-27; half 1: k in 4-7, 12-15, 20-23, 28-30), and the halves meet in one exchange
(best_rotation, csrc/iris_device.hpp) or at the end of the walk (partial_better_rot).  A tie whose
lowest k lies in half 1 and whose next k lies in half 0 is the case in which the consumed half-0
lane has to take its partner's candidate; the opposite order is the case in which it must not.

A. periodic_query(p): every row of pattern and mask is a p-bit block tiled 200 / p times, so a
   rotation by p columns is the identity and every record's (num, den) at k and k + p are equal.
B. crafted_query / crafted_record: the query mask is three whole columns 60 and more apart (H, F1,
   F2); a record opens column H + r to meet H at rotation r (num 32 of den 64: the query pattern is
   set on rows 0..31 of H) and columns F1 + s, F2 + s to meet F1 and F2 at rotation s (64 of 128:
   the query pattern is all of F1 and none of F2).  Columns 60 apart never meet at another of the
   31 rotations, so such a record has exactly the rotations it opens: 1/2 in different terms.
C. resolver_ties: resolver rows whose chosen rotations decode to den / 4 of their denominators
   (1/4 in different terms), every other rotation at 3/8 and more.
D. wide_rows: resolver rows over the whole u16 range of denominators, with neighbouring fractions
   whose cross products differ by one at the top of the range.

The tests take every expectation from the CPU oracle's counts through test_gpu_matches.Expected;
nothing here calls the library or the oracle."""
import numpy as np

from packed_boundary import COLS, ROWS, from_bits

ROT = 31
N = 1100  # test_gpu_topk.BIG_N: three workgroups of the four-tiles-per-wave form
SEED = 8  # the generated templates and masks of the other select-kernel tests


def half(k):
    """The half of the wave that holds rotation k of a 32x32 C tile."""
    return (int(k) >> 2) & 1


def lowest(e):
    """Expected.rot as k = 0..30."""
    return np.asarray(e.rot) + 15


# ---------------------------------------------------------------- A. periodic queries

PERIODS = (5, 4, 8)


def periodic_query(p, seed=1):
    assert COLS % p == 0
    rng = np.random.default_rng(seed)
    pattern = np.tile(rng.integers(0, 2, (ROWS, p), dtype=np.uint8), (1, COLS // p))
    mask = np.tile(rng.integers(0, 2, (ROWS, p), dtype=np.uint8), (1, COLS // p))
    return np.concatenate([from_bits(pattern), from_bits(mask)])


def winner(e, first, n):
    """The record the search of [first, first + n) returns: the exact fraction, then the index (int64)."""
    idx = np.arange(first, first + n)
    idx = idx[e.den[idx] != 0]
    best = idx[0]
    for i in idx[1:]:
        if e.num[i] * e.den[best] < e.num[best] * e.den[i]:
            best = i
    return int(best)


def ranges_by_lowest_k(e, want, count, length=257, limit=N):
    """`count` ranges (first, length) whose winner's lowest tied k satisfies want(k), found by the oracle."""
    out = []
    for first in range(0, limit - length, 23):
        if want(int(lowest(e)[winner(e, first, length)])):
            out.append((first, length))
            if len(out) == count:
                return out
    raise AssertionError("no such range")


# ---------------------------------------------------------------- B. equal fractions in different terms

H, F1, F2 = 20, 80, 140


def crafted_query():
    pattern, mask = np.zeros((ROWS, COLS), np.uint8), np.zeros((ROWS, COLS), np.uint8)
    mask[:, [H, F1, F2]] = 1
    pattern[:32, H] = 1
    pattern[:, F1] = 1
    return np.concatenate([from_bits(pattern), from_bits(mask)])


def crafted_record(r_half=None, r_full=None, agree=0, differ=0):
    """Rotation r_half at (32 - agree + differ) / 64 and rotation r_full at 64 / 128 (rotations as
    -15..15; None: not opened), no other valid rotation."""
    pattern, mask = np.zeros((ROWS, COLS), np.uint8), np.zeros((ROWS, COLS), np.uint8)
    if r_half is not None:
        mask[:, H + r_half] = 1
        pattern[:agree, H + r_half] = 1  # rows on which the query pattern is set: one disagreement fewer each
        pattern[32:32 + differ, H + r_half] = 1
    if r_full is not None:
        mask[:, [F1 + r_full, F2 + r_full]] = 1
    return np.concatenate([from_bits(pattern), from_bits(mask)])


# record -> (r_half, r_full): both fractions inside one record.  k = r + 15.
INSIDE = {40: (-8, 2),     # k = 7 (half 1) 32/64, k = 17 (half 0) 64/128: the smaller terms first
          41: (2, -8),     # k = 7 64/128, k = 17 32/64: the larger terms first
          42: (-13, -9),   # k = 2 (half 0) 32/64, k = 6 (half 1) 64/128
          43: (-9, -13),   # k = 2 64/128, k = 6 32/64
          44: (-15, -14),  # k = 0, 1: inside half 0
          45: (-14, -15),
          46: (15, -3),    # k = 12, 30: inside half 1, the larger terms first
          47: (13, 4)}     # k = 19 (half 0) 64/128, k = 28 (half 1) 32/64
# record -> (r_half, r_full) with one of them None: the two fractions across records, in both index
# orders (X = 32/64 alone, Y = 64/128 alone)
ACROSS = {70: (5, None), 75: (None, -12),      # one tile: X then Y
          76: (None, 9), 79: (-2, None),       # one tile: Y then X
          130: (0, None), 170: (None, -15),    # tiles 4 and 5 of one four-tile wave
          200: (None, 15), 250: (-7, None),    # tiles 6 and 7 of that wave
          300: (11, None), 450: (None, -4),    # waves 2 and 3 of one workgroup
          270: (None, 7), 400: (-10, None),
          520: (None, 6), 1040: (-11, None),   # workgroups 1 and 2
          600: (3, None), 1080: (None, 1)}
BETTER = 1090  # 31/64: strictly better than every tie, late in the range
TIED = sorted(list(INSIDE) + list(ACROSS))


def crafted_db(better=True):
    """[N, 400]: the planted records above; of the rest every third has a zero mask and the others one
    rotation at 33/64 .. 37/64, strictly worse than 1/2."""
    recs = np.zeros((N, 400), np.uint64)
    worse = {(r, d): crafted_record(r_half=r, differ=d) for r in range(-15, 16) for d in range(1, 6)}
    for i in range(N):
        if i % 3:
            recs[i] = worse[(7 * i) % ROT - 15, 1 + i % 5]
    for i, (rh, rf) in {**INSIDE, **ACROSS}.items():
        recs[i] = crafted_record(rh, rf)
    if better:
        recs[BETTER] = crafted_record(r_half=-5, agree=1)
    return recs


# ---------------------------------------------------------------- C. resolver ties

QUARTER = 0.25


def shares_of(total, parts, rng):
    """`parts` uniform additive u16 shares of total [..., 31] (mod 2^16)."""
    shares = rng.integers(0, 2**16, (parts,) + total.shape, dtype=np.uint16)
    rest = shares[:-1].astype(np.int64).sum(axis=0)
    shares[-1] = ((total - rest) % 2**16).astype(np.uint16)
    return shares


def _tie_pair(den_row, kind):
    """Rotations (a < b) of a row with den % 4 == 0, den != 0 and different denominators, in the
    halves `kind` asks for: "h1-first" (a in half 1, b in half 0), "h0-first", "same"."""
    ks = [k for k in range(ROT) if den_row[k] and den_row[k] % 4 == 0]
    for a in ks:
        for b in ks:
            if a < b and den_row[a] != den_row[b]:
                ha, hb = half(a), half(b)
                if (kind == "h1-first" and (ha, hb) == (1, 0)) or (kind == "h0-first" and (ha, hb) == (0, 1)) or \
                        (kind == "same" and ha == hb):
                    return a, b
    return None


def resolver_ties(den, rng, spots):
    """den [n, 31] -> (uneq [n, 31], {row: (kind, a, b)}, better row): from each of `spots` on a row of
    every kind whose rotations a and b decode to den / 4, and after the last of them a row that decodes
    to den / 4 - 1 at one rotation (strictly better); every other rotation of every row at 3/8 .. 1/2
    of its denominator."""
    d = den.astype(np.int64)
    uneq = d // 2 - ((d // 8) * rng.random(d.shape)).astype(np.int64)
    planted, row = {}, 0
    for spot in spots:
        row = max(row, spot)
        for kind in ("h1-first", "h0-first", "same"):
            while _tie_pair(d[row], kind) is None:
                row += 1
            a, b = _tie_pair(d[row], kind)
            uneq[row, a], uneq[row, b] = d[row, a] // 4, d[row, b] // 4
            planted[row] = (kind, a, b)
            row += 1
    while _tie_pair(d[row], "same") is None:
        row += 1
    a, _ = _tie_pair(d[row], "same")
    uneq[row, a] = d[row, a] // 4 - 1
    return uneq, planted, row


def encoded(den, uneq, odd=None):
    """The encoded dot the shares sum to: den - 2 uneq (- 1 where `odd`), mod 2^16."""
    t = den.astype(np.int64) - 2 * uneq
    return (t - (0 if odd is None else odd)) % 2**16


def ones_case():
    """All-ones masks (den = 12800 at every rotation), 257 rows: subsets of rotations tie at 3200
    with identical terms; rows without a subset are strictly worse."""
    n = 257
    subsets = {3: (5, 9, 13, 22, 30),   # the lowest k in half 1, the next in half 0
               40: (6, 8),
               41: (2, 7),              # half 0 first
               100: (13, 14, 29),       # inside half 1
               200: (29, 30),
               256: (4, 16, 17)}
    den = np.full((n, ROT), 12800, np.uint16)
    uneq = 4000 + (np.arange(n * ROT).reshape(n, ROT) * 37) % 2000
    for row, ks in subsets.items():
        uneq[row, list(ks)] = 3200
    return den, uneq, subsets


# ---------------------------------------------------------------- D. the whole u16 range

FORCED_DEN = (0, 1, 2, 32767, 32768, 65534, 65535)
# (row, k, uneq, den): neighbours whose cross products differ by one -- n / (2n + 1) against
# (n - 1) / (2n - 1): n (2n - 1) - (n - 1)(2n + 1) = 1 -- the neighbours at the top of the range, and equal
# fractions in different terms
PLANTED_WIDE = [(250, 9, 32767, 65535), (30, 4, 32766, 65533), (140, 17, 32765, 65531),
                (31, 30, 32766, 65535), (260, 0, 16383, 32768),
                (200, 6, 16383, 32766), (60, 11, 32767, 65534), (61, 5, 1, 2),
                (120, 7, 16383, 32767), (10, 21, 32767, 65535)]


def wide_rows(n=300, seed=44):
    """(den [n, 31] u16, uneq [n, 31], odd [n, 31] of 0/1): denominators from all of u16 (every value of
    FORCED_DEN among them), uneq from den / 2 + 1 up to 32767 -- above den for small denominators, and
    32767 / den just under 1/2 for the largest -- and the planted fractions of PLANTED_WIDE; row 5 has no
    valid rotation and row 6 only fractions above 1."""
    rng = np.random.default_rng(seed)
    den = rng.integers(0, 2**16, (n, ROT)).astype(np.int64)
    for j, v in enumerate(FORCED_DEN):
        den[20 + 3 * j, (5 * j) % ROT] = v
        den[21 + 3 * j, :] = np.where(rng.random(ROT) < 0.5, v, den[21 + 3 * j])
    den[5, :] = 0
    den[6, :] = rng.integers(1, 6, ROT)
    lo = np.minimum(den // 2 + 1, 32767)
    uneq = lo + (rng.random(den.shape) * (32768 - lo)).astype(np.int64)
    for row, k, u, d in PLANTED_WIDE:
        den[row, k], uneq[row, k] = d, u
    assert uneq.min() >= 0 and uneq.max() == 32767
    odd = rng.integers(0, 2, den.shape)
    return den.astype(np.uint16), uneq, odd
