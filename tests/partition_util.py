"""Case builders and the geometry of the bucket-partition CSR (the default route of coo.tocsr() on the
device: g2n_pipeline.hip csr_partition / csr_partition_w, g2n_sym.hip passes 4 / 2 / 7 into
k_sym_finish<T, true> and k_sym_place, passes 5 / 6 into k_sumw_finish and k_sumw_place): COOs aimed at the
constants that route branches on, scipy as the reference (rowsum_util.scipy_sum).

plan() restates the host's geometry, bucket_load() what each finish block is handed (a twin is one
stored element exactly when part_twins pairs it), expect_buckets() the documented premise under which the
partition keeps a call (the comment above csr_partition_w, weight_enc, WSum::exact).  A Case here is a
rowsum_util.Case; tests/test_partition_cases.py shows on the CPU that every case sits where it claims.

Left out on purpose: hb >= 17 needs 2^25 or more rows and hb = 21 (the decline by id width) 2^28 + 1 rows,
whose indptr alone costs seconds; C4 and C5 of tests/test_gpu_fullsize.py keep hb = 18.  float64's exact
bound (run magnitudes below 2^53) cannot be reached by a bucket of at most 4096 entries of |v| < 2^31
(4096 * 2^31 = 2^43): no case pretends to."""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass

import numpy as np

import rowsum_util as U
from rowsum_util import DTYPES, FLOATS, Case, make  # noqa: F401  (re-exported for the tests)

# g2n_sym.hip / g2n_pipeline.hip
FIN_TPB = 256          # kFinTPB: rows (threads) of a finish block, 2^low <= it
SYM_CAP = 4096         # kSymCap: stored elements, and expanded entries, one finish block holds
MAX_DIGIT_BITS = 10    # kMaxDigitBits
WIDE_DIGIT_BITS = 11   # kWideDigitBits (the unweighted pass 2 past 2^20 buckets)
PART_TILE = 65536      # kPartTile; a quarter of it below 2^24 elements (kPtileSmallDiv = 4)
SUB_TILE = 8192        # kSubEl<4> = kSubEl<5>: element slots of one sub-tile of passes 4 / 5
IN_REG, MID_ROW = 16, 64  # kShortRow = kR, kMidRow = kF1wMid
GAPS = (701, 301, 132, 57, 23, 10, 4, 1)  # the Shell sorts' gaps
F32_EXACT = 1 << 24    # WSum<float>::exact: run magnitudes below it
F64_EXACT = 1 << 53    # WSum<double>::exact


# ------------------------------------------------------------------ geometry ------
def bits_for(n: int) -> int:
    """Bits to hold 0 .. n - 1, at least 1 (g2n_pipeline.hip bits_for)."""
    b = 1
    while b < 63 and (1 << b) < n:
        b += 1
    return b


@dataclass(frozen=True)
class Plan:
    bits: int
    low: int       # a bucket holds 2^low rows
    hb: int        # bucket id bits
    bits1: int     # pass 1's digit
    bits2: int     # pass 2's digit (0: a single pass)
    tile: int      # elements per partition block
    n_bk: int      # buckets holding rows (finish blocks)
    fits: bool     # the ids are narrow enough for two passes


def plan(n_rows: int, n_entries: int, weighted: bool = False) -> Plan:
    """csr_partition (sum = true, one stream) / csr_partition_w for an n_rows-row COO of n_entries."""
    bits = bits_for(n_rows)
    per_row = n_entries / (n_rows if n_rows else 1)
    low = 0
    while (1 << (low + 1)) <= FIN_TPB:
        low += 1
    while low > 1 and (1 << low) * per_row > SYM_CAP // 2:
        low -= 1
    low = min(low, bits)
    hb = bits - low
    max2 = WIDE_DIGIT_BITS if (not weighted and hb > 2 * MAX_DIGIT_BITS) else MAX_DIGIT_BITS
    fits = hb <= MAX_DIGIT_BITS + max2
    bits1 = max(hb - max2, min(8, (hb + 1) // 2)) if hb > max2 else hb
    tile = PART_TILE if n_entries >= (1 << 24) else PART_TILE // 4
    return Plan(bits, low, hb, bits1, hb - bits1, tile, (n_rows + (1 << low) - 1) >> low, fits)


def is_uniform(case: Case) -> bool:
    """What g2n_coo_to_csr decides on the device: every value dtype(1) (k_values_not_one)."""
    return len(case.rows) > 0 and bool(np.all(case.values == 1))


def case_plan(case: Case) -> Plan:
    return plan(case.n_rows, len(case.rows), weighted=not is_uniform(case))


def weight_codes(case: Case):
    """(codes, bad): weight_enc of every value — the exact int32 (bool: 0 / 1); bad: a float that is none
    (a fraction, |v| >= 2^31, -0.0, inf, nan), coded 0."""
    v = case.values
    if v.dtype.kind == "f":
        d = v.astype(np.float64)
        with np.errstate(invalid="ignore"):
            bad = ~(d == np.trunc(d)) | ~((d > -2147483648.0) & (d < 2147483648.0)) | ((d == 0) & np.signbit(d))
        return np.where(bad, 0.0, d).astype(np.int64), bad
    if v.dtype.kind == "b":
        return v.astype(np.int64), np.zeros(len(v), dtype=bool)
    return v.astype(np.int64), np.zeros(len(v), dtype=bool)


def twin_firsts(case: Case) -> np.ndarray:
    """Stream offsets i of the entries the kernel pairs with entry i + 1 (part_twins as part_fetch feeds
    it): adjacent, i at an even offset from its partition block's start (a thread holds entries 2 t and
    2 t + 1 of a sub-tile; tiles and sub-tiles are even), each other's transpose, both rows in one bucket,
    and in the weighted instance of equal value code."""
    m = len(case.rows)
    if m < 2:
        return np.zeros(0, dtype=np.int64)
    p = case_plan(case)
    r, c = case.rows.astype(np.int64), case.cols.astype(np.int64)
    i = np.arange(m - 1)
    ok = ((i % p.tile) % 2 == 0) & ((i % p.tile) + 1 < p.tile)
    ok &= (r[1:] == c[:-1]) & (c[1:] == r[:-1]) & (((r[:-1] ^ c[:-1]) >> p.low) == 0)
    if not is_uniform(case):
        w, _bad = weight_codes(case)
        ok &= w[1:] == w[:-1]
    return i[ok]


def bucket_load(case: Case):
    """(stored, expanded) per bucket holding rows: the elements a finish block reads (a paired twin is
    one) and the entries it sorts (a paired twin is two again)."""
    p = case_plan(case)
    bkt = case.rows.astype(np.int64) >> p.low
    expanded = np.bincount(bkt, minlength=p.n_bk)
    stored = expanded - np.bincount(bkt[twin_firsts(case)], minlength=p.n_bk)
    return stored, expanded


def run_magnitudes(case: Case) -> np.ndarray:
    """Per (row, column) run, the sum of |code| (WSum::mag)."""
    w, _bad = weight_codes(case)
    key = case.rows.astype(np.int64) * max(case.n_cols, 1) + case.cols
    _u, inv = np.unique(key, return_inverse=True)
    return np.bincount(inv, weights=np.abs(w).astype(np.float64)).astype(np.int64) if len(w) else np.zeros(0, np.int64)


def conditions(case: Case) -> dict:
    """The premise, one condition per name; the partition keeps the call when all hold."""
    p = case_plan(case)
    stored, expanded = bucket_load(case) if len(case.rows) else (np.zeros(1, int), np.zeros(1, int))
    cond = {
        "entries": len(case.rows) > 0 and case.n_rows > 0,          # assemble_t: n_trip && n_rows
        "ids": p.fits and max(case.n_rows, case.n_cols) < (1 << 30),  # hb within two passes; 30-bit columns
        "stored": int(stored.max()) <= SYM_CAP,                     # n > kSymCap
        # nx > kSymCap, looked at only by a block whose stored elements fit
        "expanded": int(expanded[stored <= SYM_CAP].max(initial=0)) <= SYM_CAP,
        "values": True,                                             # weight_enc: every float an exact int32
        "runs": True,                                               # WSum::exact: run magnitudes in bound
    }
    if not is_uniform(case) and case.dtype in FLOATS and len(case.rows):
        _w, bad = weight_codes(case)
        cond["values"] = not bool(bad.any())
        bound = F32_EXACT if case.dtype == "float32" else F64_EXACT
        cond["runs"] = bool(bad.any()) or int(run_magnitudes(case).max()) < bound
    return cond


def expect_buckets(case: Case) -> bool:
    """RawResult.sum_buckets of g2n_coo_to_csr(test_flags = 0) on this case."""
    return all(conditions(case).values())


def failed(case: Case) -> list:
    return [k for k, v in conditions(case).items() if not v]


# ------------------------------------------------------------------ values ------
def not_one(dtype: str):
    return False if dtype == "bool" else 2


def weights(rng, m: int, dtype: str) -> np.ndarray:
    """Order-free values (rowsum_util.general_values), the first one not 1: the weighted instance."""
    v = U.general_values(rng, m, dtype)
    if m:
        v[0] = not_one(dtype)
    return v


def build(name, n_rows, n_cols, rows, cols, dtype, uniform, vals=None, seed=0, **notes) -> Case:
    """The weighted (values given, or drawn) or the uniform instance of one COO."""
    rows = np.asarray(rows, dtype=np.int64)
    if uniform:
        v = None
    elif vals is None:
        v = weights(np.random.default_rng(seed + 977), len(rows), dtype)
    else:
        v = np.asarray(vals).astype(dtype)
    cols = np.asarray(cols, dtype=np.int64)
    assert len(rows) == len(cols) and (v is None or len(v) == len(rows)), name
    assert not len(rows) or (0 <= rows.min() and rows.max() < n_rows and 0 <= cols.min() and cols.max() < n_cols), name
    c = make(f"{name}-{dtype}-{'u' if uniform else 'w'}", n_rows, n_cols, rows, cols, v, dtype)
    c.notes.update(notes)
    return c


# ------------------------------------------------------------------ A. geometry ------
A_LOW = [(8, 6), (16, 6), (32, 6), (64, 5), (128, 4), (256, 3), (512, 2), (1100, 1)]  # per_row -> low (64 rows)
A_LOW_ABOVE = {8: 6, 16: 6, 32: 5, 64: 4, 128: 3, 256: 2, 512: 1}  # one entry more: low before the cap by bits
A_LOW_UNCAPPED = {8: 8, 16: 7, 32: 6, 64: 5, 128: 4, 256: 3, 512: 2, 1100: 1}
A_CAPPED = {1: 1, 2: 1, 3: 2, 100: 7, 256: 8}  # n_rows -> low = bits_for(n_rows)
A_RAGGED = [  # (n_rows, last row filled, wholly empty buckets)
    (1281, True, (0, 3)), (1281, False, (2, 5)), (1279, True, (0, 1)), (1279, False, (4,)), (1281, True, (1, 2, 3, 4))]
A_PASSES = {"hb10": ((1 << 18), 10, 10, 0), "hb11": ((1 << 18) + 1, 11, 6, 5), "hb16": ((1 << 24), 16, 8, 8)}
A_TAILS = [1, 2, 8191, 8192, 8193]  # entries in the last quarter-tile block
A_RECT = [(300, 70000), (70000, 300)]


def low_case(per_row: int, above: bool, dtype: str, uniform: bool) -> Case:
    """64 rows of per_row entries (one more in row 0 when `above`): the step of `low` at
    2^low * per_row > kSymCap / 2."""
    n_rows, n_cols = 64, 4096
    m = n_rows * per_row + (1 if above else 0)
    rng = np.random.default_rng(per_row)
    rows = np.concatenate([np.arange(m - (1 if above else 0)) % n_rows, np.zeros(1 if above else 0, dtype=np.int64)])
    rows = rows[rng.permutation(m)]
    cols = rng.integers(0, n_cols, m)
    return build(f"low-{per_row}{'+' if above else ''}", n_rows, n_cols, rows, cols, dtype, uniform, seed=per_row)


def capped_case(n_rows: int, dtype: str, uniform: bool) -> Case:
    """A few entries per row of 1, 2, 3, 100 and 256 rows: low = bits_for(n_rows), one bucket."""
    rng = np.random.default_rng(n_rows)
    m = 5 * n_rows + 1
    rows = rng.integers(0, n_rows, m)
    rows[:2] = (0, n_rows - 1)
    cols = rng.integers(0, 37, m)
    return build(f"capped-{n_rows}", n_rows, 37, rows, cols, dtype, uniform, seed=n_rows)


def ragged_case(n_rows: int, last: bool, empty: tuple, dtype: str, uniform: bool) -> Case:
    """n_rows = 256 k +- 1 at low = 8: the last bucket ragged, the last row filled or empty, whole buckets
    empty (indptr[n_rows] is the row n_rows - 1 owner's to write, whatever its bucket holds)."""
    rng = np.random.default_rng(n_rows + 13 * len(empty) + last)
    n_bk = (n_rows + 255) // 256
    pool = np.array([r for r in range(n_rows - 1) if (r >> 8) not in empty and r % 3])
    rows = rng.choice(pool, size=900, replace=True)
    if last:
        rows = np.concatenate([rows, [n_rows - 1] * 3])
    rows = rows[rng.permutation(len(rows))]
    cols = rng.integers(0, 90, len(rows))
    return build(f"ragged-{n_rows}-{int(last)}-{'_'.join(map(str, empty))}", n_rows, n_rows, rows, cols, dtype, uniform,
                 seed=n_rows, n_bk=n_bk, empty=empty, last=last)


def single_case(dtype: str, uniform: bool) -> Case:
    return build("single", 1281, 1281, [700], [3], dtype, uniform)


def none_case(dtype: str) -> Case:
    return U.empty_case(1281, 1281, dtype)


def passes_case(which: str, dtype: str, uniform: bool) -> Case:
    """2^18 rows (hb = 10, one pass), 2^18 + 1 (hb = 11: 6 + 5) and 2^24 (hb = 16: 8 + 8): a few thousand
    entries in the first, a middle and the last bucket of the first, a middle and the last pass-1 group."""
    n_rows, hb, bits1, bits2 = A_PASSES[which]
    rng = np.random.default_rng(hb)
    n_bk = (n_rows + 255) >> 8
    last_g = (n_bk - 1) >> bits2
    groups = sorted({0, last_g // 2, last_g})
    buckets = []
    for g in groups:
        for d in sorted({0, (1 << bits2) // 2, (1 << bits2) - 1}):
            b = (g << bits2) | d
            if b < n_bk:
                buckets.append(b)
    buckets = sorted(set(buckets) | {n_bk - 1})
    rows, cols = [], []
    per = max(330, 3000 // len(buckets))
    for b in buckets:
        width = min(256, n_rows - (b << 8))
        r = (b << 8) + rng.integers(0, width, per)
        r[0], r[1] = b << 8, (b << 8) + width - 1
        rows.append(r)
        cols.append(rng.integers(0, 600, per))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    perm = rng.permutation(len(rows))
    return build(f"passes-{which}", n_rows, n_rows, rows[perm], cols[perm], dtype, uniform, seed=hb, buckets=buckets,
                 groups=groups)


def tile_case(m: int, uniform: bool) -> Case:
    """m = 2^24 - 1 (the quarter tile) or 2^24 (the full one) entries on 2^21 rows, 8 a row (the last row 7
    at 2^24 - 1), four columns twice each; float64."""
    n_rows = 1 << 21
    i = np.arange(m, dtype=np.int64)
    rows = i % n_rows
    k = i // n_rows
    cols = (rows * 7 + (k // 2) * 13) % n_rows
    vals = None if uniform else (1 + (i % 5)).astype(np.float64)
    return make(f"tile-{m}-{'u' if uniform else 'w'}", n_rows, n_rows, rows, cols, vals, "float64")


def tail_case(tail: int, dtype: str, uniform: bool) -> Case:
    """2 * 16384 + tail entries, all of them aligned twins (a, b), (b, a) of one value: the last block holds
    `tail` entries, an odd tail cuts the last twin in two."""
    n_rows = 8192
    m = 2 * (PART_TILE // 4) + tail
    rng = np.random.default_rng(tail)
    npair = (m + 1) // 2
    a = rng.integers(0, n_rows, npair)
    b = (a & ~255) | rng.integers(0, 256, npair)  # the same bucket of 256 rows
    rows = np.stack([a, b], axis=1).ravel()[:m]
    cols = np.stack([b, a], axis=1).ravel()[:m]
    v = np.repeat(weights(rng, npair, dtype), 2)[:m]
    return build(f"tail-{tail}", n_rows, n_rows, rows, cols, dtype, uniform, vals=v, tail=tail)


def rect_case(n_rows: int, n_cols: int, dtype: str, uniform: bool) -> Case:
    rng = np.random.default_rng(n_rows)
    m = 2500
    rows = rng.integers(0, n_rows, m)
    cols = rng.integers(0, n_cols, m) // 5 * 5
    rows[:2], cols[:2] = (0, n_rows - 1), (n_cols - 1 - (n_cols - 1) % 5, 0)
    rows[m // 2:], cols[m // 2:] = rows[:m - m // 2], cols[:m - m // 2]  # every pair twice, far apart
    return build(f"rect-{n_rows}x{n_cols}", n_rows, n_cols, rows, cols, dtype, uniform, seed=n_rows)


def far_columns_case(dtype: str, uniform: bool) -> Case:
    """Every column >= n_rows: no entry has a transpose inside the matrix, adjacent or not."""
    rng = np.random.default_rng(5)
    n_rows, n_cols, m = 500, 2000, 3000
    rows = rng.integers(0, n_rows, m)
    cols = rng.integers(n_rows, n_cols, m)
    return build("farcols", n_rows, n_cols, rows, cols, dtype, uniform, seed=5)


# ------------------------------------------------------------------ B. twins ------
def _filler(i: int):
    """An entry no neighbour can pair with: its row and column lie in different buckets."""
    return (i % 2048, 2048 + (i * 7) % 2048)


# (label, entries (row, col, value), offset: "even" / "odd" / an absolute one, geometric twins: the relative
# positions of the firsts part_twins accepts when the values agree)
B_ITEMS = [
    ("even", [(2100, 2103, 3), (2103, 2100, 3)], "even", [0]),
    ("odd", [(2110, 2113, 3), (2113, 2110, 3)], "odd", []),
    ("thread-pair-edge", [(2120, 2123, 3), (2123, 2120, 3)], 2047, []),
    ("aba-even", [(2130, 2133, 3), (2133, 2130, 3), (2130, 2133, 5)], "even", [0]),
    ("abb-even", [(2140, 2143, 3), (2143, 2140, 3), (2143, 2140, 5)], "even", [0]),
    ("aba-odd", [(2150, 2153, 5), (2153, 2150, 3), (2150, 2153, 3)], "odd", [1]),
    ("abb-odd", [(2160, 2163, 3), (2163, 2160, 3), (2163, 2160, 5)], "odd", []),
    ("self", [(2170, 2170, 3), (2170, 2170, 3)], "even", [0]),
    ("self-odd", [(2171, 2171, 3), (2171, 2171, 3)], "odd", []),
    ("self-three", [(2172, 2172, 3), (2172, 2172, 3), (2172, 2172, 3)], "even", [0]),
    ("two-buckets", [(2180, 2400, 3), (2400, 2180, 3)], "even", []),
    ("bucket-edge", [(2303, 2304, 3), (2304, 2303, 3)], "even", []),
    ("unequal", [(2190, 2193, 3), (2193, 2190, 5)], "even", [0]),
    ("unequal-sum-zero", [(2195, 2196, 3), (2196, 2195, -3)], "even", [0]),
    ("equal-after-cast", [(2200, 2203, 2), (2203, 2200, 3)], "even", [0]),
    ("true-false", [(2210, 2213, 2), (2213, 2210, 0)], "even", [0]),
    ("same-entry-twice", [(2220, 2223, 3), (2220, 2223, 3)], "even", []),
    ("sub-tile-last-pair", [(2240, 2243, 3), (2243, 2240, 3)], SUB_TILE - 4, [0]),
    ("sub-tile-edge", [(2230, 2233, 3), (2233, 2230, 3)], SUB_TILE - 1, []),
    ("block-last-pair", [(2260, 2263, 3), (2263, 2260, 3)], PART_TILE // 4 - 4, [0]),
    ("block-edge", [(2250, 2253, 3), (2253, 2250, 3)], PART_TILE // 4 - 1, []),
    ("second-block", [(2280, 2283, 3), (2283, 2280, 3)], PART_TILE // 4 + 2, [0]),
    ("even-again", [(2270, 2273, 3), (2273, 2270, 3)], "even", [0]),
]
B_ONLY_TWINS_BUCKET = 12  # rows 3072 .. 3327: nothing but aligned twins (fillers end below 2048 / start above)


def _lay_out(items, n_rows, n_cols, rect=False):
    ent, marks = [], []
    fill = 0

    def pad_to(cond):
        nonlocal fill
        while not cond(len(ent)):
            r, c = _filler(fill)
            if rect:
                # wide: columns past n_rows; tall: rows past n_cols — neither can be half of a twin
                r, c = (r % n_rows, n_cols - 1 - (fill * 7) % 1000) if n_cols > n_rows else (1000 + r, c % n_cols)
            ent.append((r, c, 1 + fill % 3))
            fill += 1

    for label, entries, at, firsts in sorted(items, key=lambda it: it[2] if isinstance(it[2], int) else -1):
        if at == "even":
            pad_to(lambda n: n % 2 == 0)
        elif at == "odd":
            pad_to(lambda n: n % 2 == 1)
        else:
            assert len(ent) <= at, label
            pad_to(lambda n: n == at)
        marks.append((label, len(ent), [len(ent) + f for f in firsts], entries))
        ent += entries  # (items name different ids: the last entry of one pairs with nothing of the next)
    return ent, marks


def twin_zoo(dtype: str, uniform: bool, rect: tuple | None = None, short: bool = False) -> Case:
    """Every twin shape of B_ITEMS in one 4096-row stream of fillers (rect: (n_rows, n_cols), the twins on
    ids below both).  notes["marks"]: (label, offset, the firsts that pair geometrically, the entries)."""
    n_rows, n_cols = rect or (4096, 4096)
    items = list(B_ITEMS)
    if rect:  # ids below min(n_rows, n_cols) = 700: the same shapes on rows 308 .. 511 (bucket 1) and 512 .. 608
        items = [(lb, [(r - 1792, c - 1792, v) for r, c, v in e], at, f) for lb, e, at, f in items]
    if rect or short:  # (short: without the items at absolute offsets and the fillers that lead up to them)
        items = [it for it in items if not isinstance(it[2], int)]
    ent, marks = _lay_out(items, n_rows, n_cols, rect=bool(rect))
    if not rect:  # a bucket of nothing but aligned twins, at the end of the stream
        if len(ent) % 2:
            ent.append((_filler(0)[0], _filler(0)[1], 2))
        rng = np.random.default_rng(3)
        lo = B_ONLY_TWINS_BUCKET << 8
        for _ in range(300):
            a, b = (int(x) for x in lo + rng.integers(0, 256, 2))
            v = int(rng.integers(2, 6))
            marks.append(("only-twins", len(ent), [len(ent)], [(a, b, v), (b, a, v)]))
            ent += [(a, b, v), (b, a, v)]
    rows, cols, vals = (np.array(x) for x in zip(*ent))
    name = ("twins-short" if short else "twins") if not rect else f"twins-{n_rows}x{n_cols}"
    return build(name, n_rows, n_cols, rows, cols, dtype, uniform, vals=vals, marks=marks)


def expected_twin_firsts(case: Case) -> list:
    """The firsts the marks name, the values' equality after the dtype's cast applied (weighted only)."""
    out = []
    for _label, _at, firsts, _entries in case.notes["marks"]:
        for f in firsts:
            if case.uniform or case.vals[f] == case.vals[f + 1]:
                out.append(f)
    return sorted(out)


def mostly_twins_case(n_rows: int, dtype: str, uniform: bool = True) -> Case:
    """2^18 + 1 rows (hb = 11: the pair words go through pass 7 and reach F1 16 bits wide) or 2^18 (one
    pass: pass 4's own 16-bit words): aligned twins in buckets of every pass-1 group's edge, one entry in
    ten a single."""
    p = plan(n_rows, 6000)
    rng = np.random.default_rng(n_rows % 1000)
    last_g = (p.n_bk - 1) >> p.bits2
    buckets = sorted({b for g in (0, 1, last_g // 2, last_g - 1, last_g)
                      for b in ((g << p.bits2), (g << p.bits2) + (1 << p.bits2) - 1, (g << p.bits2) + 3)
                      if 0 <= b < p.n_bk} | {p.n_bk - 1})
    ent = []
    for b in buckets:
        width = min(256, n_rows - (b << 8))
        for q in range(200):
            a, c = (int(x) for x in (b << 8) + rng.integers(0, width, 2))
            v = int(rng.integers(2, 5))
            if q % 10 == 9:
                far = int(rng.integers(0, n_rows))
                ent += [(a, far, v), (c, c, v)]
            else:
                ent += [(a, c, v), (c, a, v)]
    rows, cols, vals = (np.array(x) for x in zip(*ent))
    return build(f"mostly-twins-{n_rows}", n_rows, n_rows, rows, cols, dtype, uniform, vals=vals, buckets=buckets)


# ------------------------------------------------------------------ C. row shapes ------
C_LENGTHS = [0, 1, 2, 4, 5, 8, 9, 16, 17, 63, 64, 65, 132, 133, 301, 302, 701, 702, 4096]
C_ORDERS = ["sorted", "reversed", "shuffled", "organ"]
C_REPEATS = [1, 2, 3, 17]
C_WAVE_MAX = [1, 4, 5, 8, 9, 16]  # the longest in-register row of a wave: the network is the wave's choice


def row_columns(rng, L: int, order: str, rep: int, n_cols: int) -> np.ndarray:
    """L columns, every distinct one `rep` times (the last fewer), in the order named."""
    distinct = (L + rep - 1) // rep
    base = np.sort(rng.choice(n_cols, size=distinct, replace=False))
    c = np.repeat(base, rep)[:L]
    if order == "reversed":
        c = c[::-1]
    elif order == "shuffled":
        c = c[rng.permutation(L)]
    elif order == "organ":
        c = np.concatenate([c[0::2], c[1::2][::-1]])
    return c


def _layout_case(name, buckets, dtype, uniform, seed, per_row=8, cap=SYM_CAP) -> Case:
    """buckets: a list of {row in bucket: (L, order, rep)}; bucket k's rows start at 256 k.  The matrix is
    square and wide enough for low = 8."""
    rng = np.random.default_rng(seed)
    m = sum(L for b in buckets for L, _o, _r in b.values())
    n = max(256 * len(buckets), -(-m // per_row), 4608)
    rows, cols, layout = [], [], []
    for k, b in enumerate(buckets):
        assert sum(L for L, _o, _r in b.values()) <= cap, (name, k)
        for t, (L, order, rep) in sorted(b.items()):
            row = 256 * k + t
            layout.append((row, L, order, rep))
            if L:
                rows.append(np.full(L, row))
                cols.append(row_columns(rng, L, order, rep, n))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    perm = U._interleave(rng, rows)  # the rows interleaved in the stream, each keeping its order
    vals = weights(rng, len(rows), dtype)  # (different values per copy of a column)
    return build(name, n, n, rows[perm], cols[perm], dtype, uniform, vals=vals[perm], layout=layout)


def _pack(specs, stride=3, cap=SYM_CAP):
    """Rows (L, order, rep) into buckets in turn, `stride` rows apart (empty rows between), a bucket closed
    when the next row would pass `cap` entries."""
    buckets, cur, load, t = [], {}, 0, 0
    for spec in specs:
        if load + spec[0] > cap or t >= 256:
            buckets.append(cur)
            cur, load, t = {}, 0, 0
        cur[t] = spec
        load += spec[0]
        t += stride
    buckets.append(cur)
    return buckets


@functools.lru_cache(maxsize=None)
def lengths_case(dtype: str, uniform: bool, gfa: bool = False) -> Case:
    """Rows of every length of C_LENGTHS in every order, every column repeated 1 / 2 / 3 / 17 times, and rows
    of one column only.  gfa: for the doubled (directed=False) build — no 4096-entry row (its twins would
    double the bucket) and buckets a third full, the transposes land on top."""
    lens = [L for L in C_LENGTHS if not (gfa and L == 4096)]
    specs = [(L, o, r) for r in C_REPEATS for o in C_ORDERS for L in lens]
    specs += [(L, "sorted", max(L, 1)) for L in lens]  # all columns equal
    return _layout_case("lengths" + ("-gfa" if gfa else ""), _pack(specs, cap=1300 if gfa else SYM_CAP), dtype, uniform,
                        seed=21, per_row=4 if gfa else 8, cap=1300 if gfa else SYM_CAP)


@functools.lru_cache(maxsize=None)
def finish_case(dtype: str, uniform: bool, gfa: bool = False) -> Case:
    """Buckets 0, 1: waves whose longest in-register row is exactly 1, 4, 5, 8, 9 and 16 entries beside rows
    of 0 (and two waves of longer rows only).  Bucket 2: 240 rows of 17, 60 a wave — every row a mid row.
    Bucket 3: short rows and one mid row in the last lane of the last wave.  Bucket 4: in-register, mid and
    long rows in turn, more than 256 merged entries (the staged-skip mask's bits k >= 1).
    gfa: the buckets thinned for the doubled build."""
    rng = np.random.default_rng(8)
    b0, b1 = {}, {}
    waves = C_WAVE_MAX + [0, 0]  # 8 waves; the last two: no in-register row with entries
    for w, top in enumerate(waves):
        b = b0 if w < 4 else b1
        base = 64 * (w % 4)
        if top == 0:
            b[base + 5] = (20, "shuffled", 2)
            b[base + 40] = (70, "shuffled", 3)
            continue
        b[base + int(rng.integers(0, 64))] = (top, "shuffled", 2)
        for t in range(0, 64, 2):
            b.setdefault(base + t, (int(rng.integers(0, top + 1)), "shuffled", 2))
    n17 = 100 if gfa else 240
    b2 = {64 * (i // 60) + i % 60: (17, "shuffled" if i % 2 else "reversed", 1 + i % 3) for i in range(n17)}
    b3 = {t: (t % 7, "shuffled", 2) for t in range(0, 255, 2)}
    b3[255] = (17, "shuffled", 3)
    b4 = {}
    for i in range(16 if gfa else 36):
        b4[3 * i] = (5, "shuffled", 2)
        b4[3 * i + 1] = (20 + i % 20, "reversed", 1 + i % 2)
        b4[3 * i + 2] = (65 + i % 5, "organ", 1 + i % 3)
    return _layout_case("finish" + ("-gfa" if gfa else ""), [b0, b1, b2, b3, b4], dtype, uniform, seed=9,
                        per_row=4 if gfa else 8)


# ------------------------------------------------------------------ D. capacity ------
D_KINDS = [("stored", SYM_CAP), ("stored", SYM_CAP + 1), ("twins", SYM_CAP // 2), ("twins", SYM_CAP // 2 + 1)]
D_WHERE = ["first", "last", "alone"]


def capacity_case(kind: str, count: int, where: str, dtype: str, uniform: bool) -> Case:
    """1024 rows, four buckets of 256: one holds `count` single entries (stored: 4096 stay, 4097 decline at
    n > kSymCap) or `count` aligned twins of one value (2048 stay; 2049 are 2049 stored elements but 4098
    entries: nx > kSymCap); it is the first bucket, the last, or alone among empty ones."""
    rng = np.random.default_rng(count)
    n = 1024
    b = {"first": 0, "last": 3, "alone": 1}[where]
    lo = b << 8
    if kind == "stored":
        rows = lo + np.arange(count) % 256
        cols = (((b + 1 + rng.integers(0, 3, count)) % 4) << 8) + rng.integers(0, 256, count)  # other buckets: no twin
        vals = weights(rng, count, dtype)
    else:
        a = lo + np.arange(count) % 256
        c = lo + rng.integers(0, 256, count)
        rows, cols = np.stack([a, c], 1).ravel(), np.stack([c, a], 1).ravel()
        vals = np.repeat(weights(rng, count, dtype), 2)
    if where != "alone":  # a few entries in every other bucket, twins among them
        extra_r, extra_c = [], []
        for ob in range(4):
            if ob != b:
                r = (ob << 8) + rng.integers(0, 256, 10)
                extra_r += [r, (ob << 8) + (r * 5) % 256]
                extra_c += [(ob << 8) + (r * 5) % 256, r]
        er, ec = np.stack(extra_r, 1).ravel(), np.stack(extra_c, 1).ravel()  # (a, b), (b, a) adjacent
        ev = np.repeat(weights(rng, len(er) // 2, dtype), 2)
        if where == "first":
            rows, cols, vals = np.concatenate([rows, er]), np.concatenate([cols, ec]), np.concatenate([vals, ev])
        else:
            rows, cols, vals = np.concatenate([er, rows]), np.concatenate([ec, cols]), np.concatenate([ev, vals])
        vals[0] = not_one(dtype)
        if kind == "twins" or where == "last":
            vals[1] = vals[0]  # (the first two entries are a twin: one value)
    return build(f"cap-{kind}-{count}-{where}", n, n, rows, cols, dtype, uniform, vals=vals, bucket=b, kind=kind,
                 count=count)


# ------------------------------------------------------------------ E. the premise and its arithmetic ------
F32_MAX_INT = float(F32_EXACT - 1)
I31 = float(2 ** 31 - 1)
# kind -> (dtypes, runs: lists of values summed on one (row, column) each, the condition that fails or None)
E_KINDS = {
    "int8-wrap": (["int8"], [[127, 1], [1] * 300, [-128, -1], [100, 100, 100], [-128]], None),
    "int32-wrap": (["int32"], [[2 ** 31 - 1, 1], [-2 ** 31], [-2 ** 31, -1], [2 ** 30] * 3, [2 ** 31 - 1] * 4], None),
    "bool-mixed": (["bool"], [[0], [0, 0], [0, 1], [1, 0, 1], [1, 1], [1]], None),
    "zero-sums": (["float64", "float32", "int32", "int8"], [[3, -3], [1, 2, -3], [0], [0, 0], [-5, 5, 0]], None),
    "f64-edge-stay": (["float64"], [[I31], [-I31], [0.0], [I31, I31], [-I31, I31], [I31] * 16], None),
    "f32-edge-stay": (["float32"], [[F32_MAX_INT], [-F32_MAX_INT], [0.0], [2.0 ** 23, 2.0 ** 23 - 1],
                                    [-(2.0 ** 23), 2.0 ** 23 - 1], [2.0 ** 20] * 15 + [2.0 ** 20 - 1]], None),
    "f-2^31": (FLOATS, [[2.0 ** 31]], "values"),
    "f--2^31": (FLOATS, [[-(2.0 ** 31)]], "values"),
    "f-half": (FLOATS, [[0.5]], "values"),
    "f-negzero": (FLOATS, [[-0.0]], "values"),
    "f-inf": (FLOATS, [[np.inf]], "values"),
    "f-nan": (FLOATS, [[np.nan]], "values"),
    "f32-2^31-1-rounds": (["float32"], [[I31]], "values"),  # float32(2^31 - 1) is 2^31
    "f32-run-2^24": (["float32"], [[2.0 ** 23, 2.0 ** 23]], "runs"),
    "f32-single-2^24": (["float32"], [[2.0 ** 24]], "runs"),
    "f32-2^24-1-1": (["float32"], [[2.0 ** 24, 1.0, 1.0]], "runs"),  # scipy: 16777216; summed exactly: 16777218
    "f32-cancelling": (["float32"], [[2.0 ** 23, -(2.0 ** 23), 2.0 ** 23, -(2.0 ** 23), 1.0]], "runs"),
}


def arith_case(kind: str, dtype: str) -> Case:
    """The runs of E_KINDS[kind], each on a (row, column) of its own in stream order, among a few plain
    entries; 600 rows (three buckets), rows of at most 16 entries but the long run's, so scipy sums every
    run in stream order.  Floats that stay: float64 up to +-(2^31 - 1); a float32 run's magnitudes must stay
    below 2^24, so its edge is +-(2^24 - 1), and float32(2^31 - 1) is 2^31, which declines."""
    _dt, runs, _fails = E_KINDS[kind]
    rows, cols, vals = [], [], []
    for k, run in enumerate(runs):
        for x in run:
            rows.append(7 * k + 280 * (k % 2))
            cols.append(3 * k + 1)
            vals.append(x)
    for k in range(12):  # plain entries, a duplicate among them
        rows.append(40 + k // 2)
        cols.append(20 + (k // 2) * 3 % 7)
        vals.append(0 if dtype == "bool" and k == 0 else 2 + k % 3)
    n = 600
    return build(f"arith-{kind}", n, n, rows, cols, dtype, False, vals=np.array(vals, dtype=np.float64), runs=runs)


# ------------------------------------------------------------------ F. the group-slot source ------
def doubled(case: Case) -> Case:
    """What a directed=False build makes of the case's GFA: every entry (a, b) followed by (b, a), of one
    value."""
    assert case.n_rows == case.n_cols
    rows = np.stack([case.rows, case.cols], 1).ravel()
    cols = np.stack([case.cols, case.rows], 1).ravel()
    vals = None if case.vals is None else np.repeat(case.vals, 2)
    c = make(case.name + "-doubled", case.n_rows, case.n_cols, rows, cols, vals, case.dtype)
    return c


def render_gfa_int(case: Case) -> bytes:
    """rowsum_util.render_gfa with the weights as RC:i tags (every value here is an integer)."""
    floats = U.text_floats(case)
    data = U.render_gfa(case, floats)
    if floats is None:
        return data
    out = re.sub(rb"RC:f:(-?\d+)\.0\n", rb"RC:i:\1\n", data)
    assert b"RC:f:" not in out, case.name
    return out


def gfa_cases(dtype: str, uniform: bool) -> list:
    """The square cases of C (thinned: the transposes land in the same buckets) and the twins of B."""
    return [lengths_case(dtype, uniform, True), finish_case(dtype, uniform, True), twin_zoo(dtype, uniform, short=True)]
