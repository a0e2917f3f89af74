"""Case builders and references for the row-sum CSR path (k_pack, the LSD radix sort, k_row_bounds /
k_row_start, k_row_finish, k_row_emulate, k_row_compact, k_row_max): COOs aimed at the constants those
kernels branch on, scipy as the reference, and the stable-order summation a case is told apart by.

A Case is a COO (rows, cols in stream order; vals in its dtype, None for the uniform instance: every
value dtype(1)).  `sensitive` cases are built so that scipy's own coo.tocsr() differs from summing each
(row, column) run in stream order — the seed is searched for in a fixed range, deterministically —
and tests/test_rowsum_cases.py asserts that for every such case on the CPU."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

DTYPES = ["float64", "float32", "int32", "int8", "bool"]
FLOATS = ["float64", "float32"]
LIMIT = {"float64": 2.0 ** 53, "float32": 2.0 ** 24}  # Acc<T>::limit(): integers below it add exactly
BIG = {"float64": 2.0 ** 80, "float32": 2.0 ** 40}    # big + 1 == big
SEEDS = 64  # seeds tried for a sensitive case


@dataclass
class Case:
    name: str
    n_rows: int
    n_cols: int
    rows: np.ndarray
    cols: np.ndarray
    vals: np.ndarray | None  # None: the uniform instance
    dtype: str = "float64"
    sensitive: bool = False  # scipy's result must differ from the stable-order sums
    stable: bool = False     # scipy's result must equal the stable-order sums
    twin_rows: tuple | None = None  # (row of 16 entries, row of 17): the first stable, the second not
    notes: dict = field(default_factory=dict)

    @property
    def values(self) -> np.ndarray:
        return np.ones(len(self.rows), dtype=self.dtype) if self.vals is None else self.vals

    @property
    def uniform(self) -> bool:
        return self.vals is None


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def make(name, n_rows, n_cols, rows, cols, vals, dtype, **kw) -> Case:
    vals = None if vals is None else np.ascontiguousarray(vals, dtype=dtype)
    return Case(name, int(n_rows), int(n_cols), _i32(rows), _i32(cols), vals, dtype, **kw)


# ------------------------------------------------------------------ references ------
def scipy_sum(case: Case):
    """coo.tocsr() of the case: the reference."""
    return sp.coo_matrix((case.values, (case.rows, case.cols)), shape=(case.n_rows, case.n_cols)).tocsr()


def scipy_maxsym(case: Case, floats=None):
    """A.maximum(A.T) the way the reference forms it (builders.py:279-283): the float weights cast by
    coo_matrix(..., dtype)."""
    vals = floats if floats is not None else [1.0] * len(case.rows)
    A = sp.coo_matrix((vals, (case.rows, case.cols)), shape=(case.n_rows, case.n_cols), dtype=np.dtype(case.dtype))
    return A.maximum(A.T)


def sse_add(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """x + y as x86 SSE's addss / addsd give it with x as the destination operand (scipy's `x += y`): of
    two NaNs the FIRST one's payload, quieted — numpy's own loop may commute them."""
    r = x + y
    if x.dtype.kind == "f":
        both = np.isnan(x) & np.isnan(y)
        if both.any():
            u = np.uint64 if x.dtype.itemsize == 8 else np.uint32
            quiet = u(1) << u(51 if x.dtype.itemsize == 8 else 22)
            r[both] = (x[both].view(u) | quiet).view(x.dtype)
    return r


def stable_sum(case: Case, reverse: bool = False):
    """(indptr, indices, data): every (row, column) run summed left to right in stream order, in the
    dtype — what coo.tocsr() gives wherever std::sort keeps equal columns in order.  reverse: the runs
    summed in reversed stream order (a probe: does the order matter at all?)."""
    rows, cols, vals = case.rows.astype(np.int64), case.cols.astype(np.int64), case.values
    m = len(rows)
    idx = np.arange(m)
    order = np.lexsort((-idx if reverse else idx, cols, rows))
    r, c, v = rows[order], cols[order], vals[order]
    new = np.ones(m, dtype=bool)
    new[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    starts = np.flatnonzero(new)
    run = np.cumsum(new) - 1
    pos = idx - starts[run] if m else idx
    acc = v[starts].copy()
    with np.errstate(all="ignore"):
        for k in range(1, int(pos.max()) + 1 if m else 0):
            sel = np.flatnonzero(pos == k)
            acc[run[sel]] = sse_add(acc[run[sel]], v[sel])
    indptr = np.zeros(case.n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(r[starts], minlength=case.n_rows), out=indptr[1:])
    return indptr, c[starts], acc


def differs_from_stable(case: Case, row: int | None = None) -> bool:
    """scipy's coo.tocsr() data differs (bitwise) from the stable-order sums, in the whole matrix or in
    one row."""
    want = scipy_sum(case)
    indptr, indices, data = stable_sum(case)
    assert np.array_equal(want.indptr, indptr) and np.array_equal(want.indices, indices), case.name
    if row is None:
        return want.data.tobytes() != data.tobytes()
    lo, hi = indptr[row], indptr[row + 1]
    return want.data[lo:hi].tobytes() != data[lo:hi].tobytes()


def render_gfa(case: Case, floats=None) -> bytes:
    """The COO as a decimal-id GFA: S lines 1..N, then one L line per entry in COO order, the weight as
    an RC:f tag (none for the uniform instance).  directed=True makes one triplet of each line."""
    assert case.n_rows == case.n_cols
    out = ["S\t%d\t*\n" % (i + 1) for i in range(case.n_rows)]
    r, c = (case.rows + 1).tolist(), (case.cols + 1).tolist()
    if floats is None:
        out += ["L\t%d\t+\t%d\t+\t*\n" % rc for rc in zip(r, c)]
    else:
        out += ["L\t%d\t+\t%d\t+\t*\tRC:f:%s\n" % (a, b, repr(float(v))) for a, b, v in zip(r, c, floats)]
    return "".join(out).encode()


def text_floats(case: Case):
    """The case's values as the Python floats its GFA spells (None: uniform).  Every value of the five
    dtypes is a float64 exactly, and coo_matrix(..., dtype) casts it back to the same value."""
    if case.vals is None:
        return None
    f = case.vals.astype(np.float64)
    assert np.array_equal(f.astype(case.dtype), case.vals, equal_nan=case.dtype in FLOATS), case.name
    return f.tolist()


# ------------------------------------------------------------------ values ------
def general_values(rng, m: int, dtype: str) -> np.ndarray:
    """Values whose sums are order-free in every dtype (small integers; the floats exact), zero included
    and sums that cancel to zero."""
    if dtype == "bool":
        return rng.integers(0, 2, m).astype(bool)
    return rng.choice(np.array([1, 2, 3, -1, -2, -3, 0, 5]), m).astype(dtype)


def triple_values(rng, dtype: str, kind: str = "limit11") -> list:
    """One order-sensitive run, shuffled.  limit11: {limit, 1, 1} — (limit + 1) + 1 = limit but
    (1 + 1) + limit = limit + 2; big: {big, 1, 1, -big} — 0, 1 or 2; frac: three of 1/3, .1, 10000.1,
    -9999.9, .7 (inexact partial sums in float32 and float64)."""
    if kind == "limit11":
        v = [LIMIT[dtype], 1.0, 1.0]
    elif kind == "big":
        v = [BIG[dtype], 1.0, 1.0, -BIG[dtype]]
    else:
        v = list(rng.choice(np.array([1.0 / 3, 0.1, 10000.1, -9999.9, 0.7]), 3, replace=False))
    rng.shuffle(v)
    return v


def _interleave(rng, rows: np.ndarray) -> np.ndarray:
    """A permutation that interleaves the rows of a row-grouped stream, each row keeping its own order."""
    _u, first, inv, cnt = np.unique(rows, return_index=True, return_inverse=True, return_counts=True)
    pos = np.arange(len(rows)) - first[inv]  # (row-grouped: a row's entries are consecutive)
    return np.argsort((pos + rng.uniform(0, 1, len(cnt))[inv]) / cnt[inv], kind="stable")


def _jitter(rng, m: int, width: float) -> np.ndarray:
    """A permutation that moves an item by less than `width` places: the entries of one row stay within
    a wave step of the radix scatter or spread over neighbouring ones."""
    return np.argsort(np.arange(m) + rng.uniform(0, width, m), kind="stable")


# ------------------------------------------------------------------ A. sort geometry ------
RS_MAX_BITS = 8


def sort_digits(n_rows: int) -> list:
    """sort_pairs_u32's passes for n_rows keys: [(shift, width)], equal widths rounded up first."""
    bits = 1
    while (1 << bits) < n_rows:
        bits += 1
    passes = (bits + RS_MAX_BITS - 1) // RS_MAX_BITS
    out, lo = [], 0
    for p in range(passes):
        db = (bits - lo + (passes - p) - 1) // (passes - p)
        out.append((lo, db))
        lo += db
    return out


A_PAIRS = [  # (n_rows, entries): every row count and every entry count at least once
    (1, 1), (1, 65), (2, 63), (2, 4097), (255, 64), (255, 1023), (256, 1024), (256, 4096), (257, 1025),
    (257, 3 * 4096 + 1), (65536, 4095), (65536, 65), (65537, 4097), (65537, 3 * 4096 + 1), (65537, 1024),
]
A_HUGE = [(1 << 24, 4097), (1 << 24, 3 * 4096 + 1), ((1 << 24) + 1, 4096), ((1 << 24) + 1, 3 * 4096 + 1)]
A_WIDTHS = {1: (1,), 2: (1,), 255: (8,), 256: (8,), 257: (5, 4), 65536: (8, 8), 65537: (6, 6, 5),
            1 << 24: (8, 8, 8), (1 << 24) + 1: (7, 6, 6, 6)}


def _edge_rows(n_rows: int) -> list:
    """Rows 0 and n_rows - 1 and, for every digit of the sort, the keys with that digit all ones and the
    others all zero, and with it all zero and the others all ones (where they exist below n_rows)."""
    bits = sum(w for _lo, w in sort_digits(n_rows))
    full = (1 << bits) - 1
    want = [0, n_rows - 1]
    for lo, w in sort_digits(n_rows):
        mask = ((1 << w) - 1) << lo
        want += [mask, full & ~mask, (1 << (lo + w)) - 1, 1 << lo]
    seen, out = set(), []
    for r in want:
        if 0 <= r < n_rows and r not in seen:
            seen.add(r)
            out.append(r)
    return out


def sort_case(n_rows: int, m: int, uniform: bool, n_cols: int = 40, seed: int = 1) -> Case:
    """m entries on rows of at most 16 entries (so scipy's order is the stream order), float64, with
    {limit, 1, 1} triples on repeated columns: a sort that is not stable changes a sum, one that loses
    or misroutes an item changes indices."""
    rng = np.random.default_rng(seed + 7 * m + n_rows % 1009)
    edge = _edge_rows(n_rows)
    n_pick = max(1, min(n_rows, (m + 8) // 9))  # rows of about 9 entries
    picked = ([n_rows - 1, 0] + edge[2:] if n_rows > 1 else [0])[:n_pick]  # one entry: on the last row
    if n_pick > len(picked):
        pool = rng.permutation(np.unique(rng.integers(0, n_rows, 3 * n_pick + 64))).tolist()
        have = set(picked)
        for r in pool:
            if len(picked) == n_pick:
                break
            if r not in have:
                have.add(r)
                picked.append(r)
    lens = np.zeros(len(picked), dtype=np.int64)
    left = m
    for i in range(len(picked)):  # every picked row holds an entry, none more than 16
        lens[i] = 1
        left -= 1
    while left:
        room = np.flatnonzero(lens < 16)
        if len(room) == 0:  # (n_rows too small for m entries of short rows: rows grow past 16, all exact)
            lens[rng.integers(0, len(lens))] += left
            break
        i = room[rng.integers(0, len(room))]
        add = min(left, int(rng.integers(1, 17 - lens[i])))
        lens[i] += add
        left -= add
    rows, cols, vals = [], [], []
    for r, L in zip(picked, lens.tolist()):
        short = L <= 16
        k = L // 3 if short else 0
        cs = rng.choice(n_cols, size=min(n_cols, k + (L - 3 * k)), replace=False).tolist()
        for t in range(k):
            rows += [r] * 3
            cols += [cs[t % len(cs)]] * 3
            vals += triple_values(rng, "float64")
        for t in range(L - 3 * k):
            rows.append(r)
            cols.append(cs[(k + t) % len(cs)])
            vals.append(float(rng.choice(np.array([1.0, 2.0, 3.0, -2.0]))))
    rows, cols, vals = np.array(rows), np.array(cols), np.array(vals)
    # a row's entries shuffled among themselves and against their neighbours, then half of the cases
    # spread over the whole stream
    perm = _jitter(rng, len(rows), 40.0)
    if (m + n_rows) % 2:
        perm = perm[_jitter(rng, len(rows), float(len(rows)))]
    rows, cols, vals = rows[perm], cols[perm], vals[perm]
    return make(f"sort-{n_rows}x{m}-{'u' if uniform else 'w'}", n_rows, n_cols, rows, cols,
                None if uniform else vals, "float64", stable=True,
                notes={"widths": tuple(w for _lo, w in sort_digits(n_rows)), "edge_rows": edge,
                       "max_len": int(lens.max())})


def rect_case(n_rows: int, n_cols: int, uniform: bool) -> Case:
    """A rectangular COO, rows of at most 16 entries in both directions (the CSC sorts the columns)."""
    rng = np.random.default_rng(n_rows)
    m = 2500
    small, large = min(n_rows, n_cols), max(n_rows, n_cols)
    a = rng.choice(large, size=m // 3, replace=False)  # the long dimension: three entries each
    a[0], a[1] = 0, large - 1
    a = np.repeat(a, 3)
    b = np.repeat(np.arange(len(a) // 3) % small, 3)  # the short one: one repeated (row, column) pair each
    # the short dimension's rows hold len(a) / small <= 16 entries
    assert len(a) / small <= 16
    vals = np.concatenate([triple_values(rng, "float64") for _ in range(len(a) // 3)])
    perm = _jitter(rng, len(a), 40.0)
    a, b, vals = a[perm], b[perm], vals[perm]
    rows, cols = (a, b) if n_rows > n_cols else (b, a)
    return make(f"rect-{n_rows}x{n_cols}-{'u' if uniform else 'w'}", n_rows, n_cols, rows, cols,
                None if uniform else vals, "float64", stable=True)


# ------------------------------------------------------------------ B. row bounds ------
ROW_GAP_CAP = 64
B_GAPS = [("start", 64), ("start", 65), ("mid", 64), ("mid", 65), ("end", 64), ("end", 65), ("mid", 100_000)]


def gap_case(where: str, gap: int, dtype: str, uniform: bool) -> Case:
    """Every row populated but for one run of empty rows: `gap` = the difference k_row_bounds sees (first
    populated row + 1 at the start, since prev = -1; n_rows - last populated row at the end)."""
    rng = np.random.default_rng(gap)
    n_rows = 400 + gap
    if where == "start":
        pop = np.arange(gap - 1, n_rows)
    elif where == "end":
        pop = np.arange(0, n_rows - gap + 1)
    else:
        pop = np.concatenate([np.arange(0, 150), np.arange(149 + gap, n_rows)])
    rows = np.concatenate([pop, pop[::3], pop[::3]])
    n_cols = 50
    cols = rng.integers(0, n_cols, len(rows))
    cols[len(pop):len(pop) + len(pop[::3])] = cols[:len(pop):3]  # a duplicate on every third row
    vals = general_values(rng, len(rows), dtype)
    perm = rng.permutation(len(rows))
    c = make(f"gap-{where}-{gap}-{dtype}-{'u' if uniform else 'w'}", n_rows, n_cols, rows[perm], cols[perm],
             None if uniform else vals[perm], dtype, stable=True)
    c.notes["populated"] = (int(pop[0]), int(pop[-1]))
    return c


def empty_case(n_rows: int, n_cols: int, dtype: str) -> Case:
    z = np.zeros(0, dtype=np.int32)
    return make(f"empty-{n_rows}x{n_cols}-{dtype}", n_rows, n_cols, z, z, np.zeros(0, dtype=dtype), dtype,
                stable=True)


# ------------------------------------------------------------------ C. row length classes ------
C_LENGTHS = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 18, 31, 32, 33, 64, 1000, 5000]
C_ORDERS = ["sorted", "reversed", "shuffled"]
C_N = 5003  # 5000 distinct columns in one row; square, for MAX-SYM


def _c_repeats(dtype: str) -> list:
    return [1, 2, 3, 17] + ([128, 256] if dtype == "int8" else [])


def length_case(dtype: str, uniform: bool) -> Case:
    """Rows of every length class, each in column order, reversed and shuffled, with columns repeated
    1, 2, 3 and 17 times (int8: 128 and 256 times too, of value 1: the sums wrap to -128 and 0; int32:
    three times 2^30, past 2^31).  Float values are exact integers: no sum here depends on order."""
    rng = np.random.default_rng(11)
    rows, cols, vals = [], [], []
    row = 0
    layout = []
    for rep in _c_repeats(dtype):
        for L in C_LENGTHS:
            if rep >= 128 and L < 1000:
                continue
            for order in C_ORDERS:
                row += 23 if L >= 1000 else 5  # spread: staged and direct blocks, empty rows in between
                if L == 0:
                    layout.append((row, L, rep, order))
                    continue
                distinct = (L + rep - 1) // rep
                base = rng.choice(C_N, size=distinct, replace=False)
                base.sort()
                c = np.repeat(base, rep)[:L]
                if rep >= 128:
                    v = np.ones(L, dtype=dtype)
                elif dtype == "int32" and rep == 3:
                    v = np.full(L, 2 ** 30, dtype=dtype)
                else:
                    v = general_values(rng, L, dtype)
                if order == "reversed":
                    c, v = c[::-1], v[::-1]
                elif order == "shuffled":
                    p = rng.permutation(L)
                    c, v = c[p], v[p]
                rows.append(np.full(L, row))
                cols.append(c)
                vals.append(v)
                layout.append((row, L, rep, order))
    assert row < C_N
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    # the rows interleaved in the stream, each keeping its own order (a stable selection)
    perm = _interleave(rng, rows)
    c = make(f"lengths-{dtype}-{'u' if uniform else 'w'}", C_N, C_N, rows[perm], cols[perm],
             None if uniform else vals[perm], dtype, stable=True)
    c.notes["layout"] = layout
    return c


@functools.lru_cache(maxsize=None)
def twin_case(dtype: str) -> Case:
    """The same 16 (column, value) pairs — five {limit, 1, 1} triples and a single — as row 0 (16 entries:
    std::sort is an insertion sort, stable) and, with one more single, as row 1 (17 entries: not stable) of
    one unsorted matrix."""
    for seed in range(SEEDS):
        rng = np.random.default_rng(seed)
        cols = np.repeat(np.arange(5) * 3 + 2, 3).tolist() + [40]
        vals = sum((triple_values(rng, dtype) for _ in range(5)), []) + [3.0]
        p = rng.permutation(16)
        cols, vals = [cols[i] for i in p], [vals[i] for i in p]
        at = int(rng.integers(0, 17))
        cols17, vals17 = list(cols), list(vals)
        cols17.insert(at, 1)
        vals17.insert(at, 2.0)
        c = make(f"twin-{dtype}", 2, 41, [0] * 16 + [1] * 17, cols + cols17, vals + vals17, dtype,
                 sensitive=True, twin_rows=(0, 1), notes={"seed": seed})
        if differs_from_stable(c, 1) and stable_sum(c)[2].tobytes() != stable_sum(c, reverse=True)[2].tobytes():
            return c
    raise AssertionError(f"no seed below {SEEDS} makes the 17-entry twin order-sensitive ({dtype})")


# ------------------------------------------------------------------ D. staging thresholds ------
def staging_case(cap: int, tail: int, dtype: str, uniform: bool) -> Case:
    """Blocks of 256 consecutive rows whose entry totals are cap - 1, cap + 1, cap, cap + 1, cap - 1, cap
    (staged and direct blocks adjacent) and a ragged last block of `tail` rows holding cap + 1 entries
    (tail 255) or cap (tail 1: one long row)."""
    rng = np.random.default_rng(cap + tail)
    totals = [cap - 1, cap + 1, cap, cap + 1, cap - 1, cap, cap + 1 if tail > 1 else cap]
    n_rows = 256 * 6 + tail
    n_cols = 300
    rows, cols = [], []
    for b, tot in enumerate(totals):
        width = 256 if b < 6 else tail
        lens = np.full(width, tot // width)
        lens[rng.choice(width, size=tot - int(lens.sum()), replace=False)] += 1
        if width == 256:  # ragged lengths, zero included, the total kept
            for _ in range(200):
                i, j = rng.integers(0, width, 2)
                if lens[i] > 0 and lens[j] < 16 + cap // 256:
                    lens[i] -= 1
                    lens[j] += 1
        assert lens.sum() == tot
        r = np.repeat(np.arange(width) + 256 * b, lens)
        c = rng.integers(0, n_cols, len(r)) // 3 * 3  # a third of the columns: duplicates in most rows
        rows.append(r)
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = general_values(rng, len(rows), dtype)
    perm = rng.permutation(len(rows))
    c = make(f"stage-{cap}-{tail}-{dtype}-{'u' if uniform else 'w'}", n_rows, n_cols, rows[perm], cols[perm],
             None if uniform else vals[perm], dtype, stable=True)
    c.notes["totals"] = totals
    return c


def rowmax_case(cap: int, dtype: str, uniform: bool) -> Case:
    """MAX-SYM blocks where each of k_row_max's three staging conditions fails alone.  Block 0 (rows
    0..255): A over the cap, A.T empty; block 1: the reverse; blocks 2 and 3: A and A.T each within the
    cap on disjoint columns, their merge over it; the ragged block 4 is staged."""
    rng = np.random.default_rng(cap)
    over, half = cap + 76, cap // 2 + 150
    n = 1024 + 37

    def block(n_ent, r_lo, r_hi, c_lo, c_hi):
        return rng.integers(r_lo, r_hi, n_ent), rng.integers(c_lo, c_hi, n_ent)

    parts = [block(over, 0, 256, 256, 260),          # block 0 A / block 1 A.T: duplicates, few unique
             block(half, 512, 768, 768, 896),        # block 2 A (columns 768..895), block 3 A.T
             block(half, 896, 1024, 512, 768),       # block 2 A.T (from rows 896..1023), block 3 A
             block(half - 100, 768, 896, 900, 1024),  # block 3 A: with the above past half, below the cap
             block(60, 1024, n, 1024, n)]            # the ragged block, both sides
    rows = np.concatenate([p[0] for p in parts])
    cols = np.concatenate([p[1] for p in parts])
    # (positive values: the maximum against a missing entry keeps them; bool: one False in ten)
    vals = rng.random(len(rows)) < 0.9 if dtype == "bool" else rng.choice(np.array([1, 2, 3, 5]), len(rows))
    perm = rng.permutation(len(rows))
    c = make(f"rowmax-{cap}-{dtype}-{'u' if uniform else 'w'}", n, n, rows[perm], cols[perm],
             None if uniform else vals[perm], dtype, stable=True)
    seg_a = np.bincount(rows // 256, minlength=5)
    seg_t = np.bincount(cols // 256, minlength=5)
    c.notes["segments"] = (seg_a.tolist(), seg_t.tolist())
    return c


# ------------------------------------------------------------------ E. summation order ------
E_KINDS = {  # kind -> sensitive where scipy sorts
    "pair2": False,      # runs of 2 inexact copies: a + b == b + a
    "frac": True,        # 3 fractional terms
    "exact": False,      # integral terms, sum |x| = limit - 1: every partial sum exact
    "limit11": True,     # {limit, 1, 1}: sum |x| just past the limit
    "big": True,         # {big, 1, 1, -big}
    "infnan": False,     # {inf, 1, -inf} and {nan, 1, 2}: NaN whatever the order
}
E_LAYOUTS = ["shuffled", "row_sorted", "all_sorted"]
E_LENGTHS = [17, 18, 33, 100]


def _e_run(rng, kind: str, dtype: str, t: int) -> list:
    if kind == "pair2":
        return [0.1, 0.7] if t % 2 else [0.3, 0.2]
    if kind == "exact":
        lim = LIMIT[dtype]
        v = [lim / 2, lim / 4, lim / 4 - 1.0] if t % 2 else [lim - 3.0, -1.0, 1.0]
        rng.shuffle(v)
        return v
    if kind == "infnan":
        v = [np.inf, 1.0, -np.inf] if t % 2 else [np.nan, 1.0, 2.0]
        rng.shuffle(v)
        return v
    return triple_values(rng, dtype, kind)


def _order_build(kind: str, dtype: str, layout: str, seed: int) -> Case:
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for r, L in enumerate(E_LENGTHS):
        c, v, t = [], [], 0
        while len(c) < L:
            run = _e_run(rng, kind, dtype, t)
            if len(c) + len(run) > L:
                run = [1.0] * (L - len(c))  # singles on columns of their own
                c += [1000 + 2 * t + i for i in range(len(run))]
            else:
                c += [3 * t] * len(run)
            v += run
            t += 1
        c, v = np.array(c), np.array(v)
        if layout == "shuffled":
            p = rng.permutation(L)
        else:  # the row in column order, the runs in their built (shuffled) order
            p = np.argsort(c, kind="stable")
        rows.append(np.full(L, r))
        cols.append(c[p])
        vals.append(v[p])
    if layout != "all_sorted":  # the row that makes the matrix unsorted
        rows.append(np.full(2, len(E_LENGTHS)))
        cols.append(np.array([5, 4]))
        vals.append(np.array([1.0, 2.0]))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    perm = _interleave(rng, rows)  # rows interleaved, each in its order
    sens = E_KINDS[kind] and layout != "all_sorted"
    return make(f"order-{kind}-{layout}-{dtype}", 1300, 1300, rows[perm], cols[perm], vals[perm],
                dtype, sensitive=sens, stable=not sens, notes={"seed": seed})


@functools.lru_cache(maxsize=None)
def order_case(kind: str, dtype: str, layout: str) -> Case:
    """Rows of 17, 18, 33 and 100 entries made of runs of one kind; shuffled: the rows themselves
    unsorted; row_sorted: in column order, a fifth row makes the matrix unsorted (scipy's std::sort still
    permutes equal columns); all_sorted: scipy sorts nothing."""
    if not (E_KINDS[kind] and layout != "all_sorted"):
        return _order_build(kind, dtype, layout, 0)
    for seed in range(SEEDS):
        c = _order_build(kind, dtype, layout, seed)
        if differs_from_stable(c):
            return c
    raise AssertionError(f"no seed below {SEEDS} makes order-{kind}-{layout}-{dtype} order-sensitive")


def killer_keys(n: int) -> np.ndarray:
    """Musser's median-of-3 killer (tests/test_host_headers.py: test_stl_sort_depth_limit_fallback)."""
    k = n // 2
    keys = np.zeros(n, dtype=np.int64)
    for i in range(1, k + 1):
        if i % 2:
            keys[i - 1] = i
            keys[i] = k + i
        keys[k + i - 1] = 2 * i
    return keys


def organ_keys(n: int) -> np.ndarray:
    return np.concatenate([np.arange(n // 2), np.arange(n // 2)[::-1]])


@functools.lru_cache(maxsize=None)
def fallback_case(dtype: str) -> Case:
    """Rows of 64, 257, 1000 and 4096 entries whose columns are laid out as the median-of-3 killer and as
    the organ pipe (keys // 3 and keys // 2: runs of three and four equal columns, the layout's order
    kept), carrying {big, 1, 1, -big}-style values: introsort's heap-sort fallback decides the sums."""
    for seed in range(SEEDS):
        rng = np.random.default_rng(seed)
        rows, cols, vals = [], [], []
        r = 0
        for n in (64, 257, 1000, 4096):
            for keys in (killer_keys(n) // 3, organ_keys(n) // 2):
                v = rng.choice(np.array([BIG[dtype], 1.0, 1.0, -BIG[dtype], 1.0]), len(keys))
                rows.append(np.full(len(keys), r))
                cols.append(keys)
                vals.append(v)
                r += 1
        c = make(f"fallback-{dtype}", r, 4100, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals),
                 dtype, sensitive=True, notes={"seed": seed})
        if all(differs_from_stable(c, k) for k in range(r)):
            return c
    raise AssertionError(f"no seed below {SEEDS} makes every fallback row order-sensitive ({dtype})")


# ------------------------------------------------------------------ F. arithmetic ------
def _bits(dtype: str, patterns) -> np.ndarray:
    u = np.uint64 if dtype == "float64" else np.uint32
    return np.array(patterns, dtype=u).view(dtype)


def nan_values(dtype: str) -> dict:
    """Quiet and signalling NaNs with non-default payloads, of both signs."""
    if dtype == "float64":
        p = {"q+": 0x7FF8000000001234, "q-": 0xFFF80000000ABCDE, "s+": 0x7FF0000000000001, "s-": 0xFFF4000000005555,
             "s+hi": 0x7FF7FFFFFFFFFFFF}
    else:
        p = {"q+": 0x7FC01234, "q-": 0xFFC0ABCD, "s+": 0x7F800001, "s-": 0xFFA05555, "s+hi": 0x7FBFFFFF}
    return {k: _bits(dtype, [v])[0] for k, v in p.items()}


def arith_case(dtype: str, sorted_matrix: bool) -> Case:
    """Runs of two (and a few of three) through coo_to_csr arrays: every NaN as first and as second operand
    against a number, NaN + NaN in both orders, inf + -inf, the signed zeros, runs that cancel to zero.
    Rows hold at most 16 entries, so scipy's order is the stream order in either matrix."""
    T = np.dtype(dtype).type
    nans = nan_values(dtype)
    runs = []
    for x in nans.values():
        runs += [[x, T(1.5)], [T(1.5), x], [x, T(np.inf)], [T(-np.inf), x]]
    names = list(nans)
    for a in names:
        for b in names:
            runs.append([nans[a], nans[b]])
    runs += [[nans["s+"], nans["q-"], T(2.0)], [T(2.0), nans["s-"], nans["q+"]]]
    runs += [[T(np.inf), T(-np.inf)], [T(-np.inf), T(np.inf)], [T(np.inf), T(np.inf)], [T(np.inf), T(1.0), T(-np.inf)]]
    runs += [[T(-0.0), T(-0.0)], [T(-0.0), T(0.0)], [T(0.0), T(-0.0)], [T(-0.0)], [T(0.0)]]
    runs += [[T(1.5), T(-1.5)], [T(-1.5), T(1.5)], [T(1.0), T(2.0), T(-3.0)], [T(-2.5), T(2.5), T(0.0)]]
    rows, cols, vals = [], [], []
    per_row = 5  # runs per row: at most 15 entries
    for k, run in enumerate(runs):
        r, c = k // per_row, 3 * (k % per_row)
        for x in run:
            rows.append(r)
            cols.append(c)
            vals.append(x)
    rows, cols = np.array(rows), np.array(cols)
    vals = np.array(vals, dtype=dtype)
    assert np.bincount(rows).max() <= 16
    if not sorted_matrix:  # columns descending inside each row, every run in its order
        p = np.lexsort((np.arange(len(rows)), -cols, rows))
        rows, cols, vals = rows[p], cols[p], vals[p]
    n_rows = int(rows.max()) + 2
    return make(f"arith-{dtype}-{'sorted' if sorted_matrix else 'unsorted'}", n_rows, 16, rows, cols, vals, dtype,
                stable=True, notes={"runs": len(runs)})


@functools.lru_cache(maxsize=None)
def nan_order_case(dtype: str) -> Case:
    """Runs of TWO NaNs of different payloads in rows of more than 16 entries of an unsorted matrix: x86
    keeps the first operand's payload, so the sum follows scipy's std::sort order although a + b == b + a
    for numbers."""
    nans = nan_values(dtype)
    for seed in range(SEEDS):
        rng = np.random.default_rng(seed)
        rows, cols, vals = [], [], []
        for r, L in enumerate((17, 18, 33, 100)):
            c = np.repeat(np.arange((L + 1) // 2), 2)[:L]
            v = np.array([nans["q+"], nans["q-"]] * ((L + 1) // 2), dtype=dtype)[:L]
            p = rng.permutation(L)
            rows.append(np.full(L, r))
            cols.append(c[p])
            vals.append(v[p])
        c = make(f"nanpair-{dtype}", 4, 64, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), dtype,
                 sensitive=True, notes={"seed": seed})
        if differs_from_stable(c):
            return c
    raise AssertionError(f"no seed below {SEEDS} makes nanpair-{dtype} order-sensitive")


def maxsym_arith(dtype: str):
    """(case, the float weights its GFA spells): the MAX-SYM edges text weights can reach."""
    ent = []  # (row, col, float)
    if dtype in FLOATS:
        ent += [(0, 1, float("nan")), (1, 0, 2.0), (2, 3, 3.0), (3, 2, float("nan")), (20, 21, float("nan")),
                (22, 23, float("nan")), (23, 22, float("nan")), (24, 25, float("inf")), (25, 24, float("-inf")),
                (26, 27, float("inf")), (26, 27, float("-inf")), (27, 26, 1.0)]
        ent += [(6, 7, -0.0), (7, 6, 0.0), (28, 29, 0.0), (29, 28, -0.0), (30, 31, -0.0), (32, 32, -0.0),
                (8, 9, 1.5), (8, 9, -1.5), (9, 8, -1.0), (10, 11, 0.25), (10, 11, -0.25)]
    ent += [(4, 5, -2.0), (12, 13, -2.0), (13, 12, -3.0), (14, 15, 1.0), (14, 15, -1.0), (15, 14, -1.0),
            (16, 17, 2.0), (16, 17, -2.0), (18, 18, -1.0), (19, 19, 4.0), (33, 34, 0.0), (35, 36, 0.0), (36, 35, 3.0)]
    if dtype == "int8":
        ent += [(37, 38, -128.0), (38, 37, 127.0), (39, 40, -128.0), (41, 42, -128.0), (42, 41, -128.0),
                (43, 44, 64.0), (43, 44, 64.0), (44, 43, 1.0), (45, 46, 127.0), (45, 46, 127.0), (45, 46, 2.0)]
    if dtype == "int32":
        ent += [(37, 38, -2147483648.0), (38, 37, 2147483647.0), (39, 40, 1073741824.0), (39, 40, 1073741824.0),
                (40, 39, 5.0)]
    if dtype == "bool":  # nonzero -> True, 0.0 -> an explicit False
        ent += [(37, 38, 0.0), (38, 37, 2.0), (39, 40, 0.0), (39, 40, -1.0), (41, 42, 0.5), (41, 42, 0.25)]
    n = 48
    rows, cols, f = [e[0] for e in ent], [e[1] for e in ent], [e[2] for e in ent]
    vals = np.array(f, dtype=np.float64).astype(dtype)
    return make(f"maxarith-{dtype}", n, n, rows, cols, vals, dtype, stable=True), f
