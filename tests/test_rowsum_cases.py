"""The row-sum edge cases of tests/rowsum_util.py, checked on the CPU: each case sits on the threshold it
is named after, and every case called order-sensitive is one where scipy's own coo.tocsr() differs from
summing the duplicates in stream order (so a device that summed stably, or sorted unstably where scipy is
stable, cannot pass tests/test_gpu_rowsum_edges.py by luck)."""
import numpy as np
import pytest

import rowsum_util as U


def _stable_equals_scipy(case) -> bool:
    return not U.differs_from_stable(case)


def _order_bearing(case) -> bool:
    return U.stable_sum(case)[2].tobytes() != U.stable_sum(case, reverse=True)[2].tobytes()


def test_sort_cases_cover_the_table():
    """The passes and digit widths of sort_pairs_u32 for every row count, every row and entry count used,
    rows 0 and n_rows - 1 present, rows of at most 16 entries wherever the rows can hold the entries, the
    sums equal to the stable ones (scipy's insertion sort) and changed by reversing the stream."""
    assert {n for n, _m in U.A_PAIRS + U.A_HUGE} == set(U.A_WIDTHS)
    assert {m for _n, m in U.A_PAIRS} == {1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 + 1}
    for n, m in U.A_PAIRS + U.A_HUGE:
        c = U.sort_case(n, m, False)
        assert c.notes["widths"] == U.A_WIDTHS[n], n
        assert len(c.rows) == m and c.rows.min() >= 0 and c.rows.max() == n - 1
        assert m < 2 or c.rows.min() == 0
        present = set(c.rows.tolist())
        if m >= 1023:  # enough rows for every digit's all-ones / all-zero keys
            assert set(c.notes["edge_rows"]) <= present, (n, m)
        if 9 * n >= m:
            assert c.notes["max_len"] <= 16, (n, m)
            assert m < 9 or _order_bearing(c), (n, m)
        assert _stable_equals_scipy(c), (n, m)
        u = U.sort_case(n, m, True)
        assert u.uniform and np.array_equal(u.rows, c.rows) and np.array_equal(u.cols, c.cols)
    for shape in ((300, 70000), (70000, 300)):
        c = U.rect_case(*shape, False)
        assert np.bincount(c.rows).max() <= 16 and np.bincount(c.cols).max() <= 16
        assert _stable_equals_scipy(c) and _order_bearing(c)


def test_gap_cases_sit_on_the_cap():
    for where, gap in U.B_GAPS:
        c = U.gap_case(where, gap, "float64", False)
        pop = np.unique(c.rows)
        bounds = np.concatenate([[-1], pop, [c.n_rows]])  # what k_row_bounds differences
        diffs = np.diff(bounds)
        assert diffs.max() == gap and (diffs == gap).sum() == 1 and np.sort(diffs)[-2] == 1, (where, gap)
        at = int(np.argmax(diffs))
        assert {"start": at == 0, "end": at == len(diffs) - 1, "mid": 0 < at < len(diffs) - 1}[where]
        assert _stable_equals_scipy(c)
    assert U.ROW_GAP_CAP == 64


@pytest.mark.parametrize("dtype", U.DTYPES)
def test_length_cases_hold_every_class(dtype):
    c = U.length_case(dtype, False)
    lens = np.bincount(c.rows, minlength=c.n_rows)
    seen = set()
    for row, L, rep, order in c.notes["layout"]:
        assert lens[row] == L
        seen.add((L, rep, order))
        cols = c.cols[c.rows == row]
        if L > 1 and order == "sorted":
            assert np.all(np.diff(cols) >= 0)
        if L > rep and order == "reversed":
            assert np.all(np.diff(cols) <= 0) and cols[0] > cols[-1]
        if L:
            assert np.bincount(cols).max() == min(rep, L)
    reps = [1, 2, 3, 17]
    assert {(L, r, o) for L in U.C_LENGTHS for r in reps for o in U.C_ORDERS} <= seen
    assert lens.sum() == len(c.rows) and (lens == 0).sum() > 12
    want = U.scipy_sum(c)
    if dtype == "int8":  # 128 and 256 copies of 1 wrap to -128 and to an explicit 0
        assert {(L, r, o) for L in (1000, 5000) for r in (128, 256) for o in U.C_ORDERS} <= seen
        for row, L, rep, _o in c.notes["layout"]:
            if rep >= 128:
                d = want.data[want.indptr[row]:want.indptr[row + 1]]
                assert d[0] == (-128 if rep == 128 else 0) and len(d) == (L + rep - 1) // rep
    if dtype == "int32":  # 3 x 2^30 wraps past 2^31
        assert (want.data == np.int32(-2 ** 30)).any()
    assert _stable_equals_scipy(c)


@pytest.mark.parametrize("dtype", U.FLOATS)
def test_twin_rows(dtype):
    """The same (column, value) pairs: scipy sums the 16-entry row in stream order and the 17-entry row
    in another."""
    c = U.twin_case(dtype)
    lo, hi = c.twin_rows
    assert np.bincount(c.rows).tolist() == [16, 17]
    a = sorted(zip(c.cols[c.rows == lo].tolist(), c.vals[c.rows == lo].tolist()))
    b = sorted(zip(c.cols[c.rows == hi].tolist(), c.vals[c.rows == hi].tolist()))
    assert len(set(b) - set(a)) == 1 and [x for x in b if x != (1, 2.0)] == a
    assert not U.differs_from_stable(c, lo)
    assert U.differs_from_stable(c, hi)
    one = U.make("lo", 1, c.n_cols, c.rows[c.rows == lo], c.cols[c.rows == lo], c.vals[c.rows == lo], dtype)
    assert _order_bearing(one)  # the 16-entry row's sums do depend on order: scipy's is the stable one


def test_staging_cases_straddle_the_caps():
    for cap in (4096, 2048, 1024):
        for tail in (1, 255):
            c = U.staging_case(cap, tail, "float64", False)
            assert c.n_rows == 256 * 6 + tail
            tot = np.bincount(c.rows // 256, minlength=7).tolist()
            assert tot == c.notes["totals"] and set(tot[:6]) == {cap - 1, cap, cap + 1}
            assert any(a <= cap < b or b <= cap < a for a, b in zip(tot, tot[1:]))  # staged beside direct
            assert U.scipy_sum(c).nnz < len(c.rows) and _stable_equals_scipy(c)
    for cap in (2048, 1024):
        for dtype, uniform in [(d, False) for d in U.DTYPES] + [("float64", True)]:
            c = U.rowmax_case(cap, dtype, uniform)
            seg_a, seg_t = c.notes["segments"]
            M = U.scipy_maxsym(c, U.text_floats(c))
            out = np.diff(M.indptr[[0, 256, 512, 768, 1024, c.n_rows]]).tolist()
            assert seg_a[0] > cap and seg_t[0] == 0 and out[0] <= cap        # the A segment alone
            assert seg_t[1] > cap and seg_a[1] == 0 and out[1] <= cap        # the A.T segment alone
            assert seg_a[2] <= cap and seg_t[2] <= cap and out[2] > cap      # the merged output alone
            assert max(seg_a[4], seg_t[4], out[4]) <= cap                    # a staged block


@pytest.mark.parametrize("dtype", U.FLOATS)
def test_order_cases_are_what_they_claim(dtype):
    """Every order-sensitive case differs from the stable sums under scipy; every other equals them."""
    for kind, sens in U.E_KINDS.items():
        for layout in U.E_LAYOUTS:
            c = U.order_case(kind, dtype, layout)
            lens = np.bincount(c.rows)
            assert sorted(lens[lens > 2].tolist()) == U.E_LENGTHS  # every row of runs holds more than 16 entries
            assert (lens == 2).sum() == (layout != "all_sorted")   # the row that makes the matrix unsorted
            by_row = [c.cols[c.rows == r] for r in range(len(U.E_LENGTHS))]
            rows_sorted = all(np.all(np.diff(x) >= 0) for x in by_row)
            assert rows_sorted == (layout != "shuffled"), c.name
            assert c.sensitive == (sens and layout != "all_sorted")
            assert U.differs_from_stable(c) == c.sensitive, c.name
            if sens:
                assert _order_bearing(c), c.name
            runs = np.unique(np.stack([c.rows, c.cols]), axis=1, return_counts=True)[1]
            assert runs.max() == (2 if kind == "pair2" else 4 if kind == "big" else 3), c.name
    c = U.fallback_case(dtype)
    assert np.bincount(c.rows).tolist() == [64, 64, 257, 256, 1000, 1000, 4096, 4096]
    for r in range(8):
        assert U.differs_from_stable(c, r), r
    c = U.nan_order_case(dtype)
    assert U.differs_from_stable(c)
    runs = np.unique(np.stack([c.rows, c.cols]), axis=1, return_counts=True)[1]
    assert runs.max() == 2 and np.isnan(c.vals).all()


def test_exact_runs_stay_below_the_limit():
    """The `exact` runs: integral terms whose sum of magnitudes is limit - 1; limit11: just past it."""
    rng = np.random.default_rng(0)
    for dtype in U.FLOATS:
        for t in (0, 1):
            v = np.array(U._e_run(rng, "exact", dtype, t), dtype=dtype)
            assert np.all(v == np.trunc(v)) and sum(int(abs(x)) for x in v) == int(U.LIMIT[dtype]) - 1
        v = np.array(U.triple_values(rng, dtype, "limit11"), dtype=np.float64)
        assert sum(int(abs(x)) for x in v) == int(U.LIMIT[dtype]) + 2


@pytest.mark.parametrize("dtype", U.FLOATS)
def test_arith_cases(dtype):
    """The NaN runs keep what x86 gives: the first NaN operand's payload, quieted, sign kept; inf + -inf
    the default NaN with the sign bit set."""
    for sorted_matrix in (True, False):
        c = U.arith_case(dtype, sorted_matrix)
        assert _stable_equals_scipy(c)
        want = U.scipy_sum(c)
        assert want.has_sorted_indices
        assert np.bincount(c.rows).max() <= 16
    u = np.uint64 if dtype == "float64" else np.uint32
    bits = set(want.data.view(u).tolist())
    default_neg = 0xFFF8000000000000 if dtype == "float64" else 0xFFC00000
    assert default_neg in bits
    nans = U.nan_values(dtype)
    quiet = 1 << (51 if dtype == "float64" else 22)
    for x in nans.values():
        assert (int(np.array([x]).view(u)[0]) | quiet) in bits
    assert (want.data == 0).sum() >= 8  # runs that cancel: kept
    for dt in U.DTYPES:
        c, f = U.maxsym_arith(dt)
        M = U.scipy_maxsym(c, f)
        assert M.dtype == np.dtype(dt) and (M.data != 0).all()
