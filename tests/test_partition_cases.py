"""The bucket-partition edge cases of tests/partition_util.py, checked on the CPU: plan() gives the low, hb,
bits1, bits2 and tile each case names, the bucket loads are exactly 4096 or 4097 where a case says so,
rows have the lengths named, twins sit at the parities named, and every case called "declines" fails
exactly one stated condition (so tests/test_gpu_partition_edges.py cannot pass by a case having drifted
off its threshold)."""
import numpy as np
import pytest

import partition_util as P
import rowsum_util as U


def _lens(case):
    return np.bincount(case.rows, minlength=case.n_rows)


def test_plan_restates_the_geometry():
    """bits_for, the low steps at 2^low * per_row > kSymCap / 2, the cap by bits, the digit split and the
    tile — at the figures DESIGN.md and the kernels' comments give."""
    assert [P.bits_for(n) for n in (0, 1, 2, 3, 4, 5, 256, 257, 1 << 18, (1 << 18) + 1)] == [1, 1, 1, 2, 2, 3, 8, 9, 18, 19]
    for per_row, low in P.A_LOW_UNCAPPED.items():
        assert P.plan(1 << 20, (1 << 20) * per_row).low == low, per_row
    for per_row in (8, 16, 32, 64, 128, 256, 512):  # one entry more: the next step
        assert P.plan(1 << 20, (1 << 20) * per_row + 1).low == P.A_LOW_UNCAPPED[per_row] - 1, per_row
    assert P.plan(1 << 20, (1 << 20) * 100000).low == 1  # never below buckets of 2 rows
    # C4's shape (DESIGN: hb = 18, 8 + 10) and the widths the two routes decline at
    p = P.plan(1 << 26, 1 << 27)
    assert (p.low, p.hb, p.bits1, p.bits2, p.tile, p.fits) == (8, 18, 8, 10, 65536, True)
    assert P.plan((1 << 28) + 1, 10, weighted=True).fits is False and P.plan((1 << 28) + 1, 10).fits is True
    assert P.plan((1 << 28) + 1, 10).bits2 == 11 and not P.plan((1 << 30) + 1, 10).fits
    assert P.plan(1 << 28, 10, weighted=True).fits and P.plan(1 << 28, 10, weighted=True).bits1 == 10
    assert P.plan(100, (1 << 24) - 1).tile == 16384 and P.plan(100, 1 << 24).tile == 65536
    assert P.plan(257, 10).n_bk == 2 and P.plan(256, 10).n_bk == 1 and P.plan(1281, 10).n_bk == 6


def test_low_cases_sit_on_the_steps():
    for per_row, low in P.A_LOW:
        c = P.low_case(per_row, False, "float64", False)
        assert c.n_rows == 64 and len(c.rows) == 64 * per_row and set(_lens(c)) == {per_row}
        assert P.case_plan(c).low == low == min(P.A_LOW_UNCAPPED[per_row], 6) and P.case_plan(c).hb == 6 - low
        assert P.expect_buckets(c) and P.expect_buckets(P.low_case(per_row, False, "float64", True))
    for per_row, low in P.A_LOW_ABOVE.items():
        c = P.low_case(per_row, True, "int8", False)
        assert len(c.rows) == 64 * per_row + 1 and _lens(c).max() == per_row + 1
        assert P.case_plan(c).low == low == min(P.A_LOW_UNCAPPED[per_row] - 1, 6)
        assert P.expect_buckets(c)
    assert P.case_plan(P.low_case(1100, False, "bool", False)).n_bk == 32  # buckets of 2 rows
    for n_rows, low in P.A_CAPPED.items():
        for uniform in (False, True):
            c = P.capped_case(n_rows, "int32", uniform)
            p = P.case_plan(c)
            assert (p.low, p.hb, p.n_bk) == (low, 0, 1) and p.low == P.bits_for(n_rows), n_rows
            assert c.rows.max() == n_rows - 1 and P.expect_buckets(c) and P.is_uniform(c) == uniform


def test_ragged_cases():
    for n_rows, last, empty in P.A_RAGGED:
        c = P.ragged_case(n_rows, last, empty, "float32", False)
        p = P.case_plan(c)
        assert p.low == 8 and n_rows % 256 in (1, 255) and p.n_bk == (n_rows + 255) // 256
        lens = _lens(c)
        assert (lens[n_rows - 1] > 0) == last
        per_bucket = np.bincount(np.arange(n_rows) >> 8, weights=lens, minlength=p.n_bk)
        assert {int(b) for b in np.flatnonzero(per_bucket == 0)} >= set(empty)
        assert P.expect_buckets(c)
    wholly = [set(e) for _n, _l, e in P.A_RAGGED]
    assert any(0 in e for e in wholly) and any(e & {2, 3} for e in wholly)  # the start, the middle
    assert any((n + 255) // 256 - 1 in e for n, _l, e in P.A_RAGGED)        # the end
    c = P.single_case("float64", False)
    assert len(c.rows) == 1 and not P.is_uniform(c) and P.expect_buckets(c)
    assert P.is_uniform(P.single_case("bool", True))
    assert P.failed(P.none_case("float64")) == ["entries"]


def test_pass_count_cases():
    for which, (n_rows, hb, bits1, bits2) in P.A_PASSES.items():
        for uniform in (False, True):
            c = P.passes_case(which, "float64", uniform)
            p = P.case_plan(c)
            assert (c.n_rows, p.low, p.hb, p.bits1, p.bits2) == (n_rows, 8, hb, bits1, bits2), which
            assert 2000 <= len(c.rows) <= 9000 and P.expect_buckets(c)
        bk = np.unique(c.rows >> 8)
        assert bk.tolist() == c.notes["buckets"] and bk[0] == 0 and bk[-1] == p.n_bk - 1
        groups = np.unique(bk >> bits2)
        assert len(groups) >= 3 and groups[0] == 0 and groups[-1] == (p.n_bk - 1) >> bits2
        mid = groups[len(groups) // 2]
        digits = set((bk[(bk >> bits2) == mid] & ((1 << bits2) - 1)).tolist())
        assert digits == {0, (1 << bits2) // 2, (1 << bits2) - 1}


def test_tile_and_tail_cases():
    # (the 2^24-entry cases themselves are built by the GPU test only: here their geometry, from the counts)
    for m, tile in (((1 << 24) - 1, 16384), (1 << 24, 65536)):
        p = P.plan(1 << 21, m, weighted=True)
        assert (p.tile, p.low, p.hb, p.bits1, p.bits2) == (tile, 8, 13, 7, 6) and P.plan(1 << 21, m).tile == tile
    for tail in P.A_TAILS:
        for uniform in (False, True):
            c = P.tail_case(tail, "int32", uniform)
            p = P.case_plan(c)
            m = len(c.rows)
            assert p.tile == 16384 and p.low == 8 and m % p.tile == tail and m // p.tile == 2
            tw = P.twin_firsts(c)
            assert np.array_equal(tw, np.arange(0, m - 1, 2))  # every aligned pair, the odd tail's last entry alone
            assert P.expect_buckets(c) and P.is_uniform(c) == uniform
    assert any(t % 2 for t in P.A_TAILS)
    for shape in P.A_RECT:
        c = P.rect_case(*shape, "float64", False)
        assert (c.n_rows, c.n_cols) == shape and max(c.rows.max(), c.cols.max()) >= min(shape) and P.expect_buckets(c)
        assert U.scipy_sum(c).nnz < len(c.rows)
    assert P.case_plan(P.rect_case(300, 70000, "float64", False)).low == 7
    assert P.case_plan(P.rect_case(70000, 300, "float64", False)).hb == 9
    c = P.far_columns_case("float64", True)
    assert c.cols.min() >= c.n_rows and len(P.twin_firsts(c)) == 0 and P.expect_buckets(c)


@pytest.mark.parametrize("dtype", P.DTYPES)
def test_twins_sit_at_the_parities_named(dtype):
    for uniform in (False, True):
        for rect in (None, (700, 5000), (5000, 700)):
            c = P.twin_zoo(dtype, uniform, rect)
            p = P.case_plan(c)
            assert p.low == 8 and P.expect_buckets(c)
            marks = {m[0]: m for m in c.notes["marks"]}
            for label, at, firsts, entries in c.notes["marks"]:
                got = [(int(c.rows[at + k]), int(c.cols[at + k])) for k in range(len(entries))]
                assert got == [(r, q) for r, q, _v in entries], label
                for f in firsts:  # a twin that may pair: at an even offset, both rows in one bucket
                    assert f % 2 == 0 and (c.rows[f] >> 8) == (c.cols[f] >> 8), label
            assert P.twin_firsts(c).tolist() == P.expected_twin_firsts(c), (dtype, uniform, rect)
            assert marks["odd"][1] % 2 == 1 and marks["even"][1] % 2 == 0
            assert marks["aba-odd"][1] % 2 == 1 and marks["self-odd"][1] % 2 == 1
            a, b = marks["two-buckets"][3][0][:2]
            assert (a >> 8) != (b >> 8)
            a, b = marks["bucket-edge"][3][0][:2]
            assert b == a + 1 and (a >> 8) != (b >> 8)
            if rect is None:
                assert marks["thread-pair-edge"][1] == 2047 and marks["sub-tile-edge"][1] == 8191
                assert marks["sub-tile-last-pair"][1] == 8188 and marks["block-last-pair"][1] == p.tile - 4
                assert marks["block-edge"][1] == p.tile - 1 and marks["second-block"][1] == p.tile + 2
                b = P.B_ONLY_TWINS_BUCKET  # a bucket whose every entry is half of a paired twin
                stored, expanded = P.bucket_load(c)
                assert expanded[b] == 600 and stored[b] == 300
            else:
                assert c.rows.max() < c.n_rows and c.cols.max() < c.n_cols and c.n_rows != c.n_cols
    # the value rule: unequal values pair only where the cast makes them equal
    w = P.twin_zoo(dtype, False)
    marks = {m[0]: m for m in w.notes["marks"]}
    paired = set(P.twin_firsts(w).tolist())
    assert (marks["unequal"][1] in paired) == (dtype == "bool")
    assert (marks["equal-after-cast"][1] in paired) == (dtype == "bool")
    assert marks["true-false"][1] not in paired and marks["even"][1] in paired
    u = set(P.twin_firsts(P.twin_zoo(dtype, True)).tolist())
    assert {marks[k][1] for k in ("unequal", "equal-after-cast", "true-false", "unequal-sum-zero")} <= u


def test_mostly_twins_cases():
    for n_rows, hb, bits2 in (((1 << 18) + 1, 11, 5), (1 << 18, 10, 0)):
        c = P.mostly_twins_case(n_rows, "float64")
        p = P.case_plan(c)
        assert P.is_uniform(c) and (p.hb, p.bits2, p.low) == (hb, bits2, 8) and P.expect_buckets(c)
        assert len(P.twin_firsts(c)) > 0.85 * len(c.rows) / 2
        assert (c.rows >> 8).max() == p.n_bk - 1 and (c.rows >> 8).min() == 0
        assert len(np.unique((c.rows >> 8) >> bits2)) >= 4


@pytest.mark.parametrize("dtype", ["float64", "bool"])
def test_length_cases_hold_every_class(dtype):
    c = P.lengths_case(dtype, False)
    assert P.case_plan(c).low == 8 and P.expect_buckets(c) and P.expect_buckets(P.lengths_case(dtype, True))
    lens = _lens(c)
    seen = set()
    for row, L, order, rep in c.notes["layout"]:
        assert lens[row] == L
        seen.add((L, order, rep if rep < max(L, 1) or L <= 1 else "all"))
        cols = c.cols[c.rows == row]
        if L > 1 and order == "sorted":
            assert np.all(np.diff(cols) >= 0)
        if L > rep and order == "reversed":
            assert np.all(np.diff(cols) <= 0) and cols[0] > cols[-1]
        if L > 2 * rep and order == "organ":
            k = int(np.argmax(cols))
            assert 0 < k < L - 1 and np.all(np.diff(cols[:k + 1]) >= 0) and np.all(np.diff(cols[k:]) <= 0)
        if L:
            assert np.bincount(cols).max() == min(rep, L)
        if L > 57 and rep == 1:
            assert len(np.unique(cols)) == L  # distinct keys through every Shell gap below L
    assert {(L, o) for L, o, _r in seen} >= {(L, o) for L in P.C_LENGTHS for o in P.C_ORDERS}
    for rep in P.C_REPEATS:
        assert {L for L, _o, r in seen if r == rep} >= {L for L in P.C_LENGTHS if L > rep}
    assert {L for L, _o, r in seen if r == "all"} >= {L for L in P.C_LENGTHS if L > 17}
    # 17 | 65: the in-register / wave / lane boundaries; every Shell gap has a length on either side
    assert {P.IN_REG, P.IN_REG + 1, P.MID_ROW, P.MID_ROW + 1} <= set(P.C_LENGTHS)
    for gap in P.GAPS[:3]:
        assert gap in P.C_LENGTHS and gap + 1 in P.C_LENGTHS
    assert (lens == 0).sum() > 100 and lens.sum() == len(c.rows)
    if dtype != "bool":  # different values per copy of a column
        row = next(r for r, L, _o, rep in c.notes["layout"] if L == 702 and rep == 3)
        sel = c.rows == row
        first = c.cols[sel][0]
        assert len(set(c.vals[sel][c.cols[sel] == first].tolist())) > 1


def test_finish_cases_hold_every_class():
    c = P.finish_case("int32", False)
    assert P.case_plan(c).low == 8 and P.expect_buckets(c) and P.expect_buckets(P.finish_case("int32", True))
    lens = _lens(c)
    tops = []
    for w in range(8):  # buckets 0 and 1: the longest in-register row of each wave
        wl = lens[64 * w:64 * (w + 1)]
        inreg = wl[wl <= P.IN_REG]
        tops.append(int(inreg.max()))
        assert (wl == 0).sum() >= 16
    assert tops[:6] == P.C_WAVE_MAX and tops[6:] == [0, 0]
    assert all((lens[64 * w:64 * (w + 1)] > P.IN_REG).any() for w in (6, 7))
    b2 = lens[512:768]
    assert (b2 == 17).sum() == 240 and b2.sum() == 4080 and [int((b2[64 * w:64 * w + 64] == 17).sum()) for w in range(4)] == [60] * 4
    b3 = lens[768:1024]
    assert b3[255] == 17 and b3[:255].max() <= 6 and ((b3 > P.IN_REG) & (b3 <= P.MID_ROW)).sum() == 1
    b4 = lens[1024:1280]
    kinds = np.where(b4 > P.MID_ROW, 2, np.where(b4 > P.IN_REG, 1, 0))[:108]
    assert kinds.tolist() == [0, 1, 2] * 36 and b4.sum() <= P.SYM_CAP
    want = U.scipy_sum(c)
    assert want.indptr[1280] - want.indptr[1024] > 256  # merged entries: bits k >= 1 of the skip mask


def test_capacity_cases_are_exact():
    for kind, count in P.D_KINDS:
        for where in P.D_WHERE:
            for dtype, uniform in (("float64", False), ("bool", False), ("int8", True)):
                c = P.capacity_case(kind, count, where, dtype, uniform)
                assert P.case_plan(c).low == 8 and P.case_plan(c).n_bk == 4 and P.is_uniform(c) == uniform
                stored, expanded = P.bucket_load(c)
                b = c.notes["bucket"]
                assert b == {"first": 0, "last": 3, "alone": 1}[where]
                others = [k for k in range(4) if k != b]
                if where == "alone":
                    assert all(expanded[k] == 0 for k in others)
                else:
                    assert all(0 < expanded[k] <= 40 for k in others)
                if kind == "stored":
                    assert stored[b] == expanded[b] == count
                    fails = ["stored"] if count > P.SYM_CAP else []
                else:
                    assert stored[b] == count and expanded[b] == 2 * count
                    fails = ["expanded"] if 2 * count > P.SYM_CAP else []
                assert P.failed(c) == fails, c.name
                assert count in (P.SYM_CAP, P.SYM_CAP + 1, P.SYM_CAP // 2, P.SYM_CAP // 2 + 1)


def test_arith_cases_fail_the_condition_named():
    for kind, (dtypes, runs, fails) in P.E_KINDS.items():
        for dtype in dtypes:
            c = P.arith_case(kind, dtype)
            assert not P.is_uniform(c) and P.failed(c) == ([fails] if fails else []), (kind, dtype)
            lens = _lens(c)
            assert np.sort(lens)[-2] <= 16  # scipy sums in stream order (at most one longer row: one run)
            assert not U.differs_from_stable(c), (kind, dtype)
    want = U.scipy_sum(P.arith_case("int8-wrap", "int8"))
    assert {-128, 44, 127} <= set(want.data.tolist())           # 127 + 1; 300 x 1; -128 - 1
    want = U.scipy_sum(P.arith_case("int32-wrap", "int32"))
    assert {-2 ** 31, 2 ** 31 - 1, -2 ** 30, -4} <= set(want.data.tolist())
    want = U.scipy_sum(P.arith_case("bool-mixed", "bool"))
    assert (~want.data).sum() == 2 and want.data.sum() >= 4        # explicit False entries kept
    for dtype in ("float64", "int8"):
        want = U.scipy_sum(P.arith_case("zero-sums", dtype))
        assert (want.data == 0).sum() == 5                         # sums of 0 stay as explicit zeros
    want = U.scipy_sum(P.arith_case("f32-2^24-1-1", "float32"))
    assert 16777216.0 in want.data and 16777218.0 not in want.data
    c = P.arith_case("f32-cancelling", "float32")
    assert 1.0 in U.scipy_sum(c).data and P.run_magnitudes(c).max() == 2 ** 25 + 1
    assert P.run_magnitudes(P.arith_case("f32-edge-stay", "float32")).max() == 2 ** 24 - 1
    assert np.float32(P.I31) == np.float32(2.0 ** 31)


@pytest.mark.parametrize("uniform", [False, True])
def test_gfa_cases_stay_on_the_partition(uniform):
    """The doubled COO of every F case keeps the premise (its buckets hold the transposes too), every
    entry's twin follows it at an even offset, and the RC:i rendering spells the values."""
    for c in P.gfa_cases("int8", uniform):
        assert c.n_rows == c.n_cols
        d = P.doubled(c)
        assert len(d.rows) == 2 * len(c.rows) and P.case_plan(d).low == 8 and P.expect_buckets(d), c.name
        tw = P.twin_firsts(d)
        same = (c.rows >> 8) == (c.cols >> 8)
        assert np.array_equal(tw, 2 * np.flatnonzero(same)), c.name
    c = P.twin_zoo("int8", uniform, short=True)
    text = P.render_gfa_int(c)
    assert text.count(b"\nL\t") == len(c.rows) and text.count(b"S\t") == c.n_rows
    assert (b"RC:i:" in text) == (not uniform) and b"RC:f" not in text
    if not uniform:
        assert text.count(b"\tRC:i:-3\n") == int((c.vals == -3).sum()) > 0
