"""The row-sum CSR path (TEST_NO_BUCKETS: k_pack, the stable LSD radix sort, k_row_bounds / k_row_start,
k_row_finish (Count / Sum<T>) with its register networks and merge sort, k_row_emulate over stl_sort.h, k_row_compact,
k_row_max) against scipy at the constants its kernels branch on (tests/rowsum_util.py builds the cases,
tests/test_rowsum_cases.py shows on the CPU that they sit where they claim).  SUM: g2n_coo_to_csr on the
arrays against coo.tocsr(); MAX-SYM: the COO as a GFA with RC:f weights against A.maximum(A.T).  indptr,
indices, the data's bytes and the dtypes; the result's own report must name the row-sum path."""
import numpy as np
import pytest

import rowsum_util as U

pytestmark = pytest.mark.gpu


def _same(raw, want, what):
    assert raw.format == "csr", what
    assert raw.indptr.dtype == want.indptr.dtype and raw.indices.dtype == want.indices.dtype, what
    assert raw.data.dtype == want.data.dtype, (what, raw.data.dtype, want.data.dtype)
    assert np.array_equal(raw.indptr, want.indptr), what
    assert np.array_equal(raw.indices, want.indices), what
    if raw.data.tobytes() != want.data.tobytes():
        bad = np.flatnonzero(raw.data.view(np.uint8).reshape(len(raw.data), -1)
                             != want.data.view(np.uint8).reshape(len(want.data), -1))
        k = int(bad[0]) // want.data.dtype.itemsize
        row = int(np.searchsorted(want.indptr, k, side="right")) - 1
        raise AssertionError(f"{what}: data differs at entry {k} (row {row}, column {int(want.indices[k])}): "
                             f"{raw.data[k]!r} != {want.data[k]!r}; {len(bad)} bytes differ")


def _sum(nat, case, want=None):
    raw = nat.coo_to_csr(case.rows, case.cols, case.values, case.n_rows, case.n_cols,
                         test_flags=nat.TEST_NO_BUCKETS)
    assert raw.status == 0 and not raw.sum_buckets, case.name
    assert "sum" in raw.phase_ms and "csr" in raw.phase_ms, (case.name, raw.phase_ms)
    _same(raw, U.scipy_sum(case) if want is None else want, case.name)
    return raw


def _maxsym(nat, case, floats="values"):
    if isinstance(floats, str):
        floats = U.text_floats(case)
    data = U.render_gfa(case, floats)
    raw = nat.build_from_buffer(data, nat.make_options(weight_tag=None if floats is None else "RC", dtype=case.dtype,
                                                       test_flags=nat.TEST_NO_BUCKETS))
    assert raw.status == 0, (case.name, raw.message)
    assert not raw.sum_buckets and raw.n_nodes == case.n_rows and raw.n_edges == len(case.rows), case.name
    assert {"sum", "sum_t", "maxsym"} <= set(raw.phase_ms), (case.name, raw.phase_ms)
    _same(raw, U.scipy_maxsym(case, floats), case.name + " maxsym")
    return raw


# ---------------------------------------------------------------- A. sort geometry ------
@pytest.mark.parametrize("n_rows,m", U.A_PAIRS)
def test_sort_geometry(gpu, n_rows, m):
    """1, 2 and 3 passes at digit widths 1 to 8, entry counts around the wave step, the wave's 1024 items
    and the 4096-item tile: rows of at most 16 entries, so a float64 sum that differs is an unstable sort,
    indices that differ a lost or misrouted item.  Weighted and uniform instance."""
    for uniform in (False, True):
        _sum(gpu, U.sort_case(n_rows, m, uniform))


@pytest.mark.parametrize("n_rows,m", U.A_HUGE)
def test_sort_geometry_wide_keys(gpu, n_rows, m):
    """2^24 rows: 3 passes of 8 bits; 2^24 + 1: 4 passes of 7, 6, 6, 6 (the other ping-pong parity)."""
    for uniform in (False, True):
        _sum(gpu, U.sort_case(n_rows, m, uniform))


@pytest.mark.parametrize("shape", [(300, 70000), (70000, 300)])
def test_sort_geometry_rectangular(gpu, monkeypatch, shape):
    """The pass count follows the sorted dimension: 300 x 70000 sorts 9 bits for the CSR and 17 for the
    CSC, 70000 x 300 the reverse; through coo_to_csr and convert_format(A, "csc")."""
    import scipy.sparse as sp

    from gfa2network_amd import convert_format

    monkeypatch.setattr(gpu, "TEST_FLAGS", gpu.TEST_NO_BUCKETS)
    for uniform in (False, True):
        case = U.rect_case(*shape, uniform)
        _sum(gpu, case)
        A = sp.coo_matrix((case.values, (case.rows, case.cols)), shape=shape)
        for fmt in ("csr", "csc"):
            C, W = convert_format(A, fmt), A.asformat(fmt)
            assert C.format == fmt and C.shape == W.shape and C.dtype == W.dtype
            assert C.indptr.dtype == W.indptr.dtype and C.indices.dtype == W.indices.dtype
            assert np.array_equal(C.indptr, W.indptr) and np.array_equal(C.indices, W.indices), (shape, fmt)
            assert C.data.tobytes() == W.data.tobytes(), (shape, fmt, uniform)


# ---------------------------------------------------------------- B. row bounds ------
@pytest.mark.parametrize("where,gap", U.B_GAPS)
def test_row_gaps(gpu, where, gap):
    """k_row_bounds fills gaps up to kRowGapCap = 64 itself; 65 (and 10^5) hand start[] to k_row_start."""
    for dtype in U.DTYPES:
        for uniform in (False, True):
            _sum(gpu, U.gap_case(where, gap, dtype, uniform))


@pytest.mark.parametrize("n", [0, 1, 64, 65, 1000])
def test_no_entries(gpu, n):
    """nnz = 0: n_rows + 1 zeros (one gap of n_rows + 1 rows: filled at 63, searched from 64), and 0 x 0."""
    for dtype in U.DTYPES:
        raw = _sum(gpu, U.empty_case(n, n, dtype))
        assert len(raw.indptr) == n + 1 and len(raw.indices) == 0 and len(raw.data) == 0
    if n:
        _sum(gpu, U.empty_case(n, 7, "float64"))


# ---------------------------------------------------------------- C. row length classes ------
@pytest.mark.parametrize("uniform", [False, True], ids=["weighted", "uniform"])
@pytest.mark.parametrize("dtype", U.DTYPES)
def test_row_lengths_sum(gpu, dtype, uniform):
    """Rows of 0 .. 5000 entries (the len == 1 shortcut, the 8- and 16-slot networks, the merge sort), in
    column order, reversed and shuffled, columns repeated up to 17 (int8: 256) times."""
    _sum(gpu, U.length_case(dtype, uniform))


@pytest.mark.parametrize("uniform", [False, True], ids=["weighted", "uniform"])
@pytest.mark.parametrize("dtype", U.DTYPES)
def test_row_lengths_maxsym(gpu, dtype, uniform):
    _maxsym(gpu, U.length_case(dtype, uniform))


@pytest.mark.parametrize("dtype", U.FLOATS)
def test_twin_rows_16_and_17(gpu, dtype):
    """kRegRow = 16 = libstdc++'s _S_threshold: the same pairs summed stably in the 16-entry row and in
    std::sort's order in the 17-entry row."""
    _sum(gpu, U.twin_case(dtype))


# ---------------------------------------------------------------- D. staging thresholds ------
@pytest.mark.parametrize("tail", [1, 255])
@pytest.mark.parametrize("cap,uniform", [(4096, True), (2048, True), (2048, False), (1024, False)],
                         ids=["sum-u4096", "compact-u2048", "sum-w2048", "compact-w1024"])
def test_staging_caps_sum(gpu, cap, uniform, tail):
    """256-row blocks holding cap - 1, cap and cap + 1 entries, staged beside direct, a ragged last block:
    k_row_finish's caps (4096 uniform, 2048 weighted) and k_row_compact's (2048, 1024)."""
    for dtype in U.DTYPES:
        _sum(gpu, U.staging_case(cap, tail, dtype, uniform))


@pytest.mark.parametrize("cap,uniform", [(2048, True), (1024, False)], ids=["uniform", "weighted"])
def test_staging_caps_row_max(gpu, cap, uniform):
    """k_row_max's three staging conditions, each failing alone: the A segment, the A.T segment, the
    merged output."""
    for dtype in U.DTYPES:
        _maxsym(gpu, U.rowmax_case(cap, dtype, uniform))


# ---------------------------------------------------------------- E. summation order ------
@pytest.mark.parametrize("dtype", U.FLOATS)
@pytest.mark.parametrize("layout", U.E_LAYOUTS)
@pytest.mark.parametrize("kind", list(U.E_KINDS))
def test_summation_order(gpu, kind, layout, dtype):
    """Rows of 17, 18, 33 and 100 entries: runs the flag rule must leave alone (2 copies; integral with
    sum |x| = limit - 1) and runs it must hand to the std::sort emulation (fractional, {limit, 1, 1},
    {big, 1, 1, -big}, inf / NaN) — in unsorted rows, in sorted rows of an unsorted matrix, and in a sorted
    matrix, where scipy sorts nothing."""
    case = U.order_case(kind, dtype, layout)
    raw = _sum(gpu, case)
    assert raw.sum_sorted == (layout == "all_sorted")
    _maxsym(gpu, case)


@pytest.mark.parametrize("dtype", U.FLOATS)
def test_heapsort_fallback_rows(gpu, dtype):
    """Median-of-3 killer and organ-pipe rows of 64 .. 4096 entries: the device's introsort must fall back
    to heap sort exactly where libstdc++ does for the sums to come out."""
    _sum(gpu, U.fallback_case(dtype))


@pytest.mark.parametrize("dtype", U.FLOATS)
def test_nan_pairs_follow_sort_order(gpu, dtype):
    """Two NaNs of different payloads on one column of a long unsorted row: the payload kept is the first
    operand's in std::sort's order."""
    _sum(gpu, U.nan_order_case(dtype))


# ---------------------------------------------------------------- F. arithmetic ------
@pytest.mark.parametrize("sorted_matrix", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("dtype", U.FLOATS)
def test_arithmetic_sum(gpu, dtype, sorted_matrix):
    """Quiet and signalling NaNs with payloads as either operand, NaN + NaN, inf + -inf (the default NaN,
    sign set), the signed zeros, runs that cancel (kept)."""
    _sum(gpu, U.arith_case(dtype, sorted_matrix))


@pytest.mark.parametrize("dtype", U.DTYPES)
def test_arithmetic_maxsym(gpu, dtype):
    """std::max's operand order on nan, -0.0 against 0.0, negatives against a missing entry and sums of
    zero (dropped), int8 -128, int32 wrap, bool."""
    case, floats = U.maxsym_arith(dtype)
    _maxsym(gpu, case, floats)
