"""The bucket-partition CSR — the default route of coo.tocsr() on the device (csr_partition / csr_partition_w:
passes 4 / 2 / 7 into k_sym_finish<T, true> and k_sym_place, passes 5 / 6 into k_sumw_finish and
k_sumw_place) — against scipy at the constants it branches on.  tests/partition_util.py builds the cases and
restates the geometry; tests/test_partition_cases.py shows on the CPU that each case sits where it claims.
Every case goes through g2n_coo_to_csr with test_flags = 0 against coo_matrix(...).tocsr(): indptr, indices,
the data's bytes and the three dtypes; the result's own report must name the route the documented premise
gives (expect_buckets); and once more with TEST_NO_BUCKETS, to show both routes agree."""
import numpy as np
import pytest

import partition_util as P
import rowsum_util as U
from test_gpu_rowsum_edges import _same

pytestmark = pytest.mark.gpu

BOTH = [False, True]
IDS = ["weighted", "uniform"]


def _run(nat, case, want=None):
    want = U.scipy_sum(case) if want is None else want
    raw = nat.coo_to_csr(case.rows, case.cols, case.values, case.n_rows, case.n_cols, test_flags=0)
    assert raw.status == 0, case.name
    _same(raw, want, case.name)
    assert raw.sum_buckets == P.expect_buckets(case), (case.name, raw.sum_buckets, P.failed(case))
    assert "csr" in raw.phase_ms and "sum" in raw.phase_ms, (case.name, raw.phase_ms)
    del raw
    classic = nat.coo_to_csr(case.rows, case.cols, case.values, case.n_rows, case.n_cols,
                             test_flags=nat.TEST_NO_BUCKETS)
    assert classic.status == 0 and not classic.sum_buckets, case.name
    _same(classic, want, case.name + " (row sums)")
    return want


def _all(nat, builder, *args):
    """The weighted instance in every dtype and the uniform one."""
    for dtype in P.DTYPES:
        for uniform in BOTH:
            _run(nat, builder(*args, dtype, uniform))


# ---------------------------------------------------------------- A. geometry ------
@pytest.mark.parametrize("per_row,above", [(p, False) for p, _l in P.A_LOW] + [(p, True) for p in P.A_LOW_ABOVE])
def test_low_steps(gpu, per_row, above):
    """64 rows of 8 .. 1100 entries: low from 6 (the cap by bits) down to 1, buckets of 2 rows."""
    _all(gpu, P.low_case, per_row, above)


@pytest.mark.parametrize("n_rows", list(P.A_CAPPED))
def test_low_capped_by_bits(gpu, n_rows):
    _all(gpu, P.capped_case, n_rows)


@pytest.mark.parametrize("n_rows,last,empty", P.A_RAGGED)
def test_ragged_last_bucket(gpu, n_rows, last, empty):
    """n_rows = 256 k +- 1, the last row filled or empty, whole buckets empty at the start, in the middle
    and at the end: indptr[n_rows] comes from the block that owns row n_rows - 1."""
    _all(gpu, P.ragged_case, n_rows, last, empty)


def test_one_entry_and_none(gpu):
    _all(gpu, P.single_case)
    for dtype in P.DTYPES:
        _run(gpu, P.none_case(dtype))


@pytest.mark.parametrize("uniform", BOTH, ids=IDS)
@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("which", list(P.A_PASSES))
def test_pass_counts(gpu, which, dtype, uniform):
    """hb = 10 (one pass), 11 (6 + 5) and 16 (8 + 8): the first, a middle and the last bucket of the first, a
    middle and the last pass-1 group."""
    _run(gpu, P.passes_case(which, dtype, uniform))


@pytest.mark.parametrize("uniform", BOTH, ids=IDS)
@pytest.mark.parametrize("m", [(1 << 24) - 1, 1 << 24])
def test_quarter_and_full_tile(gpu, m, uniform):
    """2^24 - 1 entries: the last count on the quarter tile; 2^24: the full tile (float64 only)."""
    _run(gpu, P.tile_case(m, uniform))


@pytest.mark.parametrize("tail", P.A_TAILS)
def test_last_block_counts(gpu, tail):
    """A last partition block of 1, 2, 8191, 8192 and 8193 entries, an odd one cutting a twin in two."""
    _all(gpu, P.tail_case, tail)


@pytest.mark.parametrize("shape", P.A_RECT)
def test_rectangular(gpu, shape):
    _all(gpu, P.rect_case, *shape)


def test_columns_past_the_rows(gpu):
    _all(gpu, P.far_columns_case)


# ---------------------------------------------------------------- B. twins ------
@pytest.mark.parametrize("uniform", BOTH, ids=IDS)
@pytest.mark.parametrize("dtype", P.DTYPES)
@pytest.mark.parametrize("rect", [None, (700, 5000), (5000, 700)], ids=["square", "wide", "tall"])
def test_twins(gpu, rect, dtype, uniform):
    """(a, b), (b, a) at even and odd offsets, across a thread's pair, a sub-tile and a block edge, in
    threes, as self-loops, in two buckets, of equal and unequal value and of values equal after the cast; a
    bucket of twins only."""
    _run(gpu, P.twin_zoo(dtype, uniform, rect))


@pytest.mark.parametrize("n_rows", [(1 << 18) + 1, 1 << 18], ids=["pass7", "single-pass"])
def test_mostly_twins_pair_words(gpu, n_rows):
    """The pair words through pass 7 (16 bits wide into F1) and as the single pass's own 16-bit words."""
    for dtype in P.DTYPES:
        _run(gpu, P.mostly_twins_case(n_rows, dtype))
    _run(gpu, P.mostly_twins_case(n_rows, "int32", uniform=False))


# ---------------------------------------------------------------- C. row shapes ------
@pytest.mark.parametrize("uniform", BOTH, ids=IDS)
@pytest.mark.parametrize("dtype", P.DTYPES)
def test_row_lengths(gpu, dtype, uniform):
    """Rows of 0 .. 4096 entries — the networks, the wave sort, the Shell sort on either side of every gap —
    sorted, reversed, shuffled and organ-pipe, columns repeated 1 / 2 / 3 / 17 times and all equal."""
    _run(gpu, P.lengths_case(dtype, uniform))


@pytest.mark.parametrize("uniform", BOTH, ids=IDS)
@pytest.mark.parametrize("dtype", P.DTYPES)
def test_finish_blocks(gpu, dtype, uniform):
    """The wave's choice of network at 1, 4, 5, 8, 9 and 16; a bucket of 240 mid rows; one mid row in the
    last lane of the last wave; in-register, mid and long rows interleaved past 256 staged entries."""
    _run(gpu, P.finish_case(dtype, uniform))


# ---------------------------------------------------------------- D. capacity ------
@pytest.mark.parametrize("where", P.D_WHERE)
@pytest.mark.parametrize("kind,count", P.D_KINDS)
def test_bucket_capacity(gpu, kind, count, where):
    """kSymCap = 4096 stored elements stay, 4097 decline; 2048 aligned twins stay, 2049 decline (4098
    entries once expanded): still scipy's CSR, by the row sums."""
    for dtype in P.DTYPES:
        for uniform in BOTH:
            case = P.capacity_case(kind, count, where, dtype, uniform)
            assert P.expect_buckets(case) == (count in (P.SYM_CAP, P.SYM_CAP // 2)), case.name
            _run(gpu, case)


# ---------------------------------------------------------------- E. the premise and its arithmetic ------
@pytest.mark.parametrize("kind", list(P.E_KINDS))
def test_weighted_premise(gpu, kind):
    """Integer sums that wrap, bool runs, sums of zero kept, floats at the edge of the exact-int32 rule and
    of the float32 run bound, and each value that must send the call to the row sums."""
    dtypes, _runs, fails = P.E_KINDS[kind]
    for dtype in dtypes:
        case = P.arith_case(kind, dtype)
        assert P.expect_buckets(case) == (fails is None), case.name
        _run(gpu, case)


# ---------------------------------------------------------------- F. the group-slot source ------
@pytest.mark.parametrize("tag", [False, True], ids=["untagged", "RC:i"])
@pytest.mark.parametrize("dtype", P.DTYPES)
def test_group_slot_source(gpu, dtype, tag):
    """The square cases as decimal-id GFAs, S lines first, built with directed=False into a CSR: passes 4 / 5
    read the parse's group slots, one block per slot, every L line an aligned twin."""
    for case in P.gfa_cases(dtype, not tag):
        data = P.render_gfa_int(case)
        twice = P.doubled(case)
        want = U.scipy_sum(twice)
        for flags in (0, gpu.TEST_NO_BUCKETS):
            raw = gpu.build_from_buffer(data, gpu.make_options(directed=False, output=gpu.OUT_CSR, dtype=dtype,
                                                               weight_tag="RC" if tag else None, test_flags=flags))
            assert raw.status == 0, (case.name, raw.message)
            assert raw.n_nodes == case.n_rows, case.name
            _same(raw, want, f"{case.name} flags={flags}")
            assert raw.sum_buckets == (flags == 0 and P.expect_buckets(twice)), (case.name, flags, raw.sum_buckets)
