"""GPU: the bucket finish (g2n_sym.hip: 16-bit pair words from the last partition pass into
k_sym_finish, its staged entries into k_sym_place) against the oracle and against the classic
row-sum path (TEST_NO_BUCKETS), byte for byte.

A bucket is 2^low <= 256 consecutive rows (ids 256 k + 1 .. 256 k + 256 at low = 8).  A link inside
one bucket travels as a pair word (16 bits into the finish), one that leaves it as 8-byte elements.
The cases are the ones a narrower word or staged entry can get wrong: copy counts up to 300 of one
entry (int8 wraps), links that leave a bucket of mostly pair words (to its neighbours' edge rows, to
id 1 and id N), buckets of mostly pair words and of mostly 8-byte elements in one build (and through
the int64 placement), rows of every finish path (16, 17, 64, 65 and 300 entries) at odd and even
offsets, smaller buckets (low 7, 6 and 4), and one and two partition passes (the pair words of a
single pass are pass 1's own, those of two come from pass 7).
"""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ("bool", "int8", "int32", "float32", "float64")
# default flags: A.maximum(A.T) (the MAX-SYM finish); directed=False as a CSR: coo.tocsr (the SUM finish,
# explicit zeros kept)
MODES = (("parse", {}), ("csr", {"directed": False}))


def _check(nat, oracle_lib, data, dtypes=DTYPES, flags=0, classic=True):
    for out, mode in MODES:
        for dtype in dtypes:
            opt = dict(output=nat.OUT_CSR if out == "csr" else nat.OUT_PARSE, dtype=dtype, **mode)
            raw = nat.build_from_buffer(data, nat.make_options(test_flags=flags, **opt))
            o = oracle_lib.run(data, dtype=dtype, **mode)
            assert raw.status == o.status == 0, (out, dtype)
            assert raw.format == "csr", (out, dtype)
            if out == "parse":  # the bucket partition took it: the classic path has a transposed sum
                assert "sum_t" not in raw.phase_ms, (dtype, sorted(raw.phase_ms))
            R = oracle_lib.to_raw(o, out)
            if flags & nat.TEST_INDEX64:
                assert raw.indptr.dtype == np.int64 and raw.indices.dtype == np.int64, (out, dtype)
                assert np.array_equal(raw.indptr, R.indptr) and np.array_equal(raw.indices, R.indices), (out, dtype)
            else:
                assert raw.indptr.tobytes() == R.indptr.tobytes(), (out, dtype)
                assert raw.indices.tobytes() == R.indices.tobytes(), (out, dtype)
            assert raw.data.tobytes() == R.data.tobytes(), (out, dtype)
            if classic:
                c = nat.build_from_buffer(data, nat.make_options(test_flags=nat.TEST_NO_BUCKETS, **opt))
                assert c.status == 0 and c.indptr.tobytes() == raw.indptr.tobytes(), (out, dtype)
                assert c.indices.tobytes() == raw.indices.tobytes() and c.data.tobytes() == raw.data.tobytes(), (out, dtype)


def _s(n):
    return [f"S\t{k}\t*\n" for k in range(1, n + 1)]


def _l(a, b, times=1):
    return [f"L\t{a}\t+\t{b}\t+\t0M\n"] * times


def _local(r, lo, hi, n_l):
    """n_l links a -> a + 1..3 with both ids in [lo, hi]"""
    out = []
    for _ in range(n_l):
        a = r.randint(lo, hi - 3)
        out += _l(a, a + r.randint(1, 3))
    return out


RUNS = (61, 62, 63, 64, 127, 128, 255, 256, 300)


def _runs(first):
    """one link repeated RUNS[i] times at id first + 200 i, every other one with its reverse repeated less
    often (so the maximum picks a side; int8: 128 copies are -128, 256 are 0)"""
    out = []
    for i, k in enumerate(RUNS):
        a = first + 200 * i
        out += _l(a, a + 1, k)
        if i % 2 == 0:
            out += _l(a + 1, a, k // 2 + 1)
        if i % 3 == 1:
            out += _l(a + 1, a, k + 1)  # the reverse wins
    return out


def test_copy_counts_around_the_inline_limit(gpu, oracle_lib):
    r = random.Random(31)
    links = _local(r, 1, 2000, 4000) + _runs(100)
    r.shuffle(links)
    _check(gpu, oracle_lib, "".join(_s(2000) + links).encode())


def test_escapes_inside_compact_buckets(gpu, oracle_lib):
    n = 2000
    r = random.Random(32)
    lines = _local(r, 1, n, 6000)
    for k in range(0, n // 256 + 1):
        first, last = 256 * k + 1, min(256 * k + 256, n)  # the bucket's first and last row
        for a in (first, last, first + 77):
            for b in (first - 1, last + 1, 1, n):  # bucket base - 1, bucket end, id 1, id N
                if 1 <= b <= n:
                    lines += _l(a, b)
        lines += _l(first + 5, (first + 1000) % n + 1) + _l((first + 1300) % n + 1, last - 5)
    lines += _l(300, 1900, 70)  # an escape whose count is in tcn
    lines += _l(1900, 300, 3)
    r.shuffle(lines)
    _check(gpu, oracle_lib, "".join(_s(n) + lines).encode())


@pytest.mark.parametrize("index64", [False, True])
def test_compact_and_wide_buckets_in_one_build(gpu, oracle_lib, index64):
    r = random.Random(33)
    lines = _local(r, 1, 2000, 4000) + _runs(100)
    lines += [ln for _ in range(4000) for ln in _l(r.randint(2001, 4000), r.randint(2001, 4000))]  # wide buckets
    lines += _l(2500, 3900, 80) + _l(3900, 2500, 2)
    r.shuffle(lines)
    data = "".join(_s(4000) + lines).encode()
    if index64:  # the int64 placement decodes both forms too (the classic path has no int64 twin to compare)
        _check(gpu, oracle_lib, data, flags=gpu.TEST_INDEX64, classic=False)
    else:
        _check(gpu, oracle_lib, data)


SHAPES = (16, 17, 64, 65, 300)  # short row (LDS-staged), wave-sorted rows, lane-sorted rows


def _row_shapes_gfa():
    """Two buckets (ids 257..512 and 513..768), each with rows of SHAPES distinct neighbours (in-bucket
    ones first, the 300's rest outside) and 1- and 2-entry rows between them; the second bucket starts
    with one more entry, so that every shape's first entry falls on an even and on an odd bucket offset."""
    lines, special = _s(1024), {}
    for q, base in enumerate((257, 513)):
        rows = {base + 10 + 45 * i: k for i, k in enumerate(SHAPES)}  # ids of the shaped rows
        others = [c for c in range(base, base + 256) if c not in rows]
        for a, k in rows.items():
            # neighbours above the shaped rows only, so that no shaped row's offset depends on them
            pool = [c for c in others if c > base + 200] + [c for c in others if c <= base + 200][::-1]
            nb = pool[:k] if k <= len(pool) else pool + list(range(800, 800 + k - len(pool)))
            lines += [ln for c in nb for ln in _l(a, c)]
            special[a] = k
        for c in others[1::7]:  # 1- and 2-entry rows between
            if c + 1 not in rows and c + 1 < base + 256:
                lines += _l(c, c + 1)
        if q:
            lines += _l(base, 900)  # one more entry ahead of the bucket's shaped rows
    return "".join(lines).encode(), special


def test_row_shapes_beside_packed_stores(gpu, oracle_lib):
    data, special = _row_shapes_gfa()
    o = oracle_lib.run(data, dtype="float64")
    ip = o.ms_indptr
    parity = {}
    for a, k in special.items():
        row, first = a - 1, ((a - 1) >> 8) << 8
        assert ip[row + 1] - ip[row] == k, (a, k)  # the row has exactly its shape's entries
        parity.setdefault(k, set()).add(int(ip[row] - ip[first]) & 1)
    assert all(parity[k] == {0, 1} for k in SHAPES), parity  # (the input's own premise)
    _check(gpu, oracle_lib, data)


@pytest.mark.parametrize("n_s,n_l", [(256, 4000), (1000, 40000), (100, 150)])
def test_smaller_buckets(gpu, oracle_lib, n_s, n_l):
    """per_row above 8 shrinks the bucket (low 6 and 4); 100 S lines: low capped by the id bits (7)"""
    r = random.Random(n_s)
    lines = _local(r, 1, n_s, n_l - n_l // 20)
    lines += [ln for _ in range(n_l // 20) for ln in _l(r.randint(1, n_s), r.randint(1, n_s))]
    lines += _l(n_s // 2, n_s // 2 + 1, 64) + _l(n_s // 2 + 1, n_s // 2, 130)
    r.shuffle(lines)
    _check(gpu, oracle_lib, "".join(_s(n_s) + lines).encode())


@pytest.mark.parametrize("n_s,n_l,far", [(50_000, 200_000, False), (50_000, 200_000, True),
                                         (300_000, 1_200_000, False)])
def test_one_and_two_partition_passes(gpu, oracle_lib, n_s, n_l, far):
    """one pass below 2^18 rows, two (a pass over the pair words) above; far_links: wide buckets"""
    from gfa2network_amd import synth

    _check(gpu, oracle_lib, synth.host_bytes(n_s, n_l, seed=5, far_links=far), dtypes=("float64", "int8"))
