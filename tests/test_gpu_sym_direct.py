"""GPU: the MAX-SYM bucket finish in place (g2n_sym.hip: k_sym_count gives every bucket its entry
count, one scan its CSR offset, k_sym_finish writes indices, data and indptr where they belong)
against the oracle, the classic row-sum path (TEST_NO_BUCKETS) and the staged finish
(TEST_NO_DIRECT_FINISH), byte for byte, with the route asserted.

A bucket is 2^low <= 256 consecutive rows (ids 256 k + 1 .. 256 k + 256 at low = 8).  A link inside
one bucket is a pair word, counted through a bit map of its key; one that leaves it is an 8-byte
element in each of its two buckets, counted as a distinct (row, column).  The count pass declines —
the staged route then runs — when a bucket holds more than 256 of those, or the build holds more of
them than pair words; int8 (whose wrapping sums can drop a cell) never takes it.  A count that
differed from the finish's own would drop the bucket partition altogether (sum_buckets false).
"""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIN = 256  # kFinTPB: rows of a bucket at low 8, and the stream-B elements a counted bucket may hold
DIRECT_DTYPES = ("bool", "int32", "float32", "float64")


def _build(nat, data, dtype, flags=0):
    return nat.build_from_buffer(data, nat.make_options(test_flags=flags, output=nat.OUT_PARSE, dtype=dtype))


def _check(nat, oracle_lib, data, direct, dtypes=("float64",), classic=True):
    for dtype in dtypes:
        raw = _build(nat, data, dtype)
        o = oracle_lib.run(data, dtype=dtype)
        assert raw.status == o.status == 0, dtype
        # the bucket partition took it (a count that differed from the finish's would have dropped it)
        assert raw.format == "csr" and raw.sum_buckets and "sum_t" not in raw.phase_ms, (dtype, sorted(raw.phase_ms))
        assert raw.sym_direct == (direct and dtype != "int8"), (dtype, direct)
        R = oracle_lib.to_raw(o, "parse")
        assert raw.indptr.dtype == np.int32 and raw.indptr.tobytes() == R.indptr.tobytes(), dtype
        assert raw.indices.tobytes() == R.indices.tobytes(), dtype
        assert raw.data.tobytes() == R.data.tobytes(), dtype
        for flags in (nat.TEST_NO_DIRECT_FINISH,) + ((nat.TEST_NO_BUCKETS,) if classic else ()):
            c = _build(nat, data, dtype, flags)
            assert c.status == 0 and not c.sym_direct, (dtype, flags)
            assert c.sum_buckets == (flags == nat.TEST_NO_DIRECT_FINISH), (dtype, flags)
            assert c.indptr.tobytes() == raw.indptr.tobytes(), (dtype, flags)
            assert c.indices.tobytes() == raw.indices.tobytes() and c.data.tobytes() == raw.data.tobytes(), (dtype, flags)


def _s(n):
    return [f"S\t{k}\t*\n" for k in range(1, n + 1)]


def _l(a, b, times=1):
    return [f"L\t{a}\t+\t{b}\t+\t0M\n"] * times


def _local(r, lo, hi, n_l):
    """n_l links a -> a + 1..3 inside [lo, hi], both ids in one aligned group of 16 (so in one bucket at
    every low >= 4)"""
    out = []
    while len(out) < n_l:
        a = r.randint(lo, hi)
        b = a + r.randint(1, 3)
        if (a - 1) >> 4 == (b - 1) >> 4 and b <= hi:
            out += _l(a, b)
    return out


def _gfa(n, links, r=None):
    if r:
        r.shuffle(links)
    return "".join(_s(n) + links).encode()


@pytest.mark.parametrize("k", [0, 1, FIN - 1, FIN, FIN + 1])
def test_links_that_leave_one_bucket(gpu, oracle_lib, k):
    """bucket 1 (ids 257..512) with k links to rows of buckets 4..15, beside pair-only buckets: the
    count pass takes k <= 256 and declines 257"""
    r = random.Random(40 + k)
    links = _local(r, 1, 4096, 6000)
    for i in range(k):  # distinct cells, the targets spread (no other bucket near the bound)
        links += _l(257 + (i * 7) % 256, 1025 + (i * 37) % 3072)
    _check(gpu, oracle_lib, _gfa(4096, links, r), direct=k <= FIN)


REPEATS = (1, 2, 3, 300)


@pytest.mark.parametrize("leave,times", [(False, REPEATS), (True, (1, 2, 3, 100)), (True, REPEATS)])
def test_repeated_links_and_their_reverse(gpu, oracle_lib, leave, times):
    """a link repeated, its reverse present fewer times, equally often, more often and absent: inside one
    bucket (pair words: one key, copies in the value) and across two (both sides of one cell).  300
    copies across buckets are more elements than a counted bucket holds: declined"""
    r = random.Random(50)
    links = _local(r, 1, 8192, 8000)
    a = 20
    for t in times:
        for rev in (max(t - 1, 0), t, t + 1, 0):
            b = a + 4000 if leave else a + 5
            links += _l(a, b, t) + _l(b, a, rev)
            a += 256  # each in a bucket of its own
    _check(gpu, oracle_lib, _gfa(8192, links, r), direct=not (leave and max(times) > FIN // 2),
           dtypes=("float64", "int32"))


@pytest.mark.parametrize("n,others", [(1, 0), (40, 0), (2000, 3000)])
def test_self_loops(gpu, oracle_lib, n, others):
    r = random.Random(60 + n)
    links = _l(1, 1)  # alone
    if n > 1:
        links += _l(7, 7, 5) + _l(n, n, 2) + _l(8, 8) + _l(8, 9) + _l(9, 8, 2)
    if others:
        links += _local(r, 1, n, others) + _l(300, 300, 300)
    _check(gpu, oracle_lib, _gfa(n, links, r), direct=True, dtypes=("float64", "bool"))


SHAPES = (16, 17, 64, 65, 300)  # short rows (LDS-staged), wave-sorted rows, lane-sorted rows


def _row_shapes_gfa(doubled):
    """Two buckets (ids 257..512 and 513..768), each with rows of SHAPES elements (in-bucket neighbours
    first, the 300's rest outside) and 1- and 2-entry rows between them; the second bucket starts with
    one more entry, so that every shape's first entry falls on an even and on an odd bucket offset.
    doubled: one neighbour of each shaped row twice instead of another (the same elements, an entry of
    two copies)."""
    lines, special = [], {}
    for q, base in enumerate((257, 513)):
        rows = {base + 10 + 45 * i: k for i, k in enumerate(SHAPES)}  # ids of the shaped rows
        others = [c for c in range(base, base + 256) if c not in rows]
        for a, k in rows.items():
            # neighbours above the shaped rows only, so that no shaped row's offset depends on them
            pool = [c for c in others if c > base + 200] + [c for c in others if c <= base + 200][::-1]
            nb = pool[:k] if k <= len(pool) else pool + list(range(800, 800 + k - len(pool)))
            if doubled:
                nb = nb[1:] + [nb[k // 2]]
            lines += [ln for c in nb for ln in _l(a, c)]
            special[a] = k - 1 if doubled else k
        for c in others[1::7]:  # 1- and 2-entry rows between
            if c + 1 not in rows and c + 1 < base + 256:
                lines += _l(c, c + 1)
        if q:
            lines += _l(base, 900)  # one more entry ahead of the bucket's shaped rows
    return lines, special


@pytest.mark.parametrize("doubled", [False, True])
def test_row_shapes_straight_out(gpu, oracle_lib, doubled):
    """the mid and long rows' straight-out stores and the short rows' copy-out write the same final place:
    rows of 16, 17, 64, 65 and 300 elements, each at an odd and at an even offset of its bucket; doubled:
    with an entry of two copies in each (its value written apart from the copy-out's ones)"""
    lines, special = _row_shapes_gfa(doubled)
    data = _gfa(1024, lines)
    o = oracle_lib.run(data, dtype="float64")
    ip = o.ms_indptr
    parity = {}
    for a, k in special.items():
        row, first = a - 1, ((a - 1) >> 8) << 8
        assert ip[row + 1] - ip[row] == k, (a, k)  # the row has exactly its shape's entries
        parity.setdefault(k, set()).add(int(ip[row] - ip[first]) & 1)
    assert all(len(p) == 2 for p in parity.values()), parity  # (the input's own premise)
    _check(gpu, oracle_lib, data, direct=True, dtypes=("float64", "int32"))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100_003])
def test_sizes_and_empty_buckets(gpu, oracle_lib, n):
    """n not a multiple of the bucket (a partial last bucket holding the last row's links), and wholly
    empty buckets between full ones"""
    r = random.Random(70 + n)
    if n == 1:
        links = _l(1, 1, 3)
    elif n < 1000:
        links = _local(r, 1, n, 3 * n) + _l(n - 1, n) + _l(n, 1) + _l(1, n)
    else:
        links = []
        for k in range(0, n // 256 + 1, 3):  # every third bucket, the last (partial) one among them
            links += _local(r, 256 * k + 1, min(256 * k + 256, n), 600)
        assert n // 256 % 3 == 0
        links += _l(n - 1, n, 2) + _l(n, 5) + _l(n, n)
    _check(gpu, oracle_lib, _gfa(n, links, r), direct=True)


@pytest.mark.parametrize("n_s,n_l,low", [(100, 150, 7), (256, 4000, 6), (1000, 40_000, 4)])
def test_smaller_buckets(gpu, oracle_lib, n_s, n_l, low):
    """more than 8 elements per row shrink the bucket (low 6 and 4: smaller key maps); 100 S lines: low
    capped by the id bits (7).  Rows of 80 entries that merge to a few."""
    r = random.Random(n_s)
    links = _local(r, 1, n_s, n_l - 40)
    links += [ln for _ in range(20) for ln in _l(r.randint(1, n_s), r.randint(1, n_s))]
    links += _l(n_s // 2, n_s // 2 + 1, 7) + _l(n_s // 2 + 1, n_s // 2, 13)
    _check(gpu, oracle_lib, _gfa(n_s, links, r), direct=True, dtypes=("float64", "bool"))


@pytest.mark.parametrize("n_s", [50_000, 300_000])
@pytest.mark.parametrize("far", [False, True])
def test_one_and_two_partition_passes(gpu, oracle_lib, n_s, far):
    """one pass below 2^18 rows (pass 1's own 16-bit words), two above (pass 7's); no link leaves its
    bucket (counted) next to every link leaving it (declined as a whole)"""
    r = random.Random(n_s)
    if far:
        links = [ln for _ in range(60_000) for ln in _l(r.randint(1, n_s // 2), r.randint(n_s // 2 + 300, n_s))]
    else:
        links = _local(r, 1, n_s, 99_000) + _l(n_s - 1, n_s, 3)
    _check(gpu, oracle_lib, _gfa(n_s, links), direct=not far, classic=n_s < 100_000)


def test_dtypes_and_int8_staged(gpu, oracle_lib):
    """bool, int32, float32 and float64 in place; int8 (128 copies are -128, 256 are 0: a dropped cell)
    staged, with the same bytes as the oracle's"""
    r = random.Random(80)
    links = _local(r, 1, 4096, 6000)
    for i, k in enumerate((61, 127, 128, 255, 256, 300)):
        a = 100 + 256 * i
        links += _l(a, a + 1, k) + (_l(a + 1, a, k // 2 + 1) if i % 2 == 0 else [])
        links += _l(a + 9, a + 2000, k // 4) + _l(a + 2000, a + 9, 2)
    _check(gpu, oracle_lib, _gfa(4096, links, r), direct=True, dtypes=DIRECT_DTYPES + ("int8",))
