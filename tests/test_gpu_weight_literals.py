"""Weight-tag literals on the device against CPython's int() / float() (tests/literal_util.py).

A weighted build turns "<tag>:i:..." / "<tag>:f:..." bytes into a float64 on the GPU through four routes:
weight_fast in the full parse (fast_int / fast_float: the one place where the device's own fp64 multiply
or divide decides a bit), k_weights_slow (the Decimal path of pylit.h compiled for gfx950), lean_int_tag
in the extended tile-local lean parse (with its exact-int32 codes for the weighted SUM CSR), and
k_parse_deferred for lines that run past a tile's staged window.  Cast<T> / k_values then apply numpy's
cast.  Here every corpus literal goes through every route: float64 is compared with CPython's own value
bit for bit, the other dtypes (and every whole outcome: warnings, errors, node list) with the oracle.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import literal_util as LU
from test_gpu_diff import gpu_run, oracle_run, outcome

pytestmark = pytest.mark.gpu

ROUTES = ["default", "TEST_NO_EXT_LEAN", "TEST_NO_TILE_LOCAL", "TEST_NO_LEAN", "TEST_DICT_HASH"]
UNDIRECTED = (("directed", False),)
TILE = 32768  # input bytes per front-end block (kTile); a line's fields may run kTileHalo = 2048 past it


def _set_route(monkeypatch, route):
    from gfa2network_amd import _native as nat

    monkeypatch.setattr(nat, "TEST_FLAGS", 0 if route == "default" else getattr(nat, route))


def _make(kind, lits):
    return LU.hash_file(lits) if kind == "hash" else LU.decimal_file(lits)


@functools.lru_cache(maxsize=None)
def _parts(wt, dtype="float64"):
    lits = LU.values(wt) if dtype == "float64" else LU.cpu_cast_subset(dtype, wt)
    return tuple(tuple(p) for p in LU.chunks(lits))


@functools.lru_cache(maxsize=None)
def _oracle_outcome(kind, wt, part, mode, dtype):
    from oracle import oracle

    return outcome(oracle_run(oracle, _make(kind, _parts(wt, dtype)[part]), dict(mode), dtype, wt))


def _gpu_outcome(kind, wt, part, mode, dtype):
    return outcome(gpu_run(_make(kind, _parts(wt, dtype)[part]), dict(mode), dtype, wt))


def _coo_data(out, dtype="float64"):
    assert out[0] == "coo", out[:3]
    return np.frombuffer(out[-1], dtype=dtype)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", ["hash", "decimal"])
def test_values_every_route(gpu, oracle_lib, monkeypatch, kind, route):
    """One L line per literal, stream-order COO (directed=False: two triplets per edge) in float64: each
    edge's value equals CPython's, and the whole outcome the oracle's, on every parse route."""
    _set_route(monkeypatch, route)
    for wt in LU.WT_NAMES:
        for part, lits in enumerate(_parts(wt)):
            got = _gpu_outcome(kind, wt, part, UNDIRECTED, "float64")
            data = _coo_data(got)
            assert not LU.same_bits(data[0::2], lits), (wt, part, LU.same_bits(data[0::2], lits))
            assert data[0::2].tobytes() == data[1::2].tobytes()
            assert got == _oracle_outcome(kind, wt, part, UNDIRECTED, "float64"), (wt, part)


@pytest.mark.parametrize("kind", ["hash", "decimal"])
def test_values_bidirected(gpu, oracle_lib, kind):
    """bidirected: four triplets per edge (u:o -> v:o, its transpose, and the reverse twin both ways), every
    copy carrying the edge's value; with keep_directed_bidir (one triplet per edge, the MAX-SYM CSR) the
    whole outcome equals the oracle's."""
    mode = (("bidirected", True),)
    for part, lits in enumerate(_parts(LU.WT)):
        got = _gpu_outcome(kind, LU.WT, part, mode, "float64")
        data = _coo_data(got)
        assert len(data) == 4 * len(lits)
        for k in range(4):
            assert not LU.same_bits(data[k::4], lits), (k, LU.same_bits(data[k::4], lits))
        assert got == _oracle_outcome(kind, LU.WT, part, mode, "float64")
        keep = (("bidirected", True), ("keep_directed_bidir", True))
        assert _gpu_outcome(kind, LU.WT, part, keep, "float64") == _oracle_outcome(kind, LU.WT, part, keep, "float64")
        keep_coo = keep + (("asymmetric", True),)  # ... and its stream-order COO: one triplet per edge
        got = _gpu_outcome(kind, LU.WT, part, keep_coo, "float64")
        assert not LU.same_bits(_coo_data(got), lits)
        assert got == _oracle_outcome(kind, LU.WT, part, keep_coo, "float64")


# ------------------------------------------------------------------ the lean tier
def _canonical_lines(n, wt=LU.WT, n_s=LU.N_NAMES - 4, vals=LU.G_CANONICAL):
    """n decimal-id edge lines (over ids 1..n_s) whose weights are lean_int_tag's canonical spellings, and the
    literals."""
    lits = [LU._i("G", vals[k % len(vals)], wt) for k in range(n)]
    return [LU.decimal_line(k, x, n_s) for k, x in enumerate(lits)], lits


def _took_tile_local(raw):
    return "tiles" not in raw.phase_ms and "parse" in raw.phase_ms


def _edge_values(data, wt, **mode):
    from gfa2network_amd import _native as nat

    raw = nat.build_from_buffer(data, nat.make_options(weight_tag=wt, directed=False, **mode))
    assert raw.status == 0, raw.status
    return raw, np.asarray(raw.data)[0::2]


@pytest.mark.parametrize("wt", LU.WT_NAMES)
def test_lean_tier_taken_on_canonical_weights(gpu, wt):
    """A decimal-id file whose weights are all canonical (optional '-', 1-9 digits, no leading zero) builds on
    the tile-local path for tag names of up to 8 bytes; a 9-byte name takes the full parse; same values."""
    lines, lits = _canonical_lines(6000, wt)
    data = LU.decimal_head() + b"".join(lines)
    assert len(data) > 3 * TILE
    raw, got = _edge_values(data, wt)
    assert _took_tile_local(raw) == (len(wt) <= 8), sorted(raw.phase_ms)
    assert not LU.same_bits(got, lits), LU.same_bits(got, lits)


@pytest.mark.parametrize("other", ["+5", "00", "1000000000", "f:1.5", "5 ", "01"])
def test_lean_tier_declines_other_spellings(gpu, oracle_lib, other):
    """One non-canonical literal at the first, a middle (another 32 KiB tile) and the last edge line: the tile-local
    parse must hand the file to the full parse (its grammar is the canonical spellings only), and every value
    equals CPython's."""
    lines, lits = _canonical_lines(6000)
    head = LU.decimal_head()
    odd = LU._f("G", other[2:]) if other.startswith("f:") else LU._i("G", other)
    for pos in (0, 3000, 5999):
        ls, xs = list(lines), list(lits)
        ls[pos], xs[pos] = LU.decimal_line(pos, odd), odd
        data = head + b"".join(ls)
        start = len(head) + sum(len(x) for x in ls[:pos])
        if pos == 3000:  # not in the tile of the first edge line nor in that of the last
            assert start // TILE not in (len(head) // TILE, (len(data) - len(ls[-1])) // TILE)
        raw, got = _edge_values(data, LU.WT)
        assert not _took_tile_local(raw), (other, pos, sorted(raw.phase_ms))
        assert not LU.same_bits(got, xs), (other, pos, LU.same_bits(got, xs))
    out = outcome(gpu_run(data, dict(UNDIRECTED), "float64", LU.WT))
    assert out == outcome(oracle_run(oracle_lib, data, dict(UNDIRECTED), "float64", LU.WT))


# ------------------------------------------------------- codes in the weighted SUM CSR
SMALL = ["0", "1", "7", "-9", "10", "-1", "123", "-999", "-0"]


def _dup_file(pairs, fill=400):
    """S lines 1..61, `fill` edge lines with small canonical weights, and the (a, b, value) edge lines in between."""
    lines, _ = _canonical_lines(fill, vals=SMALL)
    extra = [b"L\t%d\t+\t%d\t-\t0M\tRC:i:%s\n" % (a, b, v.encode()) for a, b, v in pairs]
    half = len(lines) // 2
    return LU.decimal_head() + b"".join(lines[:half] + extra + lines[half:])


# (a, b, value) lines; ids 58..61 are touched by these lines only, so their runs are exactly the ones written here
CODE_CASES = {
    "three_999999999": [(59, 60, "999999999")] * 3,  # int32 wraps; float32: 1e9 each
    "twice_16777217": [(59, 60, "16777217")] * 2,  # float32 rounds first, then sums
    "16777216_plus_1": [(59, 60, "16777216"), (59, 60, "1")],  # float32: the sum is inexact
    "minus_and_plus": [(59, 60, "-999999999"), (59, 60, "999999999"), (60, 59, "-999999999")],
    "below_2p24": [(59, 60, "8388607")] * 2 + [(60, 61, "-16777215"), (58, 59, "16777214"), (58, 59, "1")],
    "at_2p24": [(59, 60, "8388608")] * 2,
    "row_of_20": [(61, 1 + 2 * k, LU.G_CANONICAL[k % len(LU.G_CANONICAL)]) for k in range(20)] +
                 [(61, 1 + 2 * k, "-5") for k in range(0, 20, 3)],
    "row_of_20_small": [(61, 1 + 2 * k, str(k * 7919 - 60000)) for k in range(20)] +
                       [(61, 1 + 2 * k, str(16777215 - abs(k * 7919 - 60000))) for k in range(0, 20, 3)],
}


def _f32_sums_exact(pairs):
    """The weighted bucket partition keeps a float32 build only while every (row, col) run's sum of magnitudes
    stays below 2^24 (any order of summation is then exact); directed=False: (a, b) and (b, a) are one run each."""
    mag = {}
    for a, b, v in pairs:
        for key in ((a, b), (b, a)):
            mag[key] = mag.get(key, 0) + abs(int(v))
    return max(mag.values()) < 2 ** 24


@pytest.mark.parametrize("dtype", ["float64", "float32", "int32"])
@pytest.mark.parametrize("case", sorted(CODE_CASES))
def test_codes_in_weighted_sum_csr(gpu, oracle_lib, case, dtype):
    """The weighted SUM CSR of a decimal-id file, asked for with output=OUT_CSR (build_from_buffer: that is what
    reaches ParseOpts::wenc; parse_gfa + convert_format takes the COO and k_values' codes instead, checked
    beside), sums lean_int_tag's exact-int32 codes in the bucket partition.  Expected: scipy's
    coo_matrix(...).tocsr() of the oracle's COO in that dtype, whose float64 weights are CPython's.
    (float32: the partition declines any run whose magnitudes reach 2^24, and below 2^24 a code is the same with
    or without its rounding to float32, so no input can tell the float32 code's rounding; the cases on both sides
    of 2^24 pin the decline, and the float64 / int32 cases the unrounded code.)"""
    from gfa2network_amd import _native as nat
    from gfa2network_amd import convert_format, parse_gfa
    import io

    pairs = CODE_CASES[case]
    data = _dup_file(pairs)
    o = oracle_lib.run(data, directed=False, dtype=dtype, weight_tag=LU.WT)
    assert o.status == 0
    text = [x for x in data.split(b"\n") if x.startswith(b"L")]
    want_w = [float(int(x.rsplit(b":", 1)[1])) for x in text]
    assert o.weights[0::2].tobytes() == np.array(want_w).tobytes()
    R = sp.coo_matrix((o.data, (o.rows.astype(np.int32), o.cols.astype(np.int32))), shape=(o.n_nodes, o.n_nodes),
                      dtype=dtype).tocsr()
    opts = nat.make_options(weight_tag=LU.WT, directed=False, dtype=dtype, output=nat.OUT_CSR)
    raw = nat.build_from_buffer(data, opts)
    assert raw.status == 0 and raw.format == "csr"
    assert np.asarray(raw.data).dtype == R.dtype
    assert (np.asarray(raw.indptr).tobytes(), np.asarray(raw.indices).tobytes(), np.asarray(raw.data).tobytes()) == \
        (R.indptr.astype(np.int32).tobytes(), R.indices.astype(np.int32).tobytes(), R.data.tobytes()), case
    # the bucket partition sums the codes unless a float32 sum is inexact (it then declines: the row-sum path)
    assert raw.sum_buckets == (dtype != "float32" or _f32_sums_exact(pairs)), (case, dtype, raw.sum_buckets)
    assert _took_tile_local(raw) or not raw.sum_buckets, sorted(raw.phase_ms)
    A = parse_gfa(io.BytesIO(data), build_graph=False, build_matrix=True, directed=False, weight_tag=LU.WT, dtype=dtype)
    C = convert_format(A, "csr")
    assert (C.indptr.tobytes(), C.indices.tobytes(), C.data.tobytes()) == \
        (R.indptr.tobytes(), R.indices.tobytes(), R.data.tobytes()), case


# ------------------------------------------------------------------------ casts
@pytest.mark.parametrize("kind", ["hash", "decimal"])
@pytest.mark.parametrize("dtype", ["float32", "int32", "int8", "bool"])
def test_castable_subset_equals_oracle(gpu, oracle_lib, kind, dtype):
    """Every literal the oracle casts to the dtype: values, and float32's one overflow warning per element."""
    n_warn = 0
    for part, lits in enumerate(_parts(LU.WT, dtype)):
        got = _gpu_outcome(kind, LU.WT, part, UNDIRECTED, dtype)
        assert got == _oracle_outcome(kind, LU.WT, part, UNDIRECTED, dtype), (dtype, part)
        assert got[0] == "coo" and len(_coo_data(got, "uint8" if dtype == "bool" else dtype)) == 2 * len(lits)
        n_warn += sum(m == "overflow encountered in cast" for m in got[3])
    if dtype == "float32":  # 3.4028235677973366e38, 1e39, 1e300, ... : two triplets each
        want = sum(np.isfinite(x.want) and abs(x.want) >= float.fromhex("0x1.ffffffp127") for x in LU.values())
        assert n_warn == 2 * want and want > 100
    else:
        assert n_warn == 0


CAST_ERRORS = ["i:128", "i:-129", "i:2147483648", "i:-2147483649", "f:inf", "f:-inf", "f:nan", "f:1e300", "f:0.5",
               "f:-128.9", "f:128.0", "f:-nan"]


@pytest.mark.parametrize("dtype", ["int8", "int32"])
@pytest.mark.parametrize("value", CAST_ERRORS)
def test_cast_errors_equal_oracle(gpu, oracle_lib, value, dtype):
    """One weighted line alone, and as line 3 of 5 (the element index of the error): the exception's type and
    message are the oracle's (numpy's), or there is none where the cast is fine (0.5 -> 0)."""
    from gfa2network_amd import _native as nat

    lit = LU._mk("H", ["RC:" + value])
    plain = [LU._i("G", "7"), LU._i("G", "-3")]
    n_exc = 0
    for lits in ([lit], plain + [lit] + plain):
        for kind in ("hash", "decimal"):
            data = _make(kind, lits)
            for ktrip, mode in ((2, {"directed": False}), (4, {"bidirected": True}), (1, {})):
                raw = nat.build_from_buffer(data, nat.make_options(weight_tag=LU.WT, dtype=dtype, **mode))
                o = oracle_lib.run(data, dtype=dtype, weight_tag=LU.WT, **mode)
                assert raw.status == o.status, (value, dtype, kind, mode, raw.status, o.status)
                if o.status:  # the first failing element of the triplet stream, and its float64 value
                    assert raw.err_index == o.err_index == ktrip * (len(lits) // 2), (raw.err_index, o.err_index)
                    if lit.want == lit.want:
                        assert LU.bits(raw.err_value) == LU.bits(o.err_value) == LU.bits(lit.want)
                a = outcome(gpu_run(data, mode, dtype, LU.WT))
                assert a == outcome(oracle_run(oracle_lib, data, mode, dtype, LU.WT)), (value, dtype, kind, mode, a[:3])
                n_exc += a[0] == "exc"
    fails = {"int8": set(CAST_ERRORS) - {"f:0.5", "f:-128.9"},
             "int32": {"i:2147483648", "i:-2147483649", "f:inf", "f:-inf", "f:nan", "f:1e300", "f:-nan"}}[dtype]
    assert n_exc == (12 if value in fails else 0)


# ----------------------------------------------------------------- int overflow
@pytest.mark.parametrize("route", ["default", "TEST_NO_TILE_LOCAL"])
@pytest.mark.parametrize("kind", ["hash", "decimal"])
def test_int_overflow_at_its_line(gpu, oracle_lib, monkeypatch, kind, route):
    """float(int) overflowing is OverflowError("int too large to convert to float") at that line; of two such
    lines the lower one is reported."""
    from gfa2network_amd import _native as nat

    _set_route(monkeypatch, route)
    plain = [LU._i("G", "7"), LU._f("B", "1.5"), LU._i("A", "1" * 17)]
    over = LU.overflowing()
    assert len(over) >= 8
    for x in over:
        data = _make(kind, plain + [x] + plain)
        raw = nat.build_from_buffer(data, nat.make_options(weight_tag=x.wt, directed=False))
        line = len(plain) + (LU.N_NAMES if kind == "decimal" else 0)
        assert (raw.status, raw.err_line) == (nat.E_INT_TOO_LARGE, line), (x.fields[0][:30], raw.status, raw.err_line)
        a = outcome(gpu_run(data, dict(UNDIRECTED), "float64", x.wt))
        assert a[:3] == ("exc", "OverflowError", "int too large to convert to float")
        assert a == outcome(oracle_run(oracle_lib, data, dict(UNDIRECTED), "float64", x.wt))
    two = plain + [over[3]] + plain * 40 + [over[0]] + plain
    for lits in (two, two[::-1]):
        data = _make(kind, lits)
        raw = nat.build_from_buffer(data, nat.make_options(weight_tag=LU.WT, directed=False))
        first = min(k for k, x in enumerate(lits) if x.want is None) + (LU.N_NAMES if kind == "decimal" else 0)
        assert (raw.status, raw.err_line) == (nat.E_INT_TOO_LARGE, first)


# ---------------------------------------------------------------- long literals
def _long_literals():
    lits = [x for x in LU.values(LU.WT, "C") if len(x.fields[-1]) > 800]
    assert sum(len(x.fields[-1]) > 4900 for x in lits) >= 3 and len(lits) >= 30
    return lits


def _straddling_file(kind, longs):
    """Ordinary lines with one long line first, one last, and the rest each starting within the last 128 bytes
    of a 32 KiB tile (so its fields end in the next tile, or past the tile's halo)."""
    plain = [LU._i("G", v) for v in LU.G_CANONICAL]
    line = LU.hash_line if kind == "hash" else LU.decimal_line
    out = [LU.decimal_head()] if kind == "decimal" else []
    lits, starts = [], []
    size = sum(len(x) for x in out)

    def put(x):
        nonlocal size
        out.append(line(len(lits), x))
        lits.append(x)
        size += len(out[-1])

    starts.append(size)
    put(longs[0])
    for x in longs[1:-1]:
        while TILE - size % TILE > 128:
            put(plain[len(lits) % len(plain)])
        starts.append(size)
        put(x)
    for _ in range(50):
        put(plain[len(lits) % len(plain)])
    starts.append(size)
    put(longs[-1])
    return b"".join(out), lits, starts


@pytest.mark.parametrize("route", ["default", "TEST_NO_TILE_LOCAL"])
@pytest.mark.parametrize("kind", ["hash", "decimal"])
def test_long_literals_across_tiles(gpu, oracle_lib, monkeypatch, kind, route):
    """5000-digit and > 800-digit literals first, last and across tile boundaries among ordinary lines: lines
    past the staged window go through k_parse_deferred, all of them through k_weights_slow."""
    longs = _long_literals()
    big = [x for x in longs if len(x.fields[-1]) > 4900]
    rest = [x for x in longs if len(x.fields[-1]) <= 4900]
    order = [big[0]] + rest[:len(rest) // 2] + big[1:-1] + rest[len(rest) // 2:] + [big[-1]]
    _set_route(monkeypatch, route)
    for part in range(0, len(order), 24):  # (every file under 1 MB)
        sub = order[part:part + 24]
        data, lits, starts = _straddling_file(kind, sub)
        assert len(data) < 1_000_000
        for s, x in list(zip(starts, sub))[1:-1]:
            assert s // TILE != (s + len(x.fields[-1])) // TILE
        got = outcome(gpu_run(data, dict(UNDIRECTED), "float64", LU.WT))
        vals = _coo_data(got)[0::2]
        assert not LU.same_bits(vals, lits), LU.same_bits(vals, lits)
        assert got == outcome(oracle_run(oracle_lib, data, dict(UNDIRECTED), "float64", LU.WT))
