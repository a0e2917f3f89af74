"""GPU: the dense writers (g2n_dense.hip: write_dense / dense_range / save_matrix's .csv and .npy) against
numpy — np.savetxt(dest, A.toarray(), delimiter=",", fmt="%.6g") and np.save(dest, A.toarray()) — byte for byte,
at the shapes where the render can go wrong: rows one tile -+ 2 bytes long, a 13-byte text across every offset of a
tile and a band edge, empty and full rows, the special values, long rows and many rows, bands that divide the
document exactly or leave one byte, the five dtypes, int64 indices, positions past 2^32, inputs the writer
declines, and the CLI."""
import io

import numpy as np
import pytest
import scipy.sparse as sp

from gfa2network_amd import _native, api

pytestmark = pytest.mark.gpu

LONG = -1.23457e-308  # '%.6g': -1.23457e-308, 13 bytes


def ref_csv(A) -> bytes:
    bio = io.BytesIO()
    np.savetxt(bio, A.toarray(), delimiter=",", fmt="%.6g")
    return bio.getvalue()


def ref_npy(A) -> bytes:
    bio = io.BytesIO()
    np.save(bio, A.toarray())
    return bio.getvalue()


@pytest.fixture(scope="module")
def T(tmp_path_factory) -> int:
    d = tmp_path_factory.mktemp("tile")
    info = api.write_dense(sp.csr_matrix(np.array([[2.5]])), d / "one.csv", return_info=True)
    assert (d / "one.csv").read_bytes() == b"2.5\n" and info["doc_bytes"] == 4 and info["declined"] == 0
    return info["tile_bytes"]


def check(A, tmp_path, band_bytes=None, kinds=("csv", "npy")):
    """write_dense(A) == numpy for both documents; returns the csv's info."""
    out = None
    for kind in kinds:
        dest = tmp_path / f"m.{kind}"
        info = api.write_dense(A, dest, band_bytes=band_bytes, return_info=True)
        assert info["declined"] == 0
        got = dest.read_bytes()
        want = ref_csv(A) if kind == "csv" else ref_npy(A)
        assert len(got) == len(want), (kind, A.shape, len(got), len(want))
        if got != want:
            at = next(i for i, (x, y) in enumerate(zip(got, want)) if x != y)
            raise AssertionError((kind, A.shape, at, got[max(0, at - 20):at + 20], want[max(0, at - 20):at + 20]))
        if kind == "npy":
            B = np.load(dest)
            D = A.toarray()
            assert B.dtype == D.dtype and B.shape == D.shape and B.tobytes() == D.tobytes()
        else:
            assert info["doc_bytes"] == len(want)
            out = info
    return out


def sprinkle(n_rows, n_cols, nnz, seed, dtype=np.float64):
    """a canonical CSR with nnz distinct cells and values whose texts have every length"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(n_rows * n_cols, size=min(nnz, n_rows * n_cols), replace=False)
    pool = np.array([1.0, 7.0, 10.0, -3.0, 0.5, 123456.0, 1234567.0, -0.000123456, 1e-5, 2.5e-300, LONG, 1e100, 99999.95])
    vals = pool[rng.integers(0, len(pool), size=len(cells))]
    A = sp.coo_matrix((vals, (cells // n_cols, cells % n_cols)), shape=(n_rows, n_cols)).tocsr()
    A.sort_indices()
    with np.errstate(over="ignore"):
        return A.astype(dtype)


@pytest.mark.parametrize("n_rows", [1, 2, 5])
def test_rows_of_one_tile_minus_and_plus_two_bytes(T, tmp_path, n_rows):
    for n_cols in (T // 2 - 1, T // 2, T // 2 + 1, 1):
        check(sprinkle(n_rows, n_cols, 6 * n_rows, seed=n_cols), tmp_path, band_bytes=T)
        check(sp.csr_matrix((n_rows, n_cols), dtype=np.float64), tmp_path, band_bytes=T, kinds=("csv",))
    check(sp.csr_matrix(np.array([[LONG]])), tmp_path)


@pytest.mark.parametrize("band", ["one band", "band edge"])
def test_long_text_at_every_offset_of_a_tile_edge(T, tmp_path, band):
    for k in range(14):  # the text starts at T - k
        n_cols = T
        if k % 2 == 0:
            cols, vals = [(T - k) // 2], [LONG]
        else:  # "10" in column 0 moves what follows by one byte
            cols, vals = [0, (T - k - 1) // 2], [10.0, LONG]
        A = sp.csr_matrix((vals, cols, [0, len(cols)]), shape=(1, n_cols))
        want = ref_csv(A)
        assert want.index(b"-1.23457e-308") == T - k
        check(A, tmp_path, band_bytes=T if band == "band edge" else None, kinds=("csv",))


def test_long_text_in_first_and_last_column_around_a_tile_edge(T, tmp_path):
    for n_cols in range(T // 2 - 8, T // 2 + 1):  # the rows' '\n' on either side of the edge
        rows = 3
        indptr = [0, 2, 4, 6]
        A = sp.csr_matrix(([LONG] * 6, [0, n_cols - 1] * rows, indptr), shape=(rows, n_cols))
        check(A, tmp_path, band_bytes=T, kinds=("csv",))
        check(A, tmp_path, kinds=("csv",))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_special_values_empty_and_full_rows(T, tmp_path, dtype):
    n_cols = 300
    rng = np.random.default_rng(11)
    full = rng.standard_normal(n_cols) * 10.0 ** rng.integers(-8, 9, size=n_cols)
    full[::7] = np.round(full[::7])
    special = [0.0, -0.0, np.nan, np.inf, -np.inf, 0.0, 1.0, -0.0]
    scols = [0, 1, 2, 3, 4, 150, 151, n_cols - 1]
    data = np.concatenate([full, special, [5.0]])
    indices = np.concatenate([np.arange(n_cols), scols, [n_cols - 1]])
    indptr = [0, 0, n_cols, n_cols + len(scols), n_cols + len(scols), n_cols + len(scols), len(data)]
    with np.errstate(over="ignore"):
        A = sp.csr_matrix((data.astype(dtype), indices, indptr), shape=(6, n_cols))
    assert A.nnz == len(data)  # the explicit zeros stay stored
    check(A, tmp_path)
    check(A, tmp_path, band_bytes=T)
    Z = sp.csr_matrix((np.zeros(4, dtype=dtype), [0, 5, 5, 299], [0, 2, 2, 4]), shape=(3, n_cols))  # stored zeros only
    check(Z, tmp_path)
    check(sp.csr_matrix((3, n_cols), dtype=dtype), tmp_path)  # nothing stored
    check(sp.csr_matrix(np.full((2, 40), 3.25, dtype=dtype)), tmp_path)  # no background at all


def test_one_long_row_and_many_short_rows(T, tmp_path):
    rng = np.random.default_rng(12)
    cols = np.sort(rng.choice(80_000, size=70_000, replace=False))
    vals = rng.integers(-5, 2000, size=70_000).astype(np.float64) / 8.0
    check(sp.csr_matrix((vals, cols, [0, 70_000]), shape=(1, 80_000)), tmp_path, band_bytes=16 * T)
    cols = rng.integers(0, 3, size=70_000)
    vals = rng.integers(1, 2000, size=70_000).astype(np.float64) / 4.0
    check(sp.csr_matrix((vals, cols, np.arange(70_001)), shape=(70_000, 3)), tmp_path, band_bytes=16 * T)


def test_many_bands_and_band_multiples(T, tmp_path):
    A = sprinkle(720, 720, 20_000, seed=13)  # about 1 MiB of csv
    info = check(A, tmp_path, band_bytes=4 * T)
    assert info["band_bytes"] == 4 * T and info["bands"] == -(-info["doc_bytes"] // (4 * T)) > 60
    times = _native.dense_last_times()  # (the .npy written last)
    assert times["total_ms"] > 0 and times["total_ms"] >= times["write_ms"] >= 0 and times["render_ms"] > 0
    first = (tmp_path / "m.csv").read_bytes()
    api.write_dense(A, tmp_path / "again.csv", band_bytes=4 * T)
    assert (tmp_path / "again.csv").read_bytes() == first  # run to run
    # single-digit values leave the length alone: 2 rows of 2 T columns are exactly two bands of 4 T
    rng = np.random.default_rng(14)
    cols = np.sort(rng.choice(2 * T, size=500, replace=False))
    vals = rng.integers(1, 10, size=500).astype(np.float64)
    E = sp.csr_matrix((vals, cols, [0, 200, 500]), shape=(2, 2 * T))
    info = check(E, tmp_path, band_bytes=4 * T, kinds=("csv",))
    assert info["doc_bytes"] == 8 * T and info["bands"] == 2
    E.data[-1] = 10.0  # one byte more
    info = check(E, tmp_path, band_bytes=4 * T, kinds=("csv",))
    assert info["doc_bytes"] == 8 * T + 1 and info["bands"] == 3
    info = check(E, tmp_path, band_bytes=64 * T)  # a band larger than the document
    assert info["bands"] == 1
    with pytest.raises(ValueError):
        api.write_dense(E, tmp_path / "bad.csv", band_bytes=T + 1)


@pytest.mark.parametrize("dtype", ["bool", "int8", "int32", "float32", "float64"])
@pytest.mark.parametrize("index", [np.int32, np.int64])
def test_dtypes_and_index_widths(T, tmp_path, dtype, index):
    A = sprinkle(40, 300, 900, seed=15)
    ext = {"bool": [1, 0, 1], "int8": [-128, 127, 0], "int32": [-2147483648, 2147483647, 1234567],
           "float32": [3.4028235e38, 1e-45, 16777217.0], "float64": [1.7976931348623157e308, 5e-324, -0.0]}[dtype]
    if dtype in ("int8", "int32", "bool"):
        A.data = np.random.default_rng(16).integers(-100, 100, size=A.nnz).astype(np.float64)
    with np.errstate(over="ignore"):
        A = A.astype(dtype)
    A.data[:3] = np.array(ext).astype(dtype)
    A.indptr, A.indices = A.indptr.astype(index), A.indices.astype(index)
    check(A, tmp_path, band_bytes=2 * T)
    assert A.indices.dtype == index
    C = A.tocsc()  # a canonical CSC goes through the native COO -> CSR
    check(C, tmp_path, band_bytes=2 * T)


# ---- positions past 2^32: a 50 000 x 50 000 matrix, about 5 GB of csv and 20 GB of .npy, never written
N_BIG = 50_000
CSV_ROWS = (range(42_930, 42_970), range(45_000, 45_012), range(N_BIG - 14, N_BIG))
NPY_ROWS = (range(10_730, 10_745), range(39_996, 40_004))


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(17)
    rows = [rng.integers(0, N_BIG, size=4000)]
    for rr in CSV_ROWS + NPY_ROWS:  # the windows' rows hold 30 entries each
        rows.append(np.repeat(np.fromiter(rr, dtype=np.int64), 30))
    rows = np.concatenate(rows)
    cells = np.unique(rows * N_BIG + rng.integers(0, N_BIG, size=len(rows)))
    vals = rng.standard_normal(len(cells)) * 10.0 ** rng.integers(-12, 13, size=len(cells))
    vals[::5] = np.round(vals[::5])
    A = sp.csr_matrix((vals, (cells // N_BIG, cells % N_BIG)), shape=(N_BIG, N_BIG))
    A.sort_indices()
    extra = np.array([len("%.6g" % (v + 0.0)) - 1 for v in A.data], dtype=np.int64)  # (the cell is 0 + v: -0.0 is "0")
    X = np.concatenate([[0], np.cumsum(extra)])
    R = 2 * N_BIG * np.arange(N_BIG + 1, dtype=np.int64) + X[A.indptr]  # row starts; R[N] = the length
    return A, R


def csv_window(A, R, b0, b1):
    i0 = int(np.searchsorted(R, b0, side="right")) - 1
    i1 = int(np.searchsorted(R, b1 - 1, side="right")) - 1
    text = ref_csv(A[i0:i1 + 1])
    return text[b0 - int(R[i0]):b1 - int(R[i0])]


def test_positions_past_4gib_csv(big):
    A, R = big
    total = int(R[-1])
    assert total > 5_000_000_000
    MiB = 1 << 20
    starts = [(1 << 32) - MiB // 2 - 3, int(R[45_005]) - MiB // 2 + 1, total - MiB]
    for b0 in starts:
        assert b0 + MiB <= total and (b0 + MiB > 1 << 32)
        got = api.dense_range(A, "csv", b0, b0 + MiB)
        want = csv_window(A, R, b0, b0 + MiB)
        assert len(want) == MiB and got == want, b0
        assert any(ch not in b"0,\n" for ch in want)  # the window holds entries
    assert api.dense_range(A, "csv", total - 1, total) == b"\n"
    with pytest.raises(ValueError):
        api.dense_range(A, "csv", total, total + 1)


def test_positions_past_4gib_npy(big):
    A, _R = big
    row_bytes = N_BIG * 8
    total = N_BIG * row_bytes
    MiB = 1 << 20
    for b0 in [(1 << 32) - MiB // 2 - 3, 40_000 * row_bytes - MiB // 2 + 5, total - MiB]:
        i0, i1 = b0 // row_bytes, (b0 + MiB - 1) // row_bytes
        want = A[i0:i1 + 1].toarray().tobytes()[b0 - i0 * row_bytes:b0 + MiB - i0 * row_bytes]
        got = api.dense_range(A, "npy", b0, b0 + MiB)
        assert got == want, b0
        assert any(want)


def test_declined_inputs_take_numpys_route(tmp_path, monkeypatch):
    unsorted = sp.csr_matrix(([1.5, 2.5, 3.0], [4, 1, 2], [0, 2, 3]), shape=(2, 6))
    dup = sp.csr_matrix(([1.5, 2.5, 3.0], [1, 1, 2], [0, 2, 3]), shape=(2, 6))
    calls = []
    real = api.write_dense

    def spy(A, dest, **kw):
        info = real(A, dest, **kw)
        calls.append(info["declined"])
        return info

    monkeypatch.setattr(api, "write_dense", spy)
    for A in (unsorted, dup):
        assert A.nnz == 3
        for kind in ("csv", "npy"):
            info = real(A, tmp_path / f"d.{kind}", return_info=True)
            assert info["declined"] == 1
            with pytest.raises(ValueError):
                api.dense_range(A, kind, 0, 1)
            calls.clear()
            api.save_matrix(A, tmp_path / f"s.{kind}")
            assert calls == [1]
            assert (tmp_path / f"s.{kind}").read_bytes() == (ref_csv(A) if kind == "csv" else ref_npy(A))
    good = sprinkle(5, 9, 12, seed=18)
    for fmt, want_calls in (("csr", [0]), ("csc", [0]), ("coo", []), ("dok", [])):
        calls.clear()
        B = good.asformat(fmt)
        api.save_matrix(B, tmp_path / "g.csv")
        assert calls == want_calls, fmt
        assert (tmp_path / "g.csv").read_bytes() == ref_csv(good)
    calls.clear()
    api.save_matrix(good.toarray(), tmp_path / "g.npy")  # an ndarray is numpy's
    with np.errstate(invalid="ignore", over="ignore"):
        api.save_matrix(good.astype(np.int64), tmp_path / "g64.csv")  # another dtype too
    assert calls == [] and (tmp_path / "g.npy").read_bytes() == ref_npy(good)
    with pytest.raises(ValueError):  # an index outside the shape is refused, not rendered
        bad = sp.csr_matrix((2, 6))
        bad.indices, bad.data, bad.indptr = np.array([9], dtype=np.int32), np.array([1.0]), np.array([0, 1, 1], dtype=np.int32)
        real(bad, tmp_path / "bad.csv")


@pytest.mark.parametrize("dtype", ["bool", "int8", "int32", "float32", "float64"])
@pytest.mark.parametrize("weighted", [False, True])
def test_cli_convert_dense(tmp_path, dtype, weighted, capsys):
    from gfa2network_amd import cli, convert_format, parse_gfa

    big = {"bool": 7e9, "int8": 127, "int32": 2147483000, "float32": 1.5e30, "float64": 1.5e300}[dtype]
    weights = ["0.5", "-3.25", "2.75", str(big), "-100.5", "1e-7", "12", "-1"]
    rng = np.random.default_rng(19)
    lines = [f"S\ts{i}\t*" for i in range(60)]
    for j in range(200):
        a, b = rng.integers(0, 60, size=2)
        tag = f"\tRC:f:{weights[j % len(weights)]}" if j % 5 else ""
        lines.append(f"L\ts{a}\t{'+-'[j % 2]}\ts{b}\t{'+-'[j % 3 % 2]}\t*{tag}")
    inp = tmp_path / "in.gfa"
    inp.write_text("\n".join(lines) + "\n")
    kw = dict(dtype=dtype, weight_tag="RC" if weighted else None)
    A = convert_format(parse_gfa(inp, build_graph=False, build_matrix=True, **kw), "csr")
    assert A.format == "csr" and A.dtype == np.dtype(dtype) and A.nnz > 100
    for kind in ("csv", "npy"):
        dest = tmp_path / f"out.{kind}"
        cli.main(["convert", str(inp), "--matrix", str(dest), "--dtype", dtype] + (["--weight-tag", "RC"] if weighted else []))
        assert dest.read_bytes() == (ref_csv(A) if kind == "csv" else ref_npy(A)), (dtype, weighted, kind)
        assert (tmp_path / f"out.{kind}.nodes.tsv").exists()
    capsys.readouterr()
