"""CPU: g2n_format_g6 (csrc/g6fmt.h, the code k_dn_fmt runs per stored entry) against CPython's own
'%.6g' % v — what np.savetxt(..., fmt="%.6g") writes per cell — on a seeded corpus, every value checked; and
the routing of save_matrix's dense outputs on a machine without a GPU."""
import ctypes
import random
import struct

import numpy as np
import pytest
import scipy.sparse as sp

from gfa2network_amd import _native, api

SPOTS = {
    1000005.0: "1e+06",
    1000015.0: "1.00002e+06",
    999999.5: "1e+06",
    99999.95: "99999.9",
    5e-324: "4.94066e-324",
    float(np.int32(-2147483648)): "-2.14748e+09",
}


def _neighbours(v: float) -> list[float]:
    return [v, float(np.nextafter(v, np.inf)), float(np.nextafter(v, -np.inf))]


def corpus() -> list[float]:
    r = random.Random(20240607)
    vals = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), -float("nan")]
    for k in range(-320, 309):  # every power of ten a double holds, with its two neighbours
        vals += _neighbours(float(f"1e{k}"))
    for v in (0.0001, 0.000099999951, 99999.95, 999999.5, 1e6):  # the fixed / scientific switch
        vals += _neighbours(v)
    for v in (1000005.0, 1000015.0, 100000.5, 100001.5):  # exact 6-digit ties
        vals += _neighbours(v)
    for k in range(41):
        vals += _neighbours(1234565.0 * 2.0 ** -k)
    vals += _neighbours(1.7976931348623157e308)[:1] + [float(np.nextafter(1.7976931348623157e308, 0))]
    vals += _neighbours(2.2250738585072014e-308)
    vals += [5e-324, 1e-323, 2.5e-320, 1.23e-310, 2.225073858507201e-308, -5e-324]
    vals += [float(x) for x in range(-128, 128)]  # every int8
    vals += [float(np.int32(-2147483648)), float(np.int32(2147483647)), 2147483646.0, -2147483647.0]
    f32 = np.frombuffer(np.random.default_rng(5).bytes(4 * 20000), dtype=np.float32)
    vals += [float(x) for x in f32]
    vals += [float(np.float32(x)) for x in (0.1, 1.17549435e-38, 1e-45, 3.4028235e38, 16777217.0, 0.3)]
    vals += [struct.unpack("<d", struct.pack("<Q", r.getrandbits(64)))[0] for _ in range(200_000)]
    for _ in range(200_000):
        nd = r.randrange(1, 10)
        vals.append(float(f"{r.choice('+-')}{r.randrange(10 ** (nd - 1), 10 ** nd)}e{r.randrange(-30, 31)}"))
    vals += [-v for v in vals[6:2000]]
    return vals


def test_format_g6_matches_python_on_the_corpus():
    lib = _native.load()
    out = (ctypes.c_uint8 * 16)()
    vals = corpus()
    assert len(vals) > 420_000
    bad = []
    for v in vals:
        n = lib.g2n_format_g6(v, out)
        got = bytes(out[:n])
        want = ("%.6g" % v).encode()
        if got != want or out[15] != n or n > 13 or any(out[n:15]):
            bad.append((v.hex() if v == v else "nan", got, want))
    assert not bad, (len(bad), bad[:10])


def test_format_g6_spot_values():
    for v, text in SPOTS.items():
        assert "%.6g" % v == text  # what this Python prints
        assert _native.format_g6(v) == text.encode()
    assert _native.format_g6(-1.23457e-308) == b"-1.23457e-308"  # the longest: 13 bytes
    assert _native.format_g6(-0.0) == b"-0" and _native.format_g6(float("-inf")) == b"-inf"
    assert _native.format_g6(float("nan")) == b"nan"


def test_dense_info_layout_matches_header(tmp_path):
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    fields = [f[0] for f in _native.DenseInfo._fields_]
    lines = ['printf("sizeof %zu\\n", sizeof(g2n_dense_info));']
    lines += [f'printf("{f} %zu\\n", offsetof(g2n_dense_info, {f}));' for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "g2n.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(root / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(_native.DenseInfo)
    for f in fields:
        assert int(got[f]) == getattr(_native.DenseInfo, f).offset, f


needs_no_gpu = pytest.mark.skipif(_native.device_count() > 0, reason="a GPU is visible")


def _matrix():
    rng = np.random.default_rng(3)
    A = sp.random(9, 7, 0.3, format="csr", dtype=np.float64, random_state=rng)
    A.data[:3] = [-0.0, 1e-7, 123456.5]
    return A


@needs_no_gpu
@pytest.mark.parametrize("fmt", ["csr", "csc", "coo"])
def test_save_matrix_without_a_gpu_writes_numpys_bytes(tmp_path, fmt):
    A = _matrix().asformat(fmt)
    api.save_matrix(A, tmp_path / "a.csv")
    api.save_matrix(A, tmp_path / "a.npy")
    np.savetxt(tmp_path / "ref.csv", A.toarray(), delimiter=",", fmt="%.6g")
    np.save(tmp_path / "ref.npy", A.toarray())
    assert (tmp_path / "a.csv").read_bytes() == (tmp_path / "ref.csv").read_bytes()
    assert (tmp_path / "a.npy").read_bytes() == (tmp_path / "ref.npy").read_bytes()


@needs_no_gpu
def test_write_dense_without_a_gpu_raises(tmp_path):
    with pytest.raises(RuntimeError, match="G2N_E_DEVICE"):
        api.write_dense(_matrix(), tmp_path / "a.csv")
    with pytest.raises(RuntimeError, match="G2N_E_DEVICE"):
        api.dense_range(_matrix(), "npy", 0, 8)


def test_dense_entry_points_refuse_other_inputs(tmp_path):
    A = _matrix()
    with pytest.raises(TypeError):
        api.write_dense(A.tocoo(), tmp_path / "a.csv")
    with pytest.raises(TypeError):
        api.write_dense(A.toarray(), tmp_path / "a.csv")
    with pytest.raises(NotImplementedError):
        api.write_dense(A.astype(np.int64), tmp_path / "a.csv")
    with pytest.raises(ValueError):
        api.write_dense(A, tmp_path / "a.txt")
    with pytest.raises(ValueError):
        api.write_dense(sp.csr_matrix((0, 4), dtype=np.float64), tmp_path / "a.csv")
    with pytest.raises(ValueError):
        api.dense_range(A, "tsv", 0, 1)
    assert "write_dense" in api.__all__ and "dense_range" in api.__all__
