"""CPU: the ``stats`` call surface without a GPU — the CLI schema, the exports, the density helper,
the completeness of tests/golden/expected/stats.json, the C struct's layout, the loud failure
without a device, and the contract itself: the formulas that turn the asymmetric CSR's counts into
the reference's numbers, checked against the fixture with the CPU oracle's CSR."""
import ctypes
import gzip
import json
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
from make_stats_golden import cases  # noqa: E402  (the generator's own list of cases)

KEYS = ["nodes", "edges", "paths", "components", "max_degree", "density"]


@pytest.fixture(scope="module")
def expected():
    return json.loads((GOLDEN / "expected" / "stats.json").read_text())


def test_stats_parser_takes_the_reference_flags():
    from gfa2network_amd.cli import _parser

    p = _parser()
    a = p.parse_args(["stats", "x.gfa"])
    assert (a.cmd, a.gfa, a.directed, a.strip_orientation, a.raw_bytes_id, a.device) == \
        ("stats", "x.gfa", True, False, False, 0)
    a = p.parse_args(["--raw-bytes-id", "--device", "1", "stats", "x.gfa", "--undirected", "--strip-orientation"])
    assert (a.directed, a.strip_orientation, a.raw_bytes_id, a.device) == (False, True, True, 1)
    assert p.parse_args(["stats", "x.gfa", "--directed"]).directed is True
    assert p.parse_args(["stat", "x.gfa"]).gfa == "x.gfa"  # the reference's alias
    for bad in (["stats"], ["stats", "x.gfa", "--directed", "--undirected"], ["stats", "x.gfa", "--bidirected"],
                ["stats", "x.gfa", "--raw-bytes-id"], ["stats", "x.gfa", "y.gfa"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    # distance / distance-matrix keep their stub
    assert p.parse_args(["distance", "x.gfa", "--seq", "a", "b"]).cmd == "distance"


def test_stats_functions_are_exported():
    import gfa2network_amd
    from gfa2network_amd import _native, api

    for name in ("compute_stats", "graph_stats"):
        assert name in gfa2network_amd.__all__ and callable(getattr(gfa2network_amd, name))
        assert name in api.__all__
    lib = _native.load()
    for sym in ("g2n_csr_stats", "g2n_csr_stats_host", "g2n_stats_from_path"):
        assert sym in _native.EXPORTED and hasattr(lib, sym)


def test_graph_stats_struct_matches_header(tmp_path):
    from gfa2network_amd import _native

    py = _native.GraphStats
    lines = ['printf("sizeof %zu\\n", sizeof(g2n_graph_stats));']
    lines += [f'printf("{f[0]} %zu\\n", offsetof(g2n_graph_stats, {f[0]}));' for f in py._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "g2n.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(py)
    for f in py._fields_:
        assert int(got[f[0]]) == getattr(py, f[0]).offset, f[0]


def test_fixture_holds_every_case(expected):
    """stats.json has exactly one record for every input x option combination (both input folders,
    directed x strip_orientation, raw_bytes_id for the non-ASCII files): none may be left out."""
    want = [c[0] for c in cases()]
    assert len(want) == len(set(want)) and len(want) >= 4 * 64
    assert sorted(expected) == sorted(want)
    names = {c[1].name for c in cases()}
    for f in ("inputs", "stats_inputs"):
        assert {p.name for p in (GOLDEN / f).iterdir()} <= names
    for key, rec in expected.items():
        assert (rec["stats"] is None) != (rec["exc"] is None), key
        if rec["stats"] is not None:
            assert [k for k, _ in rec["stats"]] == KEYS, key
            assert rec["stdout"].count("\n") == 6, key


def test_density_reproduces_the_fixture(expected):
    from gfa2network_amd.api import density

    seen_int = seen_float = 0
    for key, _inp, directed, _strip, _raw in cases():
        rec = expected[key]
        if rec["stats"] is None:
            continue
        s = dict(rec["stats"])
        got = density(s["nodes"], s["edges"], directed)
        assert got == s["density"] and type(got) is type(s["density"]), key
        seen_int += type(got) is int
        seen_float += type(got) is float
    assert seen_int and seen_float
    # at most one node, or no edge: the int 0 (nx.density)
    for n, m in ((0, 0), (1, 0), (1, 1), (5, 0)):
        for directed in (True, False):
            d = density(n, m, directed)
            assert d == 0 and type(d) is int
    # n (n - 1) past 2^53: the correctly rounded quotient of the exact integers, which a quotient
    # of C doubles misses (the product is rounded first)
    n, m = 2**31 - 9, 3  # (inside the supported node range: n < 2^31 - 1)
    assert n * (n - 1) > 2**53 and float(n * (n - 1)) != n * (n - 1)
    assert density(n, m, True) == float(Fraction(m, n * (n - 1)))
    assert density(n, m, False) == float(Fraction(2 * m, n * (n - 1)))
    assert density(n, m, True) != float(m) / (float(n) * float(n - 1))


def test_contract_formulas_match_the_fixture(oracle_lib, expected):
    """What g2n_csr_stats counts, taken here with numpy / scipy from the CPU oracle's asymmetric
    summed CSR and put through the shim's own helpers, is the reference's answer for every recorded
    case (and a non-ASCII node key is the only failure of a build that parses cleanly)."""
    from scipy.sparse.csgraph import connected_components

    from gfa2network_amd.api import _stats_edges, density

    for key, inp, directed, strip, raw in cases():
        data = inp.read_bytes()
        if inp.name.endswith(".gz"):
            data = gzip.decompress(data)
        o = oracle_lib.run(data, directed=directed, asymmetric=True, strip_orientation=strip, dtype="float64")
        rec = expected[key]
        if o.status != 0:
            assert rec["exc"] is not None, key
            continue
        if rec["exc"] is not None:
            assert rec["exc"][0] == "UnicodeDecodeError" and "'ascii'" in rec["exc"][1] and not raw, key
            assert max(o.names_blob.tobytes()) >= 0x80, key
            continue
        n, ip, ix = o.n_nodes, o.sum_indptr, o.sum_indices
        rows = np.repeat(np.arange(n), np.diff(ip))
        diag = np.zeros(n, dtype=np.int64)
        diag[rows[rows == ix]] = 1
        st = {"n_nodes": n, "n_entries": len(ix), "n_diag": int(diag.sum())}
        deg = np.diff(ip) + (np.bincount(ix, minlength=n) if directed else diag)
        comps = connected_components(sp.csr_matrix((np.ones(len(ix)), ix, ip), shape=(n, n)),
                                     directed=False)[0] if n else 0
        paths = sum(1 for ln in data.split(b"\n") if ln.split(b"\t")[0] in (b"P", b"O"))
        edges = _stats_edges(st, directed)
        got = [n, edges, paths, int(comps), int(deg.max()) if n else 0, density(n, edges, directed)]
        assert got == [v for _, v in rec["stats"]], key


def test_unnamed_inputs_are_refused(tmp_path):
    import io

    from gfa2network_amd import compute_stats

    with pytest.raises(NotImplementedError):
        compute_stats("-")
    with pytest.raises(NotImplementedError):
        compute_stats(io.BytesIO(b"S\ta\n"))


def test_graph_stats_argument_checks():
    from gfa2network_amd import graph_stats

    with pytest.raises(TypeError):
        graph_stats(np.zeros((2, 2)))
    with pytest.raises(ValueError):
        graph_stats(sp.csr_matrix((2, 3)))


@pytest.mark.skipif(__import__("gfa2network_amd._native", fromlist=["x"]).device_count() > 0,
                    reason="a GPU is visible")
def test_stats_without_gpu_fail_loudly(tmp_path):
    from gfa2network_amd import compute_stats, graph_stats

    p = tmp_path / "a.gfa"
    p.write_bytes(b"S\ta\nL\ta\t+\tb\t+\t*\n")
    with pytest.raises(RuntimeError, match="G2N_E_DEVICE"):
        compute_stats(p)
    with pytest.raises(RuntimeError, match="G2N_E_DEVICE"):
        graph_stats(sp.csr_matrix(np.array([[0.0, 1.0], [0.0, 0.0]])))
