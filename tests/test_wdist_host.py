"""CPU: the weighted path distances' surface — exported symbols, the g2n_wdist_info layout, the
argument errors that are raised on the host before any device call, the checker (wdist_util) against
the NetworkX call the reference makes, and the two table formulas."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from wdist_util import mean_matrix, min_matrix, same, tables

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_weighted_symbols_are_exported():
    from gfa2network_amd import _native, api

    lib = _native.load()
    for sym in ("g2n_csr_path_distances_weighted", "g2n_csr_path_distances_weighted_host"):
        assert sym in _native.EXPORTED and hasattr(lib, sym)
    for name in ("weighted_min_table", "weighted_mean_table", "path_distances"):
        assert name in api.__all__ and callable(getattr(api, name))
    assert callable(_native.csr_path_distances_weighted_host)


def test_wdist_info_struct_matches_header(tmp_path):
    from gfa2network_amd import _native

    py = _native.WDistInfo
    assert [f[0] for f in py._fields_] == ["rounds", "launches", "batches", "batch_paths", "ms_search", "ms_tables"]
    lines = ['printf("sizeof %zu\\n", sizeof(g2n_wdist_info));']
    lines += [f'printf("{f[0]} %zu\\n", offsetof(g2n_wdist_info, {f[0]}));' for f in py._fields_]
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


@pytest.mark.parametrize("bad", [-1.0, -1e-300, float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("fmt", ["csr", "coo", "csc"])
def test_bad_values_raise_before_the_device(bad, fmt):
    """No GPU here: a device call would raise RuntimeError, not ValueError."""
    from gfa2network_amd import path_distances

    A = sp.csr_matrix(np.array([[0.0, 1.0, 0.0], [0.0, 0.0, bad], [2.0, 0.0, 0.0]])).asformat(fmt)
    for method in ("min", "mean"):
        with pytest.raises(ValueError):
            path_distances(A, [[0], [2]], method=method, weighted=True)


def test_complex_and_non_square_raise_before_the_device():
    from gfa2network_amd import path_distances

    Z = sp.csr_matrix(np.array([[0, 1 + 0j], [1, 0]]))
    with pytest.raises(TypeError):
        path_distances(Z, [[0], [1]], weighted=True)
    with pytest.raises(TypeError):
        path_distances(Z.tocoo(), [[0], [1]], weighted=True)
    with pytest.raises(ValueError):
        path_distances(sp.csr_matrix((2, 3), dtype=np.float64), [[0]], weighted=True)
    with pytest.raises(TypeError):
        path_distances(np.zeros((2, 2)), [[0]], weighted=True)


def test_native_wrapper_checks_its_arrays():
    from gfa2network_amd import _native

    ip, ix = np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    ptr, steps = np.array([0, 1, 2]), np.array([0, 1])
    with pytest.raises(TypeError):
        _native.csr_path_distances_weighted_host(ip, ix, np.ones(2, dtype=np.float32), 2, ptr, steps, False)
    with pytest.raises(TypeError):
        _native.csr_path_distances_weighted_host(ip, ix.astype(np.int64), np.ones(2), 2, ptr, steps, False)
    with pytest.raises(ValueError):
        _native.csr_path_distances_weighted_host(ip, ix, np.ones(3), 2, ptr, steps, False)
    with pytest.raises(ValueError):
        _native.csr_path_distances_weighted_host(ip, ix, np.ones(2), 3, ptr, steps, False)
    with pytest.raises(ValueError):
        _native.csr_path_distances_weighted_host(ip, ix, np.ones(2), 2, np.array([0, 1, 3]), steps, True)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_checker_matches_the_references_networkx_call(seed):
    """The reference's distance helpers call nx.multi_source_dijkstra_path_length(G, nodes,
    weight="weight") on a DiGraph: the checker's scipy search returns the same bits."""
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(seed)
    n = 60
    pairs = np.unique(np.stack([rng.integers(0, n, 200), rng.integers(0, n, 200)], axis=1), axis=0)
    kinds = [rng.random(len(pairs)) * 10.0 ** rng.integers(-3, 4, len(pairs)),
             rng.integers(0, 6, len(pairs)).astype(np.float64), rng.integers(0, 50, len(pairs)) * 0.1,
             rng.random(len(pairs))]
    w = kinds[seed]
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    rows, cols, w = pairs[order, 0], pairs[order, 1], w[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    G.add_weighted_edges_from(zip(rows.tolist(), cols.tolist(), w.tolist()))
    paths = [[0], rng.integers(0, n, 7).tolist(), [5, 5, 9], list(range(20, 40))]
    D, S, C = tables(indptr, cols, w, n, paths)
    for i, p in enumerate(paths):
        d = nx.multi_source_dijkstra_path_length(G, set(p), weight="weight")
        for j, q in enumerate(paths):
            reached = [d[v] for v in q if v in d]
            assert int(C[i, j]) == len(reached)
            assert same(D[i, j], min(reached) if reached else np.inf)
            total = 0.0
            for x in reached:
                total += x
            assert same(S[i, j], total)


def test_table_formulas():
    from gfa2network_amd.api import weighted_mean_table, weighted_min_table

    inf = np.inf
    D = np.array([[0.5, 0.1, inf], [0.30000000000000004, 7.0, 2.5], [inf, inf, 0.0]])
    M = weighted_min_table(D)
    assert same(M, [[0.0, 0.1, inf], [0.30000000000000004, 0.0, 2.5], [inf, inf, 0.0]]) and same(M, min_matrix(D))
    assert D[0, 0] == 0.5  # (a copy)
    S = np.array([[0.0, 0.1, 0.0], [0.2, 0.0, 1e16], [0.0, 1.0, 0.0]])
    C = np.array([[3, 1, 0], [2, 1, 1], [0, 2, 4]], dtype=np.uint64)
    M = weighted_mean_table(S, C)
    want = [[0.0, (0.1 + 0.2) / 3.0, inf], [(0.2 + 0.1) / 3.0, 0.0, (1e16 + 1.0) / 3.0],
            [inf, (1.0 + 1e16) / 3.0, 0.0]]
    assert same(M, want) and same(M, mean_matrix(S, C))
    assert same(weighted_mean_table(np.zeros((0, 0)), np.zeros((0, 0), dtype=np.uint64)), np.zeros((0, 0)))
    assert same(weighted_min_table(np.zeros((0, 0))), np.zeros((0, 0)))
