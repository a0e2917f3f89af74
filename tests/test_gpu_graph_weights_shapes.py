"""GPU: ``graph_matrix(path, weight_tag=...)`` — the LAST finish (g2n_kernels.hip k_row_finish<RowLast> behind
g2n_graph_weights_from_path) — against a dict-overwrite loop over the records (graph_weight_util), on
generated files that hold every row shape of the kernel, through each route the weight parse can
take; and the weighted ``genome_distance_matrix`` over 73 paths (two search batches) against scipy's
Dijkstra, the mean in the reference's order of additions."""
import numpy as np
import pytest

import graph_weight_util as gw
from wdist_util import mean_matrix, min_matrix, same, tables

pytestmark = pytest.mark.gpu

# name style, options.test_flags, the record spelled as a float
ROUTES = {
    "decimal_ext": ("dec", 0, None),          # decimal names in S order: the extended tile-local parse
    "decimal_no_ext": ("dec", "NO_EXT", None),  # the same through K1 + the lean parse
    "hashed": ("hash", 0, None),              # names without a pattern: the lean hash route
    "general": ("dec", 0, 3),                 # one f-typed tag: the general parse's weights
}


@pytest.fixture(scope="module")
def shapes():
    n, records = gw.shape_records()
    return n, records, {d: gw.last_csr(records, n, d) for d in (True, False)}


def build(tmp_path, monkeypatch, names, records, flags, float_at, **kw):
    from gfa2network_amd import _native as nat
    from gfa2network_amd import graph_matrix

    p = tmp_path / "shape.gfa"
    if float_at is not None:  # (the first record from there on that has a weight to spell)
        float_at = next((k for k in range(float_at, len(records)) if records[k][2] is not None), None)
    p.write_bytes(gw.gfa_bytes(names, records, float_at=float_at))
    monkeypatch.setattr(nat, "TEST_FLAGS", nat.TEST_NO_EXT_LEAN if flags == "NO_EXT" else 0)
    try:
        return graph_matrix(p, weight_tag="RC", **kw)
    finally:
        monkeypatch.setattr(nat, "TEST_FLAGS", 0)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("directed", [True, False])
def test_row_shapes(gpu, tmp_path, monkeypatch, shapes, route, directed):
    n, records, want = shapes
    style, flags, float_at = ROUTES[route]
    names = gw.dec_names(n) if style == "dec" else gw.hashed_names(n)
    A, nodes = build(tmp_path, monkeypatch, names, records, flags, float_at, directed=directed, return_node_list=True)
    assert nodes == [x.decode() for x in names]
    assert A.indptr.dtype == np.int32 and A.indices.dtype == np.int32
    assert gw.same_csr(A, want[directed]), (route, directed)
    again = build(tmp_path, monkeypatch, names, records, flags, float_at, directed=directed)
    assert gw.same_csr(again, want[directed]), (route, directed)


@pytest.mark.parametrize("route", list(ROUTES))
def test_tiny_files(gpu, tmp_path, monkeypatch, route):
    """n = 1 (one node, a self loop whose last tagged record is in the middle) and a file without edges."""
    style, flags, float_at = ROUTES[route]
    names = (gw.dec_names if style == "dec" else gw.hashed_names)(3)
    one = [(0, 0, None), (0, 0, 4), (0, 0, 7), (0, 0, 9), (0, 0, None)]
    for directed in (True, False):
        A = build(tmp_path, monkeypatch, names[:1], one, flags, float_at, directed=directed)
        assert gw.same_csr(A, gw.last_csr(one, 1, directed))
        assert A.data.tolist() == [9.0]
        E = build(tmp_path, monkeypatch, names, [], flags, None, directed=directed)
        assert gw.same_csr(E, gw.last_csr([], 3, directed)) and E.nnz == 0


def test_without_a_tag_every_edge_is_one(gpu, tmp_path, shapes):
    from gfa2network_amd import graph_matrix

    n, records, _want = shapes
    p = tmp_path / "plain.gfa"
    p.write_bytes(gw.gfa_bytes(gw.dec_names(n), records))
    for tag in (None, ""):
        A = graph_matrix(p, weight_tag=tag)
        assert gw.same_csr(A, gw.last_csr([(u, v, None) for u, v, _w in records], n, True))


# ---------------------------------------------------------------- distances over it ------
def distance_file():
    """80 nodes on a ring with chords, lengths 0.1 / 0.2 / 0.7 (f-typed: not dyadic, so the order of
    additions shows), every third chord first tagged and then repeated without a tag; 70 single-node
    paths and three of several steps at positions 0, 30 and 72 (the last in the second batch)."""
    n = 80
    lengths = (0.1, 0.2, 0.7)
    records = []
    for k in range(n):
        records.append((k, (k + 1) % n, lengths[k % 3]))
        if k % 3 == 0:
            records.append((k, (k + 7) % n, None))
            records.append((k, (k + 7) % n, lengths[(k // 3) % 3]))
            records.append((k, (k + 7) % n, None))
    multi = {0: [3, 4, 5, 50], 30: [10, 11, 12, 13, 40], 72: [60, 20, 21, 22]}
    paths, single = [], iter(range(n))
    for k in range(73):
        paths.append(multi[k] if k in multi else [next(single)])
    names = gw.dec_names(n)
    out = [b"S\t" + nm + b"\t*\n" for nm in names]
    for u, v, w in records:
        out.append(b"L\t" + names[u] + b"\t+\t" + names[v] + b"\t+\t0M" + (b"" if w is None else b"\tRC:f:%r" % w) + b"\n")
    for k, steps in enumerate(paths):
        out.append(b"P\tp%d\t" % k + b",".join(names[s] + b"+" for s in steps) + b"\t*\n")
    return n, records, paths, b"".join(out)


def test_distance_matrix_two_batches(gpu, tmp_path):
    from gfa2network_amd import genome_distance, genome_distance_matrix, graph_matrix, path_distances

    n, records, paths, text = distance_file()
    p = tmp_path / "dist.gfa"
    p.write_bytes(text)
    csr = gw.last_csr(records, n, True)
    A = graph_matrix(p, weight_tag="RC")
    assert gw.same_csr(A, csr)
    D, S, C = tables(*csr, n, paths)
    want_min = min_matrix(D)
    iu = np.triu_indices(len(paths), 1)
    want_min.T[iu] = want_min[iu]
    want_mean = gw.reference_mean(csr, n, paths)
    # the reference's order of additions is not S[i][j] + S[j][i]: the case must show it
    other = mean_matrix(S, C)
    assert not same(want_mean, other) and np.allclose(want_mean, other, rtol=1e-12, atol=0)
    for _ in range(2):
        got_min, info = genome_distance_matrix(p, "min", weight_tag="RC", return_info=True)
        assert info["batches"] == 2 and info["batch_paths"] == 64
        assert same(np.asarray(got_min), want_min)
        got_mean, info = genome_distance_matrix(p, "mean", weight_tag="RC", return_info=True)
        assert info["batches"] == 2
        assert same(np.asarray(got_mean), want_mean)
    # path_distances keeps its documented definition and its bits
    assert same(path_distances(A, paths, method="mean", weighted=True), other)
    d = genome_distance(p, "p0", "p30", weight_tag="RC")
    assert type(d) is float and d == D[0, 30]
    assert type(genome_distance(p, "p0", "p30")) is int
