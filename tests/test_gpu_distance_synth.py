"""GPU: ``genome_distance_matrix`` on one synthetic file of 20 k segments / 60 k links (synth.py)
with 40 P / O lines appended, in the decimal-name layout and with hashed names (the names blob the
steps are looked up in is rendered from ids in one, gathered from the text in the other), plain and
gzip-compressed.  The generator's links are local (a long chain-like graph): with up to 40 steps a
path, the 40 searches' joint frontier holds a few thousand nodes for its first hundred levels (past
kDistNarrowCap = 2048: the wide regime) and far fewer for the nearly two thousand that follow (the
narrow one) — the smallest size that takes both, which the test checks with scipy before it
relies on it.  The matrix must equal dist_util's scipy answer over ``parse_gfa(path,
asymmetric=True)``'s matrix and node list, for both methods."""
import gzip

import numpy as np
import pytest

from dist_util import level_sizes, reference_matrix, same, tables

pytestmark = pytest.mark.gpu

N_SEG, N_LINK, N_PATHS = 20_000, 60_000, 40


@pytest.fixture(scope="module", params=["decimal", "hashed"])
def synth_file(request, tmp_path_factory):
    from gfa2network_amd import _native, synth

    _native.load()
    text = synth.host_bytes(N_SEG, N_LINK, seed=13, names=request.param)
    lines = text.rstrip(b"\n").split(b"\n")
    seg = [ln.split(b"\t")[1] for ln in lines if ln[:1] == b"S"]
    rng = np.random.default_rng(3)
    paths = {}
    for k in range(N_PATHS):  # 1 to 40 steps each, repeats allowed; P and O records
        steps = [seg[int(i)] for i in rng.integers(0, len(seg), int(rng.integers(1, 41)))]
        paths[b"p%d" % k] = steps
        sign = b"+-"[k % 2:k % 2 + 1]
        lines.append((b"O" if k % 5 == 0 else b"P") + b"\tp%d\t" % k + b",".join(s + sign for s in steps) + b"\t*")
    text = b"\n".join(lines) + b"\n"
    d = tmp_path_factory.mktemp("dist_synth")
    plain = d / f"{request.param}.gfa"
    plain.write_bytes(text)
    gz = d / f"{request.param}.gfa.gz"
    with gzip.open(gz, "wb", compresslevel=1) as fh:
        fh.write(text)
    return plain, gz, paths


def test_synth_distances(gpu, synth_file):
    from gfa2network_amd import convert_format, genome_distance, genome_distance_matrix, load_paths, parse_gfa

    plain, gz, paths = synth_file
    assert load_paths(plain, raw_bytes=True) == paths
    A, nodes = parse_gfa(plain, build_graph=False, build_matrix=True, asymmetric=True, return_node_list=True)
    A = convert_format(A, "csr")
    ids = {name: i for i, name in enumerate(nodes)}
    lists = [[ids[s.decode()] for s in steps] for steps in paths.values()]
    D, S, C = tables(A.indptr.astype(np.int64), A.indices.astype(np.int64), A.shape[0], lists)
    sizes = level_sizes(A.indptr, A.indices, A.shape[0], lists)
    assert sizes.max() > 2048 and (sizes <= 2048).sum() > 1000  # both regimes (kDistNarrowCap)
    for method in ("min", "mean"):
        want = reference_matrix(D, S, C, method)
        M, info = genome_distance_matrix(plain, method=method, return_info=True)
        assert [str(x) for x in M.index] == [k.decode() for k in paths]
        assert same(np.asarray(M), want), method
        assert info["batches"] == 1 and info["levels"] == len(sizes) - 1
        assert info["launches"] < info["levels"]  # (3 launches a wide level: the narrow regime carried the rest)
        assert same(np.asarray(genome_distance_matrix(gz, method=method)), want), method
        assert same(np.asarray(genome_distance_matrix(plain, method=method)), want), method  # the same on every run
    i, j = next((i, j) for i in range(N_PATHS) for j in range(N_PATHS) if i != j and D[i, j] != 0xFFFFFFFF)
    assert genome_distance(plain, f"p{i}", f"p{j}") == int(D[i, j])
