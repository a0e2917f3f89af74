"""GPU: ``compute_stats`` on one synthetic file of 200 k segments / 800 k links (synth.py), in the
decimal-name layout (the tile-local decimal-id build, whose names the ASCII check never needs) and
with hashed names (the hash tiers, whose names blob it scans), plain and gzip-compressed:
it must equal ``graph_stats`` of ``convert_format(parse_gfa(path, asymmetric=True), "csr")``, and
scipy's connected_components / numpy's degree and edge counts over that matrix; ``paths`` is the
number of P lines the test wrote into the text."""
import gzip

import numpy as np
import pytest

from stats_util import checker

pytestmark = pytest.mark.gpu

N_SEG, N_LINK, N_PATHS = 200_000, 800_000, 37


@pytest.fixture(scope="module", params=["decimal", "hashed"])
def synth_file(request, tmp_path_factory):
    from gfa2network_amd import _native, synth

    _native.load()
    text = synth.host_bytes(N_SEG, N_LINK, seed=11, names=request.param)
    lines = text.split(b"\n")
    assert not any(ln[:1] in (b"P", b"O") for ln in lines)  # the generator writes no paths
    seg = [ln.split(b"\t")[1] for ln in lines[:4000] if ln[:1] == b"S"][:3]
    step = len(lines) // N_PATHS
    for k in range(N_PATHS):  # P lines spread over the file (and one line that only looks like one)
        lines.insert(1 + k * (step + 1), b"P\tp%d\t%s+,%s+\t*" % (k, seg[0], seg[1]))
    lines.insert(5, b"Px\tnot_a_path\t" + seg[2] + b"+\t*")
    text = b"\n".join(lines)
    d = tmp_path_factory.mktemp("stats_synth")
    plain = d / f"{request.param}.gfa"
    plain.write_bytes(text)
    gz = d / f"{request.param}.gfa.gz"
    with gzip.open(gz, "wb", compresslevel=1) as fh:
        fh.write(text)
    return plain, gz


@pytest.mark.parametrize("directed", [True, False])
def test_synth_stats(gpu, synth_file, directed):
    from gfa2network_amd import compute_stats, convert_format, graph_stats, parse_gfa

    plain, gz = synth_file
    got = compute_stats(plain, directed=directed)
    assert list(got) == ["nodes", "edges", "paths", "components", "max_degree", "density"]
    assert got["paths"] == N_PATHS and got["nodes"] == N_SEG
    A = convert_format(parse_gfa(plain, build_graph=False, build_matrix=True, directed=directed, asymmetric=True),
                       "csr")
    via_matrix = graph_stats(A, directed=directed)
    assert {k: v for k, v in got.items() if k != "paths"} == via_matrix
    want = checker(A.indptr.astype(np.int64), A.indices.astype(np.int64), A.shape[0], directed)
    assert via_matrix == want
    assert compute_stats(gz, directed=directed) == got
    assert compute_stats(plain, directed=directed) == got  # and the same on every run
