"""Host: the weighted-distance golden file holds every case; the dict-overwrite checker
(graph_weight_util) agrees with the reference's recorded graph edges on the hand-written inputs, and
with NetworkX's own ``add_edge`` + ``to_scipy_sparse_array`` on the shape generators."""
import gzip
import json
import sys
from pathlib import Path

import numpy as np
import pytest

import graph_weight_util as gw

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
from make_wdistance_golden import TAG, cases, edges_csr  # noqa: E402


@pytest.fixture(scope="module")
def expected():
    return json.loads((GOLDEN / "expected" / "wdistance.json").read_text())


def test_golden_holds_every_case(expected):
    keys = [c[0] for c in cases()]
    assert sorted(keys) == sorted(expected) and len(keys) == len(set(keys))
    folders = {k.split("/")[0] for k in keys}
    assert folders == {"wdist_inputs", "inputs", "stats_inputs", "dist_inputs"}
    for key in keys:
        rec = expected[key]
        assert set(rec["graph"]) == {"0", "1"} and set(rec["matrix"]) == {"min", "mean"}, key
        assert set(rec["seq"]["runs"]) == {"0", "1"}, key


def test_golden_covers_the_semantics(expected):
    """The recorded reference graphs show each rule the LAST finish implements."""
    def edges(name, directed=True):
        g = expected[f"wdist_inputs/{name}|raw=0"]["graph"][str(int(directed))]
        return {(i, j): float.fromhex(w) for i, j, w in g["edges"]}

    e = edges("tag_then_none.gfa")
    assert e[(0, 1)] == 5.0 and e[(1, 2)] == 0.25 and e[(0, 3)] == 9.0 and e[(3, 0)] == 2.0 and e[(2, 3)] == 1.0
    u = edges("tag_then_none.gfa", directed=False)
    assert u.get((0, 3), u.get((3, 0))) == 2.0  # (a, d) then (d, a): one edge, the later record's weight
    z = edges("z_then_num.gfa")
    assert z[(0, 1)] == 0.5 and z[(1, 2)] == 7.0 and z[(0, 2)] == 1.0
    s = edges("self_loop_zero.gfa")
    assert s[(0, 0)] == 3.0 and s[(0, 1)] == 0.0 and str(s[(1, 2)]) == "-0.0" and s[(2, 3)] == 1e-320
    assert edges("losing_bad.gfa") == {(0, 1): 2.5, (1, 2): 4.0}
    for name in ("winning_inf.gfa", "winning_nan.gfa", "winning_neg.gfa"):
        rec = expected[f"wdist_inputs/{name}|raw=0"]
        assert rec["graph"]["1"]["bad"] and rec["graph"]["0"]["bad"] and rec["matrix"]["min"] == {"bad": True}
    assert expected["wdist_inputs/huge_int.gfa|raw=0"]["graph"]["1"]["exc"][1] == "OverflowError"
    assert expected["wdist_inputs/missing_step.gfa|raw=0"]["matrix"]["min"]["exc"][1] == "NodeNotFound"
    assert "inf" in expected["wdist_inputs/unreachable.gfa|raw=0"]["matrix"]["mean"]["values"][0]


@pytest.mark.parametrize("inp", sorted((GOLDEN / "wdist_inputs").iterdir()), ids=lambda p: p.name)
def test_checker_agrees_with_the_reference(expected, inp):
    data = inp.read_bytes()
    if inp.name.endswith(".gz"):
        data = gzip.decompress(data)
    for directed in (True, False):
        g = expected[f"wdist_inputs/{inp.name}|raw=0"]["graph"][str(int(directed))]
        if g["exc"] is not None:
            assert g["exc"][1] == "OverflowError"
            with pytest.raises(OverflowError):
                gw.link_records(data, TAG.encode())
            continue
        names, records = gw.link_records(data, TAG.encode())
        assert len(names) == g["n"]
        want = edges_csr(g["n"], [(i, j, float.fromhex(w)) for i, j, w in g["edges"]], directed)
        got = gw.last_csr(records, len(names), directed)
        assert [x.tobytes() for x in got[:2]] == [x.tobytes() for x in want[:2]]
        assert [float(x).hex() for x in got[2]] == [float(x).hex() for x in want[2]]


@pytest.mark.parametrize("directed", [True, False])
def test_checker_agrees_with_networkx(directed):
    nx = pytest.importorskip("networkx")
    n, records = gw.shape_records(scale=10)
    G = nx.DiGraph() if directed else nx.Graph()
    G.add_nodes_from(range(n))
    for u, v, w in records:  # what the graph build does with a record (a weight only when it has one)
        if w is None:
            G.add_edge(u, v)
        else:
            G.add_edge(u, v, weight=float(w))
    A = nx.to_scipy_sparse_array(G, nodelist=range(n), weight="weight", format="csr", dtype=np.float64)
    A.sort_indices()
    ip, ix, d = gw.last_csr(records, n, directed)
    assert A.indptr.tolist() == ip.tolist() and A.indices.tolist() == ix.tolist()
    assert np.asarray(A.data, dtype=np.float64).tobytes() == d.tobytes()


def test_reference_mean_is_the_symmetric_sum_up_to_rounding():
    """The running total per cell and S[i][j] + S[j][i] are the same sum in two orders: equal up to
    rounding, symmetric, 0.0 on the diagonal (where the orders differ in the last bit is the GPU
    shape test's case, which asserts that they do)."""
    import wdist_util

    records = [(0, 1, 0.1), (1, 2, 0.2), (2, 3, 0.7), (3, 0, 0.1), (1, 3, 0.7)]
    csr = gw.last_csr(records, 4, True)
    paths = [[0, 1, 2], [3, 1], [2, 0, 3]]
    _D, S, C = wdist_util.tables(*csr, 4, paths)
    a, b = gw.reference_mean(csr, 4, paths), wdist_util.mean_matrix(S, C)
    assert np.allclose(a, b, rtol=1e-12, atol=0) and np.array_equal(a, a.T) and not a.diagonal().any()


def test_distance_seq_needs_a_named_file(capsys):
    """``distance --seq`` is routed to sequence_distance; an input that is no named file is a usage error
    that names the flag and the function, before any GPU work."""
    from gfa2network_amd.cli import main

    for gfa in ("no-such-file.gfa", "-"):
        with pytest.raises(SystemExit) as e:
            main(["distance", gfa, "--seq", "A", "C"])
        err = capsys.readouterr().err
        assert e.value.code == 2 and "--seq" in err and "sequence_distance" in err and gfa in err
