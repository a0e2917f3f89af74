"""Host side of the node-to-node distances (no GPU): the checker of pair_util against NetworkX's
shortest_path_length (where networkx imports), the Python folds of genome_distance(method="mean") —
the 2^53 refusal, the order of additions, the empty lists —, the CLI's argument handling, the C ABI's
symbols and the completeness of tests/golden/expected/pair_distance.json."""
import inspect
import json
import sys
from pathlib import Path

import numpy as np
import pytest

import pair_util
from stats_util import csr_of

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
import make_pairdist_golden as gold  # noqa: E402

WEIGHTS = np.array([0.1, 0.2, 0.7, 0.3, 1.5, 0.0])


def random_graph(n, m, seed):
    rng = np.random.default_rng(seed)
    pairs = np.unique(np.stack([rng.integers(0, n, m), rng.integers(0, n, m)], axis=1), axis=0)
    ip, ix = csr_of(pairs[:, 0], pairs[:, 1], n)
    return ip, ix, WEIGHTS[rng.integers(0, len(WEIGHTS), len(ix))], rng


@pytest.mark.parametrize("weighted", [False, True])
def test_checker_against_networkx(weighted):
    """pair_util.table and pair_util.fold = the mean over all pairs as NetworkX computes it: one
    shortest_path_length(G, u, v, weight="weight") per pair, u outer, v inner, summed from 0.0."""
    nx = pytest.importorskip("networkx")
    n = 40
    ip, ix, val, rng = random_graph(n, 90, 5)
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    for u in range(n):
        for k in range(ip[u], ip[u + 1]):
            G.add_edge(u, int(ix[k]), **({"weight": float(val[k])} if weighted else {}))
    for trial in range(6):
        A = rng.integers(0, n, int(rng.integers(1, 9))).tolist()
        B = rng.integers(0, n, int(rng.integers(1, 9))).tolist() + [A[0]]
        T = pair_util.table(ip, ix, val if weighted else None, n, A, B)
        total, count = 0.0, 0
        for i, u in enumerate(A):
            for t, v in enumerate(B):
                try:
                    d = nx.shortest_path_length(G, u, v, weight="weight")
                except nx.NetworkXNoPath:
                    assert T[i, t] == np.inf
                    continue
                assert float(d).hex() == float(T[i, t]).hex(), (trial, u, v)
                total += d
                count += 1
        mean, c = pair_util.fold(T)
        assert c == count
        assert (mean is None) if count == 0 else (mean.hex() == (total / count).hex())
        if not weighted:
            S, C = pair_util.sums(T)
            assert int(S.sum()) == int(total) and int(C.sum()) == count


def test_checker_edges():
    ip, ix = csr_of([0, 1], [1, 2], 4)
    T = pair_util.table(ip, ix, None, 4, [0, -1, 2, 0], [2, 0, -1, 3, 2])
    inf = np.inf
    assert T.tolist() == [[2, 0, inf, inf, 2], [inf] * 5, [0, inf, inf, inf, 0], [2, 0, inf, inf, 2]]
    S, C = pair_util.sums(T)
    assert S.tolist() == [4, 0, 0, 4] and C.tolist() == [3, 0, 2, 3] and S.dtype == np.uint64 == C.dtype
    assert pair_util.table(ip, ix, None, 4, [], [1]).shape == (0, 1)
    assert pair_util.table(ip, ix, None, 4, [1], []).shape == (1, 0)
    assert pair_util.fold(np.full((2, 3), inf)) == (None, 0)


def test_mean_of_sums():
    from gfa2network_amd.api import NetworkXNoPath, mean_of_sums

    u = lambda *x: np.array(x, dtype=np.uint64)  # noqa: E731
    assert mean_of_sums(u(3, 4), u(2, 1)) == 7 / 3
    assert mean_of_sums(u(0), u(5)) == 0.0
    # totals past 2^32 and the sum of several near 2^52: Python ints, then one division
    assert mean_of_sums(u(2**52 - 1, 2**52), u(2**40, 3)) == float(2**53 - 1) / (2**40 + 3)
    with pytest.raises(NotImplementedError, match="2\\^53"):
        mean_of_sums(u(2**52, 2**52), u(1, 1))
    with pytest.raises(NotImplementedError, match="2\\^53"):
        mean_of_sums(u(2**63, 2**63), u(1, 1))  # (the uint64 sum would wrap to 0)
    for S, C in ((u(), u()), (u(0, 0), u(0, 0))):
        with pytest.raises(NetworkXNoPath, match="no path between node sets"):
            mean_of_sums(S, C)


def test_mean_of_table_order():
    """The fold is u outer, v inner, left to right from 0.0 — not numpy's pairwise sum, not a
    column-major walk: on 0.1 / 0.2 / 0.7 the three differ in the last bits."""
    from gfa2network_amd.api import NetworkXNoPath, mean_of_table

    rng = np.random.default_rng(11)
    T = np.array([0.1, 0.2, 0.7, 0.3])[rng.integers(0, 4, (37, 29))].cumsum(axis=1)
    T[rng.random(T.shape) < 0.2] = np.inf
    total, count = 0.0, 0
    for i in range(T.shape[0]):
        for t in range(T.shape[1]):
            if T[i, t] != np.inf:
                total += T[i, t]
                count += 1
    got = mean_of_table(T)
    assert got.hex() == (total / count).hex() == pair_util.fold(T)[0].hex()
    other = 0.0
    for x in T.T.reshape(-1).tolist():
        if x != np.inf:
            other += x
    assert other != total  # the shape does tell the orders apart
    assert mean_of_table(np.array([[0.0]])) == 0.0
    for empty in (np.zeros((0, 3)), np.zeros((3, 0)), np.full((2, 2), np.inf)):
        with pytest.raises(NetworkXNoPath, match="no path between node sets"):
            mean_of_table(empty)


def test_cli_arguments(capsys):
    from gfa2network_amd import cli

    p = cli._parser(extensions=True)
    assert p.parse_args(["distance", "x.gfa", "--path", "a", "b"]).method == "min"
    assert p.parse_args(["distance", "x.gfa", "--path", "a", "b", "--method", "mean"]).method == "mean"
    for argv in (["distance", "x.gfa", "--seq", "A", "C", "--method", "mean"],
                 ["distance", "x.gfa", "--path", "a", "b", "--method", "median"],
                 ["distance", "x.gfa", "--method", "mean"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    assert "--method mean takes --path" in capsys.readouterr().err


def test_function_signatures():
    import gfa2network_amd as g

    sig = inspect.signature(g.genome_distance)
    assert sig.parameters["method"].default == "min" and sig.parameters["method"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(g.node_distances).parameters) == ["A", "sources", "targets", "weighted", "device",
                                                                     "return_info"]
    assert list(inspect.signature(g.pair_sums).parameters)[:3] == ["A", "sources", "targets"]
    for name in ("node_distances", "pair_sums"):
        assert name in g.__all__


def test_abi_symbols_and_host_checks():
    from gfa2network_amd import _native

    lib = _native.load()
    for sym in ("g2n_csr_pair_distances", "g2n_csr_pair_distances_host", "g2n_csr_pair_distances_weighted",
                "g2n_csr_pair_distances_weighted_host", "g2n_pair_distances_from_path"):
        assert hasattr(lib, sym) and sym in _native.EXPORTED
    header = (ROOT / "include" / "g2n.h").read_text()
    assert "#define G2N_PAIR_SUMS 0" in header and "#define G2N_PAIR_TABLE 1" in header
    assert (_native.PAIR_SUMS, _native.PAIR_TABLE) == (0, 1)
    # what the wrapper refuses before a GPU is touched
    ip, ix = np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    with pytest.raises(TypeError):
        _native.csr_pair_distances_host(ip, ix.astype(np.int64), None, 2, [0], [1], True)
    with pytest.raises(ValueError):
        _native.csr_pair_distances_host(ip, ix, None, 3, [0], [1], True)
    with pytest.raises(ValueError):
        _native.csr_pair_distances_host(ip, ix, np.ones(2), 2, [0], [1], False)  # no weighted sums
    with pytest.raises(TypeError):
        _native.csr_pair_distances_host(ip, ix, np.ones(2, dtype=np.float32), 2, [0], [1], True)
    with pytest.raises(ValueError):
        _native.csr_pair_distances_host(ip, ix, np.ones(3), 2, [0], [1], True)
    import scipy.sparse as sp
    from gfa2network_amd import node_distances, pair_sums

    with pytest.raises(TypeError):
        node_distances(np.zeros((2, 2)), [0], [1])
    with pytest.raises(ValueError):
        pair_sums(sp.csr_matrix((2, 3)), [0], [1])
    with pytest.raises(ValueError, match="finite edge lengths"):
        node_distances(sp.csr_matrix(np.array([[0.0, -1.0], [0.0, 0.0]])), [0], [1], weighted=True)


def test_golden_is_complete():
    """pair_distance.json holds every case, both graphs and both directions, with the cases the checks
    need: values, each exception kind, runs past 1000 pairs (and one of exactly 1000 without the
    warning), and a weighted mean on which the order of additions shows."""
    exp = json.loads((GOLDEN / "expected" / "pair_distance.json").read_text())
    assert sorted(exp) == sorted(k for k, _inp, _raw in gold.cases())
    kinds, warned = set(), 0
    for rec in exp.values():
        assert rec["names"][-1] == gold.UNKNOWN
        assert sorted(rec["runs"]) == sorted(gold.run_key(k, d) for k in gold.KINDS for d in (True, False))
        for r in rec["runs"].values():
            assert sorted(r["mean"]) == sorted(f"{a}|{b}" for a in rec["names"] for b in rec["names"])
            for pair, m in r["mean"].items():
                if m.get("bad"):
                    kinds.add("bad")
                    continue
                kinds.add("value" if m["exc"] is None else m["exc"][1])
                quad = any("quadratically" in w for w in m["warnings"])
                warned += quad
                if m["exc"] is None:
                    assert quad == (rec["pairs"][pair] > 1000), pair
            if r["other"] is not None and r["other"]["exc"][1] == "ValueError":
                assert r["other"]["exc"][2] == f"unknown method: {gold.OTHER_METHOD}"
                kinds.add("other")
    assert kinds >= {"value", "bad", "other", "KeyError", "NetworkXNoPath", "NodeNotFound", "UnicodeDecodeError",
                     "OverflowError"}
    assert warned >= 8
    many = exp["pair_inputs/many_pairs.gfa|raw=0"]
    assert many["pairs"]["pc|pd"] == 1000 and many["pairs"]["pa|pb"] == 1020
    # weights whose sums round: the mean of the weighted table is not the mean of exactly summed values
    from fractions import Fraction

    nd = exp["wdist_inputs/nondyadic_mean.gfa|raw=0"]["runs"][gold.run_key("weighted", True)]["mean"]
    vals = [float.fromhex(m["value"]) for m in nd.values() if not m.get("bad") and m["value"] is not None]
    assert len(vals) >= 9 and any(Fraction(v).denominator > 2**40 for v in vals)
