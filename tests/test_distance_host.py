"""CPU: the path-distance call surface without a GPU — the CLI schema, the exports, the C struct's
layout, the completeness of tests/golden/expected/distance.json, g2n_load_paths through the C ABI
against a pure-Python restatement of the reference's two rules, the loud failure without a device,
and the contract itself: the tables D / S / C, computed by scipy over the CPU oracle's CSR
(dist_util) and put through the shim's own formulas, reproduce every recorded matrix."""
import ctypes
import gzip
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from dist_util import same, tables

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
from make_distance_golden import METHODS, SUFFIXES, UNKNOWN, cases  # noqa: E402  (the generator's own list)


@pytest.fixture(scope="module")
def expected():
    return json.loads((GOLDEN / "expected" / "distance.json").read_text())


def text_of(inp: Path) -> bytes:
    data = inp.read_bytes()
    return gzip.decompress(data) if inp.name.endswith(".gz") else data


def python_paths(data: bytes):
    """The reference's two rules restated: a P / O record is a line whose first field is exactly P or
    O with at least three fields; a repeated name keeps its position and takes the last steps; a step
    is a comma-separated piece of field 2 without one trailing sign.  Also the first record (line,
    bytes) whose name or step is not ASCII."""
    paths, bad = {}, None
    for k, line in enumerate(data.split(b"\n")):
        f = line.split(b"\t")
        if f[0] not in (b"P", b"O") or len(f) < 3:
            continue
        steps = [s[:-1] if s[-1:] in (b"+", b"-") else s for s in f[2].split(b",")]
        paths[f[1]] = steps
        if bad is None:
            for x in [f[1]] + steps:
                if max(x, default=0) >= 0x80:
                    bad = (k, x)
                    break
    return paths, bad


def test_distance_parsers_take_the_reference_flags():
    from gfa2network_amd.cli import _parser

    p = _parser()
    a = p.parse_args(["distance", "x.gfa", "--path", "a", "b"])
    assert (a.cmd, a.gfa, a.path, a.seq, a.directed, a.backend, a.verbose) == \
        ("distance", "x.gfa", ["a", "b"], None, True, "networkx", False)
    a = p.parse_args(["--raw-bytes-id", "distance", "x.gfa", "--seq", "A", "C", "--undirected", "--verbose",
                      "--backend", "igraph"])
    assert (a.seq, a.path, a.directed, a.backend, a.verbose, a.raw_bytes_id) == \
        (["A", "C"], None, False, "igraph", True, True)
    for bad in (["distance", "x.gfa"], ["distance", "x.gfa", "--path", "a"], ["distance", "--path", "a", "b"],
                ["distance", "x.gfa", "--path", "a", "b", "--seq", "A", "C"],
                ["distance", "x.gfa", "--path", "a", "b", "--directed", "--undirected"],
                ["distance", "x.gfa", "--path", "a", "b", "--backend", "cugraph"],
                ["distance", "x.gfa", "--path", "a", "b", "--method", "mean"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    a = p.parse_args(["distance-matrix", "x.gfa", "-o", "m.csv"])
    assert (a.cmd, a.gfa, a.output, a.method, a.backend, a.verbose) == \
        ("distance-matrix", "x.gfa", "m.csv", "min", "networkx", False)
    a = p.parse_args(["distance-matrix", "x.gfa", "--output", "m.npy", "--method", "mean", "--verbose"])
    assert (a.output, a.method, a.verbose) == ("m.npy", "mean", True)
    for bad in (["distance-matrix", "x.gfa"], ["distance-matrix", "-o", "m.csv"],
                ["distance-matrix", "x.gfa", "-o", "m.csv", "--method", "max"],
                ["distance-matrix", "x.gfa", "-o", "m.csv", "--undirected"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_seq_and_igraph_are_refused_by_main(capsys):
    from gfa2network_amd.cli import main

    with pytest.raises(SystemExit) as e:
        main(["distance", "x.gfa", "--seq", "A", "C"])
    assert e.value.code == 2 and "--seq" in capsys.readouterr().err
    with pytest.raises(NotImplementedError):
        main(["distance-matrix", "x.gfa", "-o", "m.csv", "--backend", "igraph"])


def test_distance_functions_are_exported():
    import gfa2network_amd
    from gfa2network_amd import _native, api

    for name in ("load_paths", "genome_distance", "genome_distance_matrix", "path_distances"):
        assert name in gfa2network_amd.__all__ and callable(getattr(gfa2network_amd, name))
        assert name in api.__all__
    lib = _native.load()
    for sym in ("g2n_load_paths", "g2n_paths_get", "g2n_paths_free", "g2n_csr_path_distances",
                "g2n_csr_path_distances_host", "g2n_distances_from_path"):
        assert sym in _native.EXPORTED and hasattr(lib, sym)
    try:
        import networkx as nx
    except ImportError:
        assert issubclass(api.NodeNotFound, KeyError) and issubclass(api.NetworkXNoPath, Exception)
        assert str(api.NodeNotFound("Node 9 not found in graph")) == "Node 9 not found in graph"
    else:
        assert api.NodeNotFound is nx.NodeNotFound and api.NetworkXNoPath is nx.NetworkXNoPath


def test_dist_info_struct_matches_header(tmp_path):
    from gfa2network_amd import _native

    py = _native.DistInfo
    lines = ['printf("sizeof %zu\\n", sizeof(g2n_dist_info));']
    lines += [f'printf("{f[0]} %zu\\n", offsetof(g2n_dist_info, {f[0]}));' for f in py._fields_]
    lines += ['printf("MIN %d\\nMEAN %d\\n", G2N_DIST_MIN, G2N_DIST_MEAN);']
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
    assert (int(got["MIN"]), int(got["MEAN"])) == (_native.DIST_MIN, _native.DIST_MEAN)


def test_fixture_holds_every_case(expected):
    """distance.json has one record for every input (three folders; raw_bytes_id for the non-ASCII
    files), each with both methods, every ordered pair of its names plus the unknown one in both
    directions, and the three output suffixes: none may be left out."""
    want = [c[0] for c in cases()]
    assert len(want) == len(set(want)) and len(want) >= 80
    assert sorted(expected) == sorted(want)
    names = {c[1].name for c in cases()}
    for f in ("inputs", "stats_inputs", "dist_inputs"):
        assert {p.name for p in (GOLDEN / f).iterdir()} <= names
    for key, rec in expected.items():
        assert sorted(rec["matrix"]) == sorted(METHODS) and sorted(rec["output"]) == sorted(SUFFIXES), key
        for m in rec["matrix"].values():
            assert (m["values"] is None) != (m["exc"] is None), key
        assert rec["names"][-1] == UNKNOWN
        assert sorted(rec["distance"]) == sorted(f"{a}|{b}|directed={d}" for a in rec["names"] for b in rec["names"]
                                                 for d in (0, 1)), key
    # what the issue records of the reference's behaviour
    drb1 = expected["inputs/DRB1-3123_unsorted.gfa|raw=0"]["matrix"]["min"]
    assert len(drb1["labels"]) == 12 and len(drb1["values"]) == 12
    for one in ("inputs/sample_path.gfa", "stats_inputs/one_segment.gfa", "stats_inputs/self_loop.gfa"):
        assert expected[one + "|raw=0"]["matrix"]["min"]["values"] == [["0x0.0p+0"]], one
    for nf in ("inputs/p_o_records.gfa", "stats_inputs/paths_walks.gfa"):
        assert expected[nf + "|raw=0"]["matrix"]["min"]["exc"][1] == "NodeNotFound", nf
    twice = expected["dist_inputs/unsupported_record.gfa|raw=0"]["matrix"]["min"]["warnings"]
    assert twice == ["Skipping unsupported record: W"] * 2


def test_load_paths_through_the_c_abi():
    """g2n_load_paths on every fixture file against the restated rules: names in first-occurrence
    order, the last record's steps, an empty field as one empty step, the .gz copies, and the first
    non-ASCII name or step with its line."""
    from gfa2network_amd import _native

    seen_repeat = seen_empty = seen_gz = seen_bad = 0
    for _key, inp, raw in cases():
        if raw:
            continue
        ps = _native.Paths(str(inp))
        if inp.name.endswith(".gz"):
            try:
                data = text_of(inp)
            except (OSError, EOFError):
                continue  # (a damaged member: the prefix rule is the gzip fixtures' to check)
            seen_gz += 1
        else:
            data = text_of(inp)
        want, bad = python_paths(data)
        assert ps.status == _native.OK, inp
        assert ps.as_dict() == want and list(ps.as_dict()) == list(want), inp
        assert (ps.bad_line, ps.bad_bytes) == ((-1, b"") if bad is None else bad), inp
        n_records = sum(1 for ln in data.split(b"\n") if ln.split(b"\t")[0] in (b"P", b"O") and ln.count(b"\t") >= 2)
        seen_repeat += n_records > len(want)
        seen_empty += any(b"" in v for v in want.values())
        seen_bad += bad is not None
    assert seen_repeat and seen_empty and seen_gz >= 2 and seen_bad >= 3
    ps = _native.Paths(str(GOLDEN / "dist_inputs" / "repeat_name.gfa"))
    assert ps.as_dict() == {b"p1": [b"1"], b"p2": [b"3"]} and ps.path_ptr.tolist() == [0, 1, 2]
    assert _native.Paths(str(GOLDEN / "dist_inputs" / "empty_steps.gfa")).as_dict()[b"e"] == [b""]
    assert _native.Paths(str(GOLDEN / "dist_inputs" / "trailing_comma.gfa")).as_dict()[b"a"] == [b"1", b""]
    missing = _native.Paths(str(GOLDEN / "no_such_file.gfa"))
    assert missing.status == _native.E_IO and missing.n_paths == 0


def test_load_paths_on_a_text_past_one_thread(tmp_path):
    """A text large enough to be cut into one range per host thread: the same paths, order and line."""
    from gfa2network_amd import _native

    rng = np.random.default_rng(5)
    lines = []
    for k in range(60_000):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            lines.append(b"S\t%d\t*" % k)
        elif kind == 1:
            lines.append(b"L\t%d\t+\t%d\t+\t*" % (k, k + 1))
        else:
            steps = b",".join(b"%d%s" % (int(x), rng.choice([b"+", b"-", b""])) for x in rng.integers(0, 999, 12))
            lines.append((b"P" if kind == 2 else b"O") + b"\tp%d\t" % int(rng.integers(0, 20_000)) + steps + b"\t*")
    lines[41_234] = b"P\tq\t1+,\xc3\xa9-,2+"
    lines[50_000] = b"P\t\xff\t1+"
    data = b"\n".join(lines)
    assert len(data) > 2 << 20
    p = tmp_path / "big.gfa"
    p.write_bytes(data)
    want, bad = python_paths(data)
    ps = _native.Paths(str(p))
    got = ps.as_dict()
    assert got == want and list(got) == list(want)
    assert (ps.bad_line, ps.bad_bytes) == bad == (41_234, b"\xc3\xa9")


def test_contract_formulas_match_the_fixture(oracle_lib, expected):
    """The tables g2n_csr_path_distances defines, taken here with scipy over the CPU oracle's directed
    asymmetric CSR from the restated paths and put through the shim's own formulas, are the
    reference's matrix for every recorded case that returns one — bit for bit."""
    from gfa2network_amd.api import mean_table, min_table

    checked = 0
    for key, inp, raw in cases():
        rec = expected[key]["matrix"]
        if rec["min"]["values"] is None:
            continue
        data = text_of(inp)
        o = oracle_lib.run(data, directed=True, asymmetric=True, dtype="float64")
        assert o.status == 0, key
        blob, offs = o.names_blob.tobytes(), o.names_offsets
        ids = {blob[offs[i]:offs[i + 1]]: i for i in range(o.n_nodes)}
        paths, _bad = python_paths(data)
        assert [n.decode() for n in paths] == rec["min"]["labels"], key
        D, S, C = tables(o.sum_indptr, o.sum_indices, o.n_nodes, [[ids[s] for s in v] for v in paths.values()])
        M = min_table(D)
        iu = np.triu_indices(len(M), 1)
        M.T[iu] = M[iu]
        for method, got in (("min", M), ("mean", mean_table(S, C))):
            want = np.array([[float("inf") if x == "inf" else float.fromhex(x) for x in row]
                             for row in rec[method]["values"]], dtype=np.float64).reshape(len(paths), len(paths))
            assert same(got, want), (key, method)
        checked += 1
    assert checked >= 40


def test_table_formulas():
    from gfa2network_amd.api import mean_table, min_table

    D = np.array([[0, 3, 0xFFFFFFFF], [0xFFFFFFFF, 0xFFFFFFFF, 2], [1, 0, 0]], dtype=np.uint32)
    assert min_table(D).tolist() == [[0.0, 3.0, np.inf], [np.inf, 0.0, 2.0], [1.0, 0.0, 0.0]]
    S = np.array([[0, 10, 0], [1, 0, 0], [0, 7, 0]], dtype=np.uint64)
    C = np.array([[1, 3, 0], [0, 1, 0], [0, 4, 2]], dtype=np.uint64)
    M = mean_table(S, C)
    assert M.tolist() == [[0.0, 11 / 3, np.inf], [11 / 3, 0.0, 7 / 4], [np.inf, 7 / 4, 0.0]]
    assert mean_table(np.zeros((0, 0), np.uint64), np.zeros((0, 0), np.uint64)).shape == (0, 0)
    with pytest.raises(NotImplementedError):
        mean_table(np.array([[0, 2**53], [0, 0]], dtype=np.uint64), np.ones((2, 2), dtype=np.uint64))


def test_unnamed_inputs_and_igraph_are_refused():
    import io

    from gfa2network_amd import genome_distance, genome_distance_matrix, load_paths, path_distances

    for fn in (load_paths, genome_distance_matrix, lambda p: genome_distance(p, "a", "b")):
        with pytest.raises(NotImplementedError):
            fn("-")
        with pytest.raises(NotImplementedError):
            fn(io.BytesIO(b"S\ta\n"))
    with pytest.raises(NotImplementedError):
        genome_distance_matrix("x.gfa", backend="igraph")
    with pytest.raises(TypeError):
        path_distances(np.zeros((2, 2)), [[0]])
    with pytest.raises(ValueError):
        path_distances(sp.csr_matrix((2, 3)), [[0]])


@pytest.mark.skipif(__import__("gfa2network_amd._native", fromlist=["x"]).device_count() > 0,
                    reason="a GPU is visible")
def test_distances_without_gpu_fail_loudly(tmp_path):
    from gfa2network_amd import genome_distance, genome_distance_matrix, load_paths, path_distances

    p = tmp_path / "a.gfa"
    p.write_bytes(b"S\ta\nS\tb\nL\ta\t+\tb\t+\t*\nP\tx\ta+\nP\ty\tb+\n")
    with pytest.raises(RuntimeError, match="G2N_E_DEVICE"):
        genome_distance_matrix(p)
    with pytest.raises(RuntimeError, match="G2N_E_DEVICE"):
        genome_distance(p, "x", "y")
    with pytest.raises(RuntimeError, match="G2N_E_DEVICE"):
        load_paths(p)
    with pytest.raises(RuntimeError, match="G2N_E_DEVICE"):
        path_distances(sp.csr_matrix(np.array([[0.0, 1.0], [0.0, 0.0]])), [[0], [1]])
