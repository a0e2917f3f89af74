"""GPU: every case of tests/golden/expected/wdistance.json (recorded from the reference over the graph
``parse_gfa(build_graph=True, weight_tag="RC")`` builds) through ``graph_matrix``,
``genome_distance_matrix``, ``genome_distance`` and ``sequence_distance`` with ``weight_tag="RC"``:
the matrix's arrays and every value bit for bit, labels, exception type and message, the list of
warnings under ``simplefilter("always")``.  A graph with a negative, NaN or infinite length is
refused with NotImplementedError.  And ``distance --seq`` through ``cli.main`` against the hop
distances of tests/golden/expected/seq_distance.json."""
import contextlib
import io
import json
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
import make_seqdist_golden as seqgold  # noqa: E402
from make_wdistance_golden import METHODS, TAG, UNKNOWN, cases, csr_digest, edges_csr, exc_record, value  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = cases()
BAD = "edge weights must be finite and >= 0"


@pytest.fixture(scope="module")
def expected():
    return json.loads((GOLDEN / "expected" / "wdistance.json").read_text())


def run(fn):
    """(result, [type name, message] of the exception, warning messages) of fn()"""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = exc = None
        try:
            got = fn()
        except KeyboardInterrupt:
            raise
        except BaseException as e:  # noqa: BLE001 - compared as data (SystemExit too)
            exc = exc_record(e)[1:]
    return got, exc, [str(w.message) for w in caught]


def want_exc(rec):
    return None if rec["exc"] is None else rec["exc"][1:]


def refused(exc) -> bool:
    return exc is not None and exc[0] == "NotImplementedError" and exc[1].startswith(BAD)


@pytest.mark.parametrize("key,inp,raw", CASES, ids=[c[0] for c in CASES])
def test_graph_matrix(gpu, expected, key, inp, raw):
    from gfa2network_amd import graph_matrix

    for directed in (True, False):
        g = expected[key]["graph"][str(int(directed))]
        A, exc, warned = run(lambda: graph_matrix(str(inp), directed=directed, weight_tag=TAG, raw_bytes_id=raw))
        if g["exc"] is not None and g["exc"][1] == "UnicodeDecodeError" and "ascii" in g["exc"][2]:
            continue  # (the graph path's ASCII decode of node keys: graph_matrix returns the matrix path's list)
        assert (exc, warned) == (want_exc(g), g["warnings"]), (key, directed)
        if g["n"] is None:
            continue
        assert A.format == "csr" and A.dtype == np.float64 and A.shape == (g["n"], g["n"])
        got = (np.asarray(A.indptr, dtype=np.int32), np.asarray(A.indices, dtype=np.int32), A.data)
        if g["edges"] is None:
            assert csr_digest(*got) == g["digest"], (key, directed)
            continue
        want = edges_csr(g["n"], [(i, j, float.fromhex(w)) for i, j, w in g["edges"]], directed)
        assert [x.tobytes() for x in got[:2]] == [x.tobytes() for x in want[:2]], (key, directed)
        assert [value(x) for x in got[2]] == [value(x) for x in want[2]], (key, directed)


@pytest.mark.parametrize("key,inp,raw", CASES, ids=[c[0] for c in CASES])
def test_matrix(gpu, expected, key, inp, raw):
    from gfa2network_amd import genome_distance_matrix

    for method in METHODS:
        rec = expected[key]["matrix"][method]
        M, exc, warned = run(lambda: genome_distance_matrix(str(inp), method=method, raw_bytes_id=raw,
                                                            weight_tag=TAG))
        if rec.get("bad"):
            assert refused(exc), (key, method, exc)
            continue
        assert exc == want_exc(rec), (key, method)
        assert warned == rec["warnings"], (key, method)
        if rec["values"] is None:
            continue
        assert [str(x) for x in M.index] == rec["labels"] == [str(x) for x in M.columns], (key, method)
        got = np.asarray(M)
        assert got.dtype == np.float64 and got.shape == (len(rec["labels"]),) * 2
        assert [[value(x) for x in row] for row in got] == rec["values"], (key, method)


@pytest.mark.parametrize("key,inp,raw", CASES, ids=[c[0] for c in CASES])
def test_path_pairs(gpu, expected, key, inp, raw):
    """``distance --path A B`` of the reference's CLI over the weighted graph = genome_distance(...,
    weight_tag=): the printed number's value as a float, SystemExit("unknown path: X") = KeyError(X)."""
    from gfa2network_amd import genome_distance

    rec = expected[key]
    for directed in (True, False):
        for a in rec["names"]:
            for b in rec["names"]:
                want = rec["distance"][f"{a}|{b}|directed={int(directed)}"]
                args = (a.encode(), b.encode()) if raw else (a, b)
                d, exc, warned = run(lambda: genome_distance(str(inp), *args, directed=directed, raw_bytes_id=raw,
                                                             weight_tag=TAG))
                if want.get("bad"):
                    assert refused(exc), (key, a, b, directed, exc)
                    continue
                wexc = want_exc(want)
                if wexc is not None and wexc[0] == "SystemExit" and wexc[1].startswith("unknown path: "):
                    name = UNKNOWN if a == UNKNOWN else b
                    wexc = ["KeyError", repr(name.encode() if raw else name)]
                assert (exc, warned) == (wexc, want["warnings"]), (key, a, b, directed)
                if want["value"] is not None:
                    assert type(d) is float and value(d) == want["value"], (key, a, b, directed)


@pytest.mark.parametrize("key,inp,raw", CASES, ids=[c[0] for c in CASES])
def test_sequence_pairs(gpu, expected, key, inp, raw):
    from gfa2network_amd import sequence_distance, sequence_nodes

    rec = expected[key]["seq"]
    for directed in (True, False):
        for pair, want in rec["runs"][str(int(directed))].items():
            a, b = pair.split("|")
            d, exc, warned = run(lambda: sequence_distance(str(inp), a, b, directed=directed, raw_bytes_id=raw,
                                                           weight_tag=TAG))
            if want.get("bad"):
                assert refused(exc), (key, pair, directed, exc)
                continue
            assert (exc, warned) == (want_exc(want), want["warnings"]), (key, pair, directed)
            assert want_exc(want["function"]) == want_exc(want)
            if want["value"] is not None:
                assert type(d) is float and value(d) == want["value"] == want["function"]["value"], (key, pair)
            if exc is not None:
                continue
            # the node sets do not depend on the tag
            assert sequence_nodes(str(inp), a, b, directed=directed, raw_bytes_id=raw, weight_tag=TAG) == \
                sequence_nodes(str(inp), a, b, directed=directed, raw_bytes_id=raw)


def test_function_surface(gpu):
    """None and "" are the hop calls, unchanged; a tag returns floats; the refusal names its reason."""
    from gfa2network_amd import genome_distance, genome_distance_matrix, sequence_distance
    from gfa2network_amd.api import NetworkXNoPath

    inp = GOLDEN / "wdist_inputs" / "tag_then_none.gfa"
    for tag in (None, ""):
        d = genome_distance(inp, "p1", "p2", weight_tag=tag)
        assert d == genome_distance(inp, "p1", "p2") and type(d) is int
        s = sequence_distance(inp, "AC", "GT", weight_tag=tag)
        assert s == 1 and type(s) is int
        assert np.array_equal(np.asarray(genome_distance_matrix(inp, weight_tag=tag)),
                              np.asarray(genome_distance_matrix(inp)))
    assert genome_distance(inp, "p1", "p2", weight_tag="RC") == 5.25
    assert genome_distance(str(inp) + ".gz", "p1", "p2", weight_tag="RC") == 5.25
    assert genome_distance(inp, "p1", "p2", directed=False, weight_tag="RC") == 2.0
    assert genome_distance(inp, "p1", "p2", weight_tag="XX") == 1.0  # no record carries XX: every edge is 1
    s, info = sequence_distance(inp, "AC", "GT", weight_tag="RC", return_info=True)
    assert s == 5.0 and type(s) is float and info["launches"] > 0
    with pytest.raises(NetworkXNoPath, match="no path between node sets"):
        genome_distance(GOLDEN / "wdist_inputs" / "unreachable.gfa", "p1", "p2", weight_tag="RC")
    with pytest.raises(NetworkXNoPath, match="no path between sequences"):
        sequence_distance(GOLDEN / "wdist_inputs" / "unreachable.gfa", "AC", "CCC", weight_tag="RC")
    with pytest.raises(NotImplementedError, match="edge weights must be finite and >= 0"):
        genome_distance(GOLDEN / "wdist_inputs" / "winning_neg.gfa", "p1", "p2", weight_tag="RC")
    with pytest.raises(OverflowError, match="int too large to convert to float"):
        genome_distance(GOLDEN / "wdist_inputs" / "huge_int.gfa", "p1", "p2", weight_tag="RC")
    assert genome_distance(GOLDEN / "wdist_inputs" / "huge_int.gfa", "p1", "p2") == 1


# ------------------------------------------------------------ distance --seq routing ------
SEQ_CASES = [c for c in seqgold.cases() if c[0].startswith("seq_inputs/")]


@pytest.fixture(scope="module")
def seq_expected():
    return json.loads((GOLDEN / "expected" / "seq_distance.json").read_text())


@pytest.mark.parametrize("key,inp,raw,directed", SEQ_CASES, ids=[c[0] for c in SEQ_CASES])
def test_distance_seq_cli(gpu, seq_expected, key, inp, raw, directed):
    """``cli.main(["distance", IN, "--seq", A, B])``: stdout ``f"{result}\\n"``, the exception and the
    warnings of every recorded pair of queries that argv can carry (str queries not starting with
    "-"; the recorded ``bytes`` ones have another repr in the KeyError)."""
    from gfa2network_amd import cli

    rec, this = seqgold.record_of(seq_expected, key)
    pre = ["--raw-bytes-id"] if raw else []
    tail = [] if directed else ["--undirected"]
    build = this["build"]

    def call(a, b):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            _got, exc, warned = run(lambda: cli.main(pre + ["distance", str(inp), "--seq", a, b] + tail))
        return buf.getvalue(), exc, warned

    if build["exc"] is not None:
        assert call("A", "C") == ("", build["exc"][1:], build["warnings"]), key
        return
    q = [seqgold.unpack(x) for x in rec["queries"]]
    seen = 0
    for i, a in enumerate(q):
        for j, b in enumerate(q):
            if not (isinstance(a, str) and isinstance(b, str)) or a.startswith("-") or b.startswith("-"):
                continue
            d, e, w = seqgold.outcome(this, i, j)
            want = ("" if d is None else f"{d}\n", None if e is None else e[1:], build["warnings"] + w)
            assert call(a, b) == want, (key, a, b)
            seen += 1
    assert seen >= 4, key


def test_distance_seq_cli_refuses_igraph(gpu):
    from gfa2network_amd import cli

    inp = GOLDEN / "seq_inputs" / "shared_seq.gfa"
    with pytest.raises(SystemExit):
        cli.main(["distance", str(inp), "--seq", "AC", "GT", "--backend", "igraph"])
