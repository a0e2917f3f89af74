"""GPU: every case of tests/golden/expected/seq_distance.json (recorded from the reference) through
``sequence_distance`` and ``sequence_nodes``: the value and its type, exception type and message, the
list of warnings under ``simplefilter("always")`` and the node lists."""
import json
import sys
import warnings
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
from make_seqdist_golden import MAX_LISTED, cases, exc_record, outcome, record_of, unpack  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = cases()


@pytest.fixture(scope="module")
def expected():
    return json.loads((GOLDEN / "expected" / "seq_distance.json").read_text())


def run(fn):
    """(result, [type name, message] of the exception, warning messages) of fn()"""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = exc = None
        try:
            got = fn()
        except KeyboardInterrupt:
            raise
        except BaseException as e:  # noqa: BLE001 - compared as data
            exc = exc_record(e)[1:]
    return got, exc, [str(w.message) for w in caught]


@pytest.mark.parametrize("key,inp,raw,directed", CASES, ids=[c[0] for c in CASES])
def test_sequence_distance(gpu, expected, key, inp, raw, directed):
    from gfa2network_amd import sequence_distance

    rec, this = record_of(expected, key)
    build = this["build"]
    if build["exc"] is not None:  # the build's own error, whatever is asked
        got, exc, warned = run(lambda: sequence_distance(str(inp), "A", "C", directed=directed, raw_bytes_id=raw))
        assert (got, exc, warned) == (None, build["exc"][1:], build["warnings"]), key
        return
    q = [unpack(x) for x in rec["queries"]]
    for i, a in enumerate(q):
        for j, b in enumerate(q):
            d, e, w = outcome(this, i, j)
            got, exc, warned = run(lambda: sequence_distance(str(inp), a, b, directed=directed, raw_bytes_id=raw))
            assert (got, exc, warned) == (d, None if e is None else e[1:], build["warnings"] + w), (key, a, b)
            assert got is None or type(got) is int, (key, a, b)


@pytest.mark.parametrize("key,inp,raw,directed", CASES, ids=[c[0] for c in CASES])
def test_sequence_nodes(gpu, expected, key, inp, raw, directed):
    """The matcher on its own: the node list of every listed sequence, in node order."""
    from gfa2network_amd import sequence_nodes

    rec, this = record_of(expected, key)
    if this["build"]["exc"] is not None:
        got, exc, warned = run(lambda: sequence_nodes(str(inp), "A", "C", directed=directed, raw_bytes_id=raw))
        assert (got, exc, warned) == (None, this["build"]["exc"][1:], this["build"]["warnings"]), key
        return
    q = [unpack(x) for x in rec["queries"]]
    first = outcome(this, 0, 0)
    if first[1] is not None and first[1][1] == "UnicodeDecodeError":
        return  # (the orientation check's decode of a raw key: test_sequence_distance compares it)
    listed = [(unpack(s), [unpack(n) for n in nodes]) for s, nodes in rec["seq2nodes"]]
    for k in range(0, len(listed), 2):
        (sa, na), (sb, nb) = listed[k], listed[min(k + 1, len(listed) - 1)]
        got, exc, _w = run(lambda: sequence_nodes(str(inp), sa, sb, directed=directed, raw_bytes_id=raw))
        assert exc is None and got == (na, nb), (key, sa, sb)
    known = {s for s, _n in listed}
    for a in q:
        if a not in known and len(listed) < MAX_LISTED:
            _got, exc, _w = run(lambda: sequence_nodes(str(inp), a, a, directed=directed, raw_bytes_id=raw))
            assert exc == ["KeyError", f"\"sequence(s) {a!r}, {a!r} not found\""], (key, a)


def test_tab_or_newline_in_a_query(gpu):
    """No field holds a tab or a newline: such a query is on no node, whatever surrounds it."""
    from gfa2network_amd import sequence_distance, sequence_nodes

    inp = GOLDEN / "seq_inputs" / "fourth_field.gfa"
    assert sequence_nodes(inp, "ACGT", "A:i:4") == (["t5", "t6"], ["t2"])
    for bad in ("ACGT\tLN:i:4", "ACGT\n", "4\tACGT", "\t", "\n", "ACGT\tLN:i:4\tRC:i:7\nS"):
        with pytest.raises(KeyError) as e:
            sequence_distance(inp, "ACGT", bad)
        assert e.value.args == (f"sequence(s) {bad!r} not found",)
        with pytest.raises(KeyError) as e:
            sequence_nodes(inp, bad.encode(), "ACGT")
        assert e.value.args == (f"sequence(s) {bad.encode()!r} not found",)


def test_function_surface(gpu):
    from gfa2network_amd import sequence_distance, sequence_nodes
    from gfa2network_amd.api import NetworkXNoPath

    inp = GOLDEN / "seq_inputs" / "shared_seq.gfa"
    d = sequence_distance(inp, "AC", "GT")
    assert d == 3 and type(d) is int
    assert sequence_distance(inp, b"AC", b"GT") == 3 and sequence_distance(str(inp) + ".gz", "AC", "GT") == 3
    assert sequence_distance(inp, "GT", "AC") == 1 and sequence_distance(inp, "GT", "AC", directed=False) == 1
    assert sequence_distance(inp, "TTT", "TTT") == 0
    with pytest.raises(NetworkXNoPath, match="no path between sequences"):
        sequence_distance(inp, "AC", "CCC")
    assert sequence_nodes(inp, "GT", "AC") == (["3", "4", "5"], ["1", "2"])
    assert sequence_nodes(inp, "GT", "AC", raw_bytes_id=True) == ([b"3", b"4", b"5"], [b"1", b"2"])
    d, info = sequence_distance(inp, "AC", "GT", return_info=True)
    assert d == 3 and info["n_s_lines"] == 8 and info["n_with_seq"] == 8
    assert info["candidates_a"] == 2 and info["candidates_b"] == 3 and info["levels"] >= 3 and info["batches"] == 1
    for f in ("ms_scan", "ms_match", "ms_bfs"):
        assert info[f] > 0.0
    with pytest.raises(FileNotFoundError):
        sequence_distance(GOLDEN / "no_such_file.gfa", "A", "C")
