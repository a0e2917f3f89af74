"""GPU: every case of tests/golden/expected/distance.json (recorded from the reference) through
``genome_distance_matrix``, ``cli.main(["distance", IN, "--path", A, B])`` and ``distance-matrix``:
values bit for bit, labels, exception type and message, the list of warnings under
``simplefilter("always")``, stdout and the written files."""
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
from make_distance_golden import METHODS, SUFFIXES, cases, exc_record, value  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = cases()


@pytest.fixture(scope="module")
def expected():
    return json.loads((GOLDEN / "expected" / "distance.json").read_text())


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


@pytest.mark.parametrize("key,inp,raw", CASES, ids=[c[0] for c in CASES])
def test_matrix(gpu, expected, key, inp, raw):
    from gfa2network_amd import genome_distance_matrix

    for method in METHODS:
        rec = expected[key]["matrix"][method]
        M, exc, warned = run(lambda: genome_distance_matrix(str(inp), method=method, raw_bytes_id=raw))
        assert exc == want_exc(rec), (key, method)
        assert warned == rec["warnings"], (key, method)
        if rec["values"] is None:
            continue
        assert [str(x) for x in M.index] == rec["labels"] == [str(x) for x in M.columns], (key, method)
        got = np.asarray(M)
        assert got.dtype == np.float64 and got.shape == (len(rec["labels"]),) * 2
        assert [[value(x) for x in row] for row in got] == rec["values"], (key, method)


@pytest.mark.parametrize("key,inp,raw", CASES, ids=[c[0] for c in CASES])
def test_distance_cli(gpu, expected, key, inp, raw):
    from gfa2network_amd import cli

    rec = expected[key]
    pre = ["--raw-bytes-id"] if raw else []
    for directed in (True, False):
        for a in rec["names"]:
            for b in rec["names"]:
                want = rec["distance"][f"{a}|{b}|directed={int(directed)}"]
                buf = io.StringIO()
                argv = pre + ["distance", str(inp), "--path", a, b] + ([] if directed else ["--undirected"])
                with contextlib.redirect_stdout(buf):
                    _got, exc, warned = run(lambda: cli.main(argv))
                assert (buf.getvalue(), exc, warned) == (want["stdout"], want_exc(want), want["warnings"]), \
                    (key, a, b, directed)


@pytest.mark.parametrize("key,inp,raw", CASES, ids=[c[0] for c in CASES])
def test_distance_matrix_cli(gpu, expected, tmp_path, key, inp, raw):
    from gfa2network_amd import cli

    pre = ["--raw-bytes-id"] if raw else []
    for suffix in SUFFIXES:
        want = expected[key]["output"][suffix]
        dest = tmp_path / ("m" + suffix)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            _got, exc, warned = run(lambda: cli.main(pre + ["distance-matrix", str(inp), "-o", str(dest)]))
        assert (exc, warned) == (want_exc(want), want["warnings"]), (key, suffix)
        if want["bytes"] is not None:
            assert dest.read_bytes().hex() == want["bytes"], (key, suffix)


def test_function_surface(gpu, expected):
    """genome_distance returns the CLI's int; load_paths returns the reference's dict; an unknown
    name is a KeyError before anything is searched."""
    from gfa2network_amd import genome_distance, genome_distance_matrix, load_paths
    from gfa2network_amd.api import NetworkXNoPath

    inp = GOLDEN / "dist_inputs" / "repeat_name.gfa"
    assert load_paths(inp) == {"p1": ["1"], "p2": ["3"]}
    assert load_paths(inp, raw_bytes=True) == {b"p1": [b"1"], b"p2": [b"3"]}
    assert load_paths(str(inp) + ".gz") == {"p1": ["1"], "p2": ["3"]}
    d = genome_distance(inp, "p1", "p2")
    assert d == 2 and type(d) is int
    assert genome_distance(inp, "p2", "p1", directed=False) == 2
    with pytest.raises(NetworkXNoPath, match="no path between node sets"):
        genome_distance(inp, "p2", "p1")
    with pytest.raises(KeyError) as e:
        genome_distance(inp, "p1", "zz")
    assert e.value.args == ("zz",)
    M, info = genome_distance_matrix(GOLDEN / "inputs" / "DRB1-3123_unsorted.gfa", return_info=True)
    assert M.shape == (12, 12) and info["batches"] == 1 and info["levels"] > 0 and info["launches"] > 0
    with pytest.raises(FileNotFoundError):
        genome_distance_matrix(GOLDEN / "no_such_file.gfa")
