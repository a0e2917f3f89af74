"""GPU: every case of tests/golden/expected/pair_distance.json (recorded from the reference's
``genome_distance(G, A, B, method="mean")`` over the plain graph and over the graph a weight tag
builds) through ``genome_distance(..., method="mean")`` and ``distance --path A B --method mean``:
the value bit for bit, exception type and message, the list of warnings under
``simplefilter("always")``.  A graph with a negative, NaN or infinite length is refused with
NotImplementedError.  And ``method="min"`` still equals tests/golden/expected/distance.json."""
import contextlib
import io
import json
import sys
import warnings
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
import make_distance_golden as distgold  # noqa: E402
from make_pairdist_golden import KINDS, TAG, UNKNOWN, cases, exc_record, run_key, value  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = cases()
BAD = "edge weights must be finite and >= 0"


@pytest.fixture(scope="module")
def expected():
    return json.loads((GOLDEN / "expected" / "pair_distance.json").read_text())


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


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key,inp,raw", CASES, ids=[c[0] for c in CASES])
def test_mean(gpu, expected, monkeypatch, key, inp, raw, kind):
    from gfa2network_amd import genome_distance

    monkeypatch.delenv("GFANET_DISABLE_WARNINGS", raising=False)
    rec = expected[key]
    tag = TAG if kind == "weighted" else None
    for directed in (True, False):
        r = rec["runs"][run_key(kind, directed)]
        for a in rec["names"]:
            for b in rec["names"]:
                want = r["mean"][f"{a}|{b}"]
                args = (a.encode(), b.encode()) if raw else (a, b)
                d, exc, warned = run(lambda: genome_distance(str(inp), *args, method="mean", directed=directed,
                                                             raw_bytes_id=raw, weight_tag=tag))
                if want.get("bad"):
                    assert exc is not None and exc[0] == "NotImplementedError" and exc[1].startswith(BAD), (key, a, b)
                    continue
                assert (exc, warned) == (want_exc(want), want["warnings"]), (key, kind, a, b, directed)
                if want["value"] is not None:
                    assert type(d) is float and value(d) == want["value"], (key, kind, a, b, directed)
        other = r["other"]
        if other is not None:
            args = (other["a"].encode(), other["b"].encode()) if raw else (other["a"], other["b"])
            _d, exc, warned = run(lambda: genome_distance(str(inp), *args, method="median", directed=directed,
                                                          raw_bytes_id=raw, weight_tag=tag))
            assert (exc, warned) == (want_exc(other), other["warnings"]), (key, kind, directed)


@pytest.mark.parametrize("key,inp,raw", CASES, ids=[c[0] for c in CASES])
def test_mean_cli(gpu, expected, monkeypatch, key, inp, raw):
    """``distance IN --path A B --method mean`` prints the function's float; an unknown name is the
    CLI's SystemExit("unknown path: X")."""
    from gfa2network_amd import cli

    monkeypatch.delenv("GFANET_DISABLE_WARNINGS", raising=False)
    rec = expected[key]
    pre = ["--raw-bytes-id"] if raw else []
    for directed in (True, False):
        r = rec["runs"][run_key("hops", directed)]
        for a in rec["names"]:
            for b in rec["names"]:
                want = r["mean"][f"{a}|{b}"]
                argv = pre + ["distance", str(inp), "--path", a, b, "--method", "mean"] + \
                    ([] if directed else ["--undirected"])
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    _got, exc, warned = run(lambda: cli.main(argv))
                wexc = want_exc(want)
                if wexc is not None and wexc[0] == "KeyError":
                    wexc = ["SystemExit", f"unknown path: {UNKNOWN}"]
                assert (exc, warned) == (wexc, want["warnings"]), (key, a, b, directed)
                if want["value"] is None:
                    assert buf.getvalue() == ""
                else:
                    text = buf.getvalue()
                    assert text.endswith("\n") and value(float(text)) == want["value"], (key, a, b, directed)
                    assert text == f"{float.fromhex(want['value'])!r}\n"


def test_quadratic_warning_can_be_disabled(gpu, expected, monkeypatch):
    from gfa2network_amd import genome_distance

    inp = GOLDEN / "pair_inputs" / "many_pairs.gfa"
    want = expected["pair_inputs/many_pairs.gfa|raw=0"]["runs"][run_key("hops", True)]["mean"]["pa|pd"]
    assert any("quadratically" in w for w in want["warnings"])
    monkeypatch.setenv("GFANET_DISABLE_WARNINGS", "1")
    d, exc, warned = run(lambda: genome_distance(inp, "pa", "pd", method="mean"))
    assert exc is None and warned == [] and value(d) == want["value"]
    monkeypatch.setenv("GFANET_DISABLE_WARNINGS", "0")
    _d, _exc, warned = run(lambda: genome_distance(inp, "pa", "pd", method="mean"))
    assert warned == want["warnings"]


DIST_CASES = [c for c in distgold.cases() if c[0].startswith("dist_inputs/")]


@pytest.mark.parametrize("key,inp,raw", DIST_CASES, ids=[c[0] for c in DIST_CASES])
def test_min_is_unchanged(gpu, key, inp, raw):
    """method="min", spelled out, against distance.json: the CLI's stdout is the function's value."""
    from gfa2network_amd import genome_distance

    rec = json.loads((GOLDEN / "expected" / "distance.json").read_text())[key]
    for directed in (True, False):
        for a in rec["names"]:
            for b in rec["names"]:
                want = rec["distance"][f"{a}|{b}|directed={int(directed)}"]
                args = (a.encode(), b.encode()) if raw else (a, b)
                d, exc, warned = run(lambda: genome_distance(str(inp), *args, method="min", directed=directed,
                                                             raw_bytes_id=raw))
                wexc = want_exc(want)
                if wexc is not None and wexc[0] == "SystemExit" and wexc[1].startswith("unknown path: "):
                    name = distgold.UNKNOWN if a == distgold.UNKNOWN else b
                    wexc = ["KeyError", repr(name.encode() if raw else name)]
                assert (exc, warned) == (wexc, want["warnings"]), (key, a, b, directed)
                assert ("" if d is None else f"{d}\n") == want["stdout"], (key, a, b, directed)
                assert d is None or type(d) is int
