"""GPU: ``compute_stats`` and the ``stats`` CLI against the reference's recorded answers
(tests/golden/expected/stats.json, written by tests/golden/make_stats_golden.py): every input of
tests/golden/inputs and tests/golden/stats_inputs, directed on / off, strip_orientation on / off,
raw_bytes_id for the files with non-ASCII node names — the dict (values and their types, key
order), the CLI's stdout byte for byte, exceptions by type and message."""
import contextlib
import io
import json
import sys
import warnings
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
from make_stats_golden import cases  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = cases()


@pytest.fixture(scope="module")
def expected():
    return json.loads((GOLDEN / "expected" / "stats.json").read_text())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_compute_stats_matches_reference(gpu, expected, case):
    from gfa2network_amd import compute_stats
    from gfa2network_amd.cli import main

    key, inp, directed, strip, raw = case
    rec = expected[key]
    got = exc = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            got = compute_stats(str(inp), directed=directed, strip_orientation=strip, raw_bytes_id=raw)
        except Exception as e:  # noqa: BLE001 - compared with the recorded one
            exc = [type(e).__name__, str(e)]
        argv = (["--raw-bytes-id"] if raw else []) + ["stats", str(inp)]
        argv += [] if directed else ["--undirected"]
        argv += ["--strip-orientation"] if strip else []
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            try:
                main(argv)
            except Exception as e:  # noqa: BLE001 - the same failure as compute_stats's
                assert [type(e).__name__, str(e)] == exc
    assert exc == rec["exc"]
    if rec["stats"] is None:
        assert got is None
    else:
        pairs = [[k, v] for k, v in got.items()]
        assert pairs == rec["stats"]
        assert [type(v) for _, v in pairs] == [type(v) for _, v in rec["stats"]]
    assert buf.getvalue() == rec["stdout"]


def test_drb1_cli_lines(gpu, capsys):
    """The issue's acceptance line: the six lines `stats DRB1-3123_unsorted.gfa` prints."""
    from gfa2network_amd.cli import main

    main(["stats", str(GOLDEN / "inputs" / "DRB1-3123_unsorted.gfa")])
    out = capsys.readouterr().out
    assert out == ("nodes\t 3214\nedges\t 6236\npaths\t 12\ncomponents\t 1\nmax_degree\t 10\n"
                   "density\t 0.000603878\n")


def test_unsupported_record_warns_once(gpu):
    """The one-shot RuntimeWarning comes out once, as parse_gfa emits it."""
    from gfa2network_amd import compute_stats

    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        compute_stats(str(GOLDEN / "stats_inputs" / "paths_walks.gfa"))
    msgs = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]
    assert msgs == ["Skipping unsupported record: W"]
