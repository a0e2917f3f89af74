"""GPU: ``node_components`` and the ``components`` CLI against the reference's recorded answers
(tests/golden/expected/components.json, written by tests/golden/make_components_golden.py): every
case of the stats fixture — labels, nodes, exceptions by type and message — and the CLI's listing
on stdout and with ``-o`` byte for byte, ``--sizes`` against ``np.bincount``."""
import json
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
from make_components_golden import unrle  # noqa: E402
from make_stats_golden import cases  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = cases()


@pytest.fixture(scope="module")
def expected():
    return json.loads((GOLDEN / "expected" / "components.json").read_text())


def cli(argv):
    """(exception as [type, message] or None) of main(argv)."""
    from gfa2network_amd.cli import main

    try:
        main(argv)
    except Exception as e:  # noqa: BLE001 - compared with the expected one
        return [type(e).__name__, str(e)]
    return None


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_node_components_match_reference(gpu, expected, case, tmp_path, capfd):
    from gfa2network_amd import node_components, parse_gfa

    key, inp, directed, strip, raw = case
    rec = expected[key]
    got = exc = None
    flags = (["--raw-bytes-id"] if raw else [])
    tail = ([] if directed else ["--undirected"]) + (["--strip-orientation"] if strip else [])
    dest = tmp_path / "components.tsv"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            got = node_components(str(inp), directed=directed, strip_orientation=strip, raw_bytes_id=raw)
        except Exception as e:  # noqa: BLE001 - compared with the recorded one
            exc = [type(e).__name__, str(e)]
        assert exc == rec["exc"]
        if rec["labels"] is None:
            assert got is None
            for argv in (["components", str(inp)], ["components", str(inp), "-o", str(dest)],
                         ["components", str(inp), "--sizes"]):
                capfd.readouterr()
                assert cli(flags + argv + tail) == exc
                assert capfd.readouterr().out == ""
            return
        nodes, labels = got
        want = np.array(unrle(rec["labels"]), dtype=np.int32)
        assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and np.array_equal(labels, want)
        _A, want_nodes = parse_gfa(str(inp), build_graph=False, build_matrix=True, return_node_list=True,
                                   directed=directed, strip_orientation=strip, raw_bytes_id=raw, asymmetric=True)
        assert nodes == want_nodes and len(nodes) == len(want)
        assert all(type(x) is (bytes if raw else str) for x in nodes)
        # the listing: the names' bytes; under --raw-bytes-id they are decoded while writing
        lines, cli_exc = [], None
        for name, lab in zip(nodes, want):
            b = name if raw else name.encode()
            if raw:
                try:
                    b.decode()
                except UnicodeDecodeError as e:
                    cli_exc = [type(e).__name__, str(e)]
                    break
            lines.append(b + b"\t%d\n" % lab)
        text = b"".join(lines)
        capfd.readouterr()
        assert cli(flags + ["components", str(inp)] + tail) == cli_exc
        assert capfd.readouterr().out.encode() == text
        assert cli(flags + ["components", str(inp), "-o", str(dest)] + tail) == cli_exc
        assert dest.read_bytes() == text and capfd.readouterr().out == ""
        assert cli(flags + ["components", str(inp), "--sizes"] + tail) is None
        sizes = np.bincount(want) if len(want) else []
        assert capfd.readouterr().out == "".join(f"{j}\t{c}\n" for j, c in enumerate(sizes))


def test_listing_through_a_replaced_stdout(gpu):
    """A sys.stdout that is no file descriptor (contextlib.redirect_stdout) receives the same text."""
    import contextlib
    import io

    from gfa2network_amd.cli import main

    inp = GOLDEN / "inputs" / "DRB1-3123_unsorted.gfa"
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        main(["components", str(inp)])
    lines = buf.getvalue().splitlines()
    assert len(lines) == 3214 and {ln.split("\t")[1] for ln in lines} == {"0"}


def test_unsupported_record_warns_once(gpu):
    from gfa2network_amd import node_components

    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        node_components(str(GOLDEN / "stats_inputs" / "paths_walks.gfa"))
    msgs = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]
    assert msgs == ["Skipping unsupported record: W"]
