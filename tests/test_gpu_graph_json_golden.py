"""GPU: export --format json (cli.py:282-306) grouped, ordered and rendered in HBM
(G2N_OUT_GRAPH_JSON), checked against the reference's own outputs (tests/golden/expected/graph_json.json):
the written bytes (or their hash; or that no file exists), the exception and the RuntimeWarnings, for
every golden input x {plain, --bidirected, --bidirected --keep-directed-bidir, plain --raw-bytes-id}."""
import warnings

import pytest

import graph_json_util as gj

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("key", sorted(gj.golden()["cases"]))
def test_gpu_graph_json_matches_reference(gpu, key, tmp_path):
    from gfa2network_amd import export_graph_json

    case = gj.golden()["cases"][key]
    mode = key.split("|")[1]
    bidirected, keep = gj.MODES.get(mode, (False, False))
    out = tmp_path / "graph.json"
    exc = None
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            export_graph_json(gj.golden_input(key), out, bidirected=bidirected, keep_directed_bidir=keep,
                              raw_bytes_id=mode == "raw")
        except Exception as e:  # noqa: BLE001
            exc = [type(e).__name__, str(e)]
    assert exc == case["exc"]
    assert [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)] == case["warnings"]
    assert gj.matches_golden_text(case, out.read_bytes() if out.exists() else None)
