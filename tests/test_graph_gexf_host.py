"""CPU: the checker of ``export --format gexf`` itself.  tests/graph_gexf_util.py's restatement is pinned
against the bytes the reference wrote (tests/golden/expected/graph_gexf.json, NetworkX and Python versions
recorded there) for the calls the reference made on its graph, and, where networkx imports, against
``nx.write_gexf`` on random small entry lists in the three graph classes and with bytes keys — so that no
GPU test compares the feature with itself."""
import io
import random

import pytest

import graph_gexf_util as gx
import graph_json_util as gj

BUILT = sorted(k for k, c in gx.golden()["cases"].items() if c["exc"] is None)


def test_golden_covers_the_modes_and_inputs():
    g = gx.golden()
    assert g["networkx"] and g["python"] and g["creator"] == f"NetworkX {g['networkx']}" and g["lastmodified"]
    names = {k.split("|")[0] for k in g["cases"]}
    assert {p.name for p in (gx.GOLDEN / "inputs").iterdir()} | \
        {"new/" + p.name for p in (gx.GOLDEN / "graph_json" / "inputs").iterdir()} | \
        {"gexf/" + p.name for p in (gx.GOLDEN / "graph_gexf" / "inputs").iterdir()} == names
    for name in names:
        for mode in ("plain", "bidirected", "keep", "raw"):
            assert f"{name}|{mode}" in g["cases"]
    for key, case in g["cases"].items():  # the graph is built first: a failure leaves no file, a build writes one
        assert (case["exc"] is None) == ("text_sha256" in case or case["body_zb64"] is not None), key
        assert (key in g["entries"]) + (key in g["entries_from_records"]) + (key in g["entries_raw_from_plain"]) == \
            (case["exc"] is None), key
    # bytes keys give a complete document, written as their repr
    raw = gx.golden_text("sample.gfa|raw")
    assert b'<node id="b\'' in raw and raw.endswith(b"  </graph>\n</gexf>\n")
    assert raw.startswith(gx.head(g["creator"], g["lastmodified"]).encode() + b"  <graph ")
    empty = gx.golden_text("empty_file.gfa|plain")
    assert empty.endswith(b'name="">\n    <nodes />\n    <edges />\n  </graph>\n</gexf>\n')


@pytest.mark.parametrize("key", BUILT)
def test_restatement_matches_reference(key):
    g = gx.golden()
    mode = key.split("|")[1]
    bidirected, keep = gx.MODES[mode]
    got = gx.render(gx.golden_events(key), bidirected, keep, raw=mode == "raw", creator=g["creator"],
                    lastmodified=g["lastmodified"])
    assert gx.matches_golden_text(key, got), key


def test_as_many_cases_build_as_for_json():
    """A golden of failures alone pins nothing: every input and mode whose JSON export wrote a complete
    document writes a GEXF document too, and so do the bytes-key runs JSON cannot finish."""
    json_ok = {k for k, c in gj.golden()["cases"].items() if c["exc"] is None}
    assert len(BUILT) >= len(json_ok) and json_ok <= set(BUILT)
    assert sum(k.endswith("|raw") for k in BUILT) >= 20
    assert sum(k.startswith("gexf/") for k in BUILT) >= 13


def test_new_inputs_hold_the_escape_classes():
    g = gx.golden()

    text = gx.golden_text
    names = text("gexf/xml_names.gfa|plain")
    for piece in (b'id="a&amp;b"', b'id="c&lt;d"', b'id="e&gt;f"', b'id="g&quot;h"', b"id=\"i'j\"", b'id="end&#13;"'):
        assert piece in names, piece
    quotes = text("gexf/repr_quotes.gfa|raw")
    for piece in (b'id="b&quot;it\'s&quot;"', b"id=\"b'say&quot;hi&quot;'\"", b"id=\"b'both\\'&quot;'\"",
                  b"id=\"b'back\\\\slash'\""):
        assert piece in quotes, piece
    raw = text("gexf/raw_bytes.gfa|raw")
    assert b"hi\\xe9gh" in raw and b"ctl\\x01\\x7f" in raw and b'b&quot;q\'\\xff&quot;' in raw
    assert g["cases"]["gexf/raw_bytes.gfa|plain"]["exc"][0] == "UnicodeDecodeError"
    fallback = text("gexf/e_fallback_xml.gfa|plain")
    assert b'value="&amp;&lt;&gt;&quot;"' in fallback and 'value="é"'.encode() in fallback
    assert "value=\"'&#13;€\"".encode() in fallback and b'value="&amp;amp;"' in fallback


def test_cli_parser_accepts_gexf_flags():
    from gfa2network_amd.cli import _parser

    a = _parser().parse_args(["--raw-bytes-id", "export", "x.gfa", "--format", "gexf", "--bidirected",
                              "--keep-directed-bidir", "--output", "o.gexf"])
    assert (a.cmd, a.format, a.bidirected, a.keep_directed_bidir, a.raw_bytes_id, a.output) == \
        ("export", "gexf", True, True, True, "o.gexf")
    a = _parser().parse_args(["export", "x.gfa", "--format", "gexf"])
    assert a.format == "gexf" and a.output == "-" and not a.bidirected


def test_head_escapes():
    h = gx.head('A&B <"c">', 'd"a&t<e>')
    assert '<meta lastmodifieddate="d&quot;a&amp;t&lt;e&gt;">' in h and '<creator>A&amp;B &lt;"c"&gt;</creator>' in h


# ---- against nx.write_gexf itself ---------------------------------------------------------------------
_ALPHABET = ["a", "b", "c", "x&y", "<t>", 'q"', "it's", "both'\"", "r\rz", "\\", "c\x01", "é", "plain", "0", ""]
_ORIS = ["+", "-", "&", "<>", '"', "'", "\r", "é€", "\U0001F600", "a&amp;b"]


def _random_events(rng, bidirected, keep, raw):
    """A few add_node / add_edge calls as the builder makes them (builders.py:163-256), over names that hold
    every escape class; with raw the keys are the names' latin-1 bytes."""
    names = [rng.choice(_ALPHABET) + rng.choice(["", "1", "2"]) for _ in range(rng.randrange(1, 7))]
    if not raw:
        names = [n for n in names if n.isascii()] or ["a"]
    records = []
    for _ in range(rng.randrange(0, 12)):
        if rng.random() < 0.3:
            records.append(("S", rng.choice(names)))
        else:
            oris = "+-" if bidirected else _ORIS  # (a bidirected key holds the orientation: ASCII)
            records.append(("L", rng.choice(names), rng.choice(oris), rng.choice(names), rng.choice(oris)))
    return gj.events_from_records(records, bidirected, keep)


@pytest.mark.parametrize("mode,raw", [("plain", False), ("bidirected", False), ("keep", False), ("plain", True),
                                      ("bidirected", True)])
def test_restatement_matches_networkx(mode, raw):
    nx = pytest.importorskip("networkx")
    import time

    bidirected, keep = gj.MODES[mode]
    directed, multi = gj.graph_class(bidirected, keep)
    cls = {(True, False): nx.DiGraph, (False, True): nx.MultiGraph, (True, True): nx.MultiDiGraph}[(directed, multi)]
    rng = random.Random(f"{mode}{raw}")
    n_links = 0
    for _ in range(300):
        events = _random_events(rng, bidirected, keep, raw)
        G = cls()
        for ev in events:
            key = [k.encode("latin-1") if raw else k for k in ev[1:3]]
            if ev[0] == "n":
                G.add_node(key[0])
            else:
                G.add_edge(key[0], key[1], **ev[3])
        n_links += G.number_of_edges()
        for _attempt in range(2):  # (again when the date changed between the two lines)
            date = time.strftime("%Y-%m-%d")
            buf = io.BytesIO()
            nx.write_gexf(G, buf)
            if date == time.strftime("%Y-%m-%d"):
                break
        want = gx.render(events, bidirected, keep, raw=raw, creator=f"NetworkX {nx.__version__}", lastmodified=date)
        assert buf.getvalue() == want, events
    assert n_links > 300
