"""CPU: the checker of ``export --format json`` itself.  tests/graph_json_util.py's restatement is pinned
against the bytes the reference wrote (tests/golden/expected/graph_json.json, NetworkX version recorded
there) for the calls the reference made on its graph, and the group / order step in the form the kernels
use (stable sorts, head flags, scans, first-entry compaction) against the dictionary form on random entry
lists — so that no GPU test compares the feature with itself."""
import base64
import random

import pytest

import graph_json_util as gj

NEW_KEYS = sorted(gj.golden()["entries"])


def test_golden_covers_the_modes_and_inputs():
    g = gj.golden()
    assert g["networkx"]
    names = {k.split("|")[0] for k in g["cases"]}
    assert {p.name for p in (gj.GOLDEN / "inputs").iterdir()} | \
        {"new/" + p.name for p in (gj.GOLDEN / "graph_json" / "inputs").iterdir()} == names
    for name in names:
        for mode in ("plain", "bidirected", "keep", "raw"):
            assert f"{name}|{mode}" in g["cases"]
    # bytes keys: json.dump stops inside the first node
    raw = g["cases"]["sample.gfa|raw"]
    assert raw["exc"] == ["TypeError", "Object of type bytes is not JSON serializable"]
    assert base64.b64decode(raw["text_b64"]) == \
        b'{"directed": true, "multigraph": false, "graph": {}, "nodes": [{"id": '
    empty = g["cases"]["empty_file.gfa|raw"]
    assert empty["exc"] is None and base64.b64decode(empty["text_b64"]).endswith(b'"nodes": [], "links": []}')


@pytest.mark.parametrize("key", NEW_KEYS)
def test_restatement_matches_reference(key):
    g = gj.golden()
    case = g["cases"][key]
    if case["exc"] is not None:  # the build failed: no file, and the calls stop at the failing record
        assert case["text_b64"] is None
        return
    bidirected, keep = gj.MODES[key.split("|")[1]]
    assert gj.matches_golden_text(case, gj.render(g["entries"][key], bidirected, keep)), key


def test_some_new_inputs_render():
    ok = [k for k in NEW_KEYS if gj.golden()["cases"][k]["exc"] is None]
    assert len(ok) >= 13  # (every mode of the inputs that build: a golden of failures alone pins nothing)


def test_cli_parser_accepts_json_flags():
    from gfa2network_amd.cli import _parser

    a = _parser().parse_args(["--raw-bytes-id", "export", "x.gfa", "--format", "json", "--bidirected",
                              "--keep-directed-bidir", "--output", "o.json"])
    assert (a.cmd, a.format, a.bidirected, a.keep_directed_bidir, a.raw_bytes_id, a.output) == \
        ("export", "json", True, True, True, "o.json")
    a = _parser().parse_args(["export", "x.gfa", "--format", "json", "--keep-directed-bidir"])
    assert a.keep_directed_bidir and not a.bidirected and a.output == "-"


def _entry_lists():
    rng = random.Random(5)
    yield "empty", [], []
    yield "one", [3], [3]
    # local duplicates over many nodes
    r = [rng.randrange(3000) for _ in range(20_000)]
    yield "random", r, [min(2999, x + rng.randrange(4)) for x in r]
    # hub sources: a few rows hold most entries, with repeated targets
    r = [rng.choice([0, 7, 2999]) if rng.random() < 0.8 else rng.randrange(3000) for _ in range(20_000)]
    yield "hubs", r, [rng.randrange(3000) for _ in r]
    # groups larger than 1024 (one pair 5000 times) between other pairs, both directions
    r, c = [], []
    for _ in range(12_000):
        if rng.random() < 0.45:
            a, b = (5, 9) if rng.random() < 0.7 else (9, 5)
        else:
            a, b = rng.randrange(40), rng.randrange(40)
        r.append(a)
        c.append(b)
    yield "big_groups", r, c
    # self pairs only
    r = [rng.randrange(5) for _ in range(3000)]
    yield "self", r, list(r)


@pytest.mark.parametrize("name", ["empty", "one", "random", "hubs", "big_groups", "self"])
@pytest.mark.parametrize("unordered,multi", [(False, False), (True, True), (False, True)])
def test_kernel_form_equals_dict_form(name, unordered, multi):
    rows, cols = next((r, c) for n, r, c in _entry_lists() if n == name)
    if name == "big_groups":
        pair = sum(1 for a, b in zip(rows, cols) if (a, b) == (5, 9))
        assert pair > 1024
    assert gj.order_kernel_form(rows, cols, unordered, multi) == gj.order_dict_form(rows, cols, unordered, multi)


def test_dict_form_is_the_restatement_order():
    """order_dict_form lists what render lists (the link between the two halves of this file)."""
    import json

    rng = random.Random(9)
    names = [f"n{k}" for k in range(30)]
    records = [("S", nm) for nm in names[:10]]
    for _ in range(400):
        records.append(("L", rng.choice(names), rng.choice("+-"), rng.choice(names), rng.choice("+-")))
    for mode, (bidirected, keep) in gj.MODES.items():
        events = gj.events_from_records(records, bidirected, keep)
        doc = json.loads(gj.render(events, bidirected, keep))
        ids = {n["id"]: k for k, n in enumerate(doc["nodes"])}
        entries = [(ids[e[1]], ids[e[2]]) for e in events if e[0] == "e"]
        directed, multi = gj.graph_class(bidirected, keep)
        want = gj.order_dict_form([a for a, _ in entries], [b for _, b in entries], not directed, multi)
        got = [(ids[ln["source"]], ids[ln["target"]]) for ln in doc["links"]]
        assert got == [(s, t) for s, t, _ in want], mode
        if multi:
            assert [ln["key"] for ln in doc["links"]] == [x for _, _, x in want]
        else:
            attrs = [e[3] for e in events if e[0] == "e"]
            assert [(ln["orientation_from"], ln["orientation_to"]) for ln in doc["links"]] == \
                [(attrs[x]["orientation_from"], attrs[x]["orientation_to"]) for _, _, x in want]
