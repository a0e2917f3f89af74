#!/usr/bin/env python3
"""Golden fixtures for ``gfa2network export --format gexf`` from the REAL reference.

Runs ONLY in the build container, where the pure-Python reference is importable from
/root/reference.  For every input under tests/golden/inputs, tests/golden/graph_json/inputs and
tests/golden/graph_gexf/inputs and the four runs {plain, --bidirected, --bidirected
--keep-directed-bidir, plain with --raw-bytes-id} it calls the reference's ``cli.main([(--raw-bytes-id),
"export", IN, "--format", "gexf", ..., "--output", OUT])`` (cli.py:296-297) in-process and records:
  * the bytes written to OUT, or null when no file exists afterwards (the graph is built before
    nx.write_gexf opens the output); outputs above 64 KiB as their length and sha256.  Every document
    opens with the same head (the date and the creator are fixed), recorded once as ``head``; a case
    holds what follows it, deflated (XML of this kind shrinks tenfold), as base64: ``body_zb64``,
  * the exception type + message (or null),
  * the RuntimeWarnings emitted (parser.py:117-131).
The date GEXFWriter takes from ``time.strftime`` is fixed to LASTMODIFIED for the run; the tests pass
it back as ``lastmodified=``, and the recorded ``creator`` as ``creator=``.
Per case it also records the calls the reference made on its graph while it ran (``add_node(key)`` /
``add_edge(a, b, **attrs)``, in order; bytes keys as base64): the entry lists tests/graph_gexf_util.py
is checked against.  Two kinds of list are checked here instead of stored: for the few inputs with more
than BIG_EVENTS calls (plain S / L files) the script checks that the list equals what graph_gexf_util
derives from the file's records (``entries_from_records``), and for a --raw-bytes-id run whose plain run
built too, that it is the plain run's list with every key encoded as ASCII (``entries_raw_from_plain``).
Output: tests/golden/expected/graph_gexf.json (plain data, with the NetworkX and Python versions;
nothing here is imported by the product, the GPU tests or bench.py).
"""
from __future__ import annotations

import base64
import gzip
import hashlib
import json
import sys
import tempfile
import warnings
import zlib
from pathlib import Path

REF = "/root/reference"
HERE = Path(__file__).resolve().parent
INPUT_DIRS = [("", HERE / "inputs"), ("new/", HERE / "graph_json" / "inputs"), ("gexf/", HERE / "graph_gexf" / "inputs")]
BIG = 64 * 1024
BIG_EVENTS = 1500
LASTMODIFIED = "2001-02-03"

MODES = {  # key suffix -> (global flags, export flags)
    "plain": ([], []),
    "bidirected": ([], ["--bidirected"]),
    "keep": ([], ["--bidirected", "--keep-directed-bidir"]),
    "raw": (["--raw-bytes-id"], []),
}


def _key(x):
    return x if isinstance(x, str) else {"bytes_b64": base64.b64encode(x).decode()}


def main() -> None:
    sys.path.insert(0, REF)
    sys.path.insert(0, str(HERE.parent))
    import networkx as nx
    import networkx.readwrite.gexf as nx_gexf

    import graph_gexf_util as gx
    import graph_json_util as gj
    from gfa2network import cli  # noqa: E402  (the reference)

    class FixedTime:  # GEXFWriter.__init__: time.strftime("%Y-%m-%d")
        @staticmethod
        def strftime(fmt):
            assert fmt == "%Y-%m-%d"
            return LASTMODIFIED

    nx_gexf.time = FixedTime
    events: list = []

    def spy(cls, name):  # records the call, then runs the class's own method
        inner = cls.__dict__[name]

        def add_node(self, key, **attrs):
            events.append(["n", _key(key)])
            return inner(self, key, **attrs)

        def add_edge(self, a, b, *args, **attrs):
            events.append(["e", _key(a), _key(b), dict(attrs)])
            return inner(self, a, b, *args, **attrs)

        setattr(cls, name, add_node if name == "add_node" else add_edge)

    for cls in (nx.Graph, nx.DiGraph):
        spy(cls, "add_node")
    for cls in (nx.DiGraph, nx.MultiGraph, nx.MultiDiGraph):
        spy(cls, "add_edge")

    out = {"networkx": nx.__version__, "python": sys.version.split()[0], "creator": f"NetworkX {nx.__version__}",
           "lastmodified": LASTMODIFIED, "head": None, "cases": {}, "entries": {}, "entries_from_records": [],
           "entries_raw_from_plain": []}
    with tempfile.TemporaryDirectory() as td:
        for prefix, folder in INPUT_DIRS:
            for inp in sorted(folder.iterdir()):
                for mode, (gflags, eflags) in MODES.items():
                    dest = Path(td) / "graph.gexf"
                    if dest.exists():
                        dest.unlink()
                    argv = gflags + ["export", str(inp), "--format", "gexf"] + eflags + ["--output", str(dest)]
                    exc = None
                    events.clear()
                    with warnings.catch_warnings(record=True) as w:
                        warnings.simplefilter("always")
                        try:
                            cli.main(argv)
                        except Exception as e:  # noqa: BLE001 - recorded as data
                            exc = [type(e).__name__, str(e)]
                    text = dest.read_bytes() if dest.exists() else None
                    key = f"{prefix}{inp.name}|{mode}"
                    case = {
                        "exc": exc,
                        "warnings": [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)],
                    }
                    if text is None:
                        case["body_zb64"] = None
                    elif len(text) > BIG:
                        case["text_len"] = len(text)
                        case["text_sha256"] = hashlib.sha256(text).hexdigest()
                    else:
                        cut = text.index(b"  <graph ")
                        if out["head"] is None:
                            out["head"] = text[:cut].decode("ascii")
                        assert text[:cut].decode("ascii") == out["head"], key
                        case["body_zb64"] = base64.b64encode(zlib.compress(text[cut:], 9)).decode()
                    out["cases"][key] = case
                    if text is None:
                        continue
                    plain = out["entries"].get(f"{prefix}{inp.name}|plain")
                    if mode == "raw" and plain is not None:
                        assert [[e[0]] + [_key(x.encode("ascii")) if isinstance(x, str) else x for x in e[1:]]
                                for e in plain] == events, key
                        out["entries_raw_from_plain"].append(key)
                        continue
                    if len(events) <= BIG_EVENTS:
                        out["entries"][key] = [list(e) for e in events]
                        continue
                    data = inp.read_bytes()
                    if inp.name.endswith(".gz"):
                        data = gzip.decompress(data)
                    bidirected, keep = gx.MODES[mode]
                    derived = gj.events_from_records(gx.records_from_gfa(data), bidirected, keep)
                    if mode == "raw":
                        derived = [[e[0]] + [_key(x.encode("ascii")) if isinstance(x, str) else x for x in e[1:]]
                                   for e in derived]
                    assert derived == events, key
                    out["entries_from_records"].append(key)
    lines = []  # one line per case and per entry list
    for name in sorted(out):
        val = out[name]
        if name in ("cases", "entries"):
            body = ",\n".join(f"{json.dumps(k)}: {json.dumps(val[k], sort_keys=True)}" for k in sorted(val))
            lines.append(f"{json.dumps(name)}: {{\n{body}\n}}")
        else:
            lines.append(f"{json.dumps(name)}: {json.dumps(val)}")
    (HERE / "expected" / "graph_gexf.json").write_text("{\n" + ",\n".join(lines) + "\n}\n")
    print(f"{len(out['cases'])} graph-gexf cases, {sum(c['exc'] is None for c in out['cases'].values())} built, "
          f"{len(out['entries_from_records'])} with derived entries")


if __name__ == "__main__":
    main()
