#!/usr/bin/env python3
"""Golden fixtures for ``gfa2network export --format json`` from the REAL reference.

Runs ONLY in the build container, where the pure-Python reference is importable from
/root/reference.  For every input under tests/golden/inputs and tests/golden/graph_json/inputs
and the four runs {plain, --bidirected, --bidirected --keep-directed-bidir, plain with
--raw-bytes-id} it calls the reference's ``cli.main([(--raw-bytes-id), "export", IN, "--format",
"json", ..., "--output", OUT])`` (cli.py:282-306) in-process and records:
  * the bytes written to OUT, or null when no file exists afterwards (the graph is built before
    the output is opened); outputs above 64 KiB as their length and sha256,
  * the exception type + message (or null),
  * the RuntimeWarnings emitted (parser.py:117-131; NetworkX's FutureWarning is not one).
For the inputs under graph_json/inputs it also records, per mode, the calls the reference made on
its graph while it ran (``add_node(key)`` / ``add_edge(a, b, **attrs)``, in order): the entry
lists tests/graph_json_util.py is checked against.
Output: tests/golden/expected/graph_json.json (plain data, with the NetworkX version; nothing
here is imported by the product, the GPU tests or bench.py).
"""
from __future__ import annotations

import base64
import hashlib
import json
import sys
import tempfile
import warnings
from pathlib import Path

REF = "/root/reference"
HERE = Path(__file__).resolve().parent
INPUTS = HERE / "inputs"
NEW_INPUTS = HERE / "graph_json" / "inputs"
BIG = 64 * 1024

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
    import networkx as nx

    from gfa2network import cli  # noqa: E402  (the reference)

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

    out = {"networkx": nx.__version__, "cases": {}, "entries": {}}
    with tempfile.TemporaryDirectory() as td:
        for inp in sorted(INPUTS.iterdir()) + sorted(NEW_INPUTS.iterdir()):
            new = inp.parent == NEW_INPUTS
            for mode, (gflags, eflags) in MODES.items():
                dest = Path(td) / "graph.json"
                if dest.exists():
                    dest.unlink()
                argv = gflags + ["export", str(inp), "--format", "json"] + eflags + ["--output", str(dest)]
                exc = None
                events.clear()
                with warnings.catch_warnings(record=True) as w:
                    warnings.simplefilter("always")
                    try:
                        cli.main(argv)
                    except Exception as e:  # noqa: BLE001 - recorded as data
                        exc = [type(e).__name__, str(e)]
                text = dest.read_bytes() if dest.exists() else None
                case = {
                    "exc": exc,
                    "warnings": [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)],
                }
                if text is None:
                    case["text_b64"] = None
                elif len(text) > BIG:
                    case["text_len"] = len(text)
                    case["text_sha256"] = hashlib.sha256(text).hexdigest()
                else:
                    case["text_b64"] = base64.b64encode(text).decode()
                key = f"{'new/' if new else ''}{inp.name}|{mode}"
                out["cases"][key] = case
                if new and mode != "raw":
                    out["entries"][key] = [list(e) for e in events]
    (HERE / "expected" / "graph_json.json").write_text(json.dumps(out, indent=0, sort_keys=True))
    print(f"{len(out['cases'])} graph-json cases")


if __name__ == "__main__":
    main()
