#!/usr/bin/env python3
"""Golden fixtures for ``genome_distance(G, A, B, method="mean")`` from the REAL reference.

Runs only where the pure-Python reference (with NetworkX) is importable: its checkout is named by
the first argument or the environment variable ``G2N_REFERENCE``.  The reference's CLI has no
``--method`` for ``distance --path``, so its handler (cli.py:323-346) is restated here around the
reference's own functions: ``load_paths``, the lookup of the two names (KeyError), ``parse_gfa(...,
build_graph=True, directed=...)``, then ``analysis.genome_distance(G, nodes_a, nodes_b, method=)``.
For every file under tests/golden/dist_inputs, wdist_inputs and pair_inputs (the files with
non-ASCII names also with ``raw_bytes_id`` on), for the plain graph (``"hops"``) and the graph
``parse_gfa(..., weight_tag="RC")`` builds (``"weighted"``), directed and undirected, it records under
``warnings.simplefilter("always")``
  * ``mean``: for every ordered pair of the file's first ``MAX_NAMES`` path names plus one unknown
    name, the value's exact bits (``float.hex``), or the exception's module, type and message, and
    the list of warning messages,
  * ``other``: the same for the first pair of names with ``method="median"`` (the reference's
    ValueError, after the build's errors and warnings),
  * ``pairs``: len(A) * len(B) of every such pair (the quadratic warning's condition).
A weighted graph with a negative, NaN or infinite length records ``{"bad": true}`` for its runs:
NetworkX's result then depends on its heap's order, and the GPU functions refuse such a graph.
Output: tests/golden/expected/pair_distance.json, one case a line (plain data; nothing here is
imported by the product or bench.py).  ``cases()`` lists the keys the file must hold.
"""
from __future__ import annotations

import functools
import json
import math
import os
import sys
import warnings
from pathlib import Path

HERE = Path(__file__).resolve().parent
FOLDERS = ("dist_inputs", "wdist_inputs", "pair_inputs")
RAW_BYTES_FILES = ("nonascii_name_before.gfa", "nonascii_name_after.gfa", "nonascii_step.gfa")
TAG = "RC"
UNKNOWN = "no-such-path"
OTHER_METHOD = "median"
MAX_NAMES = 4
KINDS = ("hops", "weighted")


def case_key(folder: str, name: str, raw_bytes_id: bool) -> str:
    return f"{folder}/{name}|raw={int(raw_bytes_id)}"


def cases() -> list[tuple[str, Path, bool]]:
    """(key, input, raw_bytes_id) of every case pair_distance.json holds."""
    out = []
    for folder in FOLDERS:
        for inp in sorted((HERE / folder).iterdir()):
            for raw in (False, True) if inp.name in RAW_BYTES_FILES else (False,):
                out.append((case_key(folder, inp.name, raw), inp, raw))
    return out


def run_key(kind: str, directed: bool) -> str:
    return f"{kind}|directed={int(directed)}"


def exc_record(e: BaseException) -> list[str]:
    return [type(e).__module__, type(e).__name__, str(e)]


def value(x: float) -> str:
    return "inf" if x == float("inf") else float(x).hex()


def run(fn):
    """(result, exception record, warning messages) of fn()"""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = exc = None
        try:
            got = fn()
        except KeyboardInterrupt:
            raise
        except BaseException as e:  # noqa: BLE001 - recorded as data
            exc = exc_record(e)
    return got, exc, [str(w.message) for w in caught]


def main() -> None:
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("G2N_REFERENCE")
    if not ref:
        raise SystemExit("usage: make_pairdist_golden.py REFERENCE_CHECKOUT  (or G2N_REFERENCE)")
    sys.path.insert(0, ref)
    os.environ.pop("GFANET_DISABLE_WARNINGS", None)
    from gfa2network import analysis, builders  # noqa: E402  (the reference)

    parsers = {"hops": builders.parse_gfa, "weighted": functools.partial(builders.parse_gfa, weight_tag=TAG)}

    def handler(inp, a, b, directed, raw, parse, method):
        """cli.py:323-346 with a method"""
        paths = analysis.load_paths(str(inp), raw_bytes=raw)
        nodes_a = paths[a.encode() if raw else a]
        nodes_b = paths[b.encode() if raw else b]
        G = parse(str(inp), build_graph=True, build_matrix=False, directed=directed, raw_bytes_id=raw)
        return analysis.genome_distance(G, nodes_a, nodes_b, method=method)

    def record(fn):
        got, exc, warned = run(fn)
        return {"value": None if got is None else value(float(got)), "exc": exc, "warnings": warned}

    out = {}
    n_values = n_warned = 0
    for key, inp, raw in cases():
        paths, _exc, _w = run(lambda: analysis.load_paths(str(inp), raw_bytes=raw))
        paths = paths or {}
        names = [n.decode() if isinstance(n, bytes) else n for n in paths][:MAX_NAMES] + [UNKNOWN]
        steps = {(n.decode() if isinstance(n, bytes) else n): len(v) for n, v in paths.items()}
        rec = {"names": names, "pairs": {}, "runs": {}}
        for a in names[:-1]:
            for b in names[:-1]:
                rec["pairs"][f"{a}|{b}"] = steps[a] * steps[b]
        for kind in KINDS:
            for directed in (True, False):
                G, _exc, _w = run(lambda: parsers[kind](str(inp), build_graph=True, build_matrix=False,
                                                        directed=directed, raw_bytes_id=raw))
                bad = G is not None and any(not (math.isfinite(float(w)) and float(w) >= 0)
                                            for _u, _v, w in G.edges(data="weight", default=1))
                r = {"bad": bad, "mean": {}, "other": None}
                for a in names:
                    for b in names:
                        if bad and UNKNOWN not in (a, b):
                            r["mean"][f"{a}|{b}"] = {"bad": True}
                            continue
                        r["mean"][f"{a}|{b}"] = got = record(
                            lambda: handler(inp, a, b, directed, raw, parsers[kind], "mean"))
                        n_values += got["value"] is not None
                        n_warned += any("quadratically" in w for w in got["warnings"])
                if len(names) > 1 and not bad:
                    a, b = names[0], names[min(1, len(names) - 2)]
                    r["other"] = dict(record(lambda: handler(inp, a, b, directed, raw, parsers[kind], OTHER_METHOD)),
                                      a=a, b=b)
                rec["runs"][run_key(kind, directed)] = r
        out[key] = rec
    lines = [json.dumps(k) + ": " + json.dumps(out[k], sort_keys=True, separators=(",", ":")) for k in sorted(out)]
    (HERE / "expected" / "pair_distance.json").write_text("{\n" + ",\n".join(lines) + "\n}\n")
    print(f"{len(out)} pair distance cases, {n_values} values, {n_warned} runs past 1000 pairs")


if __name__ == "__main__":
    main()
