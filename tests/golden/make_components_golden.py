#!/usr/bin/env python3
"""Golden fixture for ``node_components`` / ``gfa2network components`` from the REAL reference.

Runs only where the pure-Python reference (and NetworkX) is importable: its checkout is named by
the first argument or the environment variable ``G2N_REFERENCE``.  For every case of
``make_stats_golden.cases()`` it does what ``analysis.compute_stats`` does up to its component
count — ``parse_gfa(build_graph=True, ...)``, then the second pass over ``GFAParser(path)`` — and
records, per node in ``list(G)`` order, the number of its component in
``enumerate(nx.connected_components(G.to_undirected()))``, run-length encoded as [label, count]
pairs; or the exception's type and message.
Output: tests/golden/expected/components.json (plain data; nothing here is imported by the
product, the GPU tests or bench.py).
"""
from __future__ import annotations

import json
import os
import sys
import warnings
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from make_stats_golden import cases  # noqa: E402


def rle(labels) -> list[list[int]]:
    out: list[list[int]] = []
    for v in labels:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([int(v), 1])
    return out


def unrle(runs) -> list[int]:
    return [v for v, c in runs for _ in range(c)]


def main() -> None:
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("G2N_REFERENCE")
    if not ref:
        raise SystemExit("usage: make_components_golden.py REFERENCE_CHECKOUT  (or G2N_REFERENCE)")
    sys.path.insert(0, ref)
    import networkx as nx  # noqa: E402
    from gfa2network import parse_gfa  # noqa: E402  (the reference)
    from gfa2network.parser import GFAParser  # noqa: E402

    out = {}
    total = 0
    for key, inp, directed, strip, raw in cases():
        labels = exc = None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                G = parse_gfa(str(inp), build_graph=True, build_matrix=False, directed=directed,
                              strip_orientation=strip, raw_bytes_id=raw)
                for _rec in GFAParser(str(inp)):  # compute_stats' second pass
                    pass
                of = {}
                for j, comp in enumerate(nx.connected_components(G.to_undirected())):
                    for node in comp:
                        of[node] = j
                labels = rle(of[node] for node in G)
                total += G.number_of_nodes()
            except Exception as e:  # noqa: BLE001 - recorded as data
                exc = [type(e).__name__, str(e)]
        out[key] = {"labels": labels, "exc": exc}
    (HERE / "expected" / "components.json").write_text(json.dumps(out, indent=None, sort_keys=True,
                                                                  separators=(",", ":")).replace('},"', '},\n"') + "\n")
    print(f"{len(out)} component cases, {sum(v['exc'] is not None for v in out.values())} raise, {total} labels")


if __name__ == "__main__":
    main()
