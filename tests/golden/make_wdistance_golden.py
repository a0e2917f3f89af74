#!/usr/bin/env python3
"""Golden fixtures for the distance functions over a WEIGHTED graph (``weight_tag=``) from the REAL
reference.

Runs only where the pure-Python reference (with NetworkX and pandas) is importable: its checkout is
named by the first argument or the environment variable ``G2N_REFERENCE``.  The reference's distance
helpers take no weight tag of their own: they search whatever graph ``parse_gfa`` built.  So the
names ``analysis.parse_gfa`` and ``cli.parse_gfa`` are swapped here for
``functools.partial(builders.parse_gfa, weight_tag=TAG)`` and the reference's own functions run
unchanged over the graph that builds.  For every file under tests/golden/wdist_inputs, inputs,
stats_inputs and dist_inputs (the files with non-ASCII names also with ``raw_bytes_id`` on) it
records, always under ``warnings.simplefilter("always")``,
  * ``graph``: under "1" (directed) and "0" (undirected), the build's exception and warnings, the
    node count and the graph's edges as [i, j, float.hex(w)] from ``G.edges(data="weight",
    default=1)`` (i, j = positions in ``G.nodes``: first-touch order) — past ``MAX_EDGES`` edges the
    SHA-256 of the CSR they make instead (``edges_csr``) —, and ``bad``: whether a weight is negative,
    NaN or infinite,
  * ``matrix[method]`` for min and mean: ``analysis.genome_distance_matrix``'s labels and values
    (``float.hex``, ``inf`` as "inf"), or the exception, and the warnings,
  * ``distance``: for every ordered pair of the file's first ``MAX_NAMES`` path names plus one
    unknown name, directed and undirected, ``cli.main(["distance", IN, "--path", A, B])``'s value
    (``float.hex`` of the printed number: the reference prints an int when the best path crossed
    untagged edges only), exception and warnings,
  * ``seq``: the first two sequences the nodes carry; for their ordered pairs, directed and
    undirected, ``cli.main(["distance", IN, "--seq", A, B])``'s value, exception and warnings, and
    ``analysis.sequence_distance``'s on the same graph.
A case whose graph has a bad weight records only that fact for the runs over that graph: NetworkX's
result then depends on its heap's order, and the GPU functions refuse such a graph.
Output: tests/golden/expected/wdistance.json, one case a line (plain data; nothing here is imported
by the product or bench.py).  ``cases()`` lists the keys the file must hold.
"""
from __future__ import annotations

import contextlib
import functools
import io
import json
import math
import os
import sys
import warnings
from pathlib import Path

HERE = Path(__file__).resolve().parent
FOLDERS = ("wdist_inputs", "inputs", "stats_inputs", "dist_inputs")
RAW_BYTES_FILES = ("bad_utf8_name.gfa", "utf8_names.gfa", "nonascii_name_before.gfa", "nonascii_name_after.gfa",
                   "nonascii_step.gfa")
TAG = "RC"  # the tag of make_golden.py's weighted combos
UNKNOWN = "no-such-path"
METHODS = ("min", "mean")
MAX_NAMES = 3
MAX_EDGES = 1000


def edges_csr(n: int, edges, directed: bool):
    """(indptr int32, indices int32, data float64) of the graph's weighted adjacency matrix: one cell per
    edge (both cells of an undirected one), columns ascending within a row."""
    import numpy as np

    cells = {}
    for i, j, w in edges:
        cells[(i, j)] = w
        if not directed:
            cells[(j, i)] = w
    keys = sorted(cells)
    indptr = np.zeros(n + 1, dtype=np.int32)
    for i, _j in keys:
        indptr[i + 1] += 1
    np.cumsum(indptr, out=indptr)
    return (indptr, np.array([j for _i, j in keys], dtype=np.int32),
            np.array([cells[k] for k in keys], dtype=np.float64))


def csr_digest(indptr, indices, data) -> str:
    import hashlib

    return hashlib.sha256(indptr.tobytes() + indices.tobytes() + data.tobytes()).hexdigest()


def case_key(folder: str, name: str, raw_bytes_id: bool) -> str:
    return f"{folder}/{name}|raw={int(raw_bytes_id)}"


def cases() -> list[tuple[str, Path, bool]]:
    """(key, input, raw_bytes_id) of every case wdistance.json holds."""
    out = []
    for folder in FOLDERS:
        for inp in sorted((HERE / folder).iterdir()):
            for raw in (False, True) if inp.name in RAW_BYTES_FILES else (False,):
                out.append((case_key(folder, inp.name, raw), inp, raw))
    return out


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
        except BaseException as e:  # noqa: BLE001 - recorded as data (SystemExit too)
            exc = exc_record(e)
    return got, exc, [str(w.message) for w in caught]


def main() -> None:
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("G2N_REFERENCE")
    if not ref:
        raise SystemExit("usage: make_wdistance_golden.py REFERENCE_CHECKOUT  (or G2N_REFERENCE)")
    sys.path.insert(0, ref)
    import numpy as np  # noqa: E402

    from gfa2network import analysis, builders, cli  # noqa: E402  (the reference)

    weighted = functools.partial(builders.parse_gfa, weight_tag=TAG)
    analysis.parse_gfa = weighted
    cli.parse_gfa = weighted

    def cli_value(argv):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            _got, exc, warned = run(lambda: cli.main(argv))
        text = buf.getvalue()
        return {"value": value(float(text)) if exc is None else None, "exc": exc, "warnings": warned}

    out = {}
    for key, inp, raw in cases():
        rec = {"graph": {}, "matrix": {}, "distance": {}, "seq": {"queries": [], "runs": {}}}
        graphs = {}
        for directed in (True, False):
            G, exc, warned = run(lambda: weighted(str(inp), build_graph=True, build_matrix=False, directed=directed,
                                                  store_seq=True, raw_bytes_id=raw))
            g = {"exc": exc, "warnings": warned, "n": None, "edges": None, "bad": False}
            if G is not None:
                index = {node: i for i, node in enumerate(G.nodes)}
                edges = [(index[u], index[v], float(w)) for u, v, w in G.edges(data="weight", default=1)]
                g["n"] = len(index)
                if len(edges) <= MAX_EDGES:
                    g["edges"] = [[i, j, w.hex()] for i, j, w in edges]
                else:
                    g["digest"] = csr_digest(*edges_csr(len(index), edges, directed))
                g["bad"] = any(not (math.isfinite(w) and w >= 0) for _i, _j, w in edges)
            rec["graph"][str(int(directed))] = g
            graphs[directed] = G
        bad = {d: rec["graph"][str(int(d))]["bad"] for d in (True, False)}
        for method in METHODS:  # (genome_distance_matrix builds the directed graph)
            if bad[True]:
                rec["matrix"][method] = {"bad": True}
                continue
            M, exc, warned = run(lambda: analysis.genome_distance_matrix(str(inp), method=method, raw_bytes_id=raw))
            rec["matrix"][method] = {
                "labels": None if M is None else [str(x) for x in M.index],
                "values": None if M is None else [[value(x) for x in row] for row in np.asarray(M)],
                "exc": exc, "warnings": warned}
        names, _exc, _w = run(lambda: analysis.load_paths(str(inp), raw_bytes=raw))
        names = [n.decode() if isinstance(n, bytes) else n for n in (names or {})][:MAX_NAMES] + [UNKNOWN]
        rec["names"] = names
        pre = ["--raw-bytes-id"] if raw else []
        for directed in (True, False):
            tail = [] if directed else ["--undirected"]
            for a in names:
                for b in names:
                    k = f"{a}|{b}|directed={int(directed)}"
                    if bad[directed] and UNKNOWN not in (a, b):
                        rec["distance"][k] = {"bad": True}
                    else:
                        rec["distance"][k] = cli_value(pre + ["distance", str(inp), "--path", a, b] + tail)
        # ---- --seq: the first two sequences of the directed graph's nodes that argv can carry
        G = graphs[True]
        seqs: list[str] = []
        if G is not None:
            for _node, data in G.nodes(data=True):
                s = data.get("sequence")
                if isinstance(s, (bytes, bytearray)):
                    try:
                        t = bytes(s).decode()
                    except UnicodeDecodeError:
                        continue
                    if t not in seqs and not t.startswith("-"):
                        seqs.append(t)
                if len(seqs) == 2:
                    break
        rec["seq"]["queries"] = seqs
        for directed in (True, False):
            runs = {}
            tail = [] if directed else ["--undirected"]
            for a in seqs:
                for b in seqs:
                    if bad[directed]:
                        runs[f"{a}|{b}"] = {"bad": True}
                        continue
                    r = cli_value(pre + ["distance", str(inp), "--seq", a, b] + tail)
                    d, exc, warned = run(lambda: analysis.sequence_distance(graphs[directed], a, b))
                    r["function"] = {"value": None if d is None else value(float(d)), "exc": exc, "warnings": warned}
                    runs[f"{a}|{b}"] = r
            rec["seq"]["runs"][str(int(directed))] = runs
        out[key] = rec
    lines = [json.dumps(k) + ": " + json.dumps(out[k], sort_keys=True, separators=(",", ":")) for k in sorted(out)]
    (HERE / "expected" / "wdistance.json").write_text("{\n" + ",\n".join(lines) + "\n}\n")
    n_bad = sum(v["graph"]["1"]["bad"] for v in out.values())
    n_exc = sum(v["graph"]["1"]["exc"] is not None for v in out.values())
    print(f"{len(out)} weighted distance cases, {n_exc} builds raise, {n_bad} graphs have a bad weight")


if __name__ == "__main__":
    main()
