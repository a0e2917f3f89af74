#!/usr/bin/env python3
"""Golden fixtures for ``sequence_distance`` / ``gfa2network distance --seq`` from the REAL reference.

Runs only where the pure-Python reference (with NetworkX) is importable: its checkout is named by
the first argument or the environment variable ``G2N_REFERENCE``.  For every file under
tests/golden/inputs, stats_inputs, dist_inputs and seq_inputs (the files with non-ASCII names also
with ``raw_bytes_id`` on), directed and undirected, it records, always under
``warnings.simplefilter("always")``,
  * ``seq2nodes``: the first ``MAX_LISTED`` entries of the dict ``sequence_distance`` forms over the
    nodes' sequences (analysis.py:96-101), in its order: [sequence, [node, ...]],
  * ``queries``: the first ``MAX_QUERIES`` of those sequences, then ``*``, the empty string and one
    absent sequence (given as ``bytes``),
  * ``runs``: under "1" (directed) and "0" (undirected)
      - ``build``: the exception (module, type, message) and the warning messages of
        ``parse_gfa(IN, build_graph=True, build_matrix=False, directed=D, store_seq=True,
        raw_bytes_id=R)`` — what ``distance --seq`` builds (cli.py:308-320),
      - ``outcomes``: the distinct [result, exception, warnings] of ``sequence_distance(G, a, b)``,
      - ``pairs``: row i, column j = the index in ``outcomes`` of the ordered pair of queries i, j.
Bytes that are not UTF-8 are passed as ``bytes``, everything else as ``str``; in the JSON both are
latin-1 text with a flag.  Output: tests/golden/expected/seq_distance.json, one input a line (plain
data; nothing here is imported by the product or bench.py).  ``cases()`` lists the runs the file
must hold; ``outcome(rec, directed, i, j)`` reads one.
"""
from __future__ import annotations

import json
import os
import sys
import warnings
from pathlib import Path

HERE = Path(__file__).resolve().parent
FOLDERS = ("inputs", "stats_inputs", "dist_inputs", "seq_inputs")
RAW_BYTES_FILES = ("bad_utf8_name.gfa", "utf8_names.gfa", "nonascii_name_before.gfa", "nonascii_name_after.gfa",
                   "nonascii_step.gfa")
MAX_QUERIES = 3
MAX_LISTED = 12
ABSENT = b"ZZNOPE"  # (bytes: its repr in the KeyError is b'...'; "*" and "" are the absent str ones of most files)


def file_key(folder: str, name: str, raw_bytes_id: bool) -> str:
    return f"{folder}/{name}|raw={int(raw_bytes_id)}"


def case_key(folder: str, name: str, raw_bytes_id: bool, directed: bool) -> str:
    return f"{file_key(folder, name, raw_bytes_id)}|directed={int(directed)}"


def record_of(expected: dict, key: str) -> tuple[dict, dict]:
    """(the input's record, its run) of a case key."""
    fkey, d = key.rsplit("|directed=", 1)
    return expected[fkey], expected[fkey]["runs"][d]


def outcome(run_rec: dict, i: int, j: int) -> list:
    """[result, exception, warnings] of the ordered pair of queries i, j."""
    return run_rec["outcomes"][run_rec["pairs"][i][j]]


def cases() -> list[tuple[str, Path, bool, bool]]:
    """(key, input, raw_bytes_id, directed) of every case seq_distance.json holds."""
    out = []
    for folder in FOLDERS:
        for inp in sorted((HERE / folder).iterdir()):
            for raw in (False, True) if inp.name in RAW_BYTES_FILES else (False,):
                for directed in (True, False):
                    out.append((case_key(folder, inp.name, raw, directed), inp, raw, directed))
    return out


def exc_record(e: BaseException) -> list[str]:
    return [type(e).__module__, type(e).__name__, str(e)]


def pack(x) -> list:
    """A str or bytes argument / node key as [latin-1 text, is_bytes]."""
    return [x.decode("latin-1"), True] if isinstance(x, bytes) else [x.encode().decode("latin-1"), False]


def unpack(rec):
    return rec[0].encode("latin-1") if rec[1] else rec[0].encode("latin-1").decode()


def as_arg(seq: bytes):
    """A sequence as the argument a caller would pass: str when it is UTF-8, else bytes."""
    try:
        return seq.decode()
    except UnicodeDecodeError:
        return seq


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
        raise SystemExit("usage: make_seqdist_golden.py REFERENCE_CHECKOUT  (or G2N_REFERENCE)")
    sys.path.insert(0, ref)
    from gfa2network.analysis import sequence_distance  # noqa: E402  (the reference)
    from gfa2network.builders import parse_gfa  # noqa: E402

    out = {}
    for key, inp, raw, directed in cases():
        fkey = key.rsplit("|directed=", 1)[0]
        G, exc, warned = run(lambda: parse_gfa(str(inp), build_graph=True, build_matrix=False, directed=directed,
                                               store_seq=True, raw_bytes_id=raw))
        rec = out.setdefault(fkey, {"seq2nodes": [], "queries": [], "runs": {}})
        this = {"build": {"exc": exc, "warnings": warned}, "outcomes": [], "pairs": []}
        rec["runs"][str(int(directed))] = this
        if exc is not None:
            continue
        seq2nodes: dict[bytes, list] = {}
        for node, data in G.nodes(data=True):  # analysis.py:96-101
            seq = data.get("sequence")
            if isinstance(seq, (bytes, bytearray)):
                seq2nodes.setdefault(bytes(seq), []).append(node)
        listed = list(seq2nodes.items())[:MAX_LISTED]
        queries = [as_arg(s) for s, _n in listed[:MAX_QUERIES]]
        for extra in ("*", "", ABSENT):
            if extra not in queries:
                queries.append(extra)
        both = ([[pack(as_arg(s)), [pack(n) for n in nodes]] for s, nodes in listed], [pack(q) for q in queries])
        if rec["queries"]:  # the other direction's build: the same nodes carry the same sequences
            assert (rec["seq2nodes"], rec["queries"]) == both, key
        rec["seq2nodes"], rec["queries"] = both
        for a in queries:
            row = []
            for b in queries:
                got = list(run(lambda: sequence_distance(G, a, b)))
                if got not in this["outcomes"]:
                    this["outcomes"].append(got)
                row.append(this["outcomes"].index(got))
            this["pairs"].append(row)
    lines = [json.dumps(k) + ": " + json.dumps(out[k], sort_keys=True, separators=(",", ":")) for k in sorted(out)]
    (HERE / "expected" / "seq_distance.json").write_text("{\n" + ",\n".join(lines) + "\n}\n")
    n_exc = sum(r["build"]["exc"] is not None for v in out.values() for r in v["runs"].values())
    print(f"{len(out)} inputs, {sum(len(v['runs']) for v in out.values())} runs, {n_exc} builds raise")

if __name__ == "__main__":
    main()
