#!/usr/bin/env python3
"""Golden fixtures for ``genome_distance_matrix`` / ``gfa2network distance --path`` /
``distance-matrix`` from the REAL reference.

Runs only where the pure-Python reference (with NetworkX and pandas) is importable: its checkout is
named by the first argument or the environment variable ``G2N_REFERENCE``.  For every file under
tests/golden/inputs, tests/golden/stats_inputs and tests/golden/dist_inputs (the files with
non-ASCII names also with ``raw_bytes_id`` on) it records, always under
``warnings.simplefilter("always")``,
  * ``matrix[method]`` for min and mean: ``analysis.genome_distance_matrix``'s labels and values
    (each value as ``float.hex``, ``inf`` as the string "inf"), or the exception's module, type and
    message; and the list of warning messages,
  * ``distance``: for every ordered pair of the file's path names plus one unknown name, directed
    and undirected, the stdout, exception and warnings of
    ``cli.main([--raw-bytes-id] distance IN --path A B [--undirected])``,
  * ``output``: for ``.csv``, ``.npy`` and ``.npz``, the bytes (hex) ``distance-matrix -o`` wrote,
    or its exception.
Output: tests/golden/expected/distance.json (plain data; nothing here is imported by the product,
the GPU tests or bench.py).  ``cases()`` lists the keys the file must hold: the tests import it to
check that none is missing.
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys
import tempfile
import warnings
from pathlib import Path

HERE = Path(__file__).resolve().parent
FOLDERS = ("inputs", "stats_inputs", "dist_inputs")
RAW_BYTES_FILES = ("bad_utf8_name.gfa", "utf8_names.gfa", "nonascii_name_before.gfa", "nonascii_name_after.gfa",
                   "nonascii_step.gfa")
UNKNOWN = "no-such-path"
METHODS = ("min", "mean")
SUFFIXES = (".csv", ".npy", ".npz")


def case_key(folder: str, name: str, raw_bytes_id: bool) -> str:
    return f"{folder}/{name}|raw={int(raw_bytes_id)}"


def cases() -> list[tuple[str, Path, bool]]:
    """(key, input, raw_bytes_id) of every case distance.json holds."""
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


def main() -> None:
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("G2N_REFERENCE")
    if not ref:
        raise SystemExit("usage: make_distance_golden.py REFERENCE_CHECKOUT  (or G2N_REFERENCE)")
    sys.path.insert(0, ref)
    import numpy as np  # noqa: E402

    from gfa2network import cli  # noqa: E402  (the reference)
    from gfa2network.analysis import genome_distance_matrix, load_paths  # noqa: E402

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

    out = {}
    for key, inp, raw in cases():
        rec = {"matrix": {}, "distance": {}, "output": {}}
        for method in METHODS:
            M, exc, warned = run(lambda: genome_distance_matrix(str(inp), method=method, raw_bytes_id=raw))
            rec["matrix"][method] = {
                "labels": None if M is None else [str(x) for x in M.index],
                "values": None if M is None else [[value(x) for x in row] for row in np.asarray(M)],
                "exc": exc, "warnings": warned}
        names, _exc, _w = run(lambda: load_paths(str(inp), raw_bytes=raw))
        names = [n.decode() if isinstance(n, bytes) else n for n in (names or {})] + [UNKNOWN]
        pre = ["--raw-bytes-id"] if raw else []
        for directed in (True, False):
            for a in names:
                for b in names:
                    buf = io.StringIO()
                    argv = pre + ["distance", str(inp), "--path", a, b] + ([] if directed else ["--undirected"])
                    with contextlib.redirect_stdout(buf):
                        _got, exc, warned = run(lambda: cli.main(argv))
                    rec["distance"][f"{a}|{b}|directed={int(directed)}"] = {
                        "stdout": buf.getvalue(), "exc": exc, "warnings": warned}
        rec["names"] = names
        for suffix in SUFFIXES:
            with tempfile.TemporaryDirectory() as tmp:
                dest = Path(tmp) / ("m" + suffix)
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    _got, exc, warned = run(lambda: cli.main(pre + ["distance-matrix", str(inp), "-o", str(dest)]))
                rec["output"][suffix] = {"bytes": dest.read_bytes().hex() if dest.exists() and exc is None else None,
                                         "exc": exc, "warnings": warned}
        out[key] = rec
    (HERE / "expected" / "distance.json").write_text(json.dumps(out, indent=0, sort_keys=True) + "\n")
    n_exc = sum(v["matrix"]["min"]["exc"] is not None for v in out.values())
    print(f"{len(out)} distance cases, {n_exc} raise")


if __name__ == "__main__":
    main()
