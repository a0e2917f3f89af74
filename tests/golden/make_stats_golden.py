#!/usr/bin/env python3
"""Golden fixtures for ``compute_stats`` / ``gfa2network stats`` from the REAL reference.

Runs only where the pure-Python reference (and NetworkX) is importable: its checkout is named by
the first argument or the environment variable ``G2N_REFERENCE``.  For every file under
tests/golden/inputs and tests/golden/stats_inputs, with ``directed`` on and off and
``strip_orientation`` on and off (the two files with non-ASCII node names also with
``raw_bytes_id`` on), it records
  * ``analysis.compute_stats(...)``: the returned dict as [key, value] pairs in the dict's order
    (JSON keeps int 0 and float 0.0 apart), or the exception's type and message,
  * the stdout text of ``cli.main([--raw-bytes-id] stats IN [--undirected] [--strip-orientation])``
    (cli.py:364-376; whatever was printed before an exception).
Output: tests/golden/expected/stats.json (plain data; nothing here is imported by the product,
the GPU tests or bench.py).  ``cases()`` lists the keys the file must hold: the tests import it
to check that none is missing.
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys
import warnings
from pathlib import Path

HERE = Path(__file__).resolve().parent
FOLDERS = ("inputs", "stats_inputs")
RAW_BYTES_FILES = ("bad_utf8_name.gfa", "utf8_names.gfa")  # node names that are not ASCII


def case_key(folder: str, name: str, directed: bool, strip: bool, raw_bytes_id: bool) -> str:
    return f"{folder}/{name}|directed={int(directed)}|strip={int(strip)}|raw={int(raw_bytes_id)}"


def cases() -> list[tuple[str, Path, bool, bool, bool]]:
    """(key, input, directed, strip_orientation, raw_bytes_id) of every case stats.json holds."""
    out = []
    for folder in FOLDERS:
        for inp in sorted((HERE / folder).iterdir()):
            for raw in (False, True) if inp.name in RAW_BYTES_FILES else (False,):
                for directed in (True, False):
                    for strip in (False, True):
                        out.append((case_key(folder, inp.name, directed, strip, raw), inp, directed, strip, raw))
    return out


def main() -> None:
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("G2N_REFERENCE")
    if not ref:
        raise SystemExit("usage: make_stats_golden.py REFERENCE_CHECKOUT  (or G2N_REFERENCE)")
    sys.path.insert(0, ref)
    from gfa2network import cli  # noqa: E402  (the reference)
    from gfa2network.analysis import compute_stats  # noqa: E402

    out = {}
    for key, inp, directed, strip, raw in cases():
        stats = exc = None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                got = compute_stats(str(inp), directed=directed, strip_orientation=strip, raw_bytes_id=raw)
                stats = [[k, v] for k, v in got.items()]
            except Exception as e:  # noqa: BLE001 - recorded as data
                exc = [type(e).__name__, str(e)]
            argv = (["--raw-bytes-id"] if raw else []) + ["stats", str(inp)]
            argv += [] if directed else ["--undirected"]
            argv += ["--strip-orientation"] if strip else []
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                try:
                    cli.main(argv)
                except Exception:  # noqa: BLE001 - the same failure as above
                    pass
        out[key] = {"stats": stats, "exc": exc, "stdout": buf.getvalue()}
    (HERE / "expected" / "stats.json").write_text(json.dumps(out, indent=0, sort_keys=True) + "\n")
    print(f"{len(out)} stats cases, {sum(v['exc'] is not None for v in out.values())} raise")


if __name__ == "__main__":
    main()
