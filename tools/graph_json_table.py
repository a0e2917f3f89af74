"""The DESIGN.md table of export --format json (needs a GPU): per input and graph class one JSON line
with the device phase times of the native call — build (everything up to the stream-order COO and the
names), spans (the records' orientation spans, plain mode), order (group / order: G1-G7), text (T1-T3) —
the bytes written, and, from the same run, export --format edge-list's render time (its edge_text phase)
and whole device time on the same input as the yardstick.  Best of RUNS after a warm-up, by total.
Inputs: DRB1-3123, the 50 000 / 200 000 synthetic of tests/test_gpu_export.py (both launch-bound) and
a 1 000 000 / 4 000 000 one.

    python tools/graph_json_table.py
"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from gfa2network_amd import _native as nat, synth  # noqa: E402

RUNS = 5
MODES = {"plain": (False, False), "bidirected": (True, False), "keep": (True, True)}


def best_of(data, opts):
    best = None
    for it in range(RUNS + 1):
        raw = nat.build_from_buffer(data, opts)
        assert raw.status == 0, raw.message
        total = sum(raw.phase_ms.values())
        if it and (best is None or total < best[0]):
            best = (total, raw)
    return best


def measure(name, data):
    for mode, (bidirected, keep) in MODES.items():
        total, raw = best_of(data, nat.make_options(bidirected=bidirected, keep_directed_bidir=keep,
                                                    output=nat.OUT_GRAPH_JSON))
        ph = raw.phase_ms
        own = {k: ph.get(k, 0.0) for k in ("gj_spans", "gj_order", "gj_text")}
        rec = {"input": name, "mode": mode, "input_bytes": len(data), "nodes": raw.n_nodes, "edges": raw.n_edges,
               "bytes_written": int(raw.data.size), "ms_build": round(total - sum(own.values()), 3),
               "ms_spans": round(own["gj_spans"], 3), "ms_order": round(own["gj_order"], 3),
               "ms_text": round(own["gj_text"], 3), "ms_total": round(total, 3)}
        if not keep:  # the edge-list export has the two settings
            etotal, eraw = best_of(data, nat.make_options(bidirected=bidirected, output=nat.OUT_EDGE_LIST))
            rec["edge_list_bytes"] = int(eraw.data.size)
            rec["edge_list_ms_text"] = round(eraw.phase_ms.get("edge_text", 0.0), 3)
            rec["edge_list_ms_total"] = round(etotal, 3)
        print(json.dumps(rec), flush=True)


def main():
    measure("DRB1-3123", (ROOT / "tests" / "golden" / "inputs" / "DRB1-3123_unsorted.gfa").read_bytes())
    measure("synthetic 50000/200000", synth.host_bytes(50_000, 200_000, seed=7))
    # (the two above are launch-bound: a size at which bytes set the time)
    measure("synthetic 1000000/4000000", synth.host_bytes(1_000_000, 4_000_000, seed=7))
    print(json.dumps({"runs": RUNS, "version": nat.version()}), flush=True)


if __name__ == "__main__":
    main()
