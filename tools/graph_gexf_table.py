"""The DESIGN.md rendering rates of export --format gexf next to export --format json (needs a GPU): on one
synthetic input of 1 000 000 S and 4 000 000 L lines, per graph class one JSON line with the text phase of
each export (gx_text: T1-T3 of g2n_graphgexf.hip; gj_text: T1-T3 of g2n_graphjson.hip), the bytes each
wrote and the rates in bytes per millisecond.  Best of RUNS after a warm-up, by the text phase.

    python tools/graph_gexf_table.py
"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from gfa2network_amd import _native as nat, synth  # noqa: E402
from gfa2network_amd.api import _gexf_head  # noqa: E402

RUNS = 5
MODES = {"plain": (False, False), "bidirected": (True, False), "keep": (True, True)}


def best_of(run, phase):
    best = None
    for it in range(RUNS + 1):
        raw = run()
        assert raw.status == 0, raw.message
        if it and (best is None or raw.phase_ms[phase] < best.phase_ms[phase]):
            best = raw
    return best


def main():
    data = synth.host_bytes(1_000_000, 4_000_000, seed=7)
    head = _gexf_head("NetworkX 3.4.2", "2026-10-21")
    for mode, (bidirected, keep) in MODES.items():
        kw = dict(bidirected=bidirected, keep_directed_bidir=keep)
        gx = best_of(lambda: nat.graph_gexf_from_buffer(data, nat.make_options(output=nat.OUT_GRAPH_GEXF, **kw), head),
                     "gx_text")
        gj = best_of(lambda: nat.build_from_buffer(data, nat.make_options(output=nat.OUT_GRAPH_JSON, **kw)), "gj_text")
        rec = {"mode": mode, "input_bytes": len(data), "nodes": gx.n_nodes, "edges": gx.n_edges}
        for name, raw, phase in (("gexf", gx, "gx_text"), ("json", gj, "gj_text")):
            ms = raw.phase_ms[phase]
            rec[name] = {"bytes_written": int(raw.data.size), "ms_text": round(ms, 3),
                         "bytes_per_ms": round(raw.data.size / ms), "ms_total": round(sum(raw.phase_ms.values()), 3)}
        print(json.dumps(rec), flush=True)
    print(json.dumps({"runs": RUNS, "version": nat.version()}), flush=True)


if __name__ == "__main__":
    main()
