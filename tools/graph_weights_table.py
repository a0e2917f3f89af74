"""The DESIGN.md figures of the weighted graph matrix (needs a GPU), one JSON line each:

  * the hipEvent phase times of a LAST build (``graph_matrix``'s: g2n_graph_weights_from_path) beside
    the SUM build of the same file (the asymmetric float64 CSR with the same weight tag), on the
    largest weighted file ``bench.py --full`` generates (C3's bytes: 1 M S / 4 M L lines with an
    ``RC:i:`` tag), the same SUM build forced onto the row path and the untagged (uniform) build forced
    onto it, each build once after one warm-up of each, through the same host entry;
  * ``ms_search`` / ``ms_tables`` of the weighted mean tables with and without the seeded pass
    (G2N_DIST_MEAN_FOLD against G2N_DIST_MEAN) on a ring with chords, 512 paths of 8 steps.

    python tools/graph_weights_table.py
"""
import json
import pathlib
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from gfa2network_amd import _native as nat  # noqa: E402
from gfa2network_amd import synth  # noqa: E402


def phases(raw):
    if raw.status != nat.OK:
        raise RuntimeError(f"{nat.status_name(raw.status)}: {raw.message}")
    return {k: round(v, 3) for k, v in raw.phase_ms.items() if not k.startswith("_")}


def builds(tmp):
    wl = synth.WORKLOADS["C3"]
    p = str(pathlib.Path(tmp) / "c3.gfa")
    pathlib.Path(p).write_bytes(synth.host_bytes(wl.n_segments, wl.n_links, seed=0, rc_tag=True))
    last = lambda: nat.graph_weights_from_path(  # noqa: E731
        p, nat.make_options(directed=True, weight_tag="RC", want_node_names=False))
    summed = lambda: nat.build_from_path(  # noqa: E731
        p, nat.make_options(directed=True, asymmetric=True, weight_tag="RC", output=nat.OUT_CSR, dtype="float64",
                            want_node_names=False))
    nobuckets = lambda: nat.build_from_path(  # noqa: E731  (SUM through the stable row-sum path, LAST's skeleton)
        p, nat.make_options(directed=True, asymmetric=True, weight_tag="RC", output=nat.OUT_CSR, dtype="float64",
                            want_node_names=False, test_flags=nat.TEST_NO_BUCKETS))
    count = lambda: nat.build_from_path(  # noqa: E731  (the uniform SUM on the row path: the Count policy)
        p, nat.make_options(directed=True, asymmetric=True, output=nat.OUT_CSR, dtype="float64",
                            want_node_names=False, test_flags=nat.TEST_NO_BUCKETS))
    for name, fn in (("last", last), ("sum", summed), ("sum_row_path", nobuckets), ("count_row_path", count)):
        fn()
        raw = fn()
        ph = phases(raw)
        print(json.dumps({"build": name, "nnz": int(len(raw.indices)), "n_edges": int(raw.n_edges), "phase_ms": ph,
                          "device_ms": round(sum(ph.values()), 3)}), flush=True)


def means():
    n, K, L = 50_000, 512, 8
    rng = np.random.default_rng(5)
    u = np.arange(n)
    rows = np.concatenate([u, u[::3]])
    cols = np.concatenate([(u + 1) % n, (u[::3] + 97) % n])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    vals = rng.choice([0.1, 0.2, 0.7], size=len(rows))
    indptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    ptr = np.arange(K + 1, dtype=np.int64) * L
    nodes = rng.integers(0, n, size=K * L).astype(np.int64)
    for mode in (True, "fold"):
        best = None
        for it in range(4):
            _tabs, info = nat.csr_path_distances_weighted_host(indptr, cols.astype(np.int32), vals, n, ptr, nodes, mode)
            if it and (best is None or info["ms_search"] + info["ms_tables"] < best["ms_search"] + best["ms_tables"]):
                best = info
        print(json.dumps({"mean": "fold" if mode == "fold" else "plain", "n": n, "nnz": len(rows), "paths": K,
                          "steps": K * L, **{k: (round(v, 3) if isinstance(v, float) else v)
                                             for k, v in best.items()}}), flush=True)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        builds(tmp)
    means()


if __name__ == "__main__":
    main()
