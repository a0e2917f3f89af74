"""The DESIGN.md table of the weighted path distances (needs a GPU): per input one JSON line with
rounds, launches, ms_search / ms_tables (best of 5 after a warm-up, min and mean), the unweighted
levels / ms_bfs of the same structure from the same loop, and scipy's dijkstra wall time.

    python tools/wdist_table.py
"""
import json
import pathlib
import sys
import tempfile
import time

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from gfa2network_amd import convert_format, load_paths, parse_gfa, path_distances  # noqa: E402



def csr(rows, cols, w, n):
    return sp.coo_matrix((w, (rows, cols)), shape=(n, n)).tocsr()


def und(a, b, w):
    return np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w])


def measure(name, A, paths):
    rec = {"input": name, "n": int(A.shape[0]), "nnz": int(A.nnz), "paths": len(paths)}
    for method in ("min", "mean"):
        best, bestu = None, None
        for it in range(6):
            _, info = path_distances(A, paths, method=method, weighted=True, return_info=True)
            _, infou = path_distances(A, paths, method=method, return_info=True)
            if it == 0:
                continue
            if best is None or info["ms_search"] < best["ms_search"]:
                best = info
            if bestu is None or infou["ms_bfs"] < bestu["ms_bfs"]:
                bestu = infou
        rec[method] = {"rounds": best["rounds"], "launches": best["launches"], "batch_paths": best["batch_paths"],
                       "ms_search": round(best["ms_search"], 3), "ms_tables": round(best["ms_tables"], 3),
                       "levels": bestu["levels"], "ms_bfs": round(bestu["ms_bfs"], 3)}
    t0 = time.perf_counter()
    for p in paths:
        dijkstra(A, directed=True, indices=np.unique(p), min_only=True)
    rec["scipy_dijkstra_s"] = round(time.perf_counter() - t0, 4)
    print(json.dumps(rec), flush=True)


def main():
    rng = np.random.default_rng(13)
    n = 100_003
    ids = np.random.default_rng(7).permutation(n)
    r, c, w = und(ids[:-1], ids[1:], rng.random(n - 1))
    measure("chain", csr(r, c, w, n), [[int(ids[0])], [int(ids[n // 2])], [int(ids[-1])]])
    n = 100_001
    leaves = np.arange(1, n)
    r, c, w = und(np.zeros(n - 1, dtype=np.int64), leaves, rng.random(n - 1))
    measure("star", csr(r, c, w, n), [[0], [1, 78, n - 1], [6]])
    s = 300
    idx = np.arange(s * s, dtype=np.int64).reshape(s, s)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    r, c, w = und(a, b, rng.random(len(a)))
    measure("grid", csr(r, c, w, s * s), [[0], [int(idx[s // 2, s // 2])], idx[[30, 110, 190, 270], :].ravel().tolist()])
    # DRB1-3123 with an RC:i: tag (1 .. 99) on every L line
    src = (ROOT / "tests" / "golden" / "inputs" / "DRB1-3123_unsorted.gfa").read_text().splitlines()
    out = [ln + f"\tRC:i:{int(rng.integers(1, 100))}" if ln.startswith("L\t") else ln for ln in src]
    with tempfile.TemporaryDirectory() as tmp:
        p = pathlib.Path(tmp) / "drb1_rc.gfa"
        p.write_text("\n".join(out) + "\n")
        A, nodes = parse_gfa(str(p), build_graph=False, build_matrix=True, weight_tag="RC", asymmetric=True,
                             return_node_list=True)
        steps_of = load_paths(str(p))
    A = convert_format(A, "csr")
    index = {nm: k for k, nm in enumerate(nodes)}
    paths = [[index[x] for x in steps] for steps in steps_of.values()]
    measure("DRB1-3123 + RC", A, paths)


main()
