"""What the CSR distance searches report about themselves (needs a GPU): per case one JSON line with,
for each of the calls, the deterministic fields of its g2n_dist_info / g2n_wdist_info — levels or
rounds, launches, batches and, weighted, batch_paths; the ms_* fields are left out.
tests/test_gpu_dist_info.py holds this tool's output as literals, recorded at the commit before the
host code around the searches was folded onto shared batch drivers.

Calls: hop min, hop mean, weighted min, weighted mean-fold (the K x K path tables), pair sums, pair
table, weighted pair table (node to node).

Cases (weighted ones are trees with distinct weights and one node a path: shortest paths are unique,
so `rounds` does not depend on the order of the atomics):
* chain: 70 nodes, a path / source at each end, one of them with a -1 step / id — the narrow regime only;
* star: a hub, 3000 leaves, a second-level node on every leaf; the hub is a source, so its row (past
  kStatsShortRow) overflows the narrow queue (kDistNarrowCap = 2048): one wide level, then narrow again;
* two-batches: the chain with 65 one-node paths / sources — two batches, fold mode in reversed order;
* empty-*: K = 0, n_src = 0 with targets, n_tgt = 0 with sources, and a graph without entries.

    python tools/dist_info_table.py
"""
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from gfa2network_amd import _native as nat  # noqa: E402

HOP_FIELDS = ("levels", "launches", "batches")
W_FIELDS = ("rounds", "launches", "batches", "batch_paths")


def tree_csr(parent_of: dict, n: int):
    """The undirected tree child - parent as int64 indptr / indices and distinct float64 weights."""
    child = np.fromiter(parent_of.keys(), dtype=np.int64)
    parent = np.fromiter(parent_of.values(), dtype=np.int64)
    w = 0.25 + np.random.default_rng(11).permutation(len(child)) / 1024.0
    rows, cols, vals = np.concatenate([child, parent]), np.concatenate([parent, child]), np.concatenate([w, w])
    order = np.lexsort((cols, rows))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    return indptr, cols[order], vals[order]


def chain(n=70):
    return tree_csr({k: k - 1 for k in range(1, n)}, n) + (n,)


def star(leaves=3000):
    parent_of = {k: 0 for k in range(1, leaves + 1)}
    parent_of.update({leaves + k: k for k in range(1, leaves + 1)})
    return tree_csr(parent_of, 2 * leaves + 1) + (2 * leaves + 1,)


def no_entries(n=5):
    return np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), n


def cases():
    """name -> (indptr, indices, values, n), the paths, the sources, the targets"""
    few = [0, 69, -1]
    return {
        "chain": (chain(), [[0, -1], [69]], [0, 69, -1], [69, -1, 0, 35]),
        "star": (star(), [[0], [6000]], [0, 6000], [5, 3005, 0]),
        "two-batches": (chain(), [[k] for k in range(65)], list(range(65)), few),
        "empty-K0-nsrc0": (chain(), [], [], few),
        "empty-ntgt0": (chain(), [[], []], few, []),
        "empty-no-entries": (no_entries(), [[0], [3]], [0], [3, 0]),
    }


def pick(info: dict, fields) -> dict:
    return {f: info[f] for f in fields}


def run_case(name: str) -> dict:
    (ip, ix, val, n), paths, sources, targets = cases()[name]
    ptr = np.zeros(len(paths) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in paths], out=ptr[1:])
    nodes = np.array([v for p in paths for v in p], dtype=np.int64)
    src, tgt = np.array(sources, dtype=np.int64), np.array(targets, dtype=np.int64)
    out = {}
    for key, mean in (("hop min", False), ("hop mean", True)):
        out[key] = pick(nat.csr_path_distances_host(ip, ix, n, ptr, nodes, mean)[1], HOP_FIELDS)
    for key, mean in (("weighted min", False), ("weighted mean-fold", "fold")):
        out[key] = pick(nat.csr_path_distances_weighted_host(ip, ix, val, n, ptr, nodes, mean)[1], W_FIELDS)
    for key, table in (("pair sums", False), ("pair table", True)):
        out[key] = pick(nat.csr_pair_distances_host(ip, ix, None, n, src, tgt, table)[1], HOP_FIELDS)
    out["weighted pair table"] = pick(nat.csr_pair_distances_host(ip, ix, val, n, src, tgt, True)[1], W_FIELDS)
    return out


def main():
    for name in sys.argv[1:] or cases():
        print(json.dumps({name: run_case(name)}), flush=True)


if __name__ == "__main__":
    main()
