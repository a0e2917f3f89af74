"""Host restatement of ``export --format json`` (reference cli.py:282-306): what
``json.dump(nx.node_link_data(G))`` writes for the graph the reference builds, from plain dicts and
``json.dumps`` over the list of calls the builder makes on its graph — no NetworkX import.

An event is ``["n", key]`` (``G.add_node``) or ``["e", a, b, attrs]`` (``G.add_edge``, builders.py:246-256).
tests/test_graph_json_host.py pins :func:`render` against the reference's own bytes for the event lists
the reference recorded (tests/golden/expected/graph_json.json); the GPU tests then compare the product
with :func:`render` on inputs they generate.
"""
from __future__ import annotations

import base64
import hashlib
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
MODES = {"plain": (False, False), "bidirected": (True, False), "keep": (True, True)}  # (bidirected, keep)


def graph_class(bidirected: bool, keep: bool) -> tuple[bool, bool]:
    """(directed, multigraph) of the class builders.py:138-141 picks under ``directed=True``."""
    return (not bidirected) or keep, bidirected


def render(events, bidirected: bool, keep: bool) -> bytes:
    directed, multi = graph_class(bidirected, keep)
    ids: dict = {}      # node -> id, in first-touch order
    groups: dict = {}   # (source, target) -> the attrs of its entries, in stream order; dict order = first entry
    for ev in events:
        if ev[0] == "n":
            ids.setdefault(ev[1], len(ids))
            continue
        _, a, b, attrs = ev
        ids.setdefault(a, len(ids))
        ids.setdefault(b, len(ids))
        if not directed and ids[b] < ids[a]:  # an undirected edge is reported from its earlier node
            a, b = b, a
        groups.setdefault((a, b), []).append(attrs)
    links = []
    for s, t in sorted(groups, key=lambda st: ids[st[0]]):  # stable: first entries keep stream order
        members = groups[(s, t)]
        if multi:
            links += [{"source": s, "target": t, "key": k} for k in range(len(members))]
        else:  # add_edge updates the one attribute dict: the last record's values, the first one's key order
            links.append({**members[-1], "source": s, "target": t})
    doc = {"directed": directed, "multigraph": multi, "graph": {}, "nodes": [{"id": k} for k in ids], "links": links}
    return json.dumps(doc).encode()


def events_from_records(records, bidirected: bool, keep: bool) -> list:
    """builders.py:163-256 for records ``("S", name)`` / ``("L", u, ori_from, v, ori_to)`` (all ``str``)."""
    ev = []
    for rec in records:
        if rec[0] == "S":
            ev += [["n", rec[1] + ":+"], ["n", rec[1] + ":-"]] if bidirected else [["n", rec[1]]]
            continue
        _, u, of, v, ot = rec
        if not bidirected:
            ev.append(["e", u, v, {"orientation_from": of, "orientation_to": ot}])
            continue
        ev.append(["e", f"{u}:{of}", f"{v}:{ot}", {}])
        if not keep:
            ev.append(["e", f"{v}:{'-' if ot == '+' else '+'}", f"{u}:{'-' if of == '+' else '+'}", {}])
    return ev


def gfa_bytes(records) -> bytes:
    out = []
    for rec in records:
        if rec[0] == "S":
            out.append(f"S\t{rec[1]}\t*\n")
        else:
            out.append(f"L\t{rec[1]}\t{rec[2]}\t{rec[3]}\t{rec[4]}\t0M\n")
    return "".join(out).encode()


# ---- the group / order step on entry arrays, two ways -------------------------------------------------
def order_dict_form(rows, cols, unordered: bool, multi: bool) -> list:
    """Links as (source, target, x) in listing order — x the key (multi) or the stream position of the
    group's last entry — by the dictionaries NetworkX keeps."""
    groups: dict = {}
    for k, (r, c) in enumerate(zip(rows, cols)):
        if unordered and c < r:
            r, c = c, r
        groups.setdefault((int(r), int(c)), []).append(k)
    out = []
    for s, t in sorted(groups, key=lambda st: st[0]):
        ks = groups[(s, t)]
        out += [(s, t, j) for j in range(len(ks))] if multi else [(s, t, ks[-1])]
    return out


def order_kernel_form(rows, cols, unordered: bool, multi: bool) -> list:
    """The same in the form the kernels use: stable sorts, head flags, scans, first-entry compaction."""
    r = np.asarray(rows, dtype=np.int64)
    c = np.asarray(cols, dtype=np.int64)
    m = len(r)
    if m == 0:
        return []
    if unordered:
        r, c = np.minimum(r, c), np.maximum(r, c)
    idx1 = np.argsort(c, kind="stable")                      # G2: LSD, on c ...
    perm = idx1[np.argsort(r[idx1], kind="stable")]          # ... then on r: ordered by (r, c, k)
    rs, cs = r[perm], c[perm]
    head = np.ones(m, dtype=np.int64)                        # G3
    head[1:] = (rs[1:] != rs[:-1]) | (cs[1:] != cs[:-1])
    hx = np.cumsum(head) - head                              # exclusive scan
    gid = hx + head - 1
    G = int(head.sum())
    hs = np.empty(G + 1, dtype=np.int64)
    hs[hx[head == 1]] = np.nonzero(head)[0]
    hs[G] = m
    fflag = np.zeros(m, dtype=np.int64)                      # G4: first entries, in stream order
    fgroup = np.zeros(m, dtype=np.int64)
    heads = np.nonzero(head)[0]
    fflag[perm[heads]] = 1
    fgroup[perm[heads]] = hx[heads]
    fx = np.cumsum(fflag) - fflag
    lr = np.empty(G, dtype=np.int64)
    lg = np.empty(G, dtype=np.int64)
    firsts = np.nonzero(fflag)[0]
    lr[fx[firsts]] = r[firsts]
    lg[fx[firsts]] = fgroup[firsts]
    order = lg[np.argsort(lr, kind="stable")]                # G5: listing order of the groups
    cnt = (hs[order + 1] - hs[order]) if multi else np.ones(G, dtype=np.int64)  # G6
    base = np.cumsum(cnt) - cnt
    gbase = np.empty(G, dtype=np.int64)
    gbase[order] = base
    n_links = int(cnt.sum())
    out = [None] * n_links                                   # G7
    rank = np.arange(m) - hs[gid]
    for j in range(m):
        g = gid[j]
        if multi:
            out[gbase[g] + rank[j]] = (int(rs[j]), int(cs[j]), int(rank[j]))
        elif j + 1 == hs[g + 1]:
            out[gbase[g]] = (int(rs[j]), int(cs[j]), int(perm[j]))
    return out


# ---- the reference's recorded outputs -----------------------------------------------------------------
_golden = None


def golden() -> dict:
    global _golden
    if _golden is None:
        _golden = json.loads((GOLDEN / "expected" / "graph_json.json").read_text())
    return _golden


def golden_input(key: str) -> Path:
    name = key.split("|")[0]
    if name.startswith("new/"):
        return GOLDEN / "graph_json" / "inputs" / name[4:]
    return GOLDEN / "inputs" / name


def matches_golden_text(case: dict, text: bytes | None) -> bool:
    """text = the bytes of the output file, None when there is none."""
    if "text_sha256" in case:
        return text is not None and len(text) == case["text_len"] and \
            hashlib.sha256(text).hexdigest() == case["text_sha256"]
    if case["text_b64"] is None:
        return text is None
    return text == base64.b64decode(case["text_b64"])
