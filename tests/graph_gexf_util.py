"""Host restatement of ``export --format gexf`` (reference cli.py:296-297): what ``nx.write_gexf(G, path)``
writes with its defaults (utf-8, prettyprint, version 1.2draft) for the graph the reference builds, from the
list of calls the builder makes on its graph — no NetworkX and no ElementTree import.

The events and the order of nodes and links are tests/graph_json_util.py's: :func:`render` runs its
``render`` over the events (every key replaced by a token, so that ``bytes`` keys pass through JSON) and
lays the listed nodes and links out as XML.  tests/test_graph_gexf_host.py pins the result against the
reference's own bytes (tests/golden/expected/graph_gexf.json) and, where networkx imports, against
``nx.write_gexf`` on random entry lists; the GPU tests then compare the product with :func:`render`.
"""
from __future__ import annotations

import base64
import hashlib
import json
import zlib
from pathlib import Path

import graph_json_util as gj

GOLDEN = gj.GOLDEN
MODES = {**gj.MODES, "raw": (False, False)}  # (bidirected, keep); raw: plain with bytes keys
# the block size and the LDS stage of the render kernel (g2n_graphgexf.hip kGxItems, kGxLds)
BLOCK = 128
STAGE = 32 * 1024


def escape_attrib(s: str) -> str:
    """ElementTree._escape_attrib."""
    for a, b in (("&", "&amp;"), ("<", "&lt;"), (">", "&gt;"), ('"', "&quot;"), ("\r", "&#13;"), ("\n", "&#10;"),
                 ("\t", "&#09;")):
        s = s.replace(a, b)
    return s


def escape_cdata(s: str) -> str:
    """ElementTree._escape_cdata."""
    return s.replace("&", "&amp;").replace("<", "&lt;").replace(">", "&gt;")


def head(creator: str, lastmodified: str) -> str:
    return ("<?xml version='1.0' encoding='utf-8'?>\n"
            '<gexf xmlns="http://www.gexf.net/1.2draft" xmlns:xsi="http://www.w3.org/2001/XMLSchema-instance" '
            'xsi:schemaLocation="http://www.gexf.net/1.2draft http://www.gexf.net/1.2draft/gexf.xsd" version="1.2">\n'
            f'  <meta lastmodifieddate="{escape_attrib(lastmodified)}">\n'
            f"    <creator>{escape_cdata(creator)}</creator>\n"
            "  </meta>\n")


def _key(k, raw: bool):
    """An event's key as the graph holds it: ``str``, or ``bytes`` with raw (recorded as base64; a ``str``
    stands for its latin-1 bytes, one character per byte)."""
    if isinstance(k, dict):
        return base64.b64decode(k["bytes_b64"])
    if raw and isinstance(k, str):
        return k.encode("latin-1")
    return k


def render(events, bidirected: bool, keep: bool, *, raw: bool = False, creator: str, lastmodified: str) -> bytes:
    directed, multi = gj.graph_class(bidirected, keep)
    tokens: dict = {}

    def tok(k):
        return tokens.setdefault(_key(k, raw), f"k{len(tokens)}")

    listed = json.loads(gj.render([[e[0], tok(e[1])] if e[0] == "n" else [e[0], tok(e[1]), tok(e[2]), e[3]]
                                   for e in events], bidirected, keep))
    name = {t: escape_attrib(str(k)) for k, t in tokens.items()}  # str(bytes) is the bytes repr
    out = [head(creator, lastmodified),
           f'  <graph defaultedgetype="{"directed" if directed else "undirected"}" mode="static" name="">\n']
    links = listed["links"]
    if links:  # the first declared attribute inserts the block in front of <nodes>
        out.append('    <attributes mode="static" class="edge">\n')
        if multi:
            out.append('      <attribute id="0" title="networkx_key" type="long" />\n')
        else:
            out.append('      <attribute id="0" title="orientation_from" type="string" />\n')
            out.append('      <attribute id="1" title="orientation_to" type="string" />\n')
        out.append("    </attributes>\n")
    if listed["nodes"]:
        out.append("    <nodes>\n")
        out += [f'      <node id="{name[n["id"]]}" label="{name[n["id"]]}" />\n' for n in listed["nodes"]]
        out.append("    </nodes>\n")
    else:
        out.append("    <nodes />\n")
    if links:
        out.append("    <edges>\n")
        for i, ln in enumerate(links):
            out.append(f'      <edge source="{name[ln["source"]]}" target="{name[ln["target"]]}" id="{i}">\n'
                       "        <attvalues>\n")
            if multi:
                out.append(f'          <attvalue for="0" value="{ln["key"]}" />\n')
            else:
                out.append(f'          <attvalue for="0" value="{escape_attrib(ln["orientation_from"])}" />\n')
                out.append(f'          <attvalue for="1" value="{escape_attrib(ln["orientation_to"])}" />\n')
            out.append("        </attvalues>\n      </edge>\n")
        out.append("    </edges>\n")
    else:
        out.append("    <edges />\n")
    out.append("  </graph>\n</gexf>\n")
    return "".join(out).encode("utf-8")


def gfa_bytes(records, raw: bool = False) -> bytes:
    """gj.gfa_bytes; with raw a name's characters are its bytes (latin-1)."""
    if not raw:
        return gj.gfa_bytes(records)
    return gj.gfa_bytes(records).decode("utf-8").encode("latin-1")


def records_from_gfa(data: bytes) -> list:
    """The ``("S", name)`` / ``("L", u, ori_from, v, ori_to)`` records of a plain GFA1 file whose only graph
    records are S and L lines (the large golden inputs, whose recorded calls would not fit a fixture)."""
    recs = []
    for line in data.split(b"\n"):
        f = line.split(b"\t")
        if f[0] == b"S":
            recs.append(("S", f[1].decode("ascii")))
        elif f[0] == b"L":
            recs.append(("L", f[1].decode("ascii"), f[2].decode(), f[3].decode("ascii"), f[4].decode()))
        else:
            assert f[0] in (b"", b"H", b"P"), f[0]
    return recs


# ---- the reference's recorded outputs -----------------------------------------------------------------
_golden = None


def golden() -> dict:
    global _golden
    if _golden is None:
        _golden = json.loads((GOLDEN / "expected" / "graph_gexf.json").read_text())
    return _golden


def golden_input(key: str) -> Path:
    name = key.split("|")[0]
    if name.startswith("gexf/"):
        return GOLDEN / "graph_gexf" / "inputs" / name[5:]
    return gj.golden_input(key)


def golden_events(key: str) -> list:
    """The calls the reference made for a golden case: recorded, or for a large S/L-only input (the golden
    script checked this equality when it ran) derived from the file."""
    g = golden()
    if key in g["entries"]:
        return g["entries"][key]
    if key in g["entries_raw_from_plain"]:  # the plain run's calls, every key as its ASCII bytes
        return [[e[0]] + [x.encode("ascii") if isinstance(x, str) else x for x in e[1:]]
                for e in g["entries"][key.split("|")[0] + "|plain"]]
    assert key in g["entries_from_records"], key
    import gzip

    data = golden_input(key).read_bytes()
    if key.split("|")[0].endswith(".gz"):
        data = gzip.decompress(data)
    mode = key.split("|")[1]
    bidirected, keep = MODES[mode]
    ev = gj.events_from_records(records_from_gfa(data), bidirected, keep)
    if mode == "raw":
        ev = [[e[0]] + [x.encode("ascii") if isinstance(x, str) else x for x in e[1:]] for e in ev]
    return ev


def golden_text(key: str) -> bytes | None:
    """The document a golden case recorded in full (the shared head, then the case's deflated rest); None
    when the reference wrote no file."""
    g = golden()
    body = g["cases"][key]["body_zb64"]
    return None if body is None else g["head"].encode("ascii") + zlib.decompress(base64.b64decode(body))


def matches_golden_text(key: str, text: bytes | None) -> bool:
    """text = the bytes of the output file, None when there is none."""
    case = golden()["cases"][key]
    if "text_sha256" in case:
        return text is not None and len(text) == case["text_len"] and \
            hashlib.sha256(text).hexdigest() == case["text_sha256"]
    return text == golden_text(key)
