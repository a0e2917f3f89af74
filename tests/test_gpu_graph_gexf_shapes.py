"""GPU: export --format gexf on generated inputs, byte for byte against the host restatement
(tests/graph_gexf_util.py, itself pinned against the reference and against nx.write_gexf by
tests/test_graph_gexf_host.py) in the three graph classes: the render block boundary (128 items), names
that overflow a block's LDS stage (32 KiB) and a block that fits it by 0 bytes and misses it by 1, the
edge-id digit boundaries, one pair repeated 70 000 times, a 70 000-target source and 70 000 one-target
sources, every escape class, the bytes-repr quote cases, degenerate files, run-to-run identity, and the CLI."""
import random
import subprocess
import sys
import time
from pathlib import Path

import pytest

import graph_gexf_util as gx
import graph_json_util as gj

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BLOCK = gx.BLOCK  # kGxItems: items (nodes, links, the closing item) per render block
STAGE = gx.STAGE  # kGxLds
CREATOR, DATE = "NetworkX 0.test", "2001-02-03"


def _export(src, out, mode, raw=False, creator=CREATOR):
    from gfa2network_amd import export_graph_gexf

    bidirected, keep = gj.MODES[mode]
    export_graph_gexf(src, out, bidirected=bidirected, keep_directed_bidir=keep, raw_bytes_id=raw, creator=creator,
                      lastmodified=DATE)
    return out.read_bytes()


def _want(records, mode, raw=False, creator=CREATOR):
    bidirected, keep = gj.MODES[mode]
    return gx.render(gj.events_from_records(records, bidirected, keep), bidirected, keep, raw=raw, creator=creator,
                     lastmodified=DATE)


def _check(records, tmp_path, data=None, raw=False, modes=("plain", "bidirected", "keep")):
    src = tmp_path / "in.gfa"
    src.write_bytes(gx.gfa_bytes(records, raw) if data is None else data)
    for mode in modes:
        want = _want(records, mode, raw)
        got = _export(src, tmp_path / f"{mode}.gexf", mode, raw)
        assert got == want, (mode, len(got), len(want))


def _chain(n_nodes, n_links, rng):
    names = [f"s{k}" for k in range(n_nodes)]
    recs = [("S", nm) for nm in names]
    for _ in range(n_links):
        recs.append(("L", rng.choice(names), rng.choice("+-"), rng.choice(names), rng.choice("+-")))
    return recs


@pytest.mark.parametrize("n_nodes", [BLOCK - 1, BLOCK, BLOCK + 1])
@pytest.mark.parametrize("n_links", [BLOCK - 1, BLOCK, BLOCK + 1])
def test_block_boundaries(gpu, tmp_path, n_nodes, n_links):
    """Node and link counts at the render block size +- 1 (in plain mode the links are the distinct pairs
    of n_links records; in the multigraph modes every entry; bidirected has 2 * n_nodes nodes)."""
    _check(_chain(n_nodes, n_links, random.Random(n_nodes * 1000 + n_links)), tmp_path)


@pytest.mark.parametrize("n_links", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK])
def test_distinct_links_at_block_boundaries(gpu, tmp_path, n_links):
    """Exactly n_links DiGraph links (distinct pairs) behind 2 nodes' worth of items each, and behind one
    hub: the links start anywhere in a block."""
    recs = [("L", f"a{k}", "+", f"b{k}", "-") for k in range(n_links)]  # nodes minted by the records
    _check(recs, tmp_path)
    hub = [("S", "h")] + [("L", "h", "+", f"t{k}", "+") for k in range(n_links - 1)] + [("L", "h", "-", "h", "+")]
    _check(hub, tmp_path)


def test_long_names_overflow_the_stage(gpu, tmp_path):
    """Names of about 20 KB (written twice per node) mixed with short ones: a block's text exceeds the LDS
    stage and is written item by item straight to HBM, next to blocks that are staged."""
    rng = random.Random(3)
    names = []
    for k in range(700):
        names.append(f"n{k}_" + ("x" * rng.choice([15_000, 21_000]) if k % 97 == 5 else "y" * rng.choice([0, 1, 30])))
    recs = [("S", nm) for nm in names]
    for _ in range(1500):
        recs.append(("L", rng.choice(names), rng.choice("+-"), rng.choice(names), rng.choice("+-")))
    _check(recs, tmp_path)


@pytest.mark.parametrize("short_by", [-1, 0, 1])
def test_first_block_at_the_stage_size(gpu, tmp_path, short_by):
    """BLOCK segments and no edge: block 0 holds the prefix and every node, block 1 the closing item, so block
    0's text is the document without its tail.  A name's length moves it by two bytes and the creator's by
    one: it is made STAGE + short_by bytes long (0: fits exactly; 1: one byte short, written unstaged)."""
    tail = b"    </nodes>\n    <edges />\n  </graph>\n</gexf>\n"
    names = ["n" * 40] + [f"s{k}" for k in range(1, BLOCK)]
    creator = "c"
    for _ in range(2):
        recs = [("S", nm) for nm in names]
        have = len(_want(recs, "plain", creator=creator)) - len(tail)
        delta = STAGE + short_by - have
        names[0] = "n" * (len(names[0]) + delta // 2)
        creator += "c" * (delta % 2)
    recs = [("S", nm) for nm in names]
    want = _want(recs, "plain", creator=creator)
    assert want.endswith(tail) and len(want) - len(tail) == STAGE + short_by and want.count(b"<node ") == BLOCK
    src = tmp_path / "in.gfa"
    src.write_bytes(gx.gfa_bytes(recs))
    assert _export(src, tmp_path / "out.gexf", "plain", creator=creator) == want


@pytest.mark.parametrize("n_links", [9, 10, 11, 99, 100, 101, 999, 1000, 1001])
def test_edge_id_digit_boundaries(gpu, tmp_path, n_links):
    """The running edge id gains a digit at link 10, 100 and 1000: n_links distinct pairs (the DiGraph's
    links, the MultiDiGraph's; the MultiGraph lists 2 * n_links), and half as many records for the MultiGraph
    (n_links links, or n_links +- 1 when odd)."""
    recs = [("S", "h")] + [("L", "h", "+-"[k % 2], f"t{k}", "+") for k in range(n_links)]
    assert _want(recs, "plain").count(b"<edge ") == _want(recs, "keep").count(b"<edge ") == n_links
    _check(recs, tmp_path)
    for half in {n_links // 2, n_links - n_links // 2}:
        _check(recs[:1 + half], tmp_path, modes=("bidirected",))


def test_one_pair_repeated(gpu, tmp_path):
    """One pair 70 000 times: a group far larger than a block, keys and ids up to 5 digits; in plain mode one
    link with the last record's orientations."""
    recs = [("S", "a"), ("S", "b")] + [("L", "a", "+-"[k % 2], "b", "+-"[(k // 3) % 2]) for k in range(70_000)]
    recs[-1] = ("L", "a", "-", "b", "+")
    _check(recs, tmp_path)


def test_hub_source_and_many_sources(gpu, tmp_path):
    """One source with 70 000 distinct targets, then 70 000 sources with one target each: node ids cross
    256 and 65 536 (every radix digit), one row as long as the entry list allows."""
    recs = [("S", "hub")]
    recs += [("L", "hub", "+", f"t{k}", "+-"[k % 2]) for k in range(70_000)]
    recs += [("L", f"u{k}", "+-"[k % 2], f"t{(k * 7) % 70_000}", "+") for k in range(70_000)]
    _check(recs, tmp_path)


NAMES = ["a&b", "c<d", "e>f", 'q"x', "i'j", "r\rz", "end\r", "&<>\"'\r", "b\\y", "c\x01d", "e\x7ff", "\x00", "&amp;",
         "plain"]


def test_escape_classes(gpu, tmp_path):
    """Every escape class (& < > " and \\r; ' a backslash and control bytes left alone) in names and in
    orientation strings, those with 2-, 3- and 4-byte UTF-8 passed through verbatim."""
    oris = ["+", "-", "&", "<", ">", '"', "'", "\r", "é", "€", "\U0001F600", "a\"b&c<d>e\rf'g", "\x01\x7f", "&quot;",
            "x" * 300 + "é&" * 200]
    rng = random.Random(4)
    recs = [("S", nm) for nm in NAMES]
    for k in range(600):
        recs.append(("L", rng.choice(NAMES), rng.choice("+-"), rng.choice(NAMES), oris[k % len(oris)]))
    _check(recs, tmp_path, modes=("plain",))
    # the multigraph modes put the orientation into the node key: ASCII ones only
    _check([r for r in recs if r[0] == "S" or r[4].isascii()], tmp_path)


def test_bytes_keys(gpu, tmp_path):
    """raw_bytes_id: str(key), the bytes repr — the three quote cases (' only: double-quoted; " only and
    both: single-quoted), a backslash, \\t-less control bytes as \\xNN and \\r, high bytes — then escaped."""
    names = ["it's", 'say"hi"', "both'\"", "back\\slash", "r\rz", "c\x01\x7f", "hi\xe9gh", "q'\xff", "\x80", "&<>",
             "plain", "'", '"', "\\"]
    rng = random.Random(6)
    recs = [("S", nm) for nm in names]
    for _ in range(400):
        recs.append(("L", rng.choice(names), rng.choice("+-"), rng.choice(names), rng.choice("+-")))
    _check(recs, tmp_path, raw=True)
    assert b'id="b&quot;it\'s&quot;"' in _want(recs, "plain", raw=True)


def test_degenerate_files(gpu, tmp_path):
    _check([("S", f"s{k}") for k in range(300)], tmp_path)                          # segments only: <edges />
    assert b"<attributes" not in _want([("S", "s")], "plain")
    _check([("L", f"a{k % 50}", "+", f"b{k % 7}", "-") for k in range(300)], tmp_path)  # edges only
    _check([], tmp_path)                                                            # an empty file
    _check([], tmp_path, data=b"H\tVN:Z:1.0\n")                                     # an H line only
    _check([], tmp_path, raw=True)


@pytest.fixture(scope="module")
def random_case(tmp_path_factory):
    """20 000 nodes, 60 000 random entries with local duplicates; the restatement of each mode once."""
    rng = random.Random(11)
    recs = [("S", str(k + 1)) for k in range(20_000)]
    for _ in range(60_000):
        u = rng.randrange(20_000)
        v = min(19_999, max(0, u + rng.randrange(-3, 4)))
        recs.append(("L", str(u + 1), rng.choice("+-"), str(v + 1), rng.choice("+-")))
    d = tmp_path_factory.mktemp("gx_random")
    src = d / "in.gfa"
    src.write_bytes(gj.gfa_bytes(recs))
    return src, d, {mode: _want(recs, mode) for mode in gj.MODES}


@pytest.mark.parametrize("mode", ["plain", "bidirected", "keep"])
def test_same_bytes_every_run(gpu, random_case, mode):
    src, d, want = random_case
    first = _export(src, d / f"{mode}.1.gexf", mode)
    second = _export(src, d / f"{mode}.2.gexf", mode)
    assert first == second == want[mode]


def test_file_objects_and_errors(gpu, tmp_path):
    """output as a binary file object; a file-object source; a failed build leaves no file."""
    import io

    from gfa2network_amd import export_graph_gexf

    recs = [("S", "s1"), ("L", "s1", "+", "s2", "-")]
    buf = io.BytesIO()
    export_graph_gexf(io.BytesIO(gj.gfa_bytes(recs)), buf, creator=CREATOR, lastmodified=DATE)
    assert buf.getvalue() == _want(recs, "plain")
    bad = tmp_path / "bad.gfa"
    bad.write_bytes(b"S\ts1\t*\nL\ts1\t+\n")
    with pytest.raises(ValueError, match="Malformed L record"):
        export_graph_gexf(bad, tmp_path / "none.gexf", creator=CREATOR, lastmodified=DATE)
    assert not (tmp_path / "none.gexf").exists()


def test_cli_file_and_default_output(gpu, tmp_path):
    """--output FILE writes the file; the default output is the reference's: nx.write_gexf(G, "-") creates the
    file "-" in the working directory; --format gexf exits 0, graphml still 2.  The CLI passes no creator and
    no date: NetworkX's version string and today."""
    nx = pytest.importorskip("networkx")
    import os

    recs = [("S", "s1"), ("S", "s2"), ("L", "s1", "+", "s2", "-"), ("L", "s2", "+", "s1", "+"),
            ("L", "s1", "-", "s2", "+")]
    src = tmp_path / "e.gfa"
    src.write_bytes(gj.gfa_bytes(recs))
    out = tmp_path / "g.gexf"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(ROOT)] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    cmd = [sys.executable, "-m", "gfa2network_amd"]

    def want(mode, dates, raw=False):
        bidirected, keep = gj.MODES[mode]
        ev = gj.events_from_records(recs, bidirected, keep)
        return [gx.render(ev, bidirected, keep, raw=raw, creator=f"NetworkX {nx.__version__}", lastmodified=d)
                for d in dates]

    d0 = time.strftime("%Y-%m-%d")
    r = subprocess.run(cmd + ["export", str(src), "--format", "gexf", "--output", str(out)], cwd=tmp_path, env=env)
    assert r.returncode == 0
    r = subprocess.run(cmd + ["export", str(src), "--format", "gexf", "--bidirected", "--keep-directed-bidir"],
                       cwd=tmp_path, env=env, capture_output=True)
    assert r.returncode == 0 and r.stdout == b""
    r = subprocess.run(cmd + ["--raw-bytes-id", "export", str(src), "--format", "gexf", "--output", str(tmp_path / "r")],
                       cwd=tmp_path, env=env)
    assert r.returncode == 0
    dates = {d0, time.strftime("%Y-%m-%d")}  # (two when the day changed meanwhile)
    assert out.read_bytes() in want("plain", dates)
    assert (tmp_path / "-").read_bytes() in want("keep", dates)
    assert (tmp_path / "r").read_bytes() in want("plain", dates, raw=True)
    r = subprocess.run(cmd + ["export", str(src), "--format", "graphml"], cwd=tmp_path, env=env, capture_output=True)
    assert r.returncode == 2
