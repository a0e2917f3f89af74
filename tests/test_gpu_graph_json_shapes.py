"""GPU: export --format json on generated inputs, byte for byte against the host restatement
(tests/graph_json_util.py, itself pinned against the reference by tests/test_graph_json_host.py) in the
three graph classes: the render block boundary (256 items), names that overflow a block's LDS stage, one
pair repeated 70 000 times, a 70 000-target source and 70 000 one-target sources (every radix digit of the
ids), random entries with local duplicates, every escape class, degenerate files, run-to-run identity,
and the CLI."""
import random
import subprocess
import sys
from pathlib import Path

import pytest

import graph_json_util as gj

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BLOCK = 256  # kGjItems: items (nodes, links, the closing item) per render block


def _export(src, out, mode):
    from gfa2network_amd import export_graph_json

    bidirected, keep = gj.MODES[mode]
    export_graph_json(src, out, bidirected=bidirected, keep_directed_bidir=keep)
    return out.read_bytes()


def _check(records, tmp_path, data=None):
    src = tmp_path / "in.gfa"
    src.write_bytes(gj.gfa_bytes(records) if data is None else data)
    for mode, (bidirected, keep) in gj.MODES.items():
        want = gj.render(gj.events_from_records(records, bidirected, keep), bidirected, keep)
        got = _export(src, tmp_path / f"{mode}.json", mode)
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
    of n_links records over few enough nodes that some repeat; in the multigraph modes every entry)."""
    _check(_chain(n_nodes, n_links, random.Random(n_nodes * 1000 + n_links)), tmp_path)


@pytest.mark.parametrize("n_links", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK])
def test_distinct_links_at_block_boundaries(gpu, tmp_path, n_links):
    """Exactly n_links DiGraph links (distinct pairs) behind 2 nodes' worth of items, and behind none."""
    recs = [("L", f"a{k}", "+", f"b{k}", "-") for k in range(n_links)]  # nodes minted by the records
    _check(recs, tmp_path)
    hub = [("S", "h")] + [("L", "h", "+", f"t{k}", "+") for k in range(n_links - 1)] + [("L", "h", "-", "h", "+")]
    _check(hub, tmp_path)


def test_long_names_overflow_the_stage(gpu, tmp_path):
    """Names of about 40 KB mixed with short ones: a block's text exceeds the LDS stage and is written
    item by item straight to HBM, next to blocks that are staged."""
    rng = random.Random(3)
    names = []
    for k in range(700):
        names.append(f"n{k}_" + ("x" * rng.choice([39_000, 41_000]) if k % 97 == 5 else "y" * rng.choice([0, 1, 30])))
    recs = [("S", nm) for nm in names]
    for _ in range(1500):
        recs.append(("L", rng.choice(names), rng.choice("+-"), rng.choice(names), rng.choice("+-")))
    _check(recs, tmp_path)


def test_one_pair_repeated(gpu, tmp_path):
    """One pair 70 000 times: a group far larger than a block, keys up to 5 digits; in plain mode one link
    with the last record's orientations."""
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


@pytest.fixture(scope="module")
def random_case(tmp_path_factory):
    """70 000 nodes, 200 000 random entries with local duplicates; the restatement of each mode once."""
    rng = random.Random(11)
    recs = [("S", str(k + 1)) for k in range(70_000)]
    for _ in range(200_000):
        u = rng.randrange(70_000)
        v = min(69_999, max(0, u + rng.randrange(-3, 4)))
        recs.append(("L", str(u + 1), rng.choice("+-"), str(v + 1), rng.choice("+-")))
    d = tmp_path_factory.mktemp("gj_random")
    src = d / "in.gfa"
    src.write_bytes(gj.gfa_bytes(recs))
    want = {mode: gj.render(gj.events_from_records(recs, b, k), b, k) for mode, (b, k) in gj.MODES.items()}
    return src, d, want


@pytest.mark.parametrize("mode", ["plain", "bidirected", "keep"])
def test_random_entries(gpu, random_case, mode):
    src, d, want = random_case
    assert _export(src, d / f"{mode}.json", mode) == want[mode]


@pytest.mark.parametrize("mode", ["plain", "bidirected", "keep"])
def test_same_bytes_every_run(gpu, random_case, mode):
    src, d, want = random_case
    first = _export(src, d / f"{mode}.1.json", mode)
    second = _export(src, d / f"{mode}.2.json", mode)
    assert first == second == want[mode]


def test_escape_classes(gpu, tmp_path):
    """Every escape class in names (ASCII: the two-character escapes, \\u00XX below 0x20 and at 0x7f, '/'
    left alone) and in orientation strings (those, and 2-, 3- and 4-byte UTF-8: \\uXXXX, surrogate pairs)."""
    names = ['q"x', "b\\y", "r\rz", "c\x01d", "e\x7ff", "sl/ash", "bs\bff\f", "\x1f", "\x00", "~ ", "plain"]
    oris = ["+", "-", "é", "€", "\U0001F600", "a\"b\\c", "\r", "\x01\x7f", "\u0080߿ࠀ￿\U00010000\U0010ffff",
            "x" * 300 + "é" * 200]
    rng = random.Random(4)
    recs = [("S", nm) for nm in names]
    for k in range(600):
        recs.append(("L", rng.choice(names), rng.choice("+-"), rng.choice(names), oris[k % len(oris)]))
    src = tmp_path / "in.gfa"
    src.write_bytes(gj.gfa_bytes(recs))
    want = gj.render(gj.events_from_records(recs, False, False), False, False)
    assert _export(src, tmp_path / "plain.json", "plain") == want
    # the multigraph modes put the orientation into the node key: ASCII ones only
    ascii_recs = [r for r in recs if r[0] == "S" or r[4].isascii()]
    _check(ascii_recs, tmp_path)


def test_degenerate_files(gpu, tmp_path):
    _check([("S", f"s{k}") for k in range(300)], tmp_path)                          # segments only
    _check([("L", f"a{k % 50}", "+", f"b{k % 7}", "-") for k in range(300)], tmp_path)  # edges only
    _check([], tmp_path)                                                            # an empty file
    _check([], tmp_path, data=b"H\tVN:Z:1.0\n")                                     # no records


def test_cli_file_and_stdout(gpu, tmp_path):
    recs = [("S", "s1"), ("S", "s2"), ("L", "s1", "+", "s2", "-"), ("L", "s2", "+", "s1", "+"),
            ("L", "s1", "-", "s2", "+")]
    src = tmp_path / "e.gfa"
    src.write_bytes(gj.gfa_bytes(recs))
    out = tmp_path / "g.json"
    subprocess.run([sys.executable, "-m", "gfa2network_amd", "export", str(src), "--format", "json", "--output",
                    str(out)], check=True, cwd=ROOT)
    assert out.read_bytes() == gj.render(gj.events_from_records(recs, False, False), False, False)
    r = subprocess.run([sys.executable, "-m", "gfa2network_amd", "export", str(src), "--format", "json",
                        "--bidirected", "--keep-directed-bidir"], check=True, cwd=ROOT, capture_output=True)
    assert r.stdout == gj.render(gj.events_from_records(recs, True, True), True, True)
    r = subprocess.run([sys.executable, "-m", "gfa2network_amd", "export", str(src), "--format", "graphml"],
                       cwd=ROOT, capture_output=True)
    assert r.returncode == 2
