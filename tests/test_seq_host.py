"""CPU: the sequence-distance surface without a GPU — exports, the ctypes layout, the fixture's
completeness, and the CPU checker of the GPU tests (tests/seq_util.py: the restated sequence rules
plus scipy over the CPU oracle's CSR) against every case recorded from the reference."""
import ctypes
import gzip
import json
import subprocess
import sys
from pathlib import Path

import pytest

import seq_util

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
from make_seqdist_golden import ABSENT, FOLDERS, cases, outcome, record_of, unpack  # noqa: E402


@pytest.fixture(scope="module")
def expected():
    return json.loads((GOLDEN / "expected" / "seq_distance.json").read_text())


def text_of(inp: Path) -> bytes:
    data = inp.read_bytes()
    return gzip.decompress(data) if inp.name.endswith(".gz") else data


def to_bytes(x) -> bytes:
    return x if isinstance(x, bytes) else x.encode()


def test_sequence_functions_are_exported():
    import gfa2network_amd
    from gfa2network_amd import _native, api

    for name in ("sequence_distance", "sequence_nodes"):
        assert name in gfa2network_amd.__all__ and callable(getattr(gfa2network_amd, name))
        assert name in api.__all__
    lib = _native.load()
    for sym in ("g2n_seq_distance_from_path", "g2n_seq_hits_get", "g2n_seq_hits_names", "g2n_seq_hits_free"):
        assert sym in _native.EXPORTED and hasattr(lib, sym)
    assert callable(_native.seq_distance_from_path)


def test_seq_info_struct_matches_header(tmp_path):
    from gfa2network_amd import _native

    py = _native.SeqInfo
    lines = ['printf("sizeof %zu\\n", sizeof(g2n_seq_info));']
    lines += [f'printf("{f[0]} %zu\\n", offsetof(g2n_seq_info, {f[0]}));' for f in py._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "g2n.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(py)
    for f in py._fields_:
        assert int(got[f[0]]) == getattr(py, f[0]).offset, f[0]


def listed(expected, fkey):
    return {unpack(s): [unpack(n) for n in nodes] for s, nodes in expected[fkey]["seq2nodes"]}


def test_fixture_holds_every_case(expected):
    """seq_distance.json has one record for every input of the four folders (raw_bytes_id too for the
    non-ASCII files), each with a directed and an undirected run over every ordered pair of its
    queries."""
    want = [c[0] for c in cases()]
    assert len(want) == len(set(want)) and len(want) >= 180
    assert sorted(f"{k}|directed={d}" for k, rec in expected.items() for d in rec["runs"]) == sorted(want)
    names = {c[1].name for c in cases()}
    for f in FOLDERS:
        assert {p.name for p in (GOLDEN / f).iterdir()} <= names
    for key in want:
        rec, run = record_of(expected, key)
        if run["build"]["exc"] is not None:
            assert not run["pairs"] and not run["outcomes"], key
            continue
        q = [unpack(x) for x in rec["queries"]]
        assert "*" in q and "" in q and q[-1] == ABSENT and len(q) == len(set(q)), key
        assert len(run["pairs"]) == len(q) and all(len(row) == len(q) for row in run["pairs"]), key
        for i in range(len(q)):
            for j in range(len(q)):
                d, e, _w = outcome(run, i, j)
                assert (d is None) != (e is None), key
    # what the issue records of the reference's behaviour
    third = listed(expected, "seq_inputs/third_forms.gfa|raw=0")
    assert third["ACGT"] == ["i4", "ipl", "ivt"] and third["AC"] == ["isp", "iz"] and third["ACG"] == ["iu", "ibig"]
    assert third["1__0"] == ["n2u"] and third["_1"] == ["nu1"] and third["12a"] == ["n12a"] and third[""] == ["empty"]
    assert third["7" * 4301] == ["nbig"] and "ionly" not in sum(third.values(), [])
    assert listed(expected, "seq_inputs/fourth_field.gfa|raw=0") == {
        "A:i:4": ["t2"], "LN:ii:4": ["t3"], "::::": ["t4"], "ACGT": ["t5", "t6"], "AB:C": ["t7"], "": ["t9"],
        ":B:C:": ["t11"]}
    assert list(listed(expected, "seq_inputs/star_crlf.gfa|raw=0")) == ["*\r", "*", "ACGT\r", "ACGT"]
    assert listed(expected, "seq_inputs/repeat_seq.gfa|raw=0") == {"GG": ["x"], "TT": ["y", "v"], "ACGT": ["z"]}
    rec, run = record_of(expected, "seq_inputs/oriented_seq.gfa|raw=0|directed=1")
    q = [unpack(x) for x in rec["queries"]]
    d, e, w = outcome(run, q.index("AC"), q.index("*"))
    assert e == ["builtins", "KeyError", "\"sequence(s) '*' not found\""]
    assert w == ["distance functions ignore orientation; use G.to_undirected()"]
    d, e, w = outcome(run, q.index("*"), q.index(ABSENT))
    assert e[2] == "\"sequence(s) '*', b'ZZNOPE' not found\""
    assert outcome(rec["runs"]["0"], 0, 0) == [0, None, []]


def test_checker_reproduces_the_fixture(oracle_lib, expected):
    """tests/seq_util.py — the restated sequence rules, node order from the CPU oracle, scipy's
    search over the oracle's CSR — gives the reference's node lists and its result (a distance,
    KeyError or NetworkXNoPath) for every recorded case whose build is clean."""
    checked = pairs = 0
    for key, inp, raw, directed in cases():
        rec, run = record_of(expected, key)
        if run["build"]["exc"] is not None:
            continue
        data = text_of(inp)
        o = oracle_lib.run(data, directed=True, asymmetric=True, dtype="float64")
        assert o.status == 0, key
        names = seq_util.oracle_names(o)
        seqs = seq_util.node_sequences(data)
        first = [(to_bytes(unpack(s)), [to_bytes(unpack(n)) for n in nodes]) for s, nodes in rec["seq2nodes"]]
        mine = {}
        for n in names:
            if n in seqs:
                mine.setdefault(seqs[n], []).append(n)
        assert list(mine.items())[:len(first)] == first, key
        q = [to_bytes(unpack(x)) for x in rec["queries"]]
        ids = [seq_util.seq_nodes(data, names, s) for s in q]
        for i in range(len(q)):
            for j in range(len(q)):
                d, e, _w = outcome(run, i, j)
                if e is not None and e[1] == "UnicodeDecodeError":
                    continue  # (the orientation check's decode of a raw key: raised before any lookup)
                if not ids[i] or not ids[j]:
                    assert e is not None and e[1] == "KeyError", (key, i, j)
                    continue
                got = seq_util.distance(o.sum_indptr, o.sum_indices, o.n_nodes, ids[i], ids[j], directed)
                assert (got == d) if got is not None else (e is not None and e[1] == "NetworkXNoPath"), (key, i, j)
                pairs += 1
        checked += 1
    assert checked >= 140 and pairs >= 300


def test_unnamed_inputs_are_refused():
    import io

    from gfa2network_amd import sequence_distance, sequence_nodes

    for fn in (sequence_distance, sequence_nodes):
        with pytest.raises(NotImplementedError):
            fn("-", "A", "C")
        with pytest.raises(NotImplementedError):
            fn(io.BytesIO(b"S\ta\tA\n"), "A", "C")


def test_cli_points_at_the_function(capsys):
    from gfa2network_amd.cli import main

    with pytest.raises(SystemExit) as e:
        main(["distance", "x.gfa", "--seq", "A", "C"])
    assert e.value.code == 2 and "sequence_distance" in capsys.readouterr().err


@pytest.mark.skipif(__import__("gfa2network_amd._native", fromlist=["x"]).device_count() > 0,
                    reason="a GPU is visible")
def test_sequence_distance_without_gpu_fails_loudly(tmp_path):
    from gfa2network_amd import sequence_distance

    p = tmp_path / "a.gfa"
    p.write_bytes(b"S\ta\tAC\nS\tb\tGT\nL\ta\t+\tb\t+\t*\n")
    with pytest.raises(RuntimeError, match="G2N_E_DEVICE"):
        sequence_distance(p, "AC", "GT")
