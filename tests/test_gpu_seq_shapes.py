"""GPU: ``sequence_distance`` / ``sequence_nodes`` on shapes generated here, against tests/seq_util.py
(the restated sequence rules; node order and CSR from ``parse_gfa(..., asymmetric=True)``): the load,
wave, block, tile and grid-stride boundaries of the line scan, the query lengths around the 16 bytes
the per-record pass compares itself, the gzip routes, the four name tiers and repeated names at
scale."""
import gzip
import struct
import zlib

import numpy as np
import pytest

import seq_util

pytestmark = pytest.mark.gpu

TILE = 32 * 1024
STRIDE = 256 * 8 * 256 * 16  # the scan's grid stride on 256 CUs: 8 blocks a CU, 256 lanes, 16 bytes each


def graph_of(path):
    """(names as bytes in node order, indptr, indices) of the directed asymmetric build."""
    from gfa2network_amd import convert_format, parse_gfa

    A, nodes = parse_gfa(path, build_graph=False, build_matrix=True, asymmetric=True, return_node_list=True)
    A = convert_format(A, "csr")
    return [n.encode() for n in nodes], A.indptr.astype(np.int64), A.indices.astype(np.int64)


def want_nodes(data, names, seq):
    return [names[i].decode() for i in seq_util.seq_nodes(data, names, seq)]


def check(path, data, pairs, directed=True):
    """sequence_nodes and sequence_distance of every (a, b) in pairs against seq_util."""
    from gfa2network_amd import sequence_distance, sequence_nodes
    from gfa2network_amd.api import NetworkXNoPath

    names, indptr, indices = graph_of(path)
    for a, b in pairs:
        ia, ib = seq_util.seq_nodes(data, names, a), seq_util.seq_nodes(data, names, b)
        if not ia or not ib:
            with pytest.raises(KeyError):
                sequence_nodes(path, a, b, directed=directed)
            continue
        got = sequence_nodes(path, a, b, directed=directed)
        assert got == ([names[i].decode() for i in ia], [names[i].decode() for i in ib]), (a[:20], b[:20])
        want = seq_util.distance(indptr, indices, len(names), ia, ib, directed)
        if want is None:
            with pytest.raises(NetworkXNoPath):
                sequence_distance(path, a, b, directed=directed)
        else:
            d = sequence_distance(path, a, b, directed=directed)
            assert d == want and type(d) is int, (a[:20], b[:20])


def pad_to(buf: bytearray, pos: int) -> None:
    """H lines (skipped silently) up to exactly pos bytes."""
    gap = pos - len(buf)
    assert gap == 0 or gap >= 2, gap
    while gap:
        take = min(gap, 1000)
        if gap - take == 1:
            take -= 1
        buf += b"H" + b"x" * (take - 2) + b"\n"
        gap -= take


@pytest.mark.parametrize("d", range(10))
def test_scan_boundaries(gpu, tmp_path, d):
    """Byte d of "\\nS\\tnm\\tACGT" (the newline before the line, 'S', the tab, the name, the tab, the
    sequence) is the last byte before a boundary and byte d + 1 the first after it, for a 16-byte
    load, a wave (1 KiB), a block (4 KiB), a tile (32 KiB) and the grid stride (8 MiB on 256 CUs)."""
    from gfa2network_amd import sequence_distance

    bounds = {"ld": 5 * TILE + 16 * 5, "wv": 9 * TILE + 1024 * 3, "bk": 13 * TILE + 4096 * 3, "tl": 17 * TILE,
              "gs": STRIDE}
    seqs = {"ld": b"ACGT", "wv": b"ACGA", "bk": b"ACGT", "tl": b"ACGC", "gs": b"ACGT"}
    buf = bytearray(b"S\tfirst\tACGT\n")  # S as the very first line
    for nm, B in bounds.items():
        pad_to(buf, B - d)  # the newline that ends the padding is byte 0 of the text, at B - 1 - d
        assert buf[-1:] == b"\n"
        buf += b"S\t" + nm.encode() + b"\t" + seqs[nm] + b"\n"
        assert bytes(buf[B - 1 - d:B - 1 - d + 10]) == b"\nS\t" + nm.encode() + b"\t" + seqs[nm]
    pad_to(buf, len(buf) + 5000)
    buf += b"L\tfirst\t+\tld\t+\t*\nL\tld\t+\twv\t+\t*\nL\twv\t+\tbk\t+\t*\nL\tbk\t+\ttl\t+\t*\nL\ttl\t+\tgs\t+\t*\n"
    buf += b"S\tlast\tACGC"  # no newline: the sequence ends at the end of the file
    data = bytes(buf)
    p = tmp_path / "b.gfa"
    p.write_bytes(data)
    check(p, data, [(b"ACGT", b"ACGA"), (b"ACGA", b"ACGC"), (b"ACGC", b"ACGT"), (b"ACG", b"ACGT")])
    _d, info = sequence_distance(p, b"ACGT", b"ACGC", return_info=True)
    assert (info["n_s_lines"], info["n_with_seq"], info["candidates_a"], info["candidates_b"]) == (7, 7, 4, 2)


@pytest.mark.parametrize("m", [0, 1, 15, 16, 17, 255, 256, 257, 70_000])
def test_query_lengths(gpu, tmp_path, m):
    """A query of m bytes against: the exact sequence (followed by a newline, and by a tag), one that
    differs only in the last byte, one that is a byte longer, one a byte shorter, and the exact one
    again as the file's last line without a newline."""
    from gfa2network_amd import sequence_distance

    rng = np.random.default_rng(m)
    q = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), m))
    other = (q[:-1] + (b"N" if q[-1:] != b"N" else b"M")) if m else b"N"
    lines = [b"S\texact\t" + q, b"S\ttagged\t" + q + b"\tLN:i:%d" % m, b"S\tdiff\t" + other, b"S\tlonger\t" + q + b"A",
             b"S\tshorter\t" + q[:-1], b"S\tlen\t%d\t" % m + q,
             b"L\texact\t+\tdiff\t+\t*", b"L\tdiff\t+\tlonger\t+\t*", b"L\tlonger\t+\tshorter\t+\t*",
             b"L\tshorter\t+\teof\t+\t*", b"L\teof\t+\ttagged\t+\t*", b"L\ttagged\t+\tlen\t+\t*", b"S\teof\t" + q]
    data = b"\n".join(lines)
    p = tmp_path / "q.gfa"
    p.write_bytes(data)
    names, _ip, _ix = graph_of(p)
    assert want_nodes(data, names, q) == (["exact", "tagged", "len", "eof"] if m else
                                          ["exact", "tagged", "shorter", "len", "eof"])
    check(p, data, [(q, other), (q + b"A", q), (q, q[:-1]), (other, q + b"A"), (q + b"AA", q)])
    check(p, data, [(q, other), (other, q)], directed=False)
    _d, info = sequence_distance(p, q, q + b"A", return_info=True)
    assert info["n_s_lines"] == 7 and info["n_with_seq"] == 7
    # A terminator at the right place and the first 16 bytes make a candidate: up to 16 bytes these
    # are the matches; past them `diff` is one too, and so may be a field that ends earlier (the
    # comparison of the remaining bytes then meets its newline)
    n_a = 5 if m == 0 else 4
    if m <= 15:
        assert (info["candidates_a"], info["candidates_b"]) == (n_a, 1)
    else:
        assert info["candidates_a"] >= n_a + (m > 16) and info["candidates_b"] >= 1
        assert info["candidates_a"] <= 7 and info["candidates_b"] <= 7


def test_query_longer_than_the_file(gpu, tmp_path):
    from gfa2network_amd import sequence_nodes

    data = b"S\ta\tACGT\nS\tb\tAC\nL\ta\t+\tb\t+\t*\n"
    p = tmp_path / "s.gfa"
    p.write_bytes(data)
    for a in (b"ACGT" * 20, b"A" * 100_000):
        with pytest.raises(KeyError) as e:
            sequence_nodes(p, a, "AC")
        assert e.value.args == (f"sequence(s) {a!r} not found",)
    assert sequence_nodes(p, "ACGT", "AC") == (["a"], ["b"])


def bgzf(data: bytes, block: int = 65280) -> bytes:
    """htslib's bgzip layout: members of at most 64 KiB of output with the 'BC' extra subfield, then
    the 28-byte EOF marker member."""
    out = bytearray()
    for i in range(0, len(data), block):
        chunk = data[i:i + block]
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, 0)
        cdata = co.compress(chunk) + co.flush()
        hdr = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H", 6) + b"BC" + struct.pack(
            "<HH", 2, 12 + 6 + len(cdata) + 8 - 1)
        out += hdr + cdata + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk))
    out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    return bytes(out)


def test_gzip_routes(gpu, tmp_path):
    """The same text as a plain file, one gzip member, several members and BGZF (inflated on the
    GPU): the staged bytes are the same, so are the answers."""
    from gfa2network_amd import sequence_distance, sequence_nodes, synth

    data = synth.host_bytes(3000, 6000, seed=7, names="hashed")
    files = {"plain.gfa": data, "one.gfa.gz": gzip.compress(data, 6, mtime=0),
             "many.gfa.gz": b"".join(gzip.compress(data[i:i + 50_000], 1, mtime=0) for i in range(0, len(data), 50_000)),
             "bgzf.gfa.gz": bgzf(data)}
    got = {}
    for name, blob in files.items():
        p = tmp_path / name
        p.write_bytes(blob)
        d, info = sequence_distance(p, "A", "AC", return_info=True)
        got[name] = (d, sequence_nodes(p, "A", "AC"), info["n_s_lines"], info["n_with_seq"], info["candidates_a"],
                     info["candidates_b"])
    assert got["plain.gfa"][2] == 3000 and len(got["plain.gfa"][1][0]) > 50
    assert all(v == got["plain.gfa"] for v in got.values()), {k: v[0] for k, v in got.items()}
    check(tmp_path / "plain.gfa", data, [(b"A", b"AC")])


FLAGS = {"decimal": ("TEST_NO_LEAN", "TEST_NO_TILE_LOCAL"), "hashed": ("TEST_NO_HASH_LEAN", "TEST_DICT_GENERAL"),
         "permuted": ("TEST_DICT_HASH",), "prefixed": ("TEST_NO_LEAN",)}


@pytest.mark.parametrize("names", ["decimal", "hashed", "permuted", "prefixed"])
def test_name_tiers(gpu, tmp_path, monkeypatch, names):
    """20 000 segments / 30 000 links in each name layout (the names blob is rendered from ids in
    some, gathered from the text in others), and again through the builds' rarer parse paths: the
    S-line count the list is sized by is the same whichever pass counted it."""
    from gfa2network_amd import _native as nat
    from gfa2network_amd import sequence_distance, synth

    p = tmp_path / f"{names}.gfa"
    synth.write_file(p, 20_000, 30_000, seed=5, names=names)
    data = p.read_bytes()
    pairs = [(b"A", b"AC"), (b"AC", b"ACGT"), (b"ACGT", b"A")]
    check(p, data, pairs)
    check(p, data, pairs[:2], directed=False)
    d, info = sequence_distance(p, "A", "ACGT", return_info=True)
    assert info["n_s_lines"] == 20_000 and info["n_with_seq"] == 20_000
    assert info["candidates_a"] >= 500 and info["candidates_b"] >= 1
    for flag in FLAGS[names]:
        monkeypatch.setattr(nat, "TEST_FLAGS", getattr(nat, flag))
        try:
            d2, info2 = sequence_distance(p, "A", "ACGT", return_info=True)
        finally:
            monkeypatch.setattr(nat, "TEST_FLAGS", 0)
        assert d2 == d and info2["n_s_lines"] == 20_000, flag
        assert (info2["candidates_a"], info2["candidates_b"]) == (info["candidates_a"], info["candidates_b"]), flag


def test_repeated_names_at_scale(gpu, tmp_path):
    """50 000 S lines over 10 000 names, sequences of length 0-6 over three letters, a third of the
    lines with an integer third field (then a sequence, a tag or nothing): the last record that has
    a sequence wins, whichever lane saw it."""
    from gfa2network_amd import sequence_nodes

    rng = np.random.default_rng(11)
    letters = np.frombuffer(b"ACG", dtype=np.uint8)
    lines = []
    for _ in range(50_000):
        name = b"n%d" % int(rng.integers(0, 10_000))
        seq = bytes(rng.choice(letters, int(rng.integers(0, 7))))
        kind = int(rng.integers(0, 9))
        if kind == 0:
            lines.append(b"S\t" + name + b"\t%d\t" % len(seq) + seq)
        elif kind == 1:
            lines.append(b"S\t" + name + b"\t%d\tLN:i:%d" % (len(seq), len(seq)))
        elif kind == 2:
            lines.append(b"S\t" + name + b"\t%d" % len(seq))
        else:
            lines.append(b"S\t" + name + b"\t" + seq)
    lines += [b"L\tn%d\t+\tn%d\t+\t*" % (int(a), int(b)) for a, b in rng.integers(0, 10_000, (5000, 2))]
    data = b"\n".join(lines) + b"\n"
    p = tmp_path / "rep.gfa"
    p.write_bytes(data)
    names, _ip, _ix = graph_of(p)
    queries = [b"", b"A", b"C", b"AC", b"GA", b"ACG", b"GGG", b"ACGA", b"CCCCC", b"ACGACG", b"GGGGGG", b"AAAAAA"]
    for a, b in zip(queries, queries[1:] + queries[:1]):
        wa, wb = want_nodes(data, names, a), want_nodes(data, names, b)
        if wa and wb:
            assert sequence_nodes(p, a, b) == (wa, wb), (a, b)
        else:
            with pytest.raises(KeyError):
                sequence_nodes(p, a, b)
    assert len(want_nodes(data, names, b"A")) > 100
