"""Cases for the edge-list export renders at their block and digit thresholds — TEST INFRASTRUCTURE, CPU only.

export --format edge-list is rendered on the GPU by two paths (g2n_kernels.hip, run_edge_list in g2n_pipeline.hip):

* the blob render (k_name_meta, k_edge_text_len, k_edge_text) for named graphs: a block takes kTextEdges edges,
  stages their text in LDS when it fits (p1 - base <= kTextLds) and writes it line by line otherwise; a key's length
  travels in 23 bits of `meta` and 24 bits of `em`, saturated lengths are read from the offsets; the first edge
  with an undecodable key wins an atomicMin;
* the arithmetic render (k_edge_dec_sum, k_edge_dec_text, decfmt.h) when node k is named str(k + 1): every line
  from its two ids, kDecPer consecutive edges a thread, the blocks' sums scanned in tiles of kScanTile.

tests/test_gpu_edge_text_edges.py drives both with the inputs built here; tests/test_edge_text_cases.py shows on
the CPU that every input sits on the threshold its name says.  This module restates, in plain Python:

* the geometry (constants read from g2n_kernels.hip / g2n_scan.hip, restated, not imported) and block_plan();
* model(): the reference of the restricted grammar the cases use (H, S and L lines only) — for each L line in
  stream order the bytes f[1] TAB f[3] NEWLINE (bidirected: f[1]:f[2] TAB f[3]:f[4] NEWLINE); a malformed line:
  the lines before it and the status; a key that is not strict UTF-8 (Python's own bytes.decode(), u before v):
  the lines before the first such edge.  The export does not depend on the S lines, so the model never reads
  them, and a case whose S section is too large for the host (HEAD_DEVICE) needs no copy of it.

A case is a head (its S section: explicit lines, or "S 1 .. N" to be generated) and its L lines, with claims —
(what, bidirected or None for both, block, value) — that the CPU test recomputes from the bytes.  Everything up to
ORACLE_MAX_BYTES is also checked against oracle_lib.export_edge_list on the CPU; after that the GPU tests compare
with the model only.
"""
from __future__ import annotations

import functools
from collections import namedtuple

# ------------------------------------------------------------------ geometry ------
K_TPB = 256             # kTPB: threads per block of every kernel here
K_TEXT_EDGES = 1024     # kTextEdges: edges per block of k_edge_text / k_edge_dec_sum / k_edge_dec_text
K_TEXT_LDS = 32768      # kTextLds: bytes of a block's LDS stage
K_DEC_PER = 4           # kDecPer: consecutive edges per thread of the arithmetic render
K_META_LEN = 0x7FFFFF   # kMetaLen: a key length of this or more is saturated in `meta` (read from the offsets)
K_EM_LEN = 0xFFFFFF     # ... and of this or more in `em`
K_SCAN_TILE = 4096      # kScanTile: items per tile of the block-sum scan
DEC_LINE_MAX = 26       # two 10-digit keys, ":o" twice, tab and newline (the static_assert's bound)
assert K_DEC_PER == K_TEXT_EDGES // K_TPB and K_TEXT_EDGES * DEC_LINE_MAX + 16 <= K_TEXT_LDS

E_MALFORMED_L, E_UNICODE = 1, 8  # include/g2n.h G2N_E_MALFORMED_L, G2N_E_UNICODE

# Above this many input bytes a case is "multi-megabyte": the CPU test checks its claims against the model but
# not the model against the oracle (the oracle's Python loop over millions of edges), and data_of() refuses to
# materialise an S section past HEAD_PY_MAX segments in Python (the GPU tests generate those natively).
ORACLE_MAX_BYTES = 4 << 20
HEAD_PY_MAX = 200_000
HEAD_DEVICE = 50_000_000  # from this many segments the S section exists in HBM only

Case = namedtuple("Case", "name family head lines claims dec note")
Expected = namedtuple("Expected", "text status err_line err_index err_detail")


# ------------------------------------------------------------------ lines ------
def S(name) -> bytes:
    return b"S\t" + (name if isinstance(name, bytes) else b"%d" % name) + b"\t*\n"


def L(u, ou: str, v, ov: str) -> bytes:
    u = u if isinstance(u, bytes) else b"%d" % u
    v = v if isinstance(v, bytes) else b"%d" % v
    return b"L\t" + u + b"\t" + ou.encode() + b"\t" + v + b"\t" + ov.encode() + b"\t0M\n"


def key(i: int, n: int) -> bytes:
    """A name of n >= 1 bytes that is no decimal (it starts with 'k'); its content follows i."""
    s = b"k%x." % i
    return (s * (n // len(s) + 1))[:n]


def ori(j: int) -> tuple:
    return "+-"[j & 1], "+-"[(j >> 1) & 1]


def edges_of_lengths(lengths, bidir: bool, i0: int = 0, loops: bool = False) -> list:
    """L lines whose rendered lines (in mode `bidir`) have the given lengths; the split between u and v varies.
    loops: every third line whose keys can be equal is a self-loop (u == v, same orientation)."""
    out = []
    for j, n in enumerate(lengths):
        kt = n - 2 - (4 if bidir else 0)
        assert kt >= 2, (n, bidir)
        if loops and j % 3 == 0 and kt % 2 == 0:
            k = key(i0 + j, kt // 2)
            out.append(L(k, "+", k, "+"))
            continue
        ul = min(max(kt * (1 + j % 3) // 4, 1), kt - 1)
        out.append(L(key(i0 + j, ul), ori(j)[0], key(i0 + j + 7, kt - ul), ori(j)[1]))
    return out


def spread(total: int, count: int) -> list:
    """`count` lengths that add up to `total`, as even as they come."""
    base, extra = divmod(total, count)
    return [base + (1 if j < extra else 0) for j in range(count)]


def head_lines(c: Case) -> tuple:
    """The case's S section as lines (explicit, or S 1 .. N for N <= HEAD_PY_MAX)."""
    if c.head[0] == "lines":
        return c.head[1]
    assert c.head[0] == "decimal" and c.head[1] <= HEAD_PY_MAX, c.head
    return tuple(S(k) for k in range(1, c.head[1] + 1))


def n_head_lines(c: Case) -> int:
    return len(c.head[1]) if c.head[0] == "lines" else c.head[1]


def input_bytes(c: Case) -> int:
    """The input's size (a generated S section estimated at its shortest, 6 bytes a line)."""
    head = sum(len(x) for x in c.head[1]) if c.head[0] == "lines" else 6 * c.head[1]
    return head + sum(map(len, c.lines))


def data_of(c: Case) -> bytes:
    return b"".join(head_lines(c)) + b"".join(c.lines)


# ------------------------------------------------------------------ the model ------
def _bad(k: bytes) -> bool:
    try:
        k.decode()
        return False
    except UnicodeDecodeError:
        return True


def render(lines, bidirected: bool = False):
    """([one rendered line per L line before the first malformed one], [(edge, key) of the edges with an
    undecodable key: the key decoded first, u before v], the index in `lines` of the malformed line or -1)."""
    out, bad, cache = [], [], {}
    for i, x in enumerate(lines):
        if x[:1] != b"L":
            assert x[:1] in (b"H", b"S"), "the restricted grammar"
            continue
        r = cache.get(x)
        if r is None:
            f = (x[:-1] if x[-1:] == b"\n" else x).split(b"\t")
            if len(f) < 5:
                return out, bad, i
            u, v = (f[1] + b":" + f[2], f[3] + b":" + f[4]) if bidirected else (f[1], f[3])
            r = cache[x] = (u + b"\t" + v + b"\n", u if _bad(u) else v if _bad(v) else None)
        if r[1] is not None:
            bad.append((len(out), r[1]))
        out.append(r[0])
    return out, bad, -1


def model(lines, bidirected: bool = False, line0: int = 0) -> Expected:
    """What the export writes and how it ends.  `lines`: the input's lines from line `line0` on (the lines before
    hold no L line).  Status 0; or E_MALFORMED_L with err_line; or — first, when such an edge lies before the
    malformed line — E_UNICODE with err_index = the edge, err_detail = the key, the text cut before that edge."""
    out, bad, mal = render(lines, bidirected)
    if bad:
        e, k = bad[0]
        return Expected(b"".join(out[:e]), E_UNICODE, -1, e, k)
    if mal >= 0:
        return Expected(b"".join(out), E_MALFORMED_L, line0 + mal, -1, b"")
    return Expected(b"".join(out), 0, -1, -1, b"")


def block_plan(line_lengths) -> list:
    """[(p0, p1, base, staged)] of every block of kTextEdges lines: its text range, base = p0 & ~15 (the aligned
    start its LDS stage is laid out from), staged = p1 - base <= kTextLds."""
    pos = [0]
    for n in line_lengths:
        pos.append(pos[-1] + n)
    out = []
    for e0 in range(0, len(line_lengths), K_TEXT_EDGES):
        p0, p1 = pos[e0], pos[min(e0 + K_TEXT_EDGES, len(line_lengths))]
        out.append((p0, p1, p0 & ~15, p1 - (p0 & ~15) <= K_TEXT_LDS))
    return out


def plan_of(lines, bidirected: bool) -> list:
    return block_plan([len(x) for x in render(lines, bidirected)[0]])


def digits_of(lines) -> set:
    """The digit counts of every decimal key an L line names."""
    out = set()
    for x in set(lines):
        f = x.split(b"\t")
        if x[:1] == b"L" and len(f) >= 5:
            out |= {len(f[1]), len(f[3])}
    return out


def slots_of(lines, value: int) -> tuple:
    """(the thread slots — edge index mod kDecPer — in which `value` is an edge's u, ... its v)."""
    k, su, sv, want = 0, set(), set(), b"%d" % value
    for x in lines:
        if x[:1] != b"L":
            continue
        f = x.split(b"\t")
        if f[1] == want:
            su.add(k % K_DEC_PER)
        if f[3] == want:
            sv.add(k % K_DEC_PER)
        k += 1
    return tuple(sorted(su)), tuple(sorted(sv))


# ------------------------------------------------------------------ case builder ------
class Builder:
    def __init__(self, head=()):
        self.head, self.lines, self.claims = ("lines", tuple(head)), [], []

    def decimal(self, n: int):
        self.head = ("decimal", n)
        return self

    def add(self, *lines):
        self.lines += lines
        return self

    def claim(self, what: str, bidir, block, value):
        self.claims.append((what, bidir, block, value))
        return self

    def case(self, name: str, family: str, dec: bool, note: str = "") -> Case:
        return Case(name, family, self.head, tuple(self.lines), tuple(self.claims), dec, note)


NAMED_HEAD = (S(b"n0"), S(b"n1"), S(b"k"))  # S lines that are no decimal run: the blob render
MODES = (False, True)
TAG = {False: "plain", True: "bidirected"}


def named_edges(n: int, i0: int = 0) -> list:
    """n edges over the names n0 .. n999 (2 - 4 byte keys), orientations varying."""
    return [L(b"n%d" % ((i0 + j) * 7 % 1000), ori(j)[0], b"n%d" % ((i0 + j) * 13 % 1000), ori(j)[1]) for j in range(n)]


# ------------------------------------------------------------------ A. the blob render ------
A1_COUNTS = (0, 1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)


def _family_a1():
    for n in A1_COUNTS:
        b = Builder(NAMED_HEAD).add(*named_edges(n))
        b.claim("n_edges", None, None, n).claim("blocks", None, None, (n + K_TEXT_EDGES - 1) // K_TEXT_EDGES)
        yield b.case(f"A1_{n}_edges", "A1", False)
    for bidir in MODES:  # a last block of one edge: its 4-byte line (bidirected: 8) inside the word block 0 mostly owns
        first = 11 if not bidir else 7
        b = Builder(NAMED_HEAD)
        b.add(*edges_of_lengths([16] * (K_TEXT_EDGES - 1) + [16 + first], bidir))
        b.add(L(b"k", "+", b"j", "-"))
        b.claim("n_edges", None, None, K_TEXT_EDGES + 1).claim("p0_mod16", bidir, 1, first)
        b.claim("text_len", bidir, 1, 8 if bidir else 4).claim("p1_mod16", bidir, 1, 15)
        yield b.case(f"A1_last_block_of_one_edge_inside_its_neighbours_word_{TAG[bidir]}", "A1", False)


def _family_a2():
    for bidir in MODES:
        for total in (K_TEXT_LDS - 1, K_TEXT_LDS, K_TEXT_LDS + 1):  # block 0: p0 = 0, 1024 lines of 32 bytes +- 1
            b = Builder(NAMED_HEAD)
            b.add(*edges_of_lengths(spread(total, K_TEXT_EDGES), bidir))
            b.add(*named_edges(10))
            b.claim("text_len", bidir, 0, total).claim("span", bidir, 0, total)
            b.claim("staged", bidir, 0, total <= K_TEXT_LDS).claim("staged", bidir, 1, True)
            yield b.case(f"A2_block_0_text_of_{total}_bytes_{TAG[bidir]}", "A2", False)
        for r in (0, 1, 15):  # block 1: p0 & 15 = r, p1 - base = len + r on and one past the stage
            for span in (K_TEXT_LDS, K_TEXT_LDS + 1):
                b = Builder(NAMED_HEAD)
                b.add(*edges_of_lengths([16] * (K_TEXT_EDGES - 1) + [16 + r], bidir))
                b.add(*edges_of_lengths(spread(span - r, K_TEXT_EDGES), bidir, i0=5000))
                b.add(*named_edges(10))
                b.claim("p0_mod16", bidir, 1, r).claim("span", bidir, 1, span).claim("text_len", bidir, 1, span - r)
                b.claim("staged", bidir, 0, True).claim("staged", bidir, 1, span <= K_TEXT_LDS)
                b.claim("staged", bidir, 2, True)
                yield b.case(f"A2_block_1_at_phase_{r}_span_{span}_{TAG[bidir]}", "A2", False)


A3_BIG = 40 * 1024  # the one key longer than the whole stage


def _family_a3():
    for bidir in MODES:
        e = 4 if bidir else 0
        b = Builder(NAMED_HEAD)
        b.add(*edges_of_lengths(spread(K_TEXT_EDGES * (8 + e) + 1, K_TEXT_EDGES), bidir))             # staged, ends at 1
        b.add(*edges_of_lengths(spread(K_TEXT_EDGES * 40 + 7, K_TEXT_EDGES), bidir, i0=2000))         # medium names: 8
        b.add(*edges_of_lengths(spread(K_TEXT_EDGES * (10 + e) + 7, K_TEXT_EDGES), bidir, i0=4000, loops=True))  # 15
        # 1023 lines of 1-byte keys (a self-loop among them) and one line whose u is longer than the stage: ends at 1
        small, big_at = 4 + e, 500
        rest = (K_TEXT_EDGES - 1) * small + 2 + e + 1  # all of block 3 but the long key
        big = A3_BIG + (2 - (rest + A3_BIG)) % 16
        blk = [L(b"k", ori(j)[0], b"j", ori(j)[1]) for j in range(K_TEXT_EDGES - 1)]
        blk[7] = L(b"k", "-", b"k", "-")
        blk.insert(big_at, L(key(77, big), "+", b"j", "-"))
        b.add(*blk)
        b.add(*named_edges(10))
        for blk_i, (st, end) in enumerate(((True, 1), (False, 8), (True, 15), (False, 1), (True, None))):
            b.claim("staged", bidir, blk_i, st)
            if end is not None:
                b.claim("p1_mod16", bidir, blk_i, end)
        b.claim("longest_line", bidir, 3, big + 1 + 1 + e + 1).claim("self_loops", None, None, True)
        yield b.case(f"A3_staged_unstaged_staged_unstaged_{TAG[bidir]}", "A3", False)


A4_LENGTHS = (K_META_LEN - 1, K_META_LEN, K_META_LEN + 1, K_EM_LEN - 1, K_EM_LEN, K_EM_LEN + 1)


A4_NAME = "A4_keys_around_the_23_and_24_bit_length_saturation"


def _a4():
    b = Builder(NAMED_HEAD)
    b.add(*named_edges(5))
    for j, n in enumerate(A4_LENGTHS):
        k = key(100 + j, n)
        b.add(L(b"n%d" % j, "+", k, "-"), *named_edges(3, i0=10 * j), L(k, "-", b"k", "+"), L(b"k", "+", b"j", "+"))
    b.claim("long_keys", False, None, tuple(A4_LENGTHS))
    yield b.case(A4_NAME, "A4", False, "big")


BAD1, BAD2, BAD3 = b"b\xffd", b"\xc3(", b"\xed\xa0\x80z"  # no start byte; a broken pair; a surrogate


def _with_bad(n: int, where: dict) -> list:
    """named_edges(n) with the key of some edges replaced: where[edge] = (side, key)."""
    out = named_edges(n)
    for e, (side, k) in where.items():
        f = out[e].split(b"\t")
        f[1 if side == "u" else 3] = k
        out[e] = b"\t".join(f)
    return out


def _family_a5():
    n = 2500
    for e in (0, 1023, 1024, n - 1):
        b = Builder(NAMED_HEAD).add(*_with_bad(n, {e: ("u" if e & 1 else "v", BAD1)}))
        b.claim("first_bad", None, None, (e, BAD1))
        yield b.case(f"A5_first_bad_edge_at_{e}_of_{n}", "A5", False)
    b = Builder(NAMED_HEAD).add(*_with_bad(n, {100: ("v", BAD2), 1500: ("u", BAD2)}))
    b.claim("first_bad", None, None, (100, BAD2)).claim("bad_edges", None, None, (100, 1500))
    yield b.case("A5_bad_key_first_as_v_later_as_u", "A5", False)
    b = Builder(NAMED_HEAD).add(*_with_bad(n, {2100: ("u", BAD3), 1500: ("v", BAD2), 700: ("v", BAD1)}))
    b.claim("first_bad", None, None, (700, BAD1)).claim("bad_edges", None, None, (700, 1500, 2100))
    yield b.case("A5_different_bad_keys_in_three_blocks_the_earliest_wins", "A5", False)
    b = Builder(NAMED_HEAD).add(*_with_bad(n, {1023: ("u", BAD3), 1024: ("u", BAD1)}))
    b.claim("first_bad", None, None, (1023, BAD3)).claim("bad_edges", None, None, (1023, 1024))
    yield b.case("A5_bad_keys_on_both_sides_of_a_block_boundary", "A5", False)
    for bidir in MODES:
        b = Builder(NAMED_HEAD).add(*named_edges(K_TEXT_EDGES))
        blk = edges_of_lengths(spread(K_TEXT_EDGES * 40, K_TEXT_EDGES), bidir, i0=3000)
        f = blk[300].split(b"\t")
        f[3] = BAD1 + f[3][len(BAD1):]
        blk[300] = b"\t".join(f)
        b.add(*blk).add(*named_edges(10))
        b.claim("first_bad", None, None, (K_TEXT_EDGES + 300, None)).claim("staged", bidir, 1, False)
        yield b.case(f"A5_bad_key_inside_an_unstaged_block_{TAG[bidir]}", "A5", False)


SHORT_L = b"L\tn1\t+\n"


def _family_a6():
    for g in (0, 1023, 1024, 1025):
        b = Builder(NAMED_HEAD).add(*named_edges(g)).add(SHORT_L).add(*named_edges(50, i0=g))
        b.claim("malformed_after", None, None, g)
        yield b.case(f"A6_short_L_line_after_{g}_good_edges", "A6", False)
    b = Builder(NAMED_HEAD).add(*_with_bad(1025, {10: ("u", BAD1)})).add(SHORT_L).add(*named_edges(50))
    b.claim("malformed_after", None, None, 1025).claim("first_bad", None, None, (10, BAD1))
    yield b.case("A6_bad_key_before_the_short_L_line_the_unicode_failure_wins", "A6", False)
    b = Builder(NAMED_HEAD).add(*named_edges(1025)).add(SHORT_L).add(*_with_bad(50, {3: ("v", BAD1)}))
    b.claim("malformed_after", None, None, 1025).claim("bad_edges", None, None, ())
    yield b.case("A6_bad_key_after_the_short_L_line_the_malformed_line_wins", "A6", False)


# ------------------------------------------------------------------ B. the arithmetic render ------
B1_COUNTS = (0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 1027, 2049, 2050, 2051)
B1_N = 50
B1_BIG = K_SCAN_TILE * K_TEXT_EDGES + 5
B1_BIG_NAME = f"B1_{B1_BIG}_edges_two_scan_tiles"


def dec_edges(n: int, n_seg: int, i0: int = 0) -> list:
    return [L(1 + (i0 + j) * 7 % n_seg, ori(j)[0], 1 + ((i0 + j) * 11 + 3) % n_seg, ori(j)[1]) for j in range(n)]


def _family_b1():
    for n in B1_COUNTS:
        b = Builder().decimal(B1_N).add(*dec_edges(n, B1_N))
        b.claim("n_edges", None, None, n).claim("tail", None, None, n % K_DEC_PER)
        yield b.case(f"B1_{n}_edges", "B1", True)


def _b1_big():
    blk = dec_edges(K_TEXT_EDGES, B1_N)
    b = Builder().decimal(B1_N).add(*(blk * K_SCAN_TILE)).add(*dec_edges(5, B1_N, i0=9))
    b.claim("n_edges", None, None, B1_BIG).claim("scan_items", None, None, K_SCAN_TILE + 2)
    yield b.case(B1_BIG_NAME, "B1", True, "big")


def _family_b1_prefix():
    for g in (1023, 1024, 1025):  # the malformed-line prefix, cut on and beside a block boundary
        b = Builder().decimal(B1_N).add(*dec_edges(g, B1_N)).add(b"L\t1\t+\n").add(*dec_edges(50, B1_N, i0=g))
        b.claim("malformed_after", None, None, g)
        yield b.case(f"B1_short_L_line_after_{g}_good_edges", "B1", True)


B2_N = 10 ** 5 + 2
B2_MUL = 7919  # coprime to B2_N = 2 * 3 * 7 * 2381: i -> (i * B2_MUL + 13) mod N is a permutation


def _family_b2():
    b = Builder().decimal(B2_N)
    b.add(*[L(i + 1, ori(i)[0], (i * B2_MUL + 13) % B2_N + 1, ori(i)[1]) for i in range(B2_N)])
    b.claim("n_edges", None, None, B2_N).claim("every_value_as_u_and_v", None, None, B2_N)
    b.claim("digits", None, None, (1, 2, 3, 4, 5, 6))
    yield b.case("B2_every_value_to_5_digits_as_u_and_as_v", "B2", True)


def in_every_slot(values, other: int) -> list:
    """Edges in which every value is u and v in each of the kDecPer thread slots: the pairs (x, next x) four
    times, each copy shifted one slot by a filler edge (the pair count is padded to a multiple of kDecPer)."""
    vs = list(values)
    pairs = [L(vs[i], ori(i)[0], vs[(i + 1) % len(vs)], ori(i)[1]) for i in range(len(vs))]
    pairs += [L(other, "+", other, "-")] * (-len(pairs) % K_DEC_PER)
    out = []
    for _ in range(K_DEC_PER):
        out += pairs + [L(other, "-", other, "+")]
    return out


B3_N = 10 ** 7 + 2


def b3_values() -> list:
    vs = [10 ** k + d for k in range(1, 8) for d in (-1, 0, 1)]
    vs += [a * 10 ** 4 + (37 * a) % 10 ** 4 for a in range(0, 1001)]
    vs += [2 ** j + d for j in range(1, 24) for d in (-1, 0)]
    return [v for v in dict.fromkeys(vs) if 1 <= v <= B3_N]


def _family_b3():
    b = Builder().decimal(B3_N).add(*in_every_slot(b3_values(), 5))
    b.claim("slots", None, None, tuple(10 ** k + d for k in range(1, 8) for d in (-1, 0, 1)))
    b.claim("digits", None, None, (1, 2, 3, 4, 5, 6, 7, 8)).claim("high_halves", None, None, 1001)
    yield b.case("B3_boundaries_to_8_digits", "B3", True, "big")


def _padded_block(b: Builder, block: list, phase: int = 15):
    """Append filler edges up to a block boundary such that the bidirected text before `block` ends at `phase`
    mod 16, then `block` (kTextEdges lines)."""
    assert len(block) == K_TEXT_EDGES
    n = sum(1 for x in b.lines if x[:1] == b"L")
    fill = -n % K_TEXT_EDGES
    if fill < 16:
        fill += K_TEXT_EDGES
    at = sum(len(x) for x in render(b.lines, True)[0])
    short, long_ = L(1, "+", 1, "-"), L(1, "+", 10, "-")  # 8 and 9 bytes bidirected
    need = (phase - at - 8 * fill) % 16
    b.add(*([long_] * need + [short] * (fill - need)))
    blk = sum(1 for x in b.lines if x[:1] == b"L") // K_TEXT_EDGES
    b.add(*block)
    return blk


def _family_b45():
    # B4: 9 digits.  N = 10^8 + 64; the S section is generated in HBM
    n4 = 10 ** 8 + 64
    b = Builder().decimal(n4)
    edge = [10 ** 8 - 1, 10 ** 8, 10 ** 8 + 1]
    b.add(*in_every_slot(edge + [n4, 99, 999, 1000, 12345678], 10 ** 8 + 2))
    b.add(*[L(max(1, a * 10 ** 4 + (37 * a) % 10 ** 4), ori(a)[0], 10 ** 8 + (a % 64), ori(a)[1]) for a in range(10 ** 4)])
    blk = _padded_block(b, [L(10 ** 8 + j % 64, ori(j)[0], n4 - j % 61, ori(j)[1]) for j in range(K_TEXT_EDGES)])
    b.add(*dec_edges(7, 1000))
    b.claim("slots", None, None, tuple(edge)).claim("digits", None, None, tuple(range(1, 10)))
    b.claim("high_halves", None, None, 10 ** 4)
    b.claim("p0_mod16", True, blk, 15).claim("line_len", True, blk, 24).claim("text_len", True, blk, 24 * K_TEXT_EDGES)
    yield b.case("B4_9_digits", "B4", True, "device")
    # B5: 10 digits.  N = 10^9 + 64, bidirected ids up to 2 N - 1 < 2^31 - 1
    n5 = 10 ** 9 + 64
    assert 2 * n5 < 2 ** 31 - 1
    b = Builder().decimal(n5)
    edge = [10 ** 9 - 1, 10 ** 9, 10 ** 9 + 1]
    nine = [hi * 10 ** 8 + 1234 * hi for hi in range(1, 10)] + [hi * 10 ** 8 for hi in range(1, 10)]
    b.add(*in_every_slot(edge + nine + [n5, 10 ** 8 - 1, 7, 99, 999, 1000], 10 ** 9 + 2))
    b.add(*[L(max(1, a * 10 ** 4 + (37 * a) % 10 ** 4), ori(a)[0], 10 ** 9 + (a % 64), ori(a)[1]) for a in range(10 ** 4)])
    blk = _padded_block(b, [L(10 ** 9 + j % 64, ori(j)[0], n5 - j % 61, ori(j)[1]) for j in range(K_TEXT_EDGES)])
    b.add(*dec_edges(7, 1000))
    b.claim("slots", None, None, tuple(edge + nine)).claim("digits", None, None, tuple(range(1, 11)))
    b.claim("p0_mod16", True, blk, 15).claim("line_len", True, blk, DEC_LINE_MAX)
    b.claim("text_len", True, blk, DEC_LINE_MAX * K_TEXT_EDGES)
    yield b.case("B5_10_digits", "B5", True, "device")


B6_N = 10 ** 6 + 2  # node names: str(k + 1) across 10^1 .. 10^6


def name_offsets(n: int, bidirected: bool) -> list:
    """The offsets of the keys of nodes 0 .. n (a cumulative sum of their lengths)."""
    out, at = [0], 0
    for k in range(1, n + 1):
        d = len(str(k))
        if bidirected:
            out += [at + d + 2, at + 2 * d + 4]
            at += 2 * d + 4
        else:
            at += d
            out.append(at)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for gen in (_family_a1, _family_a2, _family_a3, _family_a5, _family_a6, _family_b1, _family_b1_prefix,
                _family_b2, _family_b3, _family_b45):
        out += list(gen())
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# the two cases of 50 and 150 MB: built when asked for and not kept (cases() is cached for the session)
BIG = {A4_NAME: _a4, B1_BIG_NAME: _b1_big}


def case(name: str) -> Case:
    return next(BIG[name]()) if name in BIG else next(c for c in cases() if c.name == name)
