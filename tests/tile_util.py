"""Cases for the tile parse at its tile thresholds — TEST INFRASTRUCTURE, CPU only.

The front end (g2n_kernels.hip: k_tile_count_r, k_tile_parse, k_parse_deferred, lean_tile / k_tile_lean,
k_tile_lean_check, k_tile_compact) branches on where a line sits: its byte in the 32 KiB tile, the 16-byte chunk
and 64-byte thread region it starts in, its rank in the tile's line list, its length against the 48-byte tab
view and against the staged window.  tests/test_gpu_tile_edges.py drives it with the inputs built here;
tests/test_tile_cases.py shows on the CPU that every input sits on the threshold its name says.  This module
restates, in plain Python:

* the geometry (constants read from g2n_kernels.h / g2n_kernels.hip / g2n_pipeline.hip, restated, not imported);
* model(): the reference of the restricted grammar the cases use — the bytes split at '\\n', the first byte's
  dispatch (parser.py:117-134), fields by split(b"\\t"), node ids in first-touch order (dict_util.first_touch),
  P / H / W lines skipped, the one-shot warning's line and byte, a trailing RC:i: integer as the weight;
* expect_local(): whether the one-pass tile-local parse must accept an input (the lean shape of a line, both
  tabs in view, the line's end inside the staged window, S lines first), from which every route's tier follows.

Cases come from a Builder that pads with H lines (no tier rejects one) until a named line starts at a wanted tile
offset or has a wanted rank.  Each case carries claims — (what, line, value) — that the CPU test recomputes from
the bytes.  Everything is cheap: cases() builds 113 files, 3.4 MB of text, in 0.3 s.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import dict_util as D

# ------------------------------------------------------------------ geometry ------
K_TILE = 32768          # kTile: input bytes per front-end block
K_TILE_HALO = 2048      # kTileHalo: bytes k_tile_parse stages past the tile
K_LEAN_HALO = 64        # kLeanHalo: bytes lean_tile stages past the tile
CHUNK = 16              # bytes per staged chunk (one bitmap word)
K_LEAN_REGION = 4       # kLeanRegion: chunks per lean_tile thread
REGION = CHUNK * K_LEAN_REGION  # 64 bytes: the starts one lean_tile thread owns
K_LEAN_BATCH = 4        # kLeanBatch: starts of a region classified with batched loads
K_TILE_LINES = 2048     # kTileLines: line starts per window of k_tile_parse
K_LEAN_LINES = 2048     # kLeanLines: line records per window of lean_tile
VIEW = 48               # bytes of a line the lean tab view covers
K_MASK_SPAN = 64        # kMaskSpan: bytes a delimiter mask covers
K_TILE_EDGE_CAP = K_TILE // 12 + 6  # kTileEdgeCap: edges per tile slot of the tile-local parse
K1_TPB = 512            # k_tile_count_r: threads per tile
K1_WAVE_BYTES = 64 * CHUNK          # 1024: bytes one K1 wave covers per chunk row (lane 0 / lane 63 read global bytes)
K1_ROW_BYTES = K1_TPB * CHUNK       # 8192: bytes of one K1 chunk row
assert K_TILE_EDGE_CAP == 2736 and K_TILE_LINES == K_TILE // CHUNK

A_OFFSETS = (0, 1, 15, 16, 63, 64, 1023, 1024, 8191, 8192, 32766, 32767)
RANKS = (2047, 2048, 2049, 2050, 4100)  # 4100: the third window
ROUTES = ("default", "no_group", "no_tile_local", "no_lean", "direct", "hash", "hash_classic", "general")
LOCAL_ROUTES = ("default", "no_group")  # the routes that try the tile-local parse at all

Case = namedtuple("Case", "name lines family claims note")


# ------------------------------------------------------------------ lines ------
def S(k, seq: bytes = b"*") -> bytes:
    return b"S\t" + (k if isinstance(k, bytes) else b"%d" % k) + b"\t" + seq + b"\n"


def L(a, oa: str, b, ob: str, ov: bytes = b"*", tag: bytes = b"") -> bytes:
    f = [b"L", b"%d" % a, oa.encode(), b"%d" % b, ob.encode(), ov] + ([tag] if tag else [])
    return b"\t".join(f) + b"\n"


def LRC(a, oa, b, ob, w: int) -> bytes:
    return L(a, oa, b, ob, b"*", b"RC:i:%d" % w)


def P(name: bytes, segs: bytes = b"1+,2-", ov: bytes = b"*") -> bytes:
    return b"P\t" + name + b"\t" + segs + b"\t" + ov + b"\n"


def Hn(n: int) -> bytes:
    """An H line of n >= 2 bytes, its newline included."""
    assert n >= 2
    return b"H\n" if n == 2 else b"H\t" + b"x" * (n - 3) + b"\n"


def W(body: bytes = b"walk") -> bytes:
    return b"W\t" + body + b"\n"


def sized(line: bytes, n: int, at: int = -1) -> bytes:
    """`line` with its last field (or field `at`) stretched by 'x' until the line has n bytes before the newline."""
    f = line.rstrip(b"\n").split(b"\t")
    grow = n - len(line.rstrip(b"\n"))
    assert grow >= 0, (line, n)
    f[at] = f[at] + b"x" * grow
    return b"\t".join(f) + b"\n"


class Builder:
    """Lines in order, with the running byte offset; pads with H lines to an offset or to a rank in the tile."""

    def __init__(self, fill: int = 40):
        self.lines, self.at, self.fill, self.claims, self.n_s = [], 0, fill, [], 0

    def add(self, *lines):
        for x in lines:
            self.lines.append(x)
            self.at += len(x)
        return len(self.lines) - 1  # the last added line's index

    def segs(self, n: int, seq: bytes = b"*"):
        """The next n S lines of the decimal layout (named 1, 2, ... in order)."""
        for _ in range(n):
            self.n_s += 1
            self.add(S(self.n_s, seq))
        return len(self.lines) - 1

    def pad_to(self, target: int, fill: int = 0):
        """H lines until the next line starts at absolute offset `target`."""
        gap, fill = target - self.at, fill or self.fill
        assert gap == 0 or gap >= 2, (self.at, target)
        while gap:
            n = min(fill, gap)
            if gap - n == 1:
                n -= 1
            self.add(Hn(n))
            gap -= n
        return self

    def pad_tile(self, tile: int, off: int, fill: int = 0):
        return self.pad_to(tile * K_TILE + off, fill)

    def rank_here(self) -> int:
        """The rank, among its tile's line starts, that the next line will have."""
        t0 = self.at // K_TILE * K_TILE
        return sum(1 for s in starts_of(b"".join(self.lines)) if s >= t0)

    def pad_rank(self, rank: int):
        """2-byte H lines until the next line has `rank` among the starts of its tile (which must not change)."""
        tile, n = self.at // K_TILE, rank - self.rank_here()
        assert n >= 0 and (self.at + 2 * n) // K_TILE == tile, (rank, self.at)
        self.add(*[Hn(2)] * n)
        return self

    def fill_count(self, count: int, nbytes: int):
        """`count` H lines of `nbytes` in all (each at least 2 bytes)."""
        base, extra = divmod(nbytes, count)
        assert base >= 2
        self.add(*[Hn(base + (1 if j < extra else 0)) for j in range(count)])
        return self

    def claim(self, what: str, line, value):
        self.claims.append((what, line, value))
        return self

    def case(self, name: str, family: str, note: str = "") -> Case:
        return Case(name, tuple(self.lines), family, tuple(self.claims), note)


# ------------------------------------------------------------------ what the bytes say ------
def starts_of(data: bytes) -> list:
    """Offsets of the line starts: byte 0 and every byte after a newline, below len(data)."""
    out, p = ([0] if data else []), data.find(b"\n")
    while p != -1 and p + 1 < len(data):
        out.append(p + 1)
        p = data.find(b"\n", p + 1)
    return out


def line_table(data: bytes):
    """[(start, n, tile, off, rank)] of every line: n = bytes before its newline (or the input's end)."""
    out, ranks = [], {}
    for s in starts_of(data):
        e = data.find(b"\n", s)
        e = len(data) if e == -1 else e
        t = s // K_TILE
        out.append((s, e - s, t, s - t * K_TILE, ranks.get(t, 0)))
        ranks[t] = ranks.get(t, 0) + 1
    return out


def tile_starts(data: bytes) -> dict:
    c = {}
    for s in starts_of(data):
        c[s // K_TILE] = c.get(s // K_TILE, 0) + 1
    return c


def n_tiles(data: bytes) -> int:
    return (len(data) + K_TILE - 1) // K_TILE


EDGE_LETTERS, SKIP_LETTERS, PATH_LETTERS = b"LEC", b"HF", b"PO"


def _canonical(name: bytes) -> int:
    """The value of a canonical decimal of 1 - 10 digits (dec_lds), or 0."""
    return int(name) if name.isdigit() and name[:1] != b"0" and len(name) <= 10 and name.isascii() else 0


def expect_local(data: bytes, weighted: bool = False) -> bool:
    """Must the tile-local decimal parse (k_tile_lean kLeanDecimal, then k_tile_lean_check) accept `data`?  Restated
    from lean_tile / lean_line / lean_link / lean_edge_flat for the restricted grammar (a record letter is followed
    by a tab, a newline or the input's end):
    * the host's guess: the first S line within 64 KiB names "1" (no S line there: it tries);
    * a line's end is known when its newline (or the input's end) is staged: inside kTile + kLeanHalo of its tile;
    * an edge line: end known, at most 48 bytes, "L <a> <o> <b> <o> <...>" with canonical decimal names <= the S count
      (weighted: at most one more field, a canonical <tag>:i:<int>); at most kTileEdgeCap of them start in a tile;
    * an S line: a second tab within its first 48 bytes, or the whole line within them; named its S index + 1; no
      edge line anywhere before it;
    * a P line: two tabs within its first 48 bytes;  H / F: anything;  another letter (< 0x80): the warning, accepted.
    """
    if not data:
        return False
    for s in starts_of(data[:1 << 16]):
        if s + 3 >= min(len(data), 1 << 16):
            break
        if data[s:s + 2] == b"S\t":
            if not (data[s + 2:s + 3] == b"1" and data[s + 3:s + 4] in (b"\t", b"\n")):
                return False
            break
    table = line_table(data)
    n_seg = sum(1 for s, _n, _t, _o, _r in table if data[s:s + 1] == b"S")
    seen_s = seen_e = 0
    per_tile = {}
    for s, n, t, o, _r in table:
        lim = min(len(data) - t * K_TILE, K_TILE + K_LEAN_HALO)
        known = o + n < lim or (o + n == lim and s + n == len(data))
        body = data[s:s + n]
        c0 = body[:1]
        view = body[:VIEW] if known else data[s:s + VIEW]
        tabs = [j for j in range(len(view)) if view[j] == 9]
        if c0 and c0 in EDGE_LETTERS:
            per_tile[t] = per_tile.get(t, 0) + 1
            seen_e += 1
            f = body.split(b"\t")
            if not known or n > VIEW or len(f) < 6 or f[2] not in (b"+", b"-") or f[4] not in (b"+", b"-"):
                return False
            if not 1 <= _canonical(f[1]) <= n_seg or not 1 <= _canonical(f[3]) <= n_seg:
                return False
            if weighted and len(f) > 6:
                w = f[6][5:] if f[6][:5] == b"RC:i:" else b""
                w = w[1:] if w[:1] == b"-" else w
                if len(f) > 7 or not w.isdigit() or len(w) > 9 or (w[:1] == b"0" and len(w) > 1):
                    return False
        elif c0 == b"S":
            seen_s += 1
            if seen_e or len(tabs) < 1 or (len(tabs) < 2 and (not known or n > VIEW)):
                return False
            name = body[tabs[0] + 1:tabs[1] if len(tabs) > 1 else n]
            if _canonical(name) != seen_s:
                return False
        elif c0 and c0 in PATH_LETTERS:
            if len(tabs) < 2:
                return False
        elif c0 and c0 in SKIP_LETTERS:
            pass
        elif body[:1] >= b"\x80":
            return False
    return all(v <= K_TILE_EDGE_CAP for v in per_tile.values())


def expect_tier(data: bytes, route: str, weighted: bool = False) -> str:
    """"local" (the one-pass tile-local parse: a "parse" phase and no "tiles" phase) or "k1" (K1 ran)."""
    return "local" if route in LOCAL_ROUTES and expect_local(data, weighted) else "k1"


# ------------------------------------------------------------------ the model ------
Model = namedtuple("Model", "nodes edges weights warn_line warn_byte error")


def model(lines, bidirected: bool = False, keep: bool = True) -> Model:
    """The reference on the restricted grammar.  `lines` are the input split after each newline.  nodes / edges:
    dict_util.first_touch of the S and L lines; weights: one per L line, its trailing RC:i:<int> or 1; warn_line /
    warn_byte: the first line whose first byte is no record letter (-1: none); error: (line, message) of the first
    L line of fewer than five fields or P line of fewer than three — the reference raises there."""
    sl, weights, warn_line, warn_byte, error = [], [], -1, 0, None
    for i, x in enumerate(lines):
        c0 = x[:1]
        if c0 not in (b"S", b"L", b"P", b"E", b"C", b"O"):
            if c0 not in (b"H", b"F") and warn_line < 0:
                warn_line, warn_byte = i, x[0]
            continue
        f = x.rstrip(b"\n").split(b"\t")
        assert f[0] in (b"S", b"L", b"P"), "the restricted grammar"
        if (f[0] == b"L" and len(f) < 5) or (f[0] == b"P" and len(f) < 3):
            error = (i, "Malformed %s record" % f[0].decode())
            break
        if f[0] == b"L":
            rc = [t for t in f[6:] if t[:5] == b"RC:i:"]
            weights.append(float(int(rc[-1][5:])) if rc else 1.0)
        if f[0] != b"P":
            sl.append(x)
    nodes, edges = D.first_touch(sl, bidirected, keep)
    return Model(nodes, edges, weights, warn_line, warn_byte, error)


def split_lines(data: bytes) -> list:
    """The input as the reference's `for line in fh` yields it: split after every newline."""
    parts = data.split(b"\n")
    return [x + b"\n" for x in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


# ------------------------------------------------------------------ A. positions in the tile ------
KINDS = ("S", "L", "LRC", "P", "H", "W")


def _placed(kind: str, b: Builder, k: int) -> bytes:
    """The k-th placed line of a kind (an S line continues the decimal layout; edges name S lines 1 and 2)."""
    if kind == "S":
        b.n_s += 1
        return S(b.n_s, b"ACGT")
    return {"L": L(1 + (k & 1), "+-"[k & 1], 1 + ((k >> 1) & 1), "-+"[k & 1], b"%dM" % k),
            "LRC": LRC(1 + (k & 1), "-+"[k & 1], 1 + ((k >> 1) & 1), "+", 2 + k),
            "P": P(b"p%d" % k), "H": b"H\tVN:Z:%d.0\n" % k, "W": W(b"w%d" % k)}[kind]


# tile 0: 16 64 1024 8192 32766 | tile 1: 1023 8191, its last line's newline is byte 0 of tile 2 |
# tile 2: 1 63 32767 (the letter on the tile's last byte, its tab the halo's first) | tile 3: ends in a newline |
# tile 4: 0.  Offset 15 has files of its own: a line from 32766 / 32767 ends past byte 15 of the next tile.
A_PLAN = ((0, (16, 64, 1024, 8192, 32766)), (1, (1023, 8191)), (2, (1, 63, 32767)), (4, (0,)))


def _family_a():
    for kind in KINDS:
        b = Builder()
        b.segs(2)  # 12 bytes: room for the line at offset 16; placed S lines continue 3, 4, ...
        k = 0
        for tile, offs in A_PLAN:
            for off in offs:
                b.pad_tile(tile, off)
                i = b.add(_placed(kind, b, k))
                b.claim("tile_off", i, (tile, off))
                k += 1
            if tile == 1:
                b.pad_to(2 * K_TILE + 1)
                b.claim("nl_at", len(b.lines) - 1, 2 * K_TILE)  # tile 2's first byte: the previous line's newline
        b.claim("nl_at", i - 1, 4 * K_TILE - 1)  # offset 0 follows a newline on tile 3's last byte
        b.add(L(b.n_s, "+", 1, "-"), L(2, "-", b.n_s, "+"), P(b"tail"))
        yield b.case(f"A_{kind}_line_at_11_tile_offsets", "A")
    for kinds in (("S", "L", "LRC"), ("P", "H", "W")):
        b = Builder()
        b.segs(2)
        for t, kind in enumerate(kinds):
            b.pad_tile(t, 15, fill=37)
            i = b.add(_placed(kind, b, t))
            b.claim("tile_off", i, (t, 15))
        b.add(L(b.n_s, "+", 1, "-"), L(2, "-", b.n_s, "+"))
        yield b.case(f"A_{'_'.join(kinds)}_lines_at_tile_offset_15", "A")


def _family_a_more():
    b = Builder()  # no line start at all in tile 1: an S line from tile 0 to tile 2
    b.segs(3)
    b.pad_tile(0, 30000)
    b.n_s += 1
    i = b.add(S(b.n_s, b"ACGT" * ((2 * K_TILE + 500 - 30000) // 4)))
    b.claim("tile_off", i, (0, 30000)).claim("starts", 1, 0).claim("spans_tiles", i, 3)
    b.segs(2)
    b.add(L(1, "+", 4, "-"), L(5, "-", 6, "+"), L(4, "+", 4, "+"))
    yield b.case("A_tile_without_a_start_inside_an_S_line_of_three_tiles", "A")
    b = Builder()  # exactly one start in tile 1
    b.segs(3)
    b.pad_tile(0, 32000)
    b.add(Hn(K_TILE - 32000 + 100))           # ends at tile 1, byte 100
    i = b.add(sized(S(4, b"A"), 2 * K_TILE - b.at + 7))  # the rest of tile 1 and 8 bytes of tile 2
    b.claim("tile_off", i, (1, 100)).claim("starts", 1, 1)
    b.add(L(3, "+", 4, "-"), L(4, "+", 2, "-"))
    yield b.case("A_tile_holding_exactly_one_start", "A")


# ------------------------------------------------------------------ B. view and halo ------
def _head(b: Builder, n: int = 3):
    b.segs(n)
    return b


def _family_b():
    # lean edge lines of 47 / 48 / 49 bytes, mid-tile and starting on the tile's last byte
    for n in (47, 48, 49):
        for where, off in (("mid_tile", 20000), ("at_32767", 32767)):
            b = _head(Builder())
            b.pad_tile(0, off)
            i = b.add(sized(L(2, "-", 3, "+", b"7M"), n))
            b.claim("tile_off", i, (0, off)).claim("len", i, n)
            b.add(L(1, "+", 2, "+"), P(b"p"), L(3, "-", 3, "-"))
            yield b.case(f"B_lean_edge_line_of_{n}_bytes_{where}", "B")
    # (not decimal: the name is the long field) S lines whose second tab is byte 47 / 48 / 49 of a longer line
    for p in (47, 48, 49):
        for where in ("mid_tile", "sequence_past_the_staged_window"):
            b = Builder()
            b.add(S(b"first"), S(b"second"))
            name = b"n" * (p - 2)
            if where == "mid_tile":
                b.pad_tile(0, 9000)
                i = b.add(S(name, b"ACGT" * 20))
            else:
                b.pad_tile(0, K_TILE - 50 + (p - 47))  # starts in the tile's last 50 bytes
                i = b.add(S(name, b"ACGT" * 600))
                b.claim("end_past", i, K_TILE + K_LEAN_HALO)
            b.claim("tab2", i, p)
            b.add(D.L(b"first", b"+", name, b"-"), D.L(name, b"+", b"second", b"-"))
            yield b.case(f"B_S_line_second_tab_at_byte_{p}_{where}", "B")
    # P lines with their second tab inside / outside the view (decimal files: the tier follows it)
    for p in (47, 48):
        b = _head(Builder())
        b.pad_tile(0, 5000)
        i = b.add(P(b"p" * (p - 2), b"1+,2-,3+" * 8))
        b.claim("tab2", i, p)
        b.add(L(1, "+", 2, "-"), L(2, "+", 3, "-"))
        yield b.case(f"B_P_line_second_tab_at_byte_{p}", "B")
    # the tile's last line ending at the staged window's last byte, at its end, one past it: both windows
    for halo, tag in ((K_LEAN_HALO, "lean"), (K_TILE_HALO, "full")):
        for d in (-1, 0, 1):
            end = K_TILE + halo + d  # the newline's staged offset
            for kind in ("S", "L", "P"):
                b = Builder()
                start = K_TILE - 20
                n = end - start
                if kind == "S":  # decimal: the sequence is the long field (lean); full: the name (the second
                    b.segs(2)    # delimiter is what k_tile_parse defers on), so not a decimal file
                    b.pad_tile(0, start)
                    line = sized(S(3, b"A"), n) if halo == K_LEAN_HALO else sized(S(b"long", b"A"), n, at=1)
                    b.n_s = 3
                elif kind == "L":
                    b.segs(3)
                    b.pad_tile(0, start)
                    line = sized(L(1, "+", 2, "-", b"0M", b"XX:Z:"), n)
                else:
                    b.segs(3)
                    b.pad_tile(0, start)
                    line = sized(P(b"p", b"1+,2-"), n, at=(2 if halo == K_LEAN_HALO else 1))
                i = b.add(line)
                b.claim("tile_off", i, (0, start)).claim("nl_staged", i, end)
                b.add(L(1, "+", 2, "+"), L(2, "-", 1, "+"))
                if kind == "S" and halo == K_TILE_HALO:
                    b.add(D.L(line.split(b"\t")[1], b"+", b"1", b"-"))
                yield b.case(f"B_{tag}_window_last_{kind}_line_newline_at_staged_kTile+halo{d:+d}", "B")
    # deferred lines in two adjacent tiles; a deferred line in the last tile with a start, its window ending at EOF
    b = _head(Builder())
    for t in (0, 1):
        b.pad_tile(t, K_TILE - 30)
        i = b.add(sized(L(1 + t, "+", 3, "-", b"0M", b"XX:Z:"), K_TILE_HALO + 40))
        b.claim("tile_off", i, (t, K_TILE - 30)).claim("end_past", i, K_TILE + K_TILE_HALO)
    b.add(L(3, "+", 3, "+"))
    yield b.case("B_full_window_deferred_lines_in_two_adjacent_tiles", "B")
    for nl in (True, False):
        b = _head(Builder())
        b.pad_tile(0, K_TILE - 30)
        n = K_TILE_HALO + 30 - (1 if nl else 0)
        line = sized(L(1, "+", 3, "-", b"0M", b"XX:Z:"), n)
        i = b.add(line if nl else line[:-1])
        b.claim("total", None, K_TILE + K_TILE_HALO).claim("tile_off", i, (0, K_TILE - 30))
        yield b.case(f"B_full_window_ends_at_the_end_of_input_{'newline_last' if nl else 'no_newline'}", "B")
    # lines of 63 / 64 / 65 bytes around kMaskSpan: S lines whose second delimiter is byte 62 / 63 / 64 / 65, L lines
    for n in (63, 64, 65):
        b = Builder()
        b.add(S(b"first"), S(b"second"))
        nm = b"m" * (n - 2)
        i = b.add(b"S\t" + nm + b"\n")        # the second delimiter is the newline at byte n
        j = b.add(S(nm[:-2] + b"T", b"*"))    # ... a tab at byte n - 1, then one more byte
        b.claim("len", i, n).claim("tab2", j, n - 1)
        k = b.add(sized(D.L(b"first", b"+", b"second", b"-", b"0M"), n, at=5))
        b.claim("len", k, n)
        b.add(D.L(nm[:-2] + b"T", b"-", nm, b"+"))
        yield b.case(f"B_lines_of_{n}_bytes_around_the_mask_span", "B")
    # parse_line's whole-line tab view: a bitmap window of 64 bits from the chunk's first byte, so 49 bits are left at
    # chunk phase 15 — S and P lines of 48 / 49 / 60 bytes starting there, their second tab two bytes before the end
    for n in (48, 49, 60):
        b = Builder()
        b.add(S(b"first"), S(b"second"))
        b.pad_tile(0, 100 * CHUNK + 15)
        nm = b"v" * (n - 4)
        i = b.add(S(nm, b"*"))
        j_off = (b.at + 15) // CHUNK * CHUNK + 15
        b.pad_to(j_off if j_off - b.at != 1 else j_off + CHUNK)
        j = b.add(sized(P(b"p", b"1+"), n, at=1))
        b.claim("len", i, n).claim("len", j, n).claim("chunk_phase", i, 15).claim("chunk_phase", j, 15)
        b.claim("tab2_at", i, n - 2).claim("tab2_at", j, n - 5)
        b.add(D.L(b"first", b"+", nm, b"-"), D.L(nm, b"+", b"second", b"-"))
        yield b.case(f"B_S_and_P_line_of_{n}_bytes_at_chunk_phase_15", "B")


# ------------------------------------------------------------------ C. ranks and windows ------
def _region_lines(k: int):
    """Lines whose k starts all lie in one 64-byte region and whose last line ends past it: 2-byte H lines (behind
    one longer H line where needed), then two (or one) 12-byte edge lines as the region's last starts."""
    for m in (2, 1):
        for a in [0] + list(range(2, REGION)):
            lines = ([Hn(a)] if a else []) + [Hn(2)] * (k - m - (1 if a else 0)) + [L(2, "+", 3, "-"), L(3, "-", 1, "+")][:m]
            if len(lines) != k or any(len(x) < 2 for x in lines):
                continue
            offs = [sum(len(x) for x in lines[:j]) for j in range(k)]
            if offs[-1] < REGION <= offs[-1] + len(lines[-1]):
                return lines
    raise AssertionError(k)


def _family_c_counts():
    for n in (2047, 2048, 2049, 2050, 4096, 4097):
        # edges last: S 1 .. 9, H lines, 20 edge lines as the tile's last starts, the last ending on the tile's last byte
        b = Builder()
        b.segs(9)
        edges = [L(1 + j % 9, "+-"[j & 1], 1 + (j * 5) % 9, "-", b"*") for j in range(20)]
        b.fill_count(n - 9 - 20, K_TILE - b.at - 12 * 20)
        b.add(*edges)
        b.claim("starts", 0, n)
        assert b.at == K_TILE
        b.add(L(9, "+", 9, "-"), P(b"p"), L(2, "-", 8, "+"))
        yield b.case(f"C_tile_of_{n}_starts_edges_last", "C")
        # S lines last: H lines, then S 1 .. 99 (6 - 7 bytes) as the tile's last starts; edges in the next tile
        b = Builder()
        s_bytes = 9 * 6 + 90 * 7
        b.fill_count(n - 99, K_TILE - s_bytes)
        b.segs(99)
        b.claim("starts", 0, n)
        assert b.at == K_TILE
        b.add(*[L(1 + (j * 7) % 99, "+", 99 - j, "-") for j in range(30)])
        yield b.case(f"C_tile_of_{n}_starts_S_lines_last", "C")
    for n, y in ((2049, 1037), (4097, 2450)):
        # the shortest lines: S 1 .. 9 (6 bytes), y 12-byte edge lines, one H line of m bytes that makes the bytes come
        # out, 2-byte H lines (32 starts a region, up to the tile's highest ranks), two edge lines as its last starts
        b = Builder()
        b.segs(9)
        m = K_TILE - 54 - 24 - 12 * y - 2 * (n - 12 - y)  # 18246 (1000 2-byte lines), 20 (1635)
        assert m >= 2
        b.add(*[L(1 + j % 9, "+-"[j & 1], 1 + (j * 5) % 9, "-") for j in range(y)])
        b.add(Hn(m), *[Hn(2)] * (n - 12 - y))
        i = b.add(L(3, "-", 7, "+"), L(8, "+", 2, "-"))
        b.claim("starts", 0, n).claim("rank", i, (0, n - 1)).claim("nl_at", i, K_TILE - 1)
        b.claim("two_byte_lines", None, n - 12 - y)
        b.add(L(9, "+", 9, "-"), P(b"p"), L(2, "-", 8, "+"))
        yield b.case(f"C_tile_of_{n}_starts_2_byte_H_lines", "C")


def _family_c_regions():
    for k in (4, 5, 6, 32):
        b = _head(Builder())
        b.pad_tile(1, 37 * REGION)
        first = len(b.lines)
        b.add(*_region_lines(k))
        b.claim("region_starts", first, (1, 37, k))
        b.add(L(1, "+", 1, "+"))
        yield b.case(f"C_{k}_starts_inside_one_64_byte_region", "C")


def _family_c_caps():
    b = Builder()  # an edge-only tile: 2730 12-byte lines and the start of one more (under kTileEdgeCap)
    b.segs(12)
    b.pad_tile(1, 0)
    b.add(*[L(1 + j % 9, "+-"[j & 1], 1 + (j * 7) % 9, "-+"[(j >> 1) & 1]) for j in range(2730)])
    b.add(*[L(10 + j % 3, "+", 10 + (j + 1) % 3, "-") for j in range(40)])  # 14-byte lines, the first across the tiles
    b.claim("starts", 1, 2731).claim("tile_edges", 1, 2731)
    yield b.case("C_edge_only_tile_of_2730_edge_lines_of_12_bytes", "C")
    b = _head(Builder())  # more edge-kind lines than a tile slot holds: malformed, the reference raises
    b.add(*[b"L\n"] * 2800)
    b.claim("tile_edges", 0, 2800)
    yield b.case("C_tile_of_2800_malformed_2_byte_L_lines", "C", "error")


def issue_file() -> list:
    """The S-after-edge file: a header, S 1 .. 3, L 5 + 4 + *, 2060 x L 1 + 2 - *, S 4, S 5 — 24 773 bytes, one tile,
    S 4 is line 2065 (from 0).  The reference's node order is 1 2 3 5 4; a decimal parse that missed the late S
    lines would give 1 2 3 4 5."""
    return [D.H, S(1), S(2), S(3), L(5, "+", 4, "+")] + [L(1, "+", 2, "-")] * 2060 + [S(4), S(5)]


def _family_c_premise():
    b = Builder()
    b.add(*issue_file())
    b.claim("total", None, 24773).claim("rank", len(b.lines) - 2, (0, 2065))
    yield b.case("C_S_after_edge_the_2060_edge_lines_file", "C")
    for r in RANKS:
        for variant, e in (("naming_later_S_lines", (5, 4)), ("naming_defined_nodes_only", (1, 2))):
            b = _head(Builder())
            b.add(L(e[0], "+", e[1], "+"))
            b.pad_rank(r)
            i = b.add(S(4))
            b.add(S(5), L(4, "-", 5, "+"))
            b.claim("rank", i, (0, r))
            yield b.case(f"C_S_after_edge_{variant}_at_rank_{r}", "C")
        b = Builder()  # an S line named one too high
        b.pad_rank(r - 3)
        b.segs(3)
        i = b.add(S(5))
        b.add(S(5), S(6), L(1, "+", 5, "-"), L(6, "+", 4, "-"))
        b.claim("rank", i, (0, r))
        yield b.case(f"C_S_line_named_one_too_high_at_rank_{r}", "C")
        b = _head(Builder())  # an edge key of N + 1
        b.add(L(1, "+", 2, "-"))
        b.pad_rank(r)
        i = b.add(L(4, "+", 1, "-"))
        b.add(L(3, "+", 4, "-"))
        b.claim("rank", i, (0, r))
        yield b.case(f"C_edge_key_N_plus_1_at_rank_{r}", "C")
        b = _head(Builder())  # a W line, then an X line: the one-shot warning names the first
        b.add(L(1, "+", 2, "-"))
        b.pad_rank(r)
        i = b.add(W())
        b.add(L(3, "+", 1, "-"), b"X\tlater\n", L(2, "+", 2, "-"))
        b.claim("rank", i, (0, r)).claim("warns", i, ord("W"))
        yield b.case(f"C_W_line_at_rank_{r}", "C")


# ------------------------------------------------------------------ D. end of input ------
def _family_d():
    for k in (1, 2):
        for d in (-1, 0, 1):
            b = _head(Builder())
            b.add(L(1, "+", 2, "-"))
            last = L(3, "-", 1, "+")
            b.pad_to(k * K_TILE + d - len(last))
            b.add(last)
            b.claim("total", None, k * K_TILE + d)
            yield b.case(f"D_length_{k}_tiles{d:+d}", "D")
    for kind, line in (("L", L(3, "-", 1, "+")), ("S", S(4, b"ACGT")), ("P", P(b"p"))):
        b = _head(Builder())
        if kind != "S":  # (S lines come first: the file whose last line is an S line has no edge)
            b.add(L(1, "+", 2, "-"))
        b.pad_tile(1, 700)
        b.add(line[:-1])
        b.claim("no_final_newline", None, None)
        yield b.case(f"D_last_{kind}_line_without_newline", "D")
    b = _head(Builder())
    b.add(L(1, "+", 2, "-"))
    last = L(3, "-", 1, "+")[:-1]
    b.pad_to(K_TILE - len(last))
    b.add(last)
    b.claim("total", None, K_TILE).claim("no_final_newline", None, None)
    yield b.case("D_last_line_ends_on_the_tiles_last_byte_without_newline", "D")
    for name, data in (("D_input_of_0_bytes", b""), ("D_input_of_1_byte", b"\n"), ("D_input_of_5_bytes", b"S\t1\t*"),
                       ("D_input_of_15_bytes", b"S\t1\nL\t1\t+\t1\t-\t*")):
        yield Case(name, tuple(split_lines(data)), "D", (("total", None, int(name.split("_")[3])),), "")
    b = _head(Builder())  # a final tile of one byte: the newline of the previous tile's line
    b.add(L(1, "+", 2, "-"))
    last = L(3, "-", 1, "+")
    b.pad_to(K_TILE + 1 - len(last))
    b.add(last)
    b.claim("total", None, K_TILE + 1).claim("starts", 1, 0)
    yield b.case("D_final_tile_of_one_byte_a_newline", "D")
    b = _head(Builder())  # ... one line start: the letter H
    b.add(L(1, "+", 2, "-"))
    b.pad_to(K_TILE)
    b.add(b"H")
    b.claim("total", None, K_TILE + 1).claim("starts", 1, 1)
    yield b.case("D_final_tile_of_one_byte_a_line_start", "D")


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for gen in (_family_a, _family_a_more, _family_b, _family_c_counts, _family_c_regions, _family_c_caps,
                _family_c_premise, _family_d):
        out += list(gen())
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def data_of(c: Case) -> bytes:
    return b"".join(c.lines)
