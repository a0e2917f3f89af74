"""A deflate writer, an independent bit-by-bit reader and a catalogue of BGZF files for the GPU
inflate (g2n_inflate.hip, k_inflate_members).  Pure Python, nothing imported from the product.

The writer emits RFC 1951 blocks from explicit token lists (literals and (length, distance)
pairs), with every encoding choice in the caller's hand: stored LEN, the code lengths of both
alphabets, how those lengths are themselves encoded (16 / 17 / 18 and their counts, HCLEN, the
code-length code's own lengths), symbol 285 or 284+31 for length 258, and deliberately invalid
output.  `inflate_trace` decodes one bit at a time from a {(length, code): symbol} dictionary,
accepts what zlib's inflate accepts, and records what the stream used, so a case that claims
"distance 32768" or "stored header at bit phase 5" is checked to have it.

Every case's concatenated payload is a valid GFA: ordinary S / L lines around one S line whose
sequence field is a long blob of arbitrary bytes (no tab, LF or CR); the matrix build ignores
that field, and the token games happen inside it.  Payloads are made by executing the tokens.
"""
from __future__ import annotations

import heapq
import random
import struct
import zlib

# ------------------------------------------------------------------ RFC 1951 §3.2.5 ---------


def _bases(n_syms, first_extra_sym, per_step, start):
    base, extra, b = [], [], start
    for s in range(n_syms):
        e = 0 if s < first_extra_sym else (s - first_extra_sym) // per_step + 1
        base.append(b)
        extra.append(e)
        b += 1 << e
    return base, extra


LEN_BASE, LEN_EXTRA = _bases(28, 8, 4, 3)  # symbols 257..284
LEN_BASE.append(258)  # symbol 285
LEN_EXTRA.append(0)
DIST_BASE, DIST_EXTRA = _bases(30, 4, 2, 1)
assert LEN_BASE[27] == 227 and LEN_EXTRA[27] == 5 and DIST_BASE[29] == 24577 and DIST_EXTRA[29] == 13
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
BLOB = bytes(b for b in range(256) if b not in (9, 10, 13))  # what a sequence field may hold


def canonical_codes(lens):
    """RFC 1951 §3.2.2: the code of every symbol from the code lengths alone."""
    bl_count = [0] * 17
    for l in lens:
        bl_count[l] += 1
    bl_count[0] = 0
    next_code, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = next_code[l]
            next_code[l] += 1
    return codes


def kraft_left(lens, maxbits=15):
    """> 0 incomplete, 0 complete, < 0 over-subscribed (in units of 2**-maxbits)."""
    return (1 << maxbits) - sum(1 << (maxbits - l) for l in lens if l)


def huffman_lens(freq, n, limit):
    """Code lengths (<= limit) for an n-symbol alphabet from {symbol: count}; a complete code of
    at least two symbols (an unused symbol is added when only one is used)."""
    freq = {s: f for s, f in freq.items() if f > 0}
    for s in range(n):
        if len(freq) >= 2:
            break
        freq.setdefault(s, 1)
    while True:
        heap = [(f, s, (s,)) for s, f in freq.items()]
        heapq.heapify(heap)
        depth = dict.fromkeys(freq, 0)
        while len(heap) > 1:
            fa, ta, a = heapq.heappop(heap)
            fb, tb, b = heapq.heappop(heap)
            for s in a + b:
                depth[s] += 1
            heapq.heappush(heap, (fa + fb, min(ta, tb), a + b))
        if max(depth.values()) <= limit:
            lens = [0] * n
            for s, d in depth.items():
                lens[s] = d
            return lens
        freq = {s: (f + 1) // 2 for s, f in freq.items()}  # flatter counts, shallower tree


def skew_lens(symbols, n, maxlen):
    """A complete code over an n-symbol alphabet whose longest codes have exactly `maxlen` bits:
    a chain 1, 2, .., maxlen, maxlen, leaves split until there is one per symbol.  `symbols` get
    the lengths shortest first (so the last ones are `maxlen` long); when there are fewer than
    maxlen + 1 of them, unused symbols take the remaining short codes' places at the long end."""
    symbols = list(symbols)
    spare = [s for s in range(n) if s not in set(symbols)]
    while len(symbols) < maxlen + 1:
        symbols.insert(max(0, len(symbols) - 4), spare.pop())  # keep the caller's last ones longest
    shape = list(range(1, maxlen + 1)) + [maxlen]
    while len(shape) < len(symbols):
        shape.sort()
        d = shape.pop(0)
        assert d < maxlen
        shape += [d + 1, d + 1]
    shape.sort()
    lens = [0] * n
    for s, l in zip(symbols, shape):
        lens[s] = l
    assert kraft_left(lens) == 0
    return lens


# ------------------------------------------------------------------ the writer --------------
class BitWriter:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.n

    def bits(self, v, k):
        """k bits of v, least significant first (header fields, extra bits)."""
        assert 0 <= v < (1 << k), (v, k)
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):
        """a Huffman code of k bits, most significant first."""
        assert k and 0 <= c < (1 << k), (c, k)
        self.bits(int(format(c, "0%db" % k)[::-1], 2), k)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.buf += data

    def getvalue(self):
        self.align()
        return bytes(self.buf)


def mtok(length, dist, alt258=False):
    """(length, distance) as an explicit token ("M", length symbol, extra, distance symbol, extra)."""
    assert 3 <= length <= 258 and 1 <= dist <= 32768
    if length == 258:
        ls, le = (284, 31) if alt258 else (285, 0)
    else:
        ls = max(s for s in range(28) if LEN_BASE[s] <= length) + 257
        le = length - LEN_BASE[ls - 257]
    ds = max(s for s in range(30) if DIST_BASE[s] <= dist)
    return ("M", ls, le, ds, dist - DIST_BASE[ds])


def emit_tokens(w, tokens, ll_lens, d_lens, eob=True):
    """Tokens: an int is a literal; ("S", sym) any literal/length symbol on its own; ("M", ...)
    see mtok (distance symbols 30 and 31 take no extra bits)."""
    ll, d = canonical_codes(ll_lens), canonical_codes(d_lens)
    for t in tokens:
        if isinstance(t, int):
            w.code(ll[t], ll_lens[t])
        elif t[0] == "S":
            w.code(ll[t[1]], ll_lens[t[1]])
        else:
            _, ls, le, ds, de = t
            w.code(ll[ls], ll_lens[ls])
            w.bits(le, LEN_EXTRA[ls - 257])
            w.code(d[ds], d_lens[ds])
            w.bits(de, DIST_EXTRA[ds] if ds < 30 else 0)
    if eob:
        w.code(ll[256], ll_lens[256])


def stored_block(w, data, final, len_field=None, nlen_field=None):
    w.bits(int(final), 1)
    w.bits(0, 2)
    w.align()
    ln = len(data) if len_field is None else len_field
    w.bits(ln, 16)
    w.bits(ln ^ 0xFFFF if nlen_field is None else nlen_field, 16)
    w.raw(data)


def fixed_block(w, tokens, final, eob=True):
    w.bits(int(final), 1)
    w.bits(1, 2)
    emit_tokens(w, tokens, FIXED_LL, FIXED_D, eob)


def expand_ops(ops):
    seq = []
    for op in ops:
        if op[0] < 16:
            seq.append(op[0])
        elif op[0] == 16:
            seq += [seq[-1]] * op[1]
        else:
            seq += [0] * op[1]
    return seq


def plan_cl(seq):
    """The code lengths as code-length symbols: ops (0..15,), (16, 3..6), (17, 3..10), (18, 11..138);
    greedy over the whole literal/length + distance sequence, so a run may cross between them."""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                ops.append((18, k))
                run -= k
            if run >= 3:
                ops.append((17, run))
                run = 0
            ops += [(0,)] * run
        else:
            ops.append((v,))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                ops.append((16, k))
                run -= k
            ops += [(v,)] * run
        i = j
    return ops


def dynamic_block(w, tokens, final, ll_lens, d_lens, cl_ops=None, cl_lens=None, hclen=None, eob=True,
                  stop_after_cl=False):
    """A dynamic block.  HLIT and HDIST are len(ll_lens) - 257 and len(d_lens) - 1 (so 287 / 288
    literal/length or 31 / 32 distance lengths give the invalid header fields); cl_ops encodes the
    lengths (default plan_cl), cl_lens is the code-length code (default: Huffman over the ops,
    limit 7), hclen how many of its lengths are sent (default: the fewest that hold them)."""
    if cl_ops is None:
        cl_ops = plan_cl(list(ll_lens) + list(d_lens))
    if cl_lens is None:
        freq = {}
        for op in cl_ops:
            freq[op[0]] = freq.get(op[0], 0) + 1
        cl_lens = huffman_lens(freq, 19, 7)
    if hclen is None:
        hclen = max([4] + [k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]])
    assert all(cl_lens[CL_ORDER[k]] == 0 for k in range(hclen, 19))
    w.bits(int(final), 1)
    w.bits(2, 2)
    w.bits(len(ll_lens) - 257, 5)
    w.bits(len(d_lens) - 1, 5)
    w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(cl_lens[CL_ORDER[k]], 3)
    if stop_after_cl:
        return
    cl = canonical_codes(cl_lens)
    for op in cl_ops:
        w.code(cl[op[0]], cl_lens[op[0]])
        if op[0] == 16:
            w.bits(op[1] - 3, 2)
        elif op[0] == 17:
            w.bits(op[1] - 3, 3)
        elif op[0] == 18:
            w.bits(op[1] - 11, 7)
    emit_tokens(w, tokens, list(ll_lens), list(d_lens), eob)


def auto_lens(tokens, n_ll=None, n_d=None):
    """Huffman code lengths (limit 15) for a token list, with an end-of-block code."""
    fl, fd = {256: 1}, {}
    for t in tokens:
        if isinstance(t, int):
            fl[t] = fl.get(t, 0) + 1
        else:
            fl[t[1]] = fl.get(t[1], 0) + 1
            fd[t[3]] = fd.get(t[3], 0) + 1
    ll = huffman_lens(fl, 286, 15)
    d = huffman_lens(fd, 30, 15)
    n_ll = n_ll or max(257, 1 + max(s for s in range(286) if ll[s]))
    n_d = n_d or 1 + max(s for s in range(30) if d[s])
    return ll[:n_ll], d[:n_d]


# ------------------------------------------------------------------ the reader --------------
class DeflateError(Exception):
    def __init__(self, msg, where=""):
        super().__init__(msg)
        self.where = where  # for "truncated": "header" / "symbol" / "extra" / "stored"


class _BitReader:
    def __init__(self, data):
        self.data = data
        self.pos = 0
        self.where = "header"

    def bit(self):
        if self.pos >= len(self.data) * 8:
            raise DeflateError("truncated", self.where)
        b = (self.data[self.pos >> 3] >> (self.pos & 7)) & 1
        self.pos += 1
        return b

    def bits(self, k):
        v = 0
        for i in range(k):
            v |= self.bit() << i
        return v


def _table(lens, kind):
    """{(length, code): symbol} as zlib's inflate_table admits it: over-subscribed never;
    incomplete only as a single one-bit code in the literal/length or distance alphabet, or as no
    distance code at all."""
    used = [l for l in lens if l]
    left = kraft_left(lens)
    if left < 0:
        raise DeflateError("over-subscribed %s code" % kind)
    if used and left > 0 and (kind == "cl" or max(used) != 1):
        raise DeflateError("incomplete %s code" % kind)
    codes = canonical_codes(lens)
    return {(l, codes[s]): s for s, l in enumerate(lens) if l}, max(used, default=0)


def _symbol(br, table, maxlen, kind):
    code = 0
    for l in range(1, maxlen + 1):
        code = (code << 1) | br.bit()
        s = table.get((l, code))
        if s is not None:
            return s, l
    raise DeflateError("invalid %s code" % kind)


def inflate_trace(raw):
    """(output bytes, trace) of one raw deflate stream, or DeflateError where zlib rejects it."""
    br = _BitReader(raw)
    out = bytearray()
    tr = dict(blocks=[], header_phase=[], stored_phase=[], stored_len=[], hlit=[], hdist=[], hclen=[],
              cl_ops=[], cl_cross=[], cl_last_is_repeat=[], tables=[], max_len=dict(cl=0, ll=0, d=0),
              used_len=dict(ll=0, d=0), literals=set(), len_syms=set(), dist_syms=set(), len_extra=set(),
              dist_extra=set(), lengths=set(), dists=set(), max_dist=0, copies=[], max_token_bits=0,
              token_bits=[], fixed_literals=set())
    final = 0
    while not final:
        br.where = "header"
        tr["header_phase"].append(br.pos & 7)
        final = br.bit()
        btype = br.bits(2)
        if btype == 3:
            raise DeflateError("invalid block type")
        if btype == 0:
            tr["blocks"].append("stored")
            tr["stored_phase"].append(tr["header_phase"][-1])
            br.pos = (br.pos + 7) & ~7
            ln, nln = br.bits(16), br.bits(16)
            if ln ^ 0xFFFF != nln:
                raise DeflateError("invalid stored block lengths")
            tr["stored_len"].append(ln)
            br.where = "stored"
            if br.pos // 8 + ln > len(raw):
                raise DeflateError("truncated", "stored")
            out += raw[br.pos // 8:br.pos // 8 + ln]
            br.pos += 8 * ln
            continue
        if btype == 1:
            tr["blocks"].append("fixed")
            ll_lens, d_lens = FIXED_LL, FIXED_D
        else:
            tr["blocks"].append("dynamic")
            nlen, ndist, ncode = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
            tr["hlit"].append(nlen)
            tr["hdist"].append(ndist)
            tr["hclen"].append(ncode)
            if nlen > 286 or ndist > 30:
                raise DeflateError("too many length or distance symbols")
            cl_lens = [0] * 19
            for k in range(ncode):
                cl_lens[CL_ORDER[k]] = br.bits(3)
            cl_tab, cl_max = _table(cl_lens, "cl")
            tr["max_len"]["cl"] = max(tr["max_len"]["cl"], cl_max)
            seq, ops = [], []
            while len(seq) < nlen + ndist:
                if cl_max == 0:  # zlib reads every length as a one-bit zero; no end-of-block follows
                    br.bit()
                    s = 0
                else:
                    s, _ = _symbol(br, cl_tab, cl_max, "code lengths")
                if s < 16:
                    seq.append(s)
                    ops.append((s,))
                    continue
                if s == 16:
                    if not seq:
                        raise DeflateError("invalid bit length repeat")
                    v, rep = seq[-1], 3 + br.bits(2)
                else:
                    v, rep = 0, (3 + br.bits(3) if s == 17 else 11 + br.bits(7))
                if len(seq) + rep > nlen + ndist:
                    raise DeflateError("invalid bit length repeat")
                if len(seq) < nlen < len(seq) + rep:
                    tr["cl_cross"].append(s)
                seq += [v] * rep
                ops.append((s, rep))
            tr["cl_ops"] += ops
            tr["cl_last_is_repeat"].append(ops[-1][0] >= 16)
            if seq[256] == 0:
                raise DeflateError("invalid code -- missing end-of-block")
            ll_lens, d_lens = seq[:nlen], seq[nlen:]
            tr["tables"].append((tuple(ll_lens), tuple(d_lens)))
        ll_tab, ll_max = _table(ll_lens, "literal/length")
        d_tab, d_max = _table(d_lens, "distance")
        tr["max_len"]["ll"] = max(tr["max_len"]["ll"], ll_max)
        tr["max_len"]["d"] = max(tr["max_len"]["d"], d_max)
        while True:
            br.where = "symbol"
            t0 = br.pos
            s, l = _symbol(br, ll_tab, ll_max, "literal/length")
            tr["used_len"]["ll"] = max(tr["used_len"]["ll"], l)
            if s < 256:
                out.append(s)
                tr["literals"].add(s)
                if btype == 1:
                    tr["fixed_literals"].add(s)
                continue
            if s == 256:
                break
            if s > 285:
                raise DeflateError("invalid literal/length code")
            tr["len_syms"].add(s)
            br.where = "extra"
            e = br.bits(LEN_EXTRA[s - 257])
            ln = LEN_BASE[s - 257] + e
            tr["len_extra"].add((s, e))
            br.where = "symbol"
            ds, l = _symbol(br, d_tab, d_max, "distance")
            tr["used_len"]["d"] = max(tr["used_len"]["d"], l)
            if ds > 29:
                raise DeflateError("invalid distance code")
            tr["dist_syms"].add(ds)
            br.where = "extra"
            e = br.bits(DIST_EXTRA[ds])
            dist = DIST_BASE[ds] + e
            tr["dist_extra"].add((ds, e))
            if dist > len(out):
                raise DeflateError("invalid distance too far back")
            tr["copies"].append((len(out), ln, dist, tr["blocks"][-1]))
            tr["lengths"].add(ln)
            tr["dists"].add(dist)
            tr["max_dist"] = max(tr["max_dist"], dist)
            tr["token_bits"].append(br.pos - t0)
            tr["max_token_bits"] = max(tr["max_token_bits"], br.pos - t0)
            for _ in range(ln):
                out.append(out[-dist])
    tr["end_bit"] = br.pos
    tr["consumed"] = (br.pos + 7) // 8
    tr["out_len"] = len(out)
    return bytes(out), tr


def crc_suffix(crc_before, crc_after):
    """The four bytes that take a CRC-32 from crc_before to crc_after."""
    table = []
    for k in range(256):
        c = k
        for _ in range(8):
            c = 0xEDB88320 ^ (c >> 1) if c & 1 else c >> 1
        table.append(c)
    top = {c >> 24: k for k, c in enumerate(table)}
    reg = crc_after ^ 0xFFFFFFFF
    for _ in range(4):
        k = top[reg >> 24]
        reg = (((reg ^ table[k]) << 8) & 0xFFFFFFFF) | k
    return struct.pack("<I", reg ^ crc_before ^ 0xFFFFFFFF)


def zlib_inflate(raw):
    """zlib's verdict on the same stream: the bytes, or None where it raises."""
    try:
        return zlib.decompress(raw, -15)
    except zlib.error:
        return None


# ------------------------------------------------------------------ BGZF --------------------
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_member(raw, payload, extra_before=b"", extra_after=b"", crc=None, isize=None, flg=4, name=b"",
                bc_slen=2):
    """One gzip member with the 'BC' subfield (total size - 1) between the two other runs of extra
    subfields; the trailer is the payload's unless given.  extra_after may be a function of the
    member's total size (a second BC)."""
    probe = extra_after(0) if callable(extra_after) else extra_after
    xlen = len(extra_before) + 4 + bc_slen + len(probe)
    total = 12 + xlen + len(name) + len(raw) + 8
    assert total <= 65536
    after = extra_after(total) if callable(extra_after) else extra_after
    bc = b"BC" + struct.pack("<HH", bc_slen, total - 1) + b"\0" * (bc_slen - 2)
    hdr = bytes([0x1F, 0x8B, 8, flg, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H", xlen) + extra_before + bc + after
    return hdr + name + raw + struct.pack("<II", zlib.crc32(payload) if crc is None else crc,
                                          len(payload) if isize is None else isize)


def bgzf_file(members, eof=True):
    return b"".join(members) + (EOF_MEMBER if eof else b"")


# ------------------------------------------------------------------ payloads ----------------
class Tokens:
    """A member's payload made by executing its tokens."""

    def __init__(self, rng):
        self.rng = rng
        self.out = bytearray()
        self.toks = []

    def lit(self, data):
        self.out += data
        self.toks += list(data)
        return self

    def rand(self, n, alphabet=BLOB):
        return self.lit(bytes(self.rng.choice(alphabet) for _ in range(n)))

    def copy(self, length, dist, alt258=False):
        assert 1 <= dist <= len(self.out), (dist, len(self.out))
        for _ in range(length):
            self.out.append(self.out[-dist])
        self.toks.append(mtok(length, dist, alt258))
        return self

    def take(self):
        t, self.toks = self.toks, []
        return t


PRE_TEXT = b"S\ta\tAC\nS\tb\tGT\nL\ta\t+\tb\t+\t0M\nS\tblob\t"
SUF_TEXT = b"\nS\tc\tA\nL\tb\t+\tc\t-\t0M\r\n"
MID_TEXT = b"\nL\ta\t+\tb\t-\t0M\r\nS\tq\t"  # leaves and re-enters a blob: tab, LF and CR as literals


def _zraw(data):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush()


class Member:
    def __init__(self, raw, payload, **header):
        self.raw, self.payload, self.header = bytes(raw), bytes(payload), header

    def bytes(self):
        return bgzf_member(self.raw, self.payload, **self.header)


PRE = Member(_zraw(PRE_TEXT), PRE_TEXT)
SUF = Member(_zraw(SUF_TEXT), SUF_TEXT)
EMPTY = Member(b"\x03\x00", b"")  # the EOF marker's member


class Case:
    """name; cls "A".."H"; verdict "gpu" (inflated on the device), "declined" (zlib accepts, the
    kernel hands the file to the host by design), "host" (the member locator declines the file),
    "error" (CPython raises); features [(text, predicate over the test members' merged trace)];
    members; `test` the indices of the members the features speak of."""

    def __init__(self, name, verdict, members, features=(), test=None, eof=True, tail=b""):
        self.name, self.cls, self.verdict = name, name[0], verdict
        self.members, self.features, self.eof, self.tail = list(members), list(features), eof, tail
        self.test = list(range(len(self.members))) if test is None else test

    def file(self):
        return bgzf_file([m.bytes() for m in self.members], self.eof) + self.tail

    def payload(self):
        return b"".join(m.payload for m in self.members)


def merged_trace(traces):
    m = {}
    for tr in traces:
        for k, v in tr.items():
            if k not in m:
                m[k] = v.copy() if hasattr(v, "copy") else [v]
            elif isinstance(v, set):
                m[k] |= v
            elif isinstance(v, list):
                m[k] = m[k] + v
            elif isinstance(v, dict):
                m[k] = {a: max(m[k][a], b) for a, b in v.items()}
            else:
                m[k] = m[k] + [v] if isinstance(m[k], list) else max(m[k], v)
    return m


CASES: list[Case] = []


def _wrap(case_name, verdict, raw, payload, features=(), **header):
    """prefix lines + the test member (blob bytes) + suffix lines"""
    c = Case(case_name, verdict, [PRE, Member(raw, payload, **header), SUF], features, test=[1])
    CASES.append(c)
    return c


def _build():
    rng = random.Random(0x1951)
    hi = bytes(range(144, 256))  # nine-bit fixed literals
    lo = bytes(b for b in range(32, 127))  # eight-bit ones

    # ---- A. bit reader and stored blocks -------------------------------------------------
    for k in range(8):
        t, w = Tokens(rng), BitWriter()
        t.rand(5, lo).rand((k - 2) % 8, hi)
        fixed_block(w, t.take(), False)  # 3 + 8*5 + 9*j + 7 bits
        tail = bytes(rng.choice(BLOB) for _ in range(21))
        stored_block(w, tail, True)
        _wrap("A_stored_phase_%d" % k, "gpu", w.getvalue(), t.out + tail,
              [("stored header at bit phase %d" % k, lambda tr, k=k: tr["stored_phase"] == [k])])
    for final in (False, True):
        t, w = Tokens(rng), BitWriter()
        fixed_block(w, t.rand(9).take(), False)
        stored_block(w, b"", final)
        if not final:
            fixed_block(w, t.rand(9).take(), True)
        _wrap("A_len0_%s" % ("final" if final else "middle"), "gpu", w.getvalue(), t.out,
              [("LEN = 0", lambda tr: tr["stored_len"] == [0]),
               ("its place", lambda tr, f=final: tr["blocks"][-1] == ("stored" if f else "fixed"))])
    big = bytes(rng.choice(BLOB) for _ in range(65536))
    # LEN = 65535 cannot stand in a BGZF member (at most 65536 bytes with header and trailer; the
    # largest that fits is H_largest_bsize's 65505, and F_len_65535_data_missing has the field
    # without the data); 65536 bytes of output that end in a one-byte stored block can
    t, w = Tokens(rng), BitWriter()
    t.rand(300)
    while len(t.out) + 258 <= 65535 - 20000:
        t.copy(258, rng.randint(1, 300))
    t.copy(65535 - 20000 - len(t.out), 1)
    fixed_block(w, t.take(), False)
    stored_block(w, big[:20000], False)
    stored_block(w, big[20000:20001], True)
    t.out += big[:20001]
    _wrap("A_output_65536_last_block_one_byte", "gpu", w.getvalue(), t.out,
          [("LEN = 20000 then 1", lambda tr: tr["stored_len"] == [20000, 1]),
           ("65536 bytes out", lambda tr: tr["out_len"] == [65536])])
    t, w = Tokens(rng), BitWriter()
    for n in range(17):  # every amount of prefetched input at the stored header
        fixed_block(w, t.rand(n, lo).rand(n % 8, hi).take(), False)
        s3 = bytes(rng.choice(BLOB) for _ in range(3))
        stored_block(w, s3, n == 16)
        t.out += s3
    _wrap("A_stored_after_prefetch_sweep", "gpu", w.getvalue(), t.out,
          [("fixed / stored alternate 17 times", lambda tr: tr["blocks"] == ["fixed", "stored"] * 17),
           ("every phase", lambda tr: set(tr["stored_phase"]) == set(range(8)))])
    for k in range(1, 9):
        t, w = Tokens(rng), BitWriter()
        t.rand(4, lo).rand((k - 2) % 8, hi)
        fixed_block(w, t.take(), True)
        _wrap("A_end_bit_%d" % k, "gpu", w.getvalue(), t.out,
              [("ends at bit %d of the last byte" % k, lambda tr, k=k: tr["end_bit"][0] % 8 == k % 8),
               ("no spare byte", lambda tr, n=len(w.getvalue()): tr["consumed"] == [n])])
    # 15 + 5 + 15 + 13 bits, eight in a row
    t, w = Tokens(rng), BitWriter()
    head = big[:32768]
    stored_block(w, head, False)
    t.out += head
    t.rand(12, BLOB[:12])
    for i in range(8):
        t.copy(227 + 8 + i * 3 if i < 7 else 258, 32768 - i * 1000, alt258=True)
    toks = t.take()
    ll = [0] * 285
    ll[256] = 1
    for i, b in enumerate(BLOB[:12]):
        ll[b] = 2 + i
    ll[281] = ll[282] = ll[283] = ll[284] = 15
    dl = [i + 1 for i in range(14)] + [0] * 14 + [15, 15]
    assert {x[1] for x in toks if not isinstance(x, int)} <= {284} and kraft_left(ll) == 0 == kraft_left(dl)
    dynamic_block(w, toks, True, ll, dl)
    _wrap("A_longest_tokens", "gpu", w.getvalue(), t.out,
          [("48-bit tokens, eight in a row", lambda tr: tr["token_bits"] == [48] * 8),
           ("HDIST = 30", lambda tr: tr["hdist"] == [30])])

    # ---- B. fixed code -------------------------------------------------------------------
    t, w = Tokens(rng), BitWriter()
    t.lit(BLOB).lit(MID_TEXT).rand(5)
    fixed_block(w, t.take(), True)
    _wrap("B_all_literals", "gpu", w.getvalue(), t.out,
          [("every literal 0..255 in the fixed code", lambda tr: tr["fixed_literals"] == set(range(256)))])
    t, w = Tokens(rng), BitWriter()
    t.rand(300)
    for ln in range(3, 259):
        t.copy(ln, rng.randint(1, min(len(t.out), 32768)))
    t.copy(258, 7, alt258=True)
    fixed_block(w, t.take(), True)
    _wrap("B_all_lengths", "gpu", w.getvalue(), t.out,
          [("every length", lambda tr: tr["lengths"] == set(range(3, 259))),
           ("every length symbol", lambda tr: tr["len_syms"] == set(range(257, 286))),
           ("every extra-bits boundary", lambda tr: all(
               (s + 257, 0) in tr["len_extra"] and (s + 257, (1 << LEN_EXTRA[s]) - 1) in tr["len_extra"]
               for s in range(29))),
           ("258 both ways", lambda tr: {(285, 0), (284, 31)} <= tr["len_extra"])])
    t, w = Tokens(rng), BitWriter()
    stored_block(w, head, False)
    t.out += head
    for s in range(30):
        t.copy(3 + s % 5, DIST_BASE[s])
        t.copy(4 + s % 3, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1)
    t.copy(5, 32767)
    fixed_block(w, t.take(), True)
    _wrap("B_all_distance_symbols", "gpu", w.getvalue(), t.out,
          [("every distance symbol at base and base + max", lambda tr: all(
              {(s, 0), (s, (1 << DIST_EXTRA[s]) - 1)} <= tr["dist_extra"] for s in range(30))),
           ("1, 24577, 32767, 32768", lambda tr: {1, 24577, 32767, 32768} <= tr["dists"])])

    # ---- C. dynamic codes ----------------------------------------------------------------
    t, w = Tokens(rng), BitWriter()
    t.rand(300, BLOB[100:130])
    for i in range(12):
        t.copy(3 + i, 129 + i * 10)
    toks = t.take()
    lits = sorted({x for x in toks if isinstance(x, int)}, key=lambda b: -toks.count(b))
    lsy = sorted({x[1] for x in toks if not isinstance(x, int)})
    ll = skew_lens([256] + lsy + lits, 286, 15)
    dl = skew_lens(list(range(14)) + [14, 15], 30, 15)
    assert ll[lits[-1]] == 15 and dl[14] == 15
    dynamic_block(w, toks, True, ll[:1 + max(s for s in range(286) if ll[s])], dl[:16])
    _wrap("C_len15_both_hclen19", "gpu", w.getvalue(), t.out,
          [("15-bit codes used in both alphabets", lambda tr: tr["used_len"] == dict(ll=15, d=15)),
           ("HCLEN = 19", lambda tr: tr["hclen"] == [19])])
    t, w = Tokens(rng), BitWriter()
    t.rand(40)
    for i in range(10):
        t.copy(3 + i, 1 + i % 2)
    toks = t.take()
    ll, _ = auto_lens(toks)
    dynamic_block(w, toks, True, ll, [1, 1])
    _wrap("C_two_distance_codes_1_1", "gpu", w.getvalue(), t.out,
          [("distance lengths 1, 1", lambda tr: tr["tables"][0][1] == (1, 1)),
           ("both used", lambda tr: tr["dist_syms"] == {0, 1})])
    t, w = Tokens(rng), BitWriter()
    t.lit(BLOB).lit(MID_TEXT).rand(400)
    for s in range(29):
        t.copy(LEN_BASE[s], rng.randint(1, 400))
    toks = t.take()
    ll, dl = auto_lens(toks)
    dynamic_block(w, toks, True, ll, dl)
    _wrap("C_all_286_symbols", "gpu", w.getvalue(), t.out,
          [("all 286 literal/length symbols coded and used", lambda tr: len(tr["tables"][0][0]) == 286 and all(
              tr["tables"][0][0]) and tr["literals"] == set(range(256)) and tr["len_syms"] == set(range(257, 286))),
           ("lengths not monotonic in the symbol", lambda tr: any(
               a > b for a, b in zip(tr["tables"][0][0], tr["tables"][0][0][1:])) and any(
               a < b for a, b in zip(tr["tables"][0][0], tr["tables"][0][0][1:])))])
    all286 = (toks, ll, dl, bytes(t.out))
    t, w = Tokens(rng), BitWriter()
    toks = t.rand(60).take()
    ll, _ = auto_lens(toks)
    dynamic_block(w, toks, True, ll, [1, 1])
    _wrap("C_hlit257_two_unused_distance_codes", "gpu", w.getvalue(), t.out,
          [("HLIT = 257", lambda tr: tr["hlit"] == [257]),
           ("two distance codes, unused", lambda tr: tr["tables"][0][1] == (1, 1) and not tr["dist_syms"])])
    t, w = Tokens(rng), BitWriter()
    t.rand(50)
    for i in range(6):
        t.copy(4, 3 + 7 * i)
    toks = t.take()
    ll, _ = auto_lens(toks)
    dynamic_block(w, toks, True, ll, [4, 4] + [5] * 28)
    _wrap("C_hdist30", "gpu", w.getvalue(), t.out, [("HDIST = 30", lambda tr: tr["hdist"] == [30])])
    # the code-length code: seven-bit codes, and the fewest lengths a decodable block can send.
    # HCLEN = 4 sends lengths for 16, 17, 18 and 0 only, so every code length is 0 and no block
    # with it is valid (F_hclen4); a complete distance code needs length 4 or shorter, and 4 is
    # the twelfth entry of the order
    t, w = Tokens(rng), BitWriter()
    t.rand(200, BLOB[:70])
    for i in range(8):
        t.copy(5 + i, 1 + 2 * i)
    toks = t.take()
    ll, dl = auto_lens(toks)
    ops = plan_cl(ll + dl)
    syms = sorted({o[0] for o in ops}, key=lambda s: -sum(1 for o in ops if o[0] == s))
    cl = skew_lens(syms, 19, 7)
    dynamic_block(w, toks, True, ll, dl, cl_ops=ops, cl_lens=cl)
    _wrap("C_code_length_code_of_7_bits", "gpu", w.getvalue(), t.out,
          [("code-length code 7 bits long", lambda tr: tr["max_len"]["cl"] == 7)])
    t, w = Tokens(rng), BitWriter()
    t.rand(300)
    t.copy(3, 5).copy(4, 16).copy(3, 9)
    toks = t.take()
    ll = [0] * 259  # 253 blob bytes + 256, 257, 258: 256 codes of 8 bits
    for b in list(BLOB) + [256, 257, 258]:
        ll[b] = 8
    assert kraft_left(ll) == 0
    dynamic_block(w, toks, True, ll, [4] * 16)
    _wrap("C_hclen12_fewest", "gpu", w.getvalue(), t.out,
          [("HCLEN = 12", lambda tr: tr["hclen"] == [12]),
           ("only lengths the first twelve can send", lambda tr: set(tr["tables"][0][0]) | set(
               tr["tables"][0][1]) <= {0, 8, 7, 9, 6, 10, 5, 11, 4})])
    # 16 x3 x6, 17 x3 x10, 18 x11 x138: 64 symbols of 6 bits placed so the runs come out so
    ll = [0] * 269
    for a, b in ((138, 145), (156, 160), (163, 164), (174, 213), (256, 269)):
        for s in range(a, b):
            ll[s] = 6
    assert kraft_left(ll) == 0
    t, w = Tokens(rng), BitWriter()
    t.rand(120, bytes(s for s in range(256) if ll[s]))
    for i in range(12):
        t.copy(LEN_BASE[i], 1 + i % 2)
    toks = t.take()
    dynamic_block(w, toks, True, ll, [1, 1])
    want = {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)}
    _wrap("C_repeat_counts_min_max", "gpu", w.getvalue(), t.out,
          [("16 x3 x6, 17 x3 x10, 18 x11 x138", lambda tr, want=want: want <= set(tr["cl_ops"]))])
    ll = [0] * 258
    for s in BLOB[40:72]:
        ll[s] = 6
    ll[256] = ll[257] = 2
    t, w = Tokens(rng), BitWriter()
    t.rand(50, BLOB[40:72])
    for i in range(4):
        t.copy(3, 1 + i)
    toks = t.take()
    dynamic_block(w, toks, True, ll, [2, 2, 2, 2])
    _wrap("C_repeat_16_crosses_into_distances", "gpu", w.getvalue(), t.out,
          [("a 16 runs from the literal/length lengths into the distance lengths",
            lambda tr: tr["cl_cross"] == [16]),
           ("and ends exactly at nlen + ndist", lambda tr: tr["cl_last_is_repeat"] == [True])])
    t, w = Tokens(rng), BitWriter()
    toks = t.rand(40).copy(5, 2).copy(6, 1).take()
    ll, _ = auto_lens(toks)
    dynamic_block(w, toks, True, ll, [1, 1, 0, 0, 0, 0, 0])
    _wrap("C_repeat_17_ends_at_total", "gpu", w.getvalue(), t.out,
          [("the last code length comes from a 17", lambda tr: tr["cl_ops"][-1] == (17, 5))])
    w = BitWriter()
    dynamic_block(w, all286[0], False, all286[1], all286[2])
    t = Tokens(rng)
    toks = t.rand(30, BLOB[200:204]).take()
    ll, _ = auto_lens(toks)
    dynamic_block(w, toks, True, ll, [1, 1])
    _wrap("C_two_dynamic_blocks_second_smaller", "gpu", w.getvalue(), all286[3] + t.out,
          [("two dynamic blocks", lambda tr: tr["blocks"] == ["dynamic", "dynamic"]),
           ("the second with fewer codes", lambda tr: sum(map(bool, tr["tables"][1][0])) <= 6 < 286 == sum(
               map(bool, tr["tables"][0][0])))])

    # ---- D. copies and history -----------------------------------------------------------
    def has_copy(**kw):
        def f(tr):
            return any(all(dict(pos=p, ln=l, dist=d, end=p + l, kind=k)[a] == b for a, b in kw.items())
                       for p, l, d, k in tr["copies"])
        return f

    t, w = Tokens(rng), BitWriter()
    fixed_block(w, t.rand(1).copy(258, 1).rand(2).take(), True)
    _wrap("D_distance_1_length_258", "gpu", w.getvalue(), t.out, [("d 1 l 258", has_copy(ln=258, dist=1))])
    t, w = Tokens(rng), BitWriter()
    fixed_block(w, t.rand(260).copy(258, 2).copy(100, 3).copy(258, 257).take(), True)
    _wrap("D_distance_below_length", "gpu", w.getvalue(), t.out,
          [("d 2", has_copy(ln=258, dist=2)), ("d 3", has_copy(ln=100, dist=3)), ("d 257", has_copy(ln=258, dist=257))])
    t, w = Tokens(rng), BitWriter()
    fixed_block(w, t.rand(10).copy(3, 10).rand(287).copy(258, 300).take(), True)
    _wrap("D_distance_equals_position", "gpu", w.getvalue(), t.out,
          [("at 10", has_copy(pos=10, dist=10)), ("at 300", has_copy(pos=300, dist=300, ln=258))])
    t, w = Tokens(rng), BitWriter()
    stored_block(w, big[:65278], False)
    t.out += big[:65278]
    fixed_block(w, t.copy(258, 31000).take(), True)
    _wrap("D_copy_ends_at_cap", "gpu", w.getvalue(), t.out,
          [("the copy's last byte is byte 65535 of 65536", has_copy(end=65536)),
           ("65536 bytes out", lambda tr: tr["out_len"] == [65536])])
    t, w = Tokens(rng), BitWriter()
    fixed_block(w, t.rand(30).take(), False)
    s40 = bytes(rng.choice(BLOB) for _ in range(40))
    stored_block(w, s40, False)
    t.out += s40
    toks = t.copy(12, 20).copy(12, 70).rand(6).take()
    ll, dl = auto_lens(toks)
    dynamic_block(w, toks, True, ll, dl)
    _wrap("D_sources_in_earlier_blocks", "gpu", w.getvalue(), t.out,
          [("fixed, stored, dynamic", lambda tr: tr["blocks"] == ["fixed", "stored", "dynamic"]),
           ("from the stored block", has_copy(pos=70, dist=20, kind="dynamic")),
           ("from the fixed block two back", has_copy(pos=82, dist=70, kind="dynamic"))])
    t, w = Tokens(rng), BitWriter()
    stored_block(w, head, False)
    t.out += head
    fixed_block(w, t.copy(9, 32768).rand(3).take(), True)
    _wrap("D_distance_32768_at_32768", "gpu", w.getvalue(), t.out, [("d 32768 at 32768", has_copy(pos=32768, dist=32768))])

    # ---- E. zlib accepts, the kernel declines by design ----------------------------------
    t, w = Tokens(rng), BitWriter()
    toks = t.rand(30).copy(20, 1).rand(5).copy(3, 1).take()
    ll, _ = auto_lens(toks)
    dynamic_block(w, toks, True, ll, [1])
    _wrap("E_one_distance_code_of_length_1", "declined", w.getvalue(), t.out,
          [("one distance code, used", lambda tr: tr["tables"][0][1] == (1,) and tr["dist_syms"] == {0})])
    t, w = Tokens(rng), BitWriter()
    toks = t.rand(60).take()
    ll, _ = auto_lens(toks)
    dynamic_block(w, toks, True, ll, [0])
    _wrap("E_no_distance_code", "declined", w.getvalue(), t.out,
          [("no distance code, literals only", lambda tr: tr["tables"][0][1] == (0,) and not tr["copies"])])
    # found while writing the reader: zlib's "max == 1" exception also admits a literal/length
    # code that is the end-of-block code alone (an empty dynamic block)
    t, w = Tokens(rng), BitWriter()
    fixed_block(w, t.rand(40).take(), False)
    ll = [0] * 257
    ll[256] = 1
    dynamic_block(w, [], True, ll, [1, 1])
    _wrap("E_end_of_block_code_alone", "declined", w.getvalue(), t.out,
          [("a literal/length code of one symbol", lambda tr: sum(tr["tables"][0][0]) == 1)])

    # ---- F. CPython rejects; the trailer is right for the intended payload ---------------
    def intended(n=40):
        return Tokens(rng).rand(n)

    def F(name, raw, payload, **header):
        _wrap("F_" + name, "error", raw, payload, **header)

    junk = bytes(rng.choice(BLOB) for _ in range(24))
    t, w = intended(), BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    w.align()
    w.raw(junk)
    F("block_type_3", w.getvalue(), t.out)
    t, w = intended(), BitWriter()  # type 3 with a body in the fixed code, the tables of the block before
    fixed_block(w, t.take(), False)
    w.bits(1, 1)
    w.bits(3, 2)
    emit_tokens(w, t.rand(10).copy(5, 3).take(), FIXED_LL, FIXED_D)
    F("block_type_3_after_fixed", w.getvalue(), t.out)
    t, w = intended(), BitWriter()
    stored_block(w, t.out, True, nlen_field=(len(t.out) ^ 0xFFFF) ^ 0x0100)
    F("nlen_not_complement", w.getvalue(), t.out)
    for extra in (1, 2):  # HLIT fields 30, 31; HDIST fields 30, 31
        t, w = intended(), BitWriter()
        toks = t.take()
        ll, dl = auto_lens(toks, n_ll=286)
        dynamic_block(w, toks, True, ll + [0] * extra, [1, 1])
        F("hlit_%d" % (29 + extra), w.getvalue(), t.out)
        t, w = intended(), BitWriter()
        toks = t.take()
        ll, _ = auto_lens(toks)
        dynamic_block(w, toks, True, ll, [1, 1] + [0] * (28 + extra))
        F("hdist_%d" % (29 + extra), w.getvalue(), t.out)
    # over-subscribed and incomplete codes.  The incomplete ones still carry the payload in the
    # codes they do define, so a decoder that skipped the completeness test would produce it
    t, w = intended(), BitWriter()
    cl = [0] * 19
    cl[0] = cl[8] = cl[7] = 1
    dynamic_block(w, [], True, [8] * 257, [1, 1], cl_lens=cl, stop_after_cl=True)
    w.align()
    w.raw(junk)
    F("oversubscribed_code_length_code", w.getvalue(), t.out)
    t, w = intended(), BitWriter()
    toks = t.take()
    ll, _ = auto_lens(toks)
    ops = plan_cl(ll + [1, 1])
    freq = {}
    for o in ops:
        freq[o[0]] = freq.get(o[0], 0) + 1
    cl = huffman_lens(freq, 19, 6)
    cl = [l + 1 if l else 0 for l in cl]  # every code one bit longer: half the code space unused
    dynamic_block(w, toks, True, ll, [1, 1], cl_ops=ops, cl_lens=cl)
    F("incomplete_code_length_code", w.getvalue(), t.out)
    for kind in ("oversubscribed", "incomplete"):
        t, w = intended(), BitWriter()
        toks = t.rand(20, BLOB[60:63]).take()
        ll = [0] * 257
        if kind == "incomplete":
            ll[BLOB[60]] = ll[BLOB[61]] = ll[BLOB[62]] = 3
            ll[256] = 2
            for b in sorted(set(x for x in toks if isinstance(x, int)) - set(BLOB[60:63])):
                ll[b] = 7
            assert kraft_left(ll) > 0
            dynamic_block(w, toks, True, ll, [1, 1])
        else:
            ll[BLOB[60]] = ll[BLOB[61]] = ll[256] = 1
            dynamic_block(w, [], True, ll, [1, 1], eob=False)
            w.align()
            w.raw(junk)
        F(kind + "_literal_length_code", w.getvalue(), t.out)
        t, w = intended(), BitWriter()
        toks = t.copy(5, 1).copy(4, 2).take()
        ll, _ = auto_lens(toks)
        if kind == "incomplete":
            dynamic_block(w, toks, True, ll, [2, 2, 2])
        else:
            dynamic_block(w, [], True, ll, [1, 1, 1], eob=False)
            w.align()
            w.raw(junk)
        F(kind + "_distance_code", w.getvalue(), t.out)
    t, w = intended(), BitWriter()
    toks = t.take()
    fl = {}
    for b in toks:
        fl[b] = fl.get(b, 0) + 1
    ll = huffman_lens(fl, 286, 15)[:257]
    assert ll[256] == 0
    dynamic_block(w, toks, True, ll, [1, 1], eob=False)
    w.align()
    w.raw(junk)
    F("no_end_of_block_code", w.getvalue(), t.out)
    t, w = intended(), BitWriter()
    toks = t.take()
    ll, _ = auto_lens(toks)
    ops = plan_cl(ll + [1, 1])
    dynamic_block(w, toks, True, ll, [1, 1], cl_ops=[(16, 3)] + ops)
    F("repeat_16_first", w.getvalue(), t.out)
    t, w = intended(), BitWriter()
    toks = t.take()
    ll, _ = auto_lens(toks)
    ops = plan_cl(ll + [1, 1, 0, 0, 0])
    assert ops[-1] == (17, 3)
    dynamic_block(w, toks, True, ll, [1, 1, 0, 0, 0], cl_ops=ops[:-1] + [(17, 4)])
    F("repeat_past_total", w.getvalue(), t.out)
    for s in (286, 287):
        t, w = intended(), BitWriter()
        fixed_block(w, t.take() + [("S", s)], True)
        F("length_symbol_%d" % s, w.getvalue(), t.out)
    for s in (30, 31):  # the payload a decoder would produce that read the unused code as symbol 0
        t, w = intended(), BitWriter()
        fixed_block(w, t.take() + [("M", 257, 0, s, 0)], True)
        F("distance_symbol_%d" % s, w.getvalue(), t.out + t.out[-1:] * 3)
    t, w = intended(10), BitWriter()
    fixed_block(w, t.take() + [mtok(3, 11)], True)
    F("distance_position_plus_1", w.getvalue(), t.out)
    t, w = intended(), BitWriter()
    fixed_block(w, t.take(), True)
    F("ends_inside_symbol", w.getvalue()[:20], t.out)  # 3 header bits: every 8-bit literal straddles
    t, w = intended(), BitWriter()
    t.rand(32768 - 40)
    t.copy(4, 30000)
    w.bits(1, 1)
    w.bits(1, 2)
    emit_tokens(w, t.toks[:-1], FIXED_LL, FIXED_D, eob=False)
    emit_tokens(w, [("S", 258)], FIXED_LL, FIXED_D, eob=False)
    w.code(29, 5)
    cut = w.bitpos // 8 + 1  # inside the 13 extra bits of distance symbol 29
    w.bits(30000 - 24577, 13)
    assert cut * 8 < w.bitpos
    emit_tokens(w, [], FIXED_LL, FIXED_D)
    F("ends_inside_extra_bits", w.getvalue()[:cut], t.out)
    t, w = intended(), BitWriter()
    stored_block(w, t.out, True)
    F("ends_inside_stored_block", w.getvalue()[:25], t.out)
    t, w = intended(), BitWriter()
    fixed_block(w, t.take() + [65], True)
    F("output_longer_than_isize", w.getvalue(), t.out)
    t, w = intended(), BitWriter()
    fixed_block(w, t.take()[:-1], True)
    F("output_shorter_than_isize", w.getvalue(), t.out)
    while True:  # four bytes short, and the trailer's CRC is also that of the shorter output
        t, w = intended(), BitWriter()
        x = crc_suffix(zlib.crc32(t.out), zlib.crc32(t.out))
        if not set(x) & {9, 10, 13}:
            break
    assert zlib.crc32(t.out + x) == zlib.crc32(t.out)
    fixed_block(w, t.take(), True)
    F("output_shorter_same_crc", w.getvalue(), t.out + x)
    t, w = intended(), BitWriter()  # the right length, one byte different
    toks = t.take()
    toks[7] = BLOB[(BLOB.index(bytes([toks[7]])) + 1) % len(BLOB)]
    fixed_block(w, toks, True)
    F("crc_mismatch_only", w.getvalue(), t.out)
    t, w = intended(), BitWriter()
    fixed_block(w, t.take(), True)
    F("spare_byte_before_trailer", w.getvalue() + b"\0", t.out)
    F("no_deflate_data", b"", intended().out)
    t, w = intended(65535), BitWriter()
    stored_block(w, t.out[:100], True, len_field=65535)
    F("len_65535_data_missing", w.getvalue(), t.out)
    t, w = intended(), BitWriter()
    cl = [0] * 19
    cl[0], cl[18] = 1, 1
    dynamic_block(w, [], True, [0] * 257, [0], cl_ops=[(18, 138), (18, 120)], cl_lens=cl, hclen=4, eob=False)
    w.align()
    w.raw(junk)
    F("hclen_4", w.getvalue(), t.out)

    # ---- G. lanes and member chains ------------------------------------------------------
    good = [c.members[1] for c in CASES if c.verdict == "gpu"]
    small = [m for m in good if len(m.raw) < 600]

    def chain(name, verdict, members, **kw):
        CASES.append(Case(name, verdict, members, **kw))

    chain("G_every_case_in_order", "gpu", [PRE] + good + [SUF])
    chain("G_every_case_reversed", "gpu", [PRE] + good[::-1] + [SUF])
    chain("G_every_case_rotated", "gpu", [PRE] + good[1:] + good[:1] + [SUF])
    t, w = Tokens(rng), BitWriter()
    fixed_block(w, t.lit(PRE_TEXT).rand(30).lit(SUF_TEXT).take(), True)
    chain("G_members_1", "gpu", [Member(w.getvalue(), t.out)], eof=False)
    for n in (63, 64, 65, 128, 129):
        chain("G_members_%d" % n, "gpu", [PRE] + [small[i % len(small)] for i in range(n - 2)] + [SUF], eof=False)
    chain("G_empty_members", "gpu", [EMPTY, PRE, small[0], EMPTY, EMPTY, small[1], SUF, EMPTY])

    def bad_nlen(payload):
        w = BitWriter()
        stored_block(w, payload, True, nlen_field=(len(payload) ^ 0xFFFF) ^ 1)
        return Member(w.getvalue(), payload)

    incomplete = next(c for c in CASES if c.name == "F_incomplete_literal_length_code").members[1]
    body = [small[i % len(small)] for i in range(127)]
    for at, members in ((0, [bad_nlen(PRE_TEXT)] + body + [SUF]),
                        (63, [PRE] + body[:62] + [incomplete] + body[62:126] + [SUF]),
                        (64, [PRE] + body[:63] + [incomplete] + body[63:126] + [SUF]),
                        (128, [PRE] + body + [bad_nlen(SUF_TEXT)])):
        assert len(members) == 129
        chain("G_bad_member_at_%d_of_129" % at, "error", members, eof=False)
    chain("G_empty_members_only", "host", [EMPTY, EMPTY, EMPTY], eof=False)

    # ---- H. the member locator -----------------------------------------------------------
    t, w = Tokens(rng), BitWriter()
    fixed_block(w, t.rand(50).copy(20, 7).take(), True)
    raw, pay = w.getvalue(), bytes(t.out)
    sub = b"XY" + struct.pack("<H", 3) + b"abc"
    _wrap("H_bc_after_another_subfield", "gpu", raw, pay, extra_before=sub)
    _wrap("H_bc_before_another_subfield", "gpu", raw, pay, extra_after=sub)
    _wrap("H_xlen_above_6", "gpu", raw, pay, extra_before=sub, extra_after=sub + sub)
    _wrap("H_two_bc_subfields", "gpu", raw, pay, extra_after=lambda total: b"BC" + struct.pack("<HH", 2, (total - 1) & 0xFFFF))
    _wrap("H_bc_with_slen_3", "host", raw, pay, bc_slen=3)
    _wrap("H_subfield_slen_past_xlen", "gpu", raw, pay, extra_after=b"ZZ" + struct.pack("<H", 100) + b"ab")
    w = BitWriter()
    stored_block(w, big[:65505], True)
    c = _wrap("H_largest_bsize", "gpu", w.getvalue(), big[:65505])
    assert len(c.members[1].bytes()) == 65536
    cap = next(c for c in CASES if c.name == "D_copy_ends_at_cap").members[1]
    _wrap("H_isize_65536", "gpu", cap.raw, cap.payload)
    t, w = Tokens(rng), BitWriter()
    t.rand(1)
    for _ in range(254):
        t.copy(258, 1)
    fixed_block(w, t.copy(4, 1).take(), True)
    assert len(t.out) == 65537
    _wrap("H_isize_65537", "host", w.getvalue(), t.out)
    _wrap("H_flg_with_fname", "host", raw, pay, flg=4 | 8, name=b"x.gfa\0")
    CASES.append(Case("H_zero_padding_after_eof", "host", [PRE, Member(raw, pay), SUF], tail=b"\0" * 5))


_build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
