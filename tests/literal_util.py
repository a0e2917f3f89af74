"""Weight-tag literals and what CPython makes of them: the corpus behind tests/test_literal_corpus.py
(CPU: the oracle and the host compile of pylit.h) and tests/test_gpu_weight_literals.py (the device
routes).

One `Lit` = the tag fields of one edge line, the weight tag to build with, and the weight the
reference gives the edge.  The rule, per tab-separated field after the record's fixed fields:

* the field is decoded as strict UTF-8; a field that does not decode is skipped;
* it is split on ":" at most twice; fewer than three parts: skipped;
* type "i" stores int(value), type "f" stores float(value) under the tag's name; a ValueError skips
  the field, so an earlier value of the same tag stays;
* any other type stores a value that is no number;
* the edge's weight is float(v) when the last value stored for the weight tag is an int or a float,
  1.0 otherwise; float(int) raising OverflowError fails the build at that line (`want` is None).

Expected values are CPython's own int() / float() on this interpreter, compared bit for bit.
The corpus is deterministic (random.Random with fixed seeds); classes A-G are the shapes at which a
piece of the device code (pylit.h fast_int / fast_float / the Decimal path, weight_fast,
k_weights_slow, lean_int_tag, k_parse_deferred) can still go wrong, class H the values at the edges
of numpy's casts to the other dtypes.
"""
from __future__ import annotations

import decimal
import functools
import math
import random
import struct
from dataclasses import dataclass

import numpy as np

WT = "RC"
WT_NAMES = ("W", "RC", "WEIGHT12", "WEIGHT123")  # 1, 2, 8 and 9 bytes (the extended lean parse takes <= 8)


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


def tag_weight(fields, wt: str):
    """The reference's weight for an edge line with these tag fields (bytes); raises OverflowError."""
    stored = None
    for f in fields:
        try:
            s = f.decode("utf-8")
        except UnicodeDecodeError:
            continue
        parts = s.split(":", 2)
        if len(parts) < 3:
            continue
        name, ty, value = parts
        if ty == "i":
            try:
                v = int(value)
            except ValueError:
                continue
        elif ty == "f":
            try:
                v = float(value)
            except ValueError:
                continue
        else:
            v = value
        if name == wt:
            stored = v
    if isinstance(stored, (int, float)):
        return float(stored)
    return 1.0


@dataclass(frozen=True)
class Lit:
    cls: str
    wt: str
    fields: tuple  # of bytes
    want: float | None  # None: float(int) overflows, the build fails at this line

    @property
    def bare(self):
        """(type, value bytes) when the line is one "<wt>:i|f:<value>" field, else None."""
        if len(self.fields) != 1:
            return None
        p = self.fields[0].split(b":", 2)
        if len(p) < 3 or p[0] != self.wt.encode() or p[1] not in (b"i", b"f"):
            return None
        return p[1].decode(), p[2]


def _enc(s) -> bytes:
    return s if isinstance(s, bytes) else s.encode("utf-8")


def _mk(cls: str, fields, wt: str = WT) -> Lit:
    fields = tuple(_enc(f) for f in fields)
    for f in fields:
        assert b"\t" not in f and b"\n" not in f, f
    try:
        want = tag_weight(fields, wt)
    except OverflowError:
        want = None
    return Lit(cls, wt, fields, want)


def _i(cls: str, s, wt: str = WT) -> Lit:
    return _mk(cls, [wt.encode() + b":i:" + _enc(s)], wt)


def _f(cls: str, s, wt: str = WT) -> Lit:
    return _mk(cls, [wt.encode() + b":f:" + _enc(s)], wt)


def _digits(r: random.Random, n: int, first_nonzero: bool = True) -> str:
    s = "".join(r.choice("0123456789") for _ in range(n))
    if first_nonzero and s[0] == "0":
        s = r.choice("123456789") + s[1:]
    return s


# ------------------------------------------------------------------ A: fast_int bounds
def _class_a():
    r = random.Random(101)
    out = []
    for nd in (1, 15, 16, 17):
        for sign in ("", "+", "-"):
            out.append(_i("A", sign + "9" * nd))
            out.append(_i("A", sign + "1" + "0" * (nd - 1)))
            for _ in range(6):
                out.append(_i("A", sign + _digits(r, nd)))
    for s in ("-0", "+0", "0", "007", "0" * 20 + "1", "-" + "0" * 14 + "7", "0" * 15, "0" * 16 + "9"):
        out.append(_i("A", s))
    for _ in range(150):
        out.append(_i("A", r.choice(["", "", "-", "+"]) + _digits(r, r.randint(1, 18), r.random() < 0.8)))
    return out


# ---------------------------------------------------------------- B: fast_float bounds
def _place(digs: str, p: int, e: int | None, r: random.Random) -> str:
    """digs with the decimal point after p digits, exponent e (None: no exponent field)."""
    m = digs[:p] + ("." + digs[p:] if p < len(digs) or r.random() < 0.3 else "")
    if e is None:
        return m
    return m + r.choice("eE") + (r.choice(["", "+"]) if e >= 0 else "") + str(e)


def _class_b():
    r = random.Random(102)
    out = []
    es = list(range(-23, 24))
    for k in range(2000):  # every effective exponent E = e - (fraction digits) in [-23, 23], ~42 times each
        digs = str(r.randrange(1, 10 ** 15))
        p = r.randint(0, len(digs))
        E = es[k % len(es)]
        e = E + (len(digs) - p)
        sign = r.choice(["", "", "-", "+"])
        out.append(_f("B", sign + _place(digs, p, None if e == 0 and r.random() < 0.5 else e, r)))
    for nd in (15, 16):  # the mantissa-digit bound; 16 digits above 2^53 do not fit a double
        for k in range(330):
            if nd == 16 and k % 3:
                digs = str(r.randrange(2 ** 53 + 1, 10 ** 16))
            else:
                digs = _digits(r, nd)
            p = r.randint(0, nd)
            E = r.choice(es)
            out.append(_f("B", r.choice(["", "-"]) + _place(digs, p, E + (nd - p), r)))
    for s in ("1e022", "1e0022", "1e22", "1e-022", "1e-0022", "1e+022", "1.5e0000", "1e000",
              "0e999", "0e9999", "-0e0", "-0.0", "0.0", "+0.0", ".5", "5.", "1.e5", ".", "1e", "e5", "+.e1", "-.5e1",
              "9007199254740993", "9007199254740993.0", "9007199254740992", "1e23", "1e-23", "8.41e21", "1e22",
              "123456789012345e22", "123456789012345e23", "1234567890123456e22", "123456789012345e-22",
              "123456789012345e-23", "0.000000000000001e37", "100000000000000e8", "000000000000000000001.5",
              "0.00000000000000000000000015", "1.5", "0.5", "0.1", "1.0000000000000002"):
        out.append(_f("B", s))
    return out


# --------------------------------------------------------------------- C: the slow path
def _exact_mid(x: float) -> decimal.Decimal:
    """The exact midpoint of x and the next double above it."""
    with decimal.localcontext() as ctx:
        ctx.prec = 2000
        return (decimal.Decimal(x) + decimal.Decimal(math.nextafter(x, math.inf))) / 2


def _class_c():
    r = random.Random(103)
    out = []
    for _ in range(1500):  # the recipe of test_host_headers.test_halfway_cases: 28-digit neighbours of a midpoint
        x = r.uniform(0, 1) * 2.0 ** r.randint(-1074, 1023)
        d = decimal.Decimal(x)
        half = (d + decimal.Decimal(math.nextafter(x, math.inf))) / 2
        for s in (str(half), str(half.next_plus()), str(half.next_minus())):
            out.append(_f("C", s))
    for _ in range(150):  # exact ties (every digit of the midpoint), both parities of the lower neighbour
        x = r.uniform(0.5, 1) * 2.0 ** r.randint(-60, 80)
        out.append(_f("C", str(_exact_mid(x))))
    for k in (1, 2, 3, 4, 5, 6, 7):  # integer ties above 2^53, as i and as f
        out.append(_i("C", str(2 ** 53 + 2 * k - 1)))
        out.append(_f("C", str(2 ** 53 + 2 * k - 1)))
        out.append(_i("C", str(2 ** 60 + (2 * k - 1) * 2 ** 7)))
        out.append(_i("C", "-" + str(2 ** 64 + (2 * k - 1) * 2 ** 11)))
    # subnormal ties, ~750 digits
    for x in (5e-324, 1e-323, 1.5e-323, 2.2250738585072009e-308, 2.2250738585072014e-308):
        out.append(_f("C", str(_exact_mid(x))))
    for _ in range(600):
        digs = _digits(r, r.randint(17, 40), False)
        p = r.randint(0, len(digs))
        out.append(_f("C", r.choice(["", "-"]) + digs[:p] + "." + digs[p:] + f"e{r.randint(-340, 320)}"))
    for s in ("4.9406564584124654e-324", "2.4703282292062327e-324", "2.4703282292062328e-324",
              "1.7976931348623158e308", "1.7976931348623159e308", "1e400", "-1e-400", "1e-400", "-1e400",
              "1e999999999999", "1e-999999999999", "-1e999999999999", "0e999999999999", "1e+99999999",
              "0." + "0" * 500 + "1e500", "1" * 400 + "e-390", "2.2250738585072011e-308", "1e309", "1e308",
              "17976931348623157" + "0" * 292, "17976931348623158" + "0" * 292 + ".5e0"):
        out.append(_f("C", s))
    # more than 800 significant digits, the first 800 exactly on a halfway point: the digits past the 800th
    # decide (all zero: the tie goes to even; one trailing 1: up), which only Decimal.trunc remembers
    for x in (1.0, 1.0 + 2.0 ** -52, 3.0, 0.1, 123456789.0, 5e-324, 1e-323, 6.02e23, 2.0 ** -1022):
        mid = _exact_mid(x)
        sign, dg, ex = mid.as_tuple()
        nd = len(dg)
        assert nd <= 800, nd
        body = "".join(map(str, dg)) + "0" * (800 - nd)  # 800 significant digits, value = body * 10^(ex - (800 - nd))
        e10 = ex - (800 - nd)
        up = math.nextafter(x, math.inf)
        even = x if struct.unpack("<Q", bits(x))[0] % 2 == 0 else up
        for tail in ("0" * 25, "0" * 24 + "1", "0" * 120 + "1", "1"):
            digs = body + tail  # value = digs * 10^(e10 - len(tail))
            lit = _f("C", f"{digs[0]}.{digs[1:]}e{e10 + 800 - 1}")
            assert bits(lit.want) == bits(up if "1" in tail else even), (x, tail)
            out.append(lit)
    big = _digits(r, 5000)
    out.append(_f("C", big[:1] + "." + big[1:] + "e-4700"))
    out.append(_f("C", big))  # 5000 digits: inf
    out.append(_i("C", big))  # over the 4300-digit limit: ValueError, not overflow
    out.append(_mk("C", ["RC:i:7", "RC:i:" + big]))  # ... which leaves the earlier value
    return out


# -------------------------------------------------------------------------- D: grammar
def _class_d():
    out = []
    lits = ["1_0.2_5e-1", "1__0", "_1", "1_", "1_e5", "1e1_0", "1_0", "1_000_000", "1e_5", "1._5", "1_.5", "+_5",
            " 7", "7 ", " 7 ", "  12  ", "\x0b12\x0c", "\x0c1.5\x0b", "\x1c1", "1\x1c", "\x1d2", "1\x1f", "12\r", " ",
            "", "٣٤", "１２.5", "１２", "1.25　", "　7", " 9", "1\x85", " 3", "٣.٥e٢", "۱۲۳", "१२",
            "inf", "-Infinity", "nan", "-nan", "NaN", "nAn ", "in_f", "infinit", "+inf", "INFINITY", " -INF ",
            "infinityx", "nan0", "-iNf", "i", "na",
            "1\x00", "1\x002", "\x001", "0x10", "1 2", "- 5", "--5", "+-5", "5-", "1e5", "1.0", "1e+", "1ee5", "1.2.3",
            "é", "1é", "5:6", ":5", "5:", "1,2", "½", "²", "Ⅷ", "1e٥"]
    for s in lits:
        out.append(_i("D", s))
        out.append(_f("D", s))
    # a field with a byte >= 0x80 that is not UTF-8: the field is skipped (overlong, surrogate, lone bytes)
    for bad in (b"RC:i:5\xff", b"RC:f:1.5\xc3", b"RC:i:\xc0\xb1", b"RC:i:\xed\xa0\x80", b"RC:f:\xf5\x80\x80\x802",
                b"RC\x80:i:5", b"RC:i:\x80"):
        out.append(_mk("D", [bad]))
        out.append(_mk("D", [b"RC:i:3", bad]))  # the earlier value stays
        out.append(_mk("D", [bad, b"RC:f:2.5"]))
    out.append(_mk("D", [b"XX:Z:\xff\xfe", b"RC:i:4"]))  # another tag's bad field does not matter
    out.append(_mk("D", ["XX:Z:é日本", "RC:f:0.25"]))  # non-ASCII in another tag: still this line's value
    out.append(_mk("D", ["RC:i:5\r"]))  # (the last field of a CRLF line keeps its CR: whitespace to int())
    out.append(_mk("D", ["RC:f:5.5\r"]))
    return out


# --------------------------------------------------------------------- E: tag selection
def _class_e():
    out = []
    for fields in (["RC:i:2", "RC:i:3"], ["RC:i:2", "RC:f:3.5"], ["RC:f:2.5", "RC:i:3"], ["RC:i:2", "RC:i:x"],
                   ["RC:i:2", "RC:f:1e"], ["RC:f:2.5", "RC:i:1.0"], ["RC:i:2", "RC:Z:3"], ["RC:Z:3", "RC:f:4.5"],
                   ["RC:i:2", "RC:B:1,2"], ["RC:B:1,2"], ["RC:Z:7"], ["RC:A:7"], ["RC:ii:7"], ["RC::7"], ["RC:I:7"],
                   ["RC:i:2", "RC:ii:7"], ["RC:i"], ["RC"], ["RC:"], ["RC::3"], ["RC:i:5:6"], ["RC:i:2", "RC:i"],
                   ["RC:i:2", "RC:i:5:6"], ["RC:Z:x", "RC:i"], ["rc:i:5"], ["Rc:i:5"], ["RC:i:2", "rc:i:5"],
                   ["RCX:i:5"], ["R:i:5"], ["RC:i:2", "RCX:i:5"], ["XRC:i:5"], [":i:5"], ["::5"], ["::"], [""],
                   ["XX:i:9", "RC:i:2"], ["RC:i:2", "XX:i:9"], ["XX:i:bad", "RC:i:2"], ["RC:i:2", "XX:f:bad"],
                   ["RC:i:1", "RC:i:2", "RC:i:3", "RC:i:4"], ["RC:i:1", "RC:i:99999999999999999999"],
                   ["RC:i:99999999999999999999", "RC:i:1"], ["RC:f:1e400", "RC:i:1"], ["RC:i:1", "RC:f:nan"],
                   ["RC:i:" + "9" * 400, "RC:i:1"],  # an overflowing int that a later value replaces: no error
                   ["RC:i:" + "9" * 400, "RC:Z:1"], ["RC:i:" + "9" * 400, "RC:i:zz"],  # (the last one: still overflow)
                   ["RC:f:2.5", "RC:f:2.5x", "XX:Z:q"], ["XX:Z:q", "YY:i:1", "ZZ:f:2", "RC:f:0.125"], []):
        out.append(_mk("E", fields))
    for wt in WT_NAMES:
        for fields in ([f"{wt}:i:5"], [f"{wt}:i:-999999999"], [f"{wt}:f:1.5"], [f"{wt}:i:+5"], [f"{wt}X:i:5"],
                       [f"{wt[:-1]}:i:5"], [f"{wt}:i:2", f"{wt}:i:3"], [f"{wt}:i:2", f"{wt}:Z:3"],
                       [f"{wt.lower()}:i:5"], [f"{wt}:i:12345678901234567890"], [f"{wt}:f:9007199254740993"], []):
            out.append(_mk("E", fields, wt))
    return out


# -------------------------------------------------------------------------- F: integers
DBL_MAX_INT = 2 ** 1024 - 2 ** 970  # DBL_MAX; ints from 2^1024 - 2^969 (the tie to 2^1024) on overflow


def _class_f():
    out = []
    edge = 2 ** 1024 - 2 ** 969
    for v in (10 ** 307, 10 ** 308 - 1, 10 ** 308, DBL_MAX_INT - 1, DBL_MAX_INT, DBL_MAX_INT + 1, edge - 2 ** 60,
              edge - 1, edge, edge + 1, 2 ** 1024, 10 ** 309 - 1, -(edge - 1), -edge, 2 ** 1023,
              2 ** 1023 + 2 ** 970, 2 ** 1023 + 2 ** 970 + 1):
        out.append(_i("F", str(v)))
    out.append(_i("F", "1" * 4300))  # the longest int() takes: a valid int, far too large for a float
    out.append(_i("F", "1" * 4301))  # one more digit: ValueError, so no value and no error
    out.append(_i("F", "0" * 4299 + "7"))
    out.append(_i("F", "0" * 4300 + "7"))
    for s in ("٣٤", "٣" * 16, "-٩٩٩", "٣" * 310, "1٣", "۹" * 309):
        out.append(_i("F", s))
    out.append(_i("F", "1_" * 320 + "1"))  # 321 digits with underscores: overflow
    out.append(_i("F", " " + "9" * 309 + " "))
    return out


# --------------------------------------------------------- G: lean_int_tag's canonical spellings
G_CANONICAL = ["0", "1", "7", "9", "-1", "-9", "10", "123456789", "100000000", "999999999", "-999999999", "-100000000",
               "16777216", "16777217", "-16777217", "33554433", "2147483", "99999999", "-12345678", "-0"]
G_OTHER = ["00", "+5", "5 ", " 5", "1000000000", "9999999999", "-1000000000", "01", "-01", "1_0", "", "-", "5x",
           "2147483648", "٣"]


def _class_g():
    return [_i("G", s) for s in G_CANONICAL + G_OTHER]


# ------------------------------------------------------- H: values at the edges of the dtype casts
def _class_h():
    out = []
    for s in ("3.4028235e38", "3.4028236e38", "3.4028235677973366e38", "3.4028235677973362e38", "1e39", "-1e39",
              "-3.4028236e38", "1e300", "-1e300", "1.7976931348623157e308",
              # decimal -> double lands exactly on a float32 tie that the decimal itself is not on
              "1.00000005960464477539062500001", "1.00000017881393432617187499999", "1.000000059604644775390625",
              "1.000000178813934326171875", "16777217.0000000001", "16777219", "33554434.00000000001",
              # float32 subnormals
              "1e-40", "1.4e-45", "7e-46", "7.006492321624085e-46", "7.0064923216240854e-46", "1.1754942e-38",
              "1.17549435e-38", "-1e-45", "1e-46", "5.877471754111438e-39",
              "0.5", "-0.5", "0.999999", "-0.9", "127.9", "128.0", "-128.9", "-129.0", "2147483647.9", "2147483648.0",
              "-2147483648.9", "-2147483649.0", "255.5", "1e10", "inf", "-inf", "nan", "-0.0", "1e-320"):
        out.append(_f("H", s))
    for s in ("127", "128", "-128", "-129", "255", "256", "2147483647", "2147483648", "-2147483648", "-2147483649",
              "4294967296", "16777217", "9007199254740993"):
        out.append(_i("H", s))
    return out


@functools.lru_cache(maxsize=None)
def corpus() -> tuple:
    """Every literal, in a fixed order."""
    out = _class_a() + _class_b() + _class_c() + _class_d() + _class_e() + _class_f() + _class_g() + _class_h()
    return tuple(out)


def values(wt: str = WT, cls: str | None = None) -> list:
    """The literals of one weight tag that give a value (no build error), in corpus order."""
    return [x for x in corpus() if x.wt == wt and x.want is not None and (cls is None or x.cls == cls)]


def overflowing() -> list:
    return [x for x in corpus() if x.want is None]


# ------------------------------------------------------------------------------ files
N_NAMES = 61


def hash_line(k: int, lit: Lit) -> bytes:
    """Edge line k with names that are no decimal ids (no S lines: the hash dictionary tiers)."""
    a, b = k % N_NAMES, (k * 7 + 1) % N_NAMES
    if a == b:
        b = (b + 1) % N_NAMES
    return b"\t".join((b"L", b"s%d" % a, b"+", b"t%d" % b, b"-", b"*") + lit.fields) + b"\n"


def hash_file(lits) -> bytes:
    return b"".join(hash_line(k, x) for k, x in enumerate(lits))


def decimal_line(k: int, lit: Lit, n_s: int = N_NAMES) -> bytes:
    a, b = 1 + k % n_s, 1 + (k * 7 + 1) % n_s
    if a == b:
        b = 1 + b % n_s
    return b"\t".join((b"L", b"%d" % a, b"+", b"%d" % b, b"-", b"0M") + lit.fields) + b"\n"


def decimal_head(n_s: int = N_NAMES) -> bytes:
    return b"".join(b"S\t%d\t*\n" % k for k in range(1, n_s + 1))


def decimal_file(lits, n_s: int = N_NAMES) -> bytes:
    """S lines "1".."n_s" in order, then one L line per literal over those ids (the decimal-id tiers)."""
    return decimal_head(n_s) + b"".join(decimal_line(k, x, n_s) for k, x in enumerate(lits))


def chunks(lits, limit: int = 900_000):
    """lits split in order into runs whose files stay under `limit` bytes."""
    out, cur, size = [], [], 0
    for x in lits:
        n = 40 + sum(len(f) + 1 for f in x.fields)
        if cur and size + n > limit:
            out.append(cur)
            cur, size = [], 0
        cur.append(x)
        size += n
    if cur:
        out.append(cur)
    return out


def want_array(lits) -> np.ndarray:
    return np.array([x.want for x in lits], dtype=np.float64)


def same_bits(got: np.ndarray, lits) -> list:
    """Indices at which got (float64, one per literal) differs from the expectation, bit for bit."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = want_array(lits)
    if got.shape != want.shape:
        return [("shape", got.shape, want.shape)]
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    return [(int(k), lits[k].fields, float(got[k]), lits[k].want) for k in bad[:5]]


@functools.lru_cache(maxsize=None)
def _castable(dtype: str, wbits: bytes) -> bool:
    from oracle import oracle

    w = struct.unpack("<d", wbits)[0]
    text = repr(w).encode() if w == w else (b"-nan" if wbits[7] & 0x80 else b"nan")
    line = b"L\ta\t+\tb\t-\t*\tRC:f:" + text + b"\n"
    o = oracle.run(line, directed=False, dtype=dtype, weight_tag=WT)
    assert o.status != 0 or bits(float(o.weights[0])) == wbits, (w, o.weights)
    return o.status == 0


def cpu_cast_subset(dtype: str, wt: str = WT) -> list:
    """The value literals whose weight the oracle casts to `dtype` without an error (the oracle's
    cast of the float64 weight decides, one run per distinct weight), in corpus order."""
    return [x for x in values(wt) if _castable(np.dtype(dtype).name, bits(x.want))]
