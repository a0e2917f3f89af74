"""CPU: the weight-literal corpus (tests/literal_util.py) against the two references the GPU tests lean
on: the oracle's `weights` for the same bytes, and the host compile of pylit.h on the bare literals.
Every literal is checked, bit for bit; none is excluded.
"""
import ctypes
from collections import Counter

import literal_util as LU
from test_host_headers import hc  # noqa: F401  (the compiled tests/native/hostcheck.cpp)


def test_corpus_shape():
    lits = LU.corpus()
    assert 6000 <= len(lits) <= 10000, len(lits)
    n = Counter(x.cls for x in lits)
    assert set(n) == set("ABCDEFGH"), n
    assert len(LU.overflowing()) >= 8
    for wt in LU.WT_NAMES:
        for part in LU.chunks(LU.values(wt)):
            assert len(LU.hash_file(part)) < 1_000_000 and len(LU.decimal_file(part)) < 1_000_000
    key = lambda t: [(x.cls, x.wt, x.fields, None if x.want is None else LU.bits(x.want)) for x in t]  # noqa: E731
    assert key(lits) == key(LU.corpus.__wrapped__())  # deterministic


def test_corpus_against_oracle_and_host_pylit(oracle_lib, hc):  # noqa: F811
    bad = []
    for wt in LU.WT_NAMES:
        for part in LU.chunks(LU.values(wt)):
            for make in (LU.hash_file, LU.decimal_file):
                o = oracle_lib.run(make(part), directed=False, weight_tag=wt)
                assert o.status == 0, (wt, o.status, o.err_line)
                bad += LU.same_bits(o.weights[::2], part)
    for x in LU.overflowing():  # the build error G2N_E_INT_TOO_LARGE (9) at the literal's line
        before = LU.values(x.wt)[:3]
        data = LU.hash_file(before + [x] + before)
        o = oracle_lib.run(data, directed=False, weight_tag=x.wt)
        if (o.status, o.err_line) != (9, len(before)):
            bad.append((x.fields[0][:40], o.status, o.err_line))
    over, plain = LU.overflowing(), LU.values()[:3]
    two = plain + [over[3]] + plain * 5 + [over[0]] + plain  # two overflowing lines: the lower one is reported
    for lits in (two, two[::-1]):
        o = oracle_lib.run(LU.hash_file(lits), directed=False, weight_tag=LU.WT)
        if (o.status, o.err_line) != (9, min(k for k, x in enumerate(lits) if x.want is None)):
            bad.append(("two", o.status, o.err_line))
    assert not bad, bad[:5]

    n_bare = 0
    for x in LU.corpus():
        if x.bare is None:
            continue
        ty, val = x.bare
        n_bare += 1
        out = ctypes.c_double()
        if ty == "f":
            r = hc.hc_py_float(val, len(val), ctypes.byref(out))
        else:
            r = hc.hc_py_int(val, len(val), 1, ctypes.byref(out))
        # a literal neither int() nor float() takes leaves the weight at 1.0 (there is no earlier value)
        try:
            (int if ty == "i" else float)(val.decode("utf-8"))
            valid = True
        except (UnicodeDecodeError, ValueError):
            valid = False
        if x.want is None:
            ok = r == 2
        elif not valid:
            ok = r == 0 and x.want == 1.0
        else:
            ok = r == 1 and LU.bits(out.value) == LU.bits(x.want)
        if not ok:
            bad.append((ty, val[:40], r, out.value, x.want))
    assert n_bare > 6000 and not bad, (n_bare, bad[:5])


def test_cast_subsets_keep_the_float32_edges(oracle_lib):
    """cpu_cast_subset: the oracle's cast decides; float32's overflow, double-rounding and subnormal cases
    stay in, and the integer dtypes lose exactly the values numpy refuses."""
    f32 = {x.bare[1] for x in LU.cpu_cast_subset("float32") if x.bare and x.bare[0] == "f"}
    for s in (b"3.4028235e38", b"3.4028236e38", b"3.4028235677973366e38", b"1e39", b"1.00000005960464477539062500001",
              b"1e-40", b"1.4e-45", b"7e-46", b"nan", b"inf"):
        assert s in f32, s
    assert len(LU.cpu_cast_subset("float32")) == len(LU.values()) == len(LU.cpu_cast_subset("bool"))
    i8 = {x.bare[1] for x in LU.cpu_cast_subset("int8") if x.cls == "H"}
    i32 = {x.bare[1] for x in LU.cpu_cast_subset("int32") if x.cls == "H"}
    assert {b"127", b"-128", b"127.9", b"-128.9", b"0.5", b"-0.0"} <= i8
    assert not {b"128", b"-129", b"nan", b"inf", b"128.0"} & i8
    assert {b"2147483647", b"-2147483648", b"2147483647.9", b"128"} <= i32
    assert not {b"2147483648", b"-2147483649", b"1e300", b"-inf", b"2147483648.0"} & i32
