"""Which rung every build takes (needs a GPU): a fixed matrix of tiny builds through the native entry
points, each reported as [status, n_nodes, nnz, format, the phase names in order] — the record of the
path run_build chose (front-end tier, dictionary tier, names branch, values or triplets, output stage,
the no-group retry).  tests/test_gpu_build_phases.py compares every group with
tests/golden/expected/build_phases.json, this tool's output at the commit before the driver was split
into stages.

Groups (one test parameter each):
* route-<name>: every plain .gfa of tests/golden/inputs x test_gpu_diff.MODES x float64 / int8 under the
  route's test flags, without a weight tag and with RC;
* partition-decline: the partition_util cases made to send the bucket partition to the row sums, as
  decimal-id GFAs with their RC tag, output COO and CSR (the no-group retry);
* callers: the entry points that set a context flag around the build (edge list, graph JSON, stats, the
  graph's weighted CSR, sequence distance), each on a golden input of its own;
* decimal-range: syn3k cut at one line boundary, each range as shard.py builds it (the offset evidence,
  evidence + group slots without values, a known s_base).

    python tools/build_phases.py > tests/golden/expected/build_phases.json
"""
import ctypes
import gzip
import json
import pathlib
import re
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from gfa2network_amd import _native as nat  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
DTYPES = ("float64", "int8")
TAGS = (None, "RC")
ROUTES = {
    "0": 0,
    "no_group": nat.TEST_NO_GROUP,
    "no_tile_local": nat.TEST_NO_TILE_LOCAL,
    "no_ext_lean": nat.TEST_NO_EXT_LEAN,
    "no_lean": nat.TEST_NO_LEAN,
    "no_dec_prefix": nat.TEST_NO_DEC_PREFIX,
    "dict_direct": nat.TEST_DICT_DIRECT,
    "dict_hash": nat.TEST_DICT_HASH,
    "dict_hash_no_hash_lean": nat.TEST_DICT_HASH | nat.TEST_NO_HASH_LEAN,
    "dict_general": nat.TEST_DICT_GENERAL,
    "no_buckets": nat.TEST_NO_BUCKETS,
}
GROUPS = [f"route-{r}" for r in ROUTES] + ["partition-decline", "callers", "decimal-range"]
FORMATS = {nat.FMT_COO: "coo", nat.FMT_CSR: "csr", nat.FMT_TEXT: "text"}


def _record(rc, r):
    """[status, n_nodes, nnz, format, phases] of one g2n_result (None: the call threw before it had one)."""
    if r is None:
        return [rc, None, None, None, []]
    return [rc, r.n_nodes, r.nnz, FORMATS.get(r.format, r.format),
            [r.phase_names[k].decode() for k in range(r.n_phases)]]


def build(data: bytes, **kw):
    """One g2n_build_from_buffer."""
    lib = nat.load()
    arr = np.frombuffer(data, dtype=np.uint8)
    opts = nat.make_options(**kw)
    res = ctypes.POINTER(nat.Result)()
    rc = lib.g2n_build_from_buffer(arr.ctypes.data if arr.size else None, arr.size, ctypes.byref(opts), ctypes.byref(res))
    rec = _record(rc, res.contents if res else None)
    if res:
        lib.g2n_result_free(res)
    return rec


def from_path(call):
    """One of _native's *_from_path wrappers, its result recorded before the wrapper turns it into a
    RawResult (whose phase_ms sums repeated phases)."""
    seen = []
    wrapped = nat._from_result

    def spy(ptr, rc):
        seen.append(_record(rc, ptr.contents if ptr else None))
        return wrapped(ptr, rc)

    nat._from_result = spy
    try:
        call()
    except RuntimeError as exc:  # (a call that returned no result)
        seen.append([str(exc).split(":")[0], None, None, None, []])
    finally:
        nat._from_result = wrapped
    return seen[0]


def golden_inputs():
    return sorted(p for p in (GOLDEN / "inputs").iterdir() if p.name.endswith(".gfa"))


def route_group(flags: int) -> dict:
    from test_gpu_diff import MODES

    out = {}
    for path in golden_inputs():
        data = path.read_bytes()
        out[path.name] = [build(data, test_flags=flags, dtype=dt, weight_tag=wt, **mode)
                          for mode in MODES for dt in DTYPES for wt in TAGS]
    return out


def decline_cases():
    """The partition_util cases whose premise fails (a bucket past kSymCap, a value or a run the exact-int32
    sums cannot hold), weighted."""
    import partition_util as P

    for kind, count in P.D_KINDS:
        if count in (P.SYM_CAP, P.SYM_CAP // 2):
            continue
        for where in P.D_WHERE:
            for dtype in P.DTYPES:
                yield P.capacity_case(kind, count, where, dtype, False)
    for kind, (dtypes, _runs, fails) in P.E_KINDS.items():
        if fails is not None:
            for dtype in dtypes:
                yield P.arith_case(kind, dtype)


def render(case) -> bytes:
    """The case as a decimal-id GFA; integer weights as RC:i tags (the parse's own codes), others as RC:f."""
    import rowsum_util as U

    return re.sub(rb"RC:f:(-?\d+)\.0\n", rb"RC:i:\1\n", U.render_gfa(case, U.text_floats(case)))


def partition_group() -> dict:
    import partition_util as P

    out = {}
    for case in decline_cases():
        assert not P.expect_buckets(case), case.name
        data = render(case)
        out[case.name] = [build(data, output=output, dtype=case.dtype, weight_tag="RC", **mode)
                          for mode in ({"asymmetric": True}, {"directed": False})
                          for output in (nat.OUT_COO, nat.OUT_CSR)]
    return out


def callers_group() -> dict:
    inputs = GOLDEN / "inputs"
    syn3k = gzip.decompress((inputs / "syn3k.gfa.gz").read_bytes())
    out = {}
    for name, data in (("sample.gfa", (inputs / "sample.gfa").read_bytes()), ("syn3k", syn3k)):
        out[f"edge_list {name}"] = [build(data, bidirected=bidir, output=nat.OUT_EDGE_LIST, test_flags=flags)
                                    for bidir in (False, True) for flags in (0, nat.TEST_NO_DEC_TEXT)]
        out[f"graph_json {name}"] = [build(data, bidirected=bidir, keep_directed_bidir=keep, want_node_names=names,
                                           output=nat.OUT_GRAPH_JSON)
                                     for bidir, keep in ((False, False), (True, False), (True, True))
                                     for names in (True, False)]
    stats_in = [inputs / "DRB1-3123_unsorted.gfa", inputs / "sx.gfa", GOLDEN / "stats_inputs" / "paths_walks.gfa"]
    for path in stats_in:
        out[f"stats {path.name}"] = [
            from_path(lambda: nat.stats_from_path(str(path), nat.make_options(
                directed=directed, strip_orientation=strip, asymmetric=True, output=nat.OUT_CSR, want_node_names=names)))
            for directed in (True, False) for strip in (False, True) for names in (True, False)]
    for path in (GOLDEN / "wdist_inputs" / "tag_then_none.gfa", inputs / "neg_weights.gfa", inputs / "sx.gfa"):
        out[f"graph_weights {path.name}"] = [
            from_path(lambda: nat.graph_weights_from_path(str(path), nat.make_options(
                directed=directed, weight_tag="RC", want_node_names=names)))
            for directed in (True, False) for names in (True, False)]
    path = GOLDEN / "seq_inputs" / "shared_seq.gfa"
    out[f"seq_distance {path.name}"] = [
        from_path(lambda: nat.seq_distance_from_path(str(path), nat.make_options(
            directed=directed, asymmetric=True, output=nat.OUT_CSR, want_node_names=True, weight_tag=wt),
            b"A", b"C", weighted=bool(wt)))
        for directed in (True, False) for wt in (None, "RC")]
    return out


def range_group() -> dict:
    from gfa2network_amd.shard import HipEngine, line_ranges

    data = gzip.decompress((GOLDEN / "inputs" / "syn3k.gfa.gz").read_bytes())
    n_seg = sum(1 for ln in data.split(b"\n") if ln.startswith(b"S\t"))
    eng = HipEngine(0, torch_buffers=False)
    lib = eng.lib
    out = {}
    try:
        ctx = eng._build_ctx()
        for r, (lo, hi) in enumerate(line_ranges(data, 2)):
            s_base = sum(1 for ln in data[:lo].split(b"\n") if ln.startswith(b"S\t"))
            buf = eng.upload(np.frombuffer(data[lo:hi], dtype=np.uint8))
            recs = []
            for mode in ({}, {"directed": False}):
                for flags in (0, nat.RANGE_NO_VALUES | nat.RANGE_SLOTS):  # (the entry point adds DECIMAL | EVIDENCE)
                    o = nat.make_options(output=nat.OUT_COO, want_node_names=False, **mode)
                    o.range_flags = flags
                    res, ev = nat.Result(), (ctypes.c_int64 * 6)()
                    rc = lib.g2n_build_decimal_range(ctx, buf.data_ptr(), buf.numel(), ctypes.byref(o), ev,
                                                     ctypes.byref(res))
                    recs.append(_record(rc, res))
                o = nat.make_options(output=nat.OUT_COO, want_node_names=False, **mode)
                o.range_s_base, o.range_n_segments, o.range_flags = s_base, n_seg, nat.RANGE_DECIMAL
                res = nat.Result()
                rc = lib.g2n_build_device(ctx, buf.data_ptr(), buf.numel(), ctypes.byref(o), ctypes.byref(res))
                recs.append(_record(rc, res))
            out[f"range {r}"] = recs
    finally:
        eng.close()
    return out


def run_group(name: str) -> dict:
    """{case: [record, ...]} of one group, the records in the group's fixed order."""
    if name.startswith("route-"):
        return route_group(ROUTES[name[len("route-"):]])
    return {"partition-decline": partition_group, "callers": callers_group, "decimal-range": range_group}[name]()


def pack(groups: dict) -> dict:
    """Distinct records once (most builds of a group share one), the cases as indices into them."""
    records, index = [], {}

    def ref(rec):
        key = json.dumps(rec)
        if key not in index:
            index[key] = len(records)
            records.append(rec)
        return index[key]

    cases = {g: {case: [ref(rec) for rec in recs] for case, recs in by_case.items()} for g, by_case in groups.items()}
    return {"records": records, "cases": cases}


def unpack(doc: dict, group: str) -> dict:
    return {case: [doc["records"][i] for i in idx] for case, idx in doc["cases"][group].items()}


def main():
    doc = pack({g: run_group(g) for g in (sys.argv[1:] or GROUPS)})
    lines = ['{"records": [', ",\n".join(json.dumps(r) for r in doc["records"]), '], "cases": {']
    lines.append(",\n".join(f"{json.dumps(g)}: {{\n" + ",\n".join(f"{json.dumps(c)}: {json.dumps(i)}"
                                                                 for c, i in by_case.items()) + "}"
                            for g, by_case in doc["cases"].items()))
    lines.append("}}")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
