"""GPU: the BGZF inflate kernel (g2n_inflate.hip, k_inflate_members) on deflate streams zlib never
writes: the catalogue of tests/deflate_util.py (test_deflate_cases.py shows on the CPU that each
file is what it claims, against zlib and gzip).

The kernel is reached as in production, g2n_build_from_path on a ``.gz`` that the member locator
recognises.  It checks every member's CRC and length itself, so "the gz_inflate phase is present
and the build equals the plain file's" means every member's bytes were right; a wrong decode is
quiet (the file goes to the host reader), so the phase is asserted per case:

  gpu       inflated on the device: phase present
  declined  zlib accepts, the kernel hands the file to the host by design: absent
  host      the member locator declines the file: absent
  error     CPython raises: absent, and the exception is gzip.open's, type and message

Every comparison is byte for byte; the same build is repeated with the host readers forced
(TEST_HOST_INFLATE)."""
import gzip
import zlib

import pytest

import deflate_util as du

pytestmark = pytest.mark.gpu
MODES = ({}, {"directed": False})


def _key(res):
    A, nodes = res
    arrs = (A.indptr, A.indices, A.data) if A.format == "csr" else (A.row, A.col, A.data)
    return (A.format, A.shape, str(A.dtype), tuple(a.tobytes() for a in arrs), nodes)


def _outcome(path, mode):
    from gfa2network_amd import parse_gfa

    try:
        return ("ok", _key(parse_gfa(path, build_graph=False, build_matrix=True, return_node_list=True,
                                     raw_bytes_id=True, **mode)))
    except Exception as e:  # noqa: BLE001
        return ("exc", type(e), str(e).replace(str(path), "<path>"))


def _gzip_outcome(path):
    try:
        for _ in gzip.open(path):
            pass
        return None
    except (gzip.BadGzipFile, EOFError, zlib.error) as e:
        return ("exc", type(e), str(e))


def _check(case, tmp_path, nat, monkeypatch):
    """The reasons this case fails, none when it holds."""
    why = []
    z, plain = tmp_path / (case.name + ".gfa.gz"), tmp_path / (case.name + ".gfa")
    z.write_bytes(case.file())
    plain.write_bytes(case.payload())
    for flags in (0, nat.TEST_HOST_INFLATE):
        monkeypatch.setattr(nat, "TEST_FLAGS", flags)
        raw = nat.build_from_path(str(z), nat.make_options())
        on_gpu = "gz_inflate" in raw.phase_ms
        if on_gpu != (case.verdict == "gpu" and not flags):
            why.append("gz_inflate phase %s (flags %d, status %d)" % ("present" if on_gpu else "absent", flags,
                                                                        raw.status))
        if (raw.status == 0) != (case.verdict != "error"):
            why.append("status %d (flags %d)" % (raw.status, flags))
        for mode in MODES:
            got = _outcome(z, mode)
            want = _gzip_outcome(z) if case.verdict == "error" else _outcome(plain, mode)
            if case.verdict == "error" and want is None:
                why.append("gzip.open reads it")
            elif case.verdict != "error" and want[0] != "ok" and case.payload():
                why.append("the plain file does not build: %r" % (want[1:],))
            if got != want:
                why.append("differs from %s (flags %d, %r): %r" % (
                    "gzip.open" if case.verdict == "error" else "the plain file", flags, mode,
                    got[1:] if got[0] == "exc" else "a different build"))
    monkeypatch.setattr(nat, "TEST_FLAGS", 0)
    return why


@pytest.mark.parametrize("case", du.CASES, ids=lambda c: c.name)
def test_bgzf_stream_case(gpu, tmp_path, monkeypatch, case):
    why = _check(case, tmp_path, gpu, monkeypatch)
    assert not why, (case.name, why)


def test_no_case_outside_the_closed_list_is_declined():
    """The cap on "declined": exactly the limits DESIGN.md section 7 names."""
    assert [c.name for c in du.CASES if c.verdict == "declined"] == [
        "E_one_distance_code_of_length_1", "E_no_distance_code", "E_end_of_block_code_alone"]
    assert all(c.verdict == "gpu" for c in du.CASES if c.cls in "ABCD")
