"""CPU: the BGZF catalogue of tests/deflate_util.py is what it says it is.  Every member's raw
deflate stream gets the same verdict and bytes from the bit-by-bit reader (inflate_trace) and
from zlib; the bytes are the payload the tokens produced; the trace shows every feature the case
claims; Python's gzip on the assembled file gives the concatenated payloads or raises; and every
"error" case carries the trailer of its intended payload, so only the decoder can catch it.
test_gpu_bgzf_streams.py then shows the same files to the GPU inflate."""
import gzip
import io
import zlib

import pytest

import deflate_util as du

CASES = du.CASES

# what `gzip` raises on each "error" file (zlib's message without its "Error -3 ..." prefix, the
# CRC message without its values); None where the message depends on how the bytes that follow
# the broken stream happen to decode
RAISES = {
    "F_block_type_3": ("error", "invalid block type"),
    "F_block_type_3_after_fixed": ("error", "invalid block type"),
    "F_nlen_not_complement": ("error", "invalid stored block lengths"),
    "F_hlit_30": ("error", "too many length or distance symbols"),
    "F_hdist_30": ("error", "too many length or distance symbols"),
    "F_hlit_31": ("error", "too many length or distance symbols"),
    "F_hdist_31": ("error", "too many length or distance symbols"),
    "F_oversubscribed_code_length_code": ("error", "invalid code lengths set"),
    "F_incomplete_code_length_code": ("error", "invalid code lengths set"),
    "F_oversubscribed_literal_length_code": ("error", "invalid literal/lengths set"),
    "F_oversubscribed_distance_code": ("error", "invalid distances set"),
    "F_incomplete_literal_length_code": ("error", "invalid literal/lengths set"),
    "F_incomplete_distance_code": ("error", "invalid distances set"),
    "F_no_end_of_block_code": ("error", "invalid code -- missing end-of-block"),
    "F_repeat_16_first": ("error", "invalid bit length repeat"),
    "F_repeat_past_total": ("error", "invalid bit length repeat"),
    "F_length_symbol_286": ("error", "invalid literal/length code"),
    "F_length_symbol_287": ("error", "invalid literal/length code"),
    "F_distance_symbol_30": ("error", "invalid distance code"),
    "F_distance_symbol_31": ("error", "invalid distance code"),
    "F_distance_position_plus_1": ("error", "invalid distance too far back"),
    "F_ends_inside_symbol": (None, None),
    "F_ends_inside_extra_bits": (None, None),
    "F_ends_inside_stored_block": (None, None),
    "F_output_longer_than_isize": ("BadGzipFile", "CRC check failed"),
    "F_output_shorter_than_isize": ("BadGzipFile", "CRC check failed"),
    "F_output_shorter_same_crc": ("BadGzipFile", "Incorrect length of data produced"),
    "F_crc_mismatch_only": ("BadGzipFile", "CRC check failed"),
    "F_spare_byte_before_trailer": ("BadGzipFile", "CRC check failed"),
    "F_no_deflate_data": (None, None),
    "F_len_65535_data_missing": ("EOFError", "Compressed file ended before the end-of-stream marker was reached"),
    "F_hclen_4": ("error", "invalid code -- missing end-of-block"),
    "G_bad_member_at_0_of_129": ("error", "invalid stored block lengths"),
    "G_bad_member_at_63_of_129": ("error", "invalid literal/lengths set"),
    "G_bad_member_at_64_of_129": ("error", "invalid literal/lengths set"),
    "G_bad_member_at_128_of_129": ("error", "invalid stored block lengths"),
}


def _gzip_outcome(blob):
    try:
        return ("ok", gzip.GzipFile(fileobj=io.BytesIO(blob)).read())
    except (gzip.BadGzipFile, EOFError, zlib.error) as e:
        return ("exc", type(e).__name__, str(e))


def _trace(raw):
    try:
        return du.inflate_trace(raw)
    except du.DeflateError as e:
        return None, e


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_is_what_it_claims(case):
    traces = []
    for i, m in enumerate(case.members):
        got, tr = _trace(m.raw)
        z = du.zlib_inflate(m.raw)
        assert got == z, (case.name, i, tr)  # same bytes, or both reject
        if got is not None and (case.verdict != "error" or i not in case.test):
            assert got == m.payload, (case.name, i)
        if got is not None and i in case.test:
            traces.append(tr)
    if case.features:
        assert len(traces) == len(case.test)
        merged = du.merged_trace(traces)
        for text, holds in case.features:
            assert holds(merged), (case.name, text)
    out = _gzip_outcome(case.file())
    if case.verdict == "error":
        assert out[0] == "exc", case.name
        kind, msg = RAISES[case.name]
        if kind is not None:
            got = out[2].replace("Error -3 while decompressing data: ", "").split(" 0x")[0]
            assert (out[1], got) == (kind, msg), case.name
        blob = case.file()
        pos = 0
        for m in case.members:  # the trailer belongs to the intended payload
            b = m.bytes()
            assert blob[pos:pos + len(b)] == b
            pos += len(b)
            assert b[-8:] == zlib.crc32(m.payload).to_bytes(4, "little") + len(m.payload).to_bytes(4, "little")
    else:
        assert out == ("ok", case.payload()), case.name


def test_error_cases_fail_in_the_decoder():
    """Each F member is rejected by zlib itself, or (length and spare-byte cases) decodes to
    something other than the payload its trailer describes."""
    for case in CASES:
        if case.cls != "F":
            continue
        m = case.members[1]
        z = du.zlib_inflate(m.raw)
        used = None if z is None else du.inflate_trace(m.raw)[1]["consumed"]
        assert z is None or z != m.payload or used != len(m.raw), case.name


def test_truncations_end_where_they_say():
    for name, where in (("F_ends_inside_symbol", "symbol"), ("F_ends_inside_extra_bits", "extra"),
                        ("F_ends_inside_stored_block", "stored"), ("F_no_deflate_data", "header")):
        with pytest.raises(du.DeflateError) as ei:
            du.inflate_trace(du.BY_NAME[name].members[1].raw)
        assert (str(ei.value), ei.value.where) == ("truncated", where), name


def test_declined_list_is_accepted_by_zlib_and_closed():
    declined = [c.name for c in CASES if c.verdict == "declined"]
    assert declined == ["E_one_distance_code_of_length_1", "E_no_distance_code", "E_end_of_block_code_alone"]
    for name in declined:
        m = du.BY_NAME[name].members[1]
        assert zlib.decompress(m.raw, -15) == m.payload == du.inflate_trace(m.raw)[0]


def test_alternative_258_is_accepted_by_zlib():
    w = du.BitWriter()
    du.fixed_block(w, [65, du.mtok(258, 1, alt258=True)], True)
    assert zlib.decompress(w.getvalue(), -15) == b"A" * 259


def test_catalogue_covers_the_classes():
    assert sorted(RAISES) == sorted(c.name for c in CASES if c.verdict == "error")
    per = {}
    for c in CASES:
        per.setdefault(c.cls, []).append(c)
    assert sorted(per) == list("ABCDEFGH")
    assert all(c.verdict == "gpu" for k in "ABCD" for c in per[k])
    assert all(c.verdict == "error" for c in per["F"])
    in_order = du.BY_NAME["G_every_case_in_order"].members[1:-1]
    assert [m.raw for m in in_order] == [c.members[1].raw for k in "ABCD" for c in per[k]]
    assert {len(du.BY_NAME["G_members_%d" % n].members) for n in (1, 63, 64, 65, 128, 129)} == {1, 63, 64, 65, 128, 129}


def test_reader_and_writer_round_trip_zlib_streams():
    """inflate_trace on what zlib writes, at every level and strategy: the reader is not only
    right about this file's own writer."""
    data = du.BY_NAME["G_every_case_in_order"].payload()[:200_000]
    for level, strategy in ((6, 0), (1, 0), (0, 0), (9, 1), (6, 2), (6, 3), (6, 4)):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        raw = co.compress(data) + co.flush()
        assert du.inflate_trace(raw)[0] == data
