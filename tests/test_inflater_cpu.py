"""CPU checks of the resumable inflater's boundary (include/flate_hip.h: flate_hip_inflater_*): its statuses have
names, its symbols are exported, and the generator of the > 4 GiB member that the GPU tests decode is right."""
import zlib

import pytest

import _big_member as B


def test_inflater_status_names_and_symbols():
    from flate_amd import _capi
    assert _capi.status_name(104) == "NeedInput"
    assert _capi.status_name(105) == "NeedOutput"
    assert (_capi.ST_NEED_INPUT, _capi.ST_NEED_OUTPUT) == (104, 105)
    L = _capi.lib()
    for s in ("flate_hip_inflater_create", "flate_hip_inflater_destroy", "flate_hip_inflater_reset",
              "flate_hip_inflater_feed"):
        assert s in _capi.SYMBOLS and hasattr(L, s), s


def test_decompressor_piece_keyword():
    from flate_amd import api, gzip
    import inspect
    sig = inspect.signature(gzip.decompressor)
    assert sig.parameters["piece"].kind == inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["piece"].default is None
    with pytest.raises(ValueError):
        api._PieceDecompressor.__init__(object.__new__(api._PieceDecompressor), 1, b"", engine=object(), piece=0)


@pytest.mark.parametrize("groups", [2, 3, 1000, 20000])
def test_big_member_generator_prefix(groups):
    d = zlib.decompressobj(-15)
    out = b"".join(d.decompress(c) for c in B.raw_chunks(groups, reps=97))
    out += d.flush()
    assert d.eof
    assert out == b"a" * B.output_size(groups)


def test_big_member_generator_gzip_footer():
    groups = 5000
    blob = b"".join(B.gzip_chunks(groups, reps=50))
    assert zlib.decompress(blob, 31) == b"a" * B.output_size(groups)
    big = 2081000  # the GPU test's member: just over 4 GiB of output
    assert B.output_size(big) > 1 << 32
    it = B.raw_chunks(big)
    head = next(it) + next(it) + next(it)[:13 * 1000]
    d = zlib.decompressobj(-15)
    got = d.decompress(head)
    assert set(got) == {ord("a")} and len(got) > 2064 * 900
