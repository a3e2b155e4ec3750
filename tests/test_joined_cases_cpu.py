"""CPU checks of tests/_joined_cases.py, the yardstick of flate_hip_compress_joined: every expectation is ONE stream
stdlib zlib inflates to the input, a flushed piece is the finished one with its final-block bit cleared and a marker of
four or five bytes -- both lengths occur --, the two-block piece is there as a piece that is not last and as the last
one, and the Q1 pieces really do not inflate."""
import zlib as pyzlib

import pytest

import _joined_cases as jc
import _oracle as O

WBITS = {O.RAW: -15, O.GZIP: 31, O.ZLIB: 15}


def inflate(z, container):
    o = pyzlib.decompressobj(WBITS[container])
    out = o.decompress(z)
    assert o.eof and not o.unused_data
    return out


@pytest.mark.parametrize("piece", jc.PIECES)
@pytest.mark.parametrize("level", jc.LEVELS)
def test_every_expectation_inflates_with_stdlib_zlib(level, piece):
    for name, data in jc.batch(piece):
        for container in jc.CONTAINERS:
            z = jc.expected(data, piece, container, level)
            assert inflate(z, container) == data, (name, container)
        if len(data) <= piece:  # one piece: the reference's stream
            assert all(jc.expected(data, piece, c, level) == O.compress(data, c, level) for c in jc.CONTAINERS), name


@pytest.mark.parametrize("level", jc.LEVELS)
def test_a_flushed_piece_is_the_finished_one_opened_and_marked(level):
    """F(x) = L(x) with one bit cleared, then 00 00 ff ff behind at most one zero byte"""
    seen = set()
    for piece in jc.PIECES:
        for name, data in jc.batch(piece):
            for x in jc.pieces_of(data, piece)[:-1]:
                f, l = jc.flushed(x, level), jc.finished(x, level)
                m = jc.marker_bytes(x, level)
                assert m in (4, 5) and f[-4:] == b"\x00\x00\xff\xff" and (m == 4 or f[-5] == 0), name
                diff = [i for i in range(len(l)) if f[i] != l[i]]
                assert len(diff) == 1 and bin(f[diff[0]] ^ l[diff[0]]).count("1") == 1 and f[diff[0]] < l[diff[0]], name
                seen.add(m)
    assert seen == {4, 5}  # (a later change of the inputs cannot drop one form silently)


@pytest.mark.parametrize("level", jc.LEVELS)
def test_both_marker_lengths_occur_in_every_batch_of_long_pieces(level):
    for piece in (4096, 65535):
        seen = {jc.marker_bytes(x, level) for _, data in jc.batch(piece) for x in jc.pieces_of(data, piece)[:-1]}
        assert seen == {4, 5}, piece


@pytest.mark.parametrize("level", jc.LEVELS)
def test_the_two_block_piece_is_not_last_and_last(level):
    data = dict(jc.batch(jc.MAX_PIECE))["sym64_%d" % (2 * jc.MAX_PIECE)]
    ps = jc.pieces_of(data, jc.MAX_PIECE)
    assert len(ps) == 2 and all(jc.block_count(p, level) == 2 for p in ps)
    f, l = jc.flushed(ps[0], level), jc.finished(ps[0], level)
    diff = [i for i in range(len(l)) if f[i] != l[i]]
    assert len(diff) == 1 and diff[0] > 1000  # (the cleared bit lies in the SECOND block's header)
    assert jc.finished(ps[1], level)[0] & 1 == 0  # (the last piece's first block is not final)


def test_noise_pieces_end_stored_and_take_the_long_marker():
    data = jc.content("noise", 2 * 4096)
    x = jc.pieces_of(data, 4096)[0]
    assert jc.finished(x, 6)[0] & 7 == 1 and jc.marker_bytes(x, 6) == 5  # BFINAL, BTYPE 00; the block ends on a byte


@pytest.mark.parametrize("level", jc.LEVELS)
def test_q1_pieces_do_not_inflate(level):
    bad = 0
    for name, x in jc.q1_inputs(level).items():
        z = O.compress(x, O.RAW, level)
        st, back, _ = O.decompress(z, O.RAW, 0, cap=len(x) + 600)
        if back != x:
            bad += 1
            for sname, data, piece in jc.q1_streams(level):
                if sname.startswith(name):
                    zz = jc.expected(data, piece, O.RAW, level)
                    assert O.decompress(zz, O.RAW, 0, cap=len(data) + 600)[1] != data, sname
    assert bad >= 2  # (both kinds: the bytes lost, the bytes twice)


def test_lengths_and_pieces():
    assert jc.lengths(7) == [0, 1, 6, 7, 8, 14, 15, 38]
    assert jc.lengths(65535)[-1] == 2 * 65535 + 1
    assert jc.pieces_of(b"", 7) == [b""] and [len(p) for p in jc.pieces_of(bytes(15), 7)] == [7, 7, 1]
    big = jc.expected(jc.TEXT[:38], 7, O.GZIP, 6)
    assert big[-4:] == (38).to_bytes(4, "little") and big[-8:-4] == pyzlib.crc32(jc.TEXT[:38]).to_bytes(4, "little")
