"""The host decisions of flate_hip_compress_joined (flate_amd/csrc/join_plan.h) through tests/cpu_shim: the argument
verdicts, the piece tables -- piece -> stream, the last-of-stream flag, the input range, offsets beyond 2^32 included --,
the bound's formula, the scratch slots and the marker's length for every bit residue."""
import pytest

import _join_plan as jp

PIECES = (1, 7, 65535)


def stream_lengths(piece):
    return [0, 1, piece - 1, piece, piece + 1, 2 * piece, 2 ** 32 + 5]


def test_constants():
    assert jp.const("max_piece") == 65535 and jp.const("marker_max") == 5
    assert jp.const("slot_align") == 16 and jp.const("slot_spare") >= 16
    assert jp.const("max_pieces") == 2 ** 31 - 1
    assert jp.const("sizeof_stream") == 48


def test_marker_bytes_for_every_residue():
    # 1..5 padding bits in the block's last byte hold the empty stored block's three header bits; at 0, 6 and 7 they
    # take (part of) a byte of their own
    assert [jp.marker_bytes(r) for r in range(8)] == [5, 4, 4, 4, 4, 4, 5, 5]
    assert [jp.marker_bytes(8 + r) for r in range(8)] == [5, 4, 4, 4, 4, 4, 5, 5]


def test_argument_verdicts():
    for mode in range(-1, 12):
        assert jp.args_ok(4096, 1, mode) == (4 <= mode <= 9), mode
    for container in range(-2, 5):
        assert jp.args_ok(4096, container, 6) == (0 <= container <= 2), container
    for piece, ok in ((0, True), (1, True), (65535, True), (65536, False), (2 ** 32 - 1, False)):
        assert jp.args_ok(piece, 0, 6) == ok, piece
    assert jp.piece_bytes(0) == 65535 and jp.piece_bytes(1) == 1 and jp.piece_bytes(65535) == 65535


@pytest.mark.parametrize("piece", PIECES)
def test_piece_count_and_pieces_of_a_stream(piece):
    for n in stream_lengths(piece):
        P = jp.piece_count(n, piece)
        assert P == max(1, -(-n // piece)), n
        base = 2 ** 33 + 11
        ks = sorted(k for k in {0, 1, P // 2, P - 2, P - 1} if 0 <= k < P)
        for k in ks:
            off, ln, last = jp.piece_of(base, n, piece, k)
            assert off == base + k * piece and ln == min((k + 1) * piece, n) - k * piece and last == (k == P - 1), (n, k)
        # the pieces cover the stream: whole ones and the last
        assert (P - 1) * piece + jp.piece_of(base, n, piece, P - 1)[1] == n


@pytest.mark.parametrize("piece", (7, 65535))
def test_layout_and_tables_of_a_call(piece):
    lens = [l for l in stream_lengths(piece) if l < 2 ** 32]
    caps = [jp.bound(l, piece, 1) + 3 for l in lens]
    total, streams = jp.layout(lens, caps, piece, in_base=2 ** 32 + 100, out_base=77, in_shift=2 ** 32 + 100, out_shift=77)
    assert total == sum(max(1, -(-l // piece)) for l in lens)
    at = p0 = o = 0
    for s, l, c in zip(streams, lens, caps):
        assert s == dict(in_off=at, n=l, out_off=o, out_cap=c, piece0=p0, n_pieces=max(1, -(-l // piece)))
        at, o, p0 = at + l, o + c, p0 + s["n_pieces"]
    base = 2 ** 32 + 100  # (device memory: the offsets stay as they are)
    scratch, ps, pin, pslot = jp.tables(lens, piece, in_base=base)
    assert len(ps) == total and pin[-1] == base + sum(lens) and pslot[-1] == scratch
    j = 0
    at = base
    for i, l in enumerate(lens):
        for k in range(max(1, -(-l // piece))):
            ln = min((k + 1) * piece, l) - k * piece
            assert ps[j] == i and pin[j] == at + k * piece and pin[j + 1] - pin[j] == ln, (i, k)
            assert pslot[j] % 16 == 0 and pslot[j + 1] - pslot[j] == jp.slot_bytes(ln)
            j += 1
        at += l
    assert j == total


def test_layout_counts_pieces_without_a_table():
    # 2^32 + 5 bytes in pieces of one byte: more pieces than a call may have -- counted, never laid out
    total, streams = jp.layout([5, 2 ** 32 + 5, 0], [0, 0, 0], 1)
    assert total == 5 + 2 ** 32 + 5 + 1 and total > jp.const("max_pieces")
    assert [s["piece0"] for s in streams] == [0, 5, 2 ** 32 + 10]


def test_slots_hold_the_bound_the_marker_and_spare_bytes():
    for n in (0, 1, 7, 4096, 32767, 32768, 65534, 65535):
        s = jp.slot_bytes(n)
        assert s % 16 == 0 and s >= jp.raw_bound(n) + 5 + 16 and s < jp.raw_bound(n) + 5 + 32
        assert jp.raw_bound(n) >= n + 5 * (n // 65535 + 1)  # (stored blocks always fit)


@pytest.mark.parametrize("piece", PIECES)
def test_bound_formula(piece):
    hdr_ftr = {0: 0, 1: 18, 2: 6}
    for n in stream_lengths(piece):
        P = max(1, -(-n // piece))
        last = n - (P - 1) * piece
        for container in (0, 1, 2):
            want = hdr_ftr[container] + (P - 1) * (jp.raw_bound(piece) + 5) + jp.raw_bound(last) + 5
            assert jp.bound(n, piece, container) == want, (n, container)
    # the sum over the pieces, piece by piece, for a stream short enough to walk
    n = 5 * piece + 3
    assert jp.bound(n, piece, 0) == sum(jp.raw_bound(min(piece, n - a)) + 5 for a in range(0, n, piece))
