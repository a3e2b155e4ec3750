"""flate_hip_checksum_combine (host code of the library: no GPU) against Python's zlib, both containers: real buffers split at
every boundary of the case list, empty second parts, associativity, and second parts of up to 2^40 bytes -- where the reference is
the definition (tests/_checksum_cases.py: x^(8n) mod P by square and multiply, Adler-32's b = b1 + b2 + n (a1 - 1)), itself
checked here against zlib on real buffers and, for one n >= 2^32, against zlib.crc32 run over that many zeros.

Before fl_crc_xpow8n wrapped its table index the two literals of test_crc_shift_known_answers failed: bit 32 of the length read
the entry behind the table of 32 (x^0 where x^8 belongs)."""
import random
import zlib

import pytest

import _checksum_cases as K

CRC_123456789 = 0xCBF43926
BIG_LENS = [65521 * k for k in (1, 2, 65521, 65522)] + [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 33, 2 ** 40 + 7, 2 ** 64 - 1]


def lib_combine(container, a, b, len_b):
    from flate_amd import _capi
    return int(_capi.lib().flate_hip_checksum_combine(container, a, b, len_b))


def test_the_definition_agrees_with_zlib_on_real_buffers():
    """the from-the-definition reference of this file, before it is used as one"""
    assert K.crc32(b"123456789") == CRC_123456789
    rng = random.Random(11)
    for container in (1, 2):
        for la, lb in [(0, 0), (0, 7), (7, 0), (1, 1), (9, 65521), (65521, 9), (5552, 5553), (100000, 200001), (3, 1 << 20)]:
            a, b = rng.randbytes(la), rng.randbytes(lb)
            assert K.combine(container, K.reference(container, a), K.reference(container, b), lb) == K.reference(container, a + b)
    ff = b"\xff" * (3 * 65521 + 5)  # Adler-32's worst content
    for cut in (0, 1, 5552, 65520, 65521, 65522, len(ff)):
        assert K.combine(2, K.adler32(ff[:cut]), K.adler32(ff[cut:]), len(ff) - cut) == K.adler32(ff)


def test_the_definition_agrees_with_zlib_past_4_gib():
    """crc32("123456789" || 0^n) for n = 2^32 + 5, zlib run over the zeros in 64 MiB pieces, against the definition's combine
    (and so its x^(8n) for an n of more than 32 bits)"""
    n = 2 ** 32 + 5
    piece = bytes(64 << 20)
    whole, zeros, left = CRC_123456789, 0, n
    while left:
        k = min(left, len(piece))
        part = piece if k == len(piece) else piece[:k]
        whole, zeros, left = zlib.crc32(part, whole), zlib.crc32(part, zeros), left - k
    assert K.combine(1, CRC_123456789, zeros, n) == whole
    assert lib_combine(1, CRC_123456789, zeros, n) == whole
    # the bare shift crc(A) x^(8n): the literal of test_crc_shift_known_answers comes out of the same run
    assert whole ^ zeros == 0xE93AC48D


def test_crc_shift_known_answers():
    """value_b = 0: the bare shift crc(A) * x^(8 len_b).  x has order 2^32 - 1, so 2^32 - 1 bytes shift by x^0 ... and 2^32
    bytes by x^8, not by x^0 again"""
    assert lib_combine(1, CRC_123456789, 0, 2 ** 32 - 1) == 0xCBF43926
    assert lib_combine(1, CRC_123456789, 0, 2 ** 32) == 0xD2C671C4
    assert lib_combine(1, CRC_123456789, 0, 2 ** 32 + 5) == 0xE93AC48D
    assert lib_combine(1, CRC_123456789, 0, 5) == 0x5961B806  # (what 2^32 + 5 used to give)


@pytest.mark.parametrize("container", [1, 2])
def test_combine_of_real_buffers_split_at_every_case_boundary(container):
    """every content of the case list, 2 x 65 x 65535 bytes and some, cut at every length of the list (and that far from the end)"""
    total = 2 * 65 * K.BLOCK + 4099
    cuts = sorted({c for n in K.lengths(hi=total) for c in (n, total - n)})
    assert len(cuts) > 60
    for content in K.CONTENTS:
        data = K.make(content, total, seed=container)
        want = K.reference(container, data)
        for cut in cuts:
            got = lib_combine(container, K.reference(container, data[:cut]), K.reference(container, data[cut:]), total - cut)
            assert got == want, (content, cut, hex(got), hex(want))


@pytest.mark.parametrize("container", [1, 2])
def test_combine_with_an_empty_second_part(container):
    empty = K.reference(container, b"")
    rng = random.Random(5)
    for v in [empty, K.reference(container, b"\xff" * 70000), K.reference(container, b"a")] + [K.reference(container, rng.randbytes(99)) for _ in range(20)]:
        assert lib_combine(container, v, empty, 0) == v
        assert lib_combine(container, empty, v, 99) == v  # (behind nothing, whatever the length it stands for)
    assert lib_combine(container, empty, empty, 0) == empty


@pytest.mark.parametrize("container", [1, 2])
def test_combine_is_associative(container):
    """(A || B) || C == A || (B || C) on random triples of values and lengths, lengths of more than 32 bits among them"""
    rng = random.Random(77 + container)

    def value():
        if container == 1:
            return rng.getrandbits(32)
        return rng.randrange(65521) | (rng.randrange(65521) << 16)

    for k in range(400):
        a, b, c = value(), value(), value()
        lb, lc = (rng.getrandbits(rng.choice((3, 17, 33, 48))) for _ in range(2))
        left = lib_combine(container, lib_combine(container, a, b, lb), c, lc)
        right = lib_combine(container, a, lib_combine(container, b, c, lc), lb + lc)
        assert left == right, (k, a, b, c, lb, lc)


@pytest.mark.parametrize("container", [1, 2])
def test_combine_with_lengths_nobody_can_allocate(container):
    rng = random.Random(3)
    heads = [b"123456789", b"\xff" * 65521, b"", rng.randbytes(1000)]
    tails = [b"", b"\xff" * 5552, rng.randbytes(77)]  # (only the VALUE of the second part is real: its length is len_b)
    for n in BIG_LENS:
        for h in heads:
            for t in tails:
                a, b = K.reference(container, h), K.reference(container, t)
                assert lib_combine(container, a, b, n) == K.combine(container, a, b, n), (container, n, len(h), len(t))
        for _ in range(8):  # any pair of values
            a = rng.getrandbits(32) if container == 1 else rng.randrange(65521) | (rng.randrange(65521) << 16)
            b = rng.getrandbits(32) if container == 1 else rng.randrange(65521) | (rng.randrange(65521) << 16)
            assert lib_combine(container, a, b, n) == K.combine(container, a, b, n), (container, n, a, b)
