"""Pins the CPU oracle's INFLATE side against the reference's own tests
 and against the reference's differential inflater
bin/puff/puff.c (built into oracle/_ref).  No GPU."""
import os
import random
import zlib as pyzlib

import pytest

import _oracle as O
from conftest import golden

HELLO = b"Hello world\n"
ABCD = b"ABCDEABCD ABCDEABCD"
STORED = bytes([0x01, 0x0C, 0x00, 0xF3, 0xFF]) + HELLO
FIXED = bytes([0xF3, 0x48, 0xCD, 0xC9, 0xC9, 0x57, 0x28, 0xCF, 0x2F, 0xCA, 0x49, 0xE1, 0x02, 0x00])
DYN = bytes([0x3D, 0xC6, 0x39, 0x11, 0x00, 0x00, 0x0C, 0x02, 0x30, 0x2B, 0xB5, 0x52, 0x1E, 0xFF, 0x96, 0x38,
             0x16, 0x96, 0x5C, 0x1E, 0x94, 0xCB, 0x6D, 0x01])
GZ_HDR = bytes([0x1F, 0x8B, 0x08, 0, 0, 0, 0, 0, 0, 0x03])


# inflate.zig:357-393
def test_raw_vectors():
    assert O.decompress(STORED, O.RAW)[:2] == ("Ok", HELLO)
    assert O.decompress(FIXED, O.RAW)[:2] == ("Ok", HELLO)
    assert O.decompress(DYN, O.RAW)[:2] == ("Ok", ABCD)


# inflate.zig:395-452
def test_gzip_vectors():
    foot_hello = bytes([0xD5, 0xE0, 0x39, 0xB7, 0x0C, 0, 0, 0])
    assert O.decompress(GZ_HDR + STORED + foot_hello, O.GZIP)[:2] == ("Ok", HELLO)
    hdr4 = bytes([0x1F, 0x8B, 0x08, 0, 0, 0, 0, 0, 0x04, 0x03])
    assert O.decompress(hdr4 + FIXED + foot_hello, O.GZIP)[:2] == ("Ok", HELLO)
    assert O.decompress(GZ_HDR + DYN + bytes([0x17, 0x1C, 0x39, 0xB4, 0x13, 0, 0, 0]), O.GZIP)[:2] == ("Ok", ABCD)
    named = bytes([0x1F, 0x8B, 0x08, 0x08, 0xE5, 0x70, 0xB1, 0x65, 0x00, 0x03, 0x68, 0x65, 0x6C, 0x6C, 0x6F, 0x2E,
                   0x74, 0x78, 0x74, 0x00]) + FIXED + foot_hello
    assert O.decompress(named, O.GZIP)[:2] == ("Ok", HELLO)


# inflate.zig:454-479
def test_zlib_vector():
    blob = bytes([0x78, 0x9C]) + STORED + bytes([0x1C, 0xF2, 0x04, 0x47])
    assert O.decompress(blob, O.ZLIB)[:2] == ("Ok", HELLO)


# inflate.zig:481-542 -- the 40-case error taxonomy
FUZZ = [
    ("deflate-stream", None, "@deflate-stream.expect"),
    ("empty-distance-alphabet01", None, b""),
    ("empty-distance-alphabet02", None, b""),
    ("end-of-stream", "EndOfStream", None),
    ("invalid-distance", "InvalidMatch", None),
    ("invalid-tree01", "IncompleteHuffmanTree", None),
    ("invalid-tree02", "IncompleteHuffmanTree", None),
    ("invalid-tree03", "IncompleteHuffmanTree", None),
    ("lengths-overflow", "InvalidDynamicBlockHeader", None),
    ("out-of-codes", "InvalidCode", None),
    ("puff01", "WrongStoredBlockNlen", None),
    ("puff02", "EndOfStream", None),
    ("puff03", None, bytes([0x0A])),
    ("puff04", "InvalidCode", None),
    ("puff05", "EndOfStream", None),
    ("puff06", "EndOfStream", None),
    ("puff08", "InvalidCode", None),
    ("puff09", None, b"P"),
    ("puff10", "InvalidCode", None),
    ("puff11", "InvalidMatch", None),
    ("puff12", "InvalidDynamicBlockHeader", None),
    ("puff13", "IncompleteHuffmanTree", None),
    ("puff14", "EndOfStream", None),
    ("puff15", "IncompleteHuffmanTree", None),
    ("puff16", "InvalidDynamicBlockHeader", None),
    ("puff17", "InvalidDynamicBlockHeader", None),
    ("fuzz1", "InvalidDynamicBlockHeader", None),
    ("fuzz2", "InvalidDynamicBlockHeader", None),
    ("fuzz3", "InvalidMatch", None),
    ("fuzz4", "OversubscribedHuffmanTree", None),
    ("puff18", "OversubscribedHuffmanTree", None),
    ("puff19", "OversubscribedHuffmanTree", None),
    ("puff20", "OversubscribedHuffmanTree", None),
    ("puff21", "OversubscribedHuffmanTree", None),
    ("puff22", "OversubscribedHuffmanTree", None),
    ("puff23", "InvalidDynamicBlockHeader", None),
    ("puff24", "InvalidDynamicBlockHeader", None),
    ("puff25", "OversubscribedHuffmanTree", None),
    ("puff26", "InvalidDynamicBlockHeader", None),
    ("puff27", "InvalidDynamicBlockHeader", None),
]


@pytest.mark.parametrize("flags", [0, 1], ids=["rfc", "reference-strict-q6"])
@pytest.mark.parametrize("name,err,out", FUZZ, ids=[f[0] for f in FUZZ])
def test_fuzz_corpus_error_taxonomy(name, err, out, flags):
    data = golden("fuzz", name + ".input")
    st, got, _ = O.decompress(data, O.RAW, flags=flags)
    if err is not None:
        assert st == err
    else:
        assert st == "Ok"
        want = golden("fuzz", out[1:]) if isinstance(out, str) else out
        assert got == want


def test_fuzz_corpus_agrees_with_puff_on_success_vs_error():
    # bin/fuzz_puff.zig:42-50: both must agree on error-vs-success and on bytes (puff.c's verdicts: O.puff_verdict)
    for name, err, out in FUZZ:
        data = golden("fuzz", name + ".input")
        st, got, _ = O.decompress(data, O.RAW)
        rc, pout = O.puff_verdict(data)
        assert (st == "Ok") == (rc == 0), name
        if rc == 0:
            assert O.digest(got) == pout, name


# inflate.zig:544-563 "bug 18967": two concatenated zlib streams
def test_two_concatenated_zlib_streams():
    a, b = golden("fuzz", "first.input"), golden("fuzz", "second.input")
    st, o1, used = O.decompress(a + b, O.ZLIB)
    assert st == "Ok" and used == len(a)
    st, o2, used2 = O.decompress((a + b)[used:], O.ZLIB)
    assert st == "Ok" and used2 == len(b)
    assert o1 + o2 == golden("fuzz", "first.expect") + golden("fuzz", "second.expect")


# flate.zig:255-265
def test_dont_read_past_stream_end():
    blob = bytes([0x08, 0xD7, 0x63, 0xF8, 0xCF, 0xC0, 0xC0, 0x00, 0xC1, 0xFF, 0xFF, 0x43, 0x30, 0x03, 0x03, 0xC3,
                  0xFF, 0xFF, 0xFF, 0x01, 0x83, 0x95, 0x0B, 0xF5])
    want = bytes([0x00, 0xFF, 0x00, 0x00, 0x00, 0xFF, 0x00, 0x00, 0x00, 0xFF, 0x00, 0xFF, 0xFF, 0xFF, 0x00, 0xFF,
                  0xFF, 0xFF, 0x00, 0x00, 0x00, 0x00, 0xFF, 0xFF, 0xFF])
    assert O.decompress(blob, O.ZLIB)[:2] == ("Ok", want)


# flate.zig:267-295
def test_zlib_header_errors():
    assert O.decompress(bytes([0x78]), O.ZLIB)[0] == "EndOfStream"
    assert O.decompress(bytes([0x79, 0x94]), O.ZLIB)[0] == "BadZlibHeader"
    assert O.decompress(bytes([0x88, 0x98]), O.ZLIB)[0] == "BadZlibHeader"
    assert O.decompress(bytes([0x78, 0xDA, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00]), O.ZLIB)[0] == "WrongZlibChecksum"
    assert O.decompress(bytes([0x78, 0xDA, 0x03, 0x00, 0x00]), O.ZLIB)[0] == "EndOfStream"


# flate.zig:297-354
def test_gzip_header_errors():
    assert O.decompress(bytes([0x1F, 0x8B]), O.GZIP)[0] == "EndOfStream"
    assert O.decompress(bytes([0x1F, 0x8B, 0x09, 0, 0, 0, 0, 0, 0, 0x03]), O.GZIP)[0] == "BadGzipHeader"
    assert O.decompress(GZ_HDR + bytes([0x03, 0, 0, 0, 0, 0x01, 0, 0, 0, 0]), O.GZIP)[0] == "WrongGzipChecksum"
    assert O.decompress(GZ_HDR + bytes([0x03, 0, 0, 0, 0]), O.GZIP)[0] == "EndOfStream"
    assert O.decompress(GZ_HDR + bytes([0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0x01]), O.GZIP)[0] == "WrongGzipSize"
    assert O.decompress(GZ_HDR + bytes([0x03, 0, 0, 0, 0, 0, 0, 0, 0]), O.GZIP)[0] == "EndOfStream"
    blob = bytes([0x1F, 0x8B, 0x08, 0x12, 0x00, 0x09, 0x6E, 0x88, 0x00, 0xFF, 0x48, 0x65, 0x6C, 0x6C, 0x6F, 0x00,
                  0x99, 0xD6, 0x01, 0x00, 0x00, 0xFF, 0xFF, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00])
    assert O.decompress(blob, O.GZIP)[:2] == ("Ok", b"")


def test_invalid_block_type():
    assert O.decompress(bytes([0x07, 0x00]), O.RAW)[0] == "InvalidBlockType"  # inflate.zig:267


# quirk Q6: a code-length repeat crossing the HLIT/HDIST
# boundary is legal (RFC 1951 3.2.7), is emitted by the reference's own
# encoder, and is rejected by the reference's inflater.
def test_q6_cross_boundary_repeat(rfc1951):
    data = rfc1951[20395:20395 + 1662]
    c = O.compress(data, O.RAW, 6)
    assert pyzlib.decompress(c, -15) == data
    assert O.decompress(c, O.RAW, flags=0)[:2] == ("Ok", data)
    assert O.decompress(c, O.RAW, flags=1)[0] == "InvalidDynamicBlockHeader"
    assert O.puff_verdict(c) == (0, O.digest(data))


def random_stream_inputs():
    rng = random.Random(1234)
    words = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(2, 9))) for _ in range(200)]
    for trial in range(12):
        n = rng.choice([0, 1, 5, 100, 3000, 70000, 140000])
        kind = trial % 3
        if kind == 0:
            yield b" ".join(rng.choice(words) for _ in range(n // 5 + 1))[:n]
        elif kind == 1:
            yield bytes(rng.getrandbits(8) for _ in range(n))
        else:
            yield bytes(rng.choice(b"ab\0\0\0\0") for _ in range(n))


RANDOM_STREAM_MODES = (O.STORE, O.HUFFMAN, 4, 6, 9)


def test_differential_vs_puff_and_zlib_random_streams():
    # all-levels round trip (bin/roundtrip.zig:14-33) + differential inflate
    for data in random_stream_inputs():
        for mode in RANDOM_STREAM_MODES:
            for cont in (O.RAW, O.GZIP, O.ZLIB):
                c = O.compress(data, cont, mode)
                st, out, used = O.decompress(c, cont, cap=len(data) + 16)
                assert st == "Ok" and out == data and used == len(c)
                assert pyzlib.decompress(c, {0: -15, 1: 31, 2: 15}[cont]) == data
            assert O.puff_verdict(O.compress(data, O.RAW, mode), cap=len(data) + 16) == (0, O.digest(data))
        # zlib-produced streams decode identically
        for lvl in (1, 6, 9):
            co = pyzlib.compressobj(lvl, pyzlib.DEFLATED, -15)
            c = co.compress(data) + co.flush()
            assert O.decompress(c, O.RAW, cap=len(data) + 16)[:2] == ("Ok", data)


def test_directed_edge_streams_agree_with_puff():
    """tests/_inflate_edge_cases.py (what the GPU decoders are checked on under -m gpu): the oracle's success / failure and bytes ==
    the reference's own differential inflater (bin/puff/puff.c, oracle/_ref)."""
    from _inflate_edge_cases import CASES
    for n, s in sorted(CASES.items()):
        name, out, _ = O.decompress(s, O.RAW, 0, cap=80000)
        rc, pout = O.puff_verdict(s, cap=80000)
        assert (name == "Ok") == (rc == 0), (n, name, rc)
        if rc == 0:
            assert pout == O.digest(out), n


# ---- synthesized streams (tests/_deflate_synth.py): dynamic blocks no encoder emits.  The generator's own expansion of its token
# list is the reference for every valid stream; the oracle, puff.c and zlib are checked against it here, on every case.
SYNTH_SEED, SYNTH_SWEEP, SYNTH_STORED = 0, 400, 100  # random streams: the seeds; how many of them have a stored puff.c verdict


def synth_cap(want):
    return len(want) + 16 if want is not None else 1 << 18


def _synth_agrees(name, stream, want, q6, stored_verdict=True):
    cap = synth_cap(want)
    st, out, used = O.decompress(stream, O.RAW, 0, cap=cap)
    assert (st, used) == ("Ok", len(stream)) and out == want, (name, st, used, len(stream))
    assert pyzlib.decompress(stream, -15) == want, name
    if stored_verdict or O.puff_available():  # (the rest of the sweep: puff.c itself, where oracle/_ref is built)
        rc, pout = O.puff_verdict(stream, cap) if stored_verdict else O.puff(stream, cap)
        assert rc == 0 and (pout if stored_verdict else O.digest(pout)) == O.digest(want), (name, rc)
    # reference-strict: refused if and only if a code-length repeat crosses from the literal into the distance lengths (Q6)
    assert O.decompress(stream, O.RAW, 1, cap=cap)[0] == ("InvalidDynamicBlockHeader" if q6 else "Ok"), name


def test_synth_directed_cases_agree_with_every_reference():
    import _deflate_synth as S
    assert len(S.VALID) >= 25 and len(S.INVALID) >= 25
    for name in S.VALID:
        _synth_agrees(name, *S.CASES[name], S.INFO[name]["q6"])
    for name in S.INVALID:
        stream = S.CASES[name][0]
        for flags in (0, 1):
            st = O.decompress(stream, O.RAW, flags, cap=synth_cap(None))[0]
            assert st != "Ok", (name, flags)
            if flags == 0:
                assert st == S.INFO[name]["error"], (name, st)  # the name written next to the case
        assert O.puff_verdict(stream, synth_cap(None))[0] != 0, name
        with pytest.raises(pyzlib.error):
            pyzlib.decompress(stream, -15)


def test_synth_random_sweep_agrees_with_every_reference():
    import _deflate_synth as S
    info = []
    streams = S.random_streams(SYNTH_SEED, SYNTH_SWEEP, info)
    for k, ((stream, want), (q6, _)) in enumerate(zip(streams, info)):
        _synth_agrees("seed %d" % (SYNTH_SEED + k), stream, want, q6, stored_verdict=k < SYNTH_STORED)
    assert 0 < sum(q6 for q6, _ in info) < SYNTH_SWEEP // 4  # some cross (refused with flags = 1), most do not


# what each directed family must hold, counted from the generator's own records: a family that drifts, or is deleted, fails here
SYNTH_FAMILIES = {
    "lut_edge": ["ll_bits_10", "ll_bits_11", "d_bits_8", "d_bits_9", "d_bits_10", "tok_bits_37", "hdr_with_16", "hdr_with_17",
                 "hdr_with_18"],
    "deep15": ["ll_bits_15", "d_bits_15", "tok_bits_48", "tok48_pairs", "dist_eq_written", "error_InvalidMatch"],
    "degenerate_trees": ["blocks_0_tokens", "error_InvalidCode", "error_IncompleteHuffmanTree"],
    "header_fields": ["error_InvalidDynamicBlockHeader", "error_MissingEndOfBlockCode", "error_OversubscribedHuffmanTree",
                      "error_IncompleteHuffmanTree", "error_InvalidBlockType", "hdr_with_16", "hdr_with_17", "hdr_with_18"],
    "tiny_blocks": ["blocks_0_tokens", "stored_blocks", "fixed_blocks", "hdr_without_16", "hdr_without_17", "hdr_without_18"],
    "long_header": ["hdr_without_16", "hdr_without_17", "hdr_without_18", "ll_bits_15"],
    "truncated": ["error_EndOfStream"],
    "big_random": ["dynamic_blocks", "stored_blocks", "fixed_blocks", "hdr_with_16", "hdr_with_17", "hdr_with_18"],
}


def test_synth_census():
    """The classes the GPU tests of the synthesized streams rely on, none of them empty -- in the directed cases alone, and per
    family.  (-s prints the counts, and the bit length of the longest header.)"""
    import _deflate_synth as S
    total = S.census()
    for cls in S.CENSUS_CLASSES:
        print("%-36s %d" % (cls, total[cls]))
        assert total[cls] > 0, cls
    for fam, classes in sorted(SYNTH_FAMILIES.items()):
        names = [n for n in S.CASES if n.startswith(fam + "_")]
        assert names, fam
        c = S.census(names)
        for cls in classes:
            print("%-18s %-36s %d" % (fam, cls, c[cls]))
            assert c[cls] > 0, (fam, cls)
    assert all(any(n.startswith(fam + "_") for fam in SYNTH_FAMILIES) for n in S.CASES)
    # Q6 by each of 16, 17, 18, and a 16 that stands at the first distance length
    assert sum(S.INFO[n]["q6"] for n in S.CASES) >= 4
    # at least 2000 consecutive tiny blocks in more than 128 KiB; the long streams; the longest header
    tiny = [n for n in S.LARGE if n.startswith("tiny_blocks_")]
    assert tiny and S.INFO[tiny[0]]["census"]["dynamic_blocks"] >= 2000
    assert sum(n.startswith("big_random_") for n in S.LARGE) >= 3
    assert all(len(S.CASES[n][1]) > 2 << 20 for n in S.LARGE if n.startswith("big_random_"))
    (longest,) = [n for n in S.CASES if n.startswith("long_header_")]
    print(longest, S.INFO[longest]["header_bits"], "bits")
    assert longest == "long_header_%d_bits" % S.INFO[longest]["header_bits"] and S.INFO[longest]["header_bits"] >= 2286
    # every split point of families 1-4, 6 and 7 is tried by test_gpu_inflater: they fit
    assert all(n in S.SMALL for n in S.CASES if not n.startswith(("tiny_blocks_2200", "big_random_")))
    assert sum(n.startswith("truncated_deep15_") for n in S.CASES) == sum(n.startswith("truncated_tiny_blocks_") for n in S.CASES) == 64
    # the random sweep adds to the classes, it is not needed for any
    sweep = S.census([], range(SYNTH_SEED, SYNTH_SEED + 40))
    for cls in ("ll_bits_15", "d_bits_15", "blocks_0_tokens", "stored_blocks", "fixed_blocks", "hdr_with_16", "hdr_with_18"):
        assert sweep[cls] > 0, cls
