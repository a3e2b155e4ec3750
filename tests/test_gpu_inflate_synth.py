"""GPU parity tests of every inflate path on synthesized streams (tests/_deflate_synth.py): dynamic blocks no encoder emits --
codes at the edges of the decoders' tables, trees 15 deep and runs of 48-bit tokens, degenerate trees, header fields at their
limits, thousands of tiny blocks, the longest header -- valid and invalid.  For every stream, through every path: the status
name is the oracle's; when that is Ok the bytes are the generator's own expansion (and the oracle's) and the consumed count is
the oracle's.  (The oracle, puff.c and zlib agree with the generator on all of these streams: test_oracle_inflate_pins.)"""
import random
import zlib as pyzlib

import pytest

import _deflate_synth as S
import _oracle as O
from gpu_util import engine

pytestmark = pytest.mark.gpu

KNOBS = ("FLATE_HIP_INFLATE_PAR", "FLATE_HIP_INFLATE_SPANS", "FLATE_HIP_INFLATE_RING", "FLATE_HIP_SPAN_TWO_RUNS")
PATHS = {  # selected the way test_gpu_inflate / test_gpu_inflate_spans select them
    "k_inflate-ring2048": {"FLATE_HIP_INFLATE_PAR": "0", "FLATE_HIP_INFLATE_SPANS": "0", "FLATE_HIP_INFLATE_RING": "2048"},
    "k_inflate-ring32768": {"FLATE_HIP_INFLATE_PAR": "0", "FLATE_HIP_INFLATE_SPANS": "0", "FLATE_HIP_INFLATE_RING": "32768"},
    "k_inflate_par": {"FLATE_HIP_INFLATE_PAR": "1"},
    "spans-symbols": {"FLATE_HIP_INFLATE_SPANS": "64"},
    "spans-two-runs": {"FLATE_HIP_INFLATE_SPANS": "64", "FLATE_HIP_SPAN_TWO_RUNS": "1"},
}
N_RANDOM, RANDOM_SEED = 200, 5000
ERR_CAP = 1 << 18  # the output slot of an invalid stream (none of them writes that much before it fails)


def choose(monkeypatch, path):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS.get(path, {}).items():
        monkeypatch.setenv(k, v)


_oracle_memo = {}


def oracle(stream, container, flags, cap):
    key = (stream, container, flags, cap)
    if key not in _oracle_memo:
        _oracle_memo[key] = O.decompress(stream, container, flags, cap=cap)
    return _oracle_memo[key]


_random = []


def random_items():
    if not _random:
        _random.extend(("seed %d" % (RANDOM_SEED + k), s, want, len(want) + 8)
                       for k, (s, want) in enumerate(S.random_streams(RANDOM_SEED, N_RANDOM)))
    return list(_random)


def directed_items(names=None):
    """(name, stream, the generator's expansion or None, output slot)"""
    return [(n, S.CASES[n][0], S.CASES[n][1], len(S.CASES[n][1]) + 8 if S.CASES[n][1] is not None else ERR_CAP)
            for n in (sorted(S.CASES) if names is None else names)]


def check(eng, items, flags=0, container=O.RAW, batch=48, label=""):
    """items through decompress_many in batches: status name == the oracle's; Ok: bytes == the generator's == the oracle's, consumed
    == the oracle's.  A valid stream in a slot that holds it must be Ok for the oracle too.  Returns (streams, Ok, errors)."""
    n_ok = n_err = 0
    bad = []
    for k in range(0, len(items), batch):
        part = items[k:k + batch]
        outs, st, used = eng.decompress_many([it[1] for it in part], container, flags, caps=[it[3] for it in part])
        for (name, stream, want, cap), o, s_, u in zip(part, outs, st, used):
            wname, wout, wused = oracle(stream, container, flags, (cap + 7) & ~7)
            got = O.STATUS.get(s_, str(s_))
            if want is not None and flags == 0 and container == O.RAW and cap >= len(want):
                assert wname == "Ok" and wout == want, name  # (the references against the generator, once more)
            if got != wname or (wname == "Ok" and (o != wout or u != wused or (want is not None and o != want))):
                bad.append((name, got, wname, len(o), len(wout), u, wused))
            n_ok += wname == "Ok"
            n_err += wname != "Ok"
    print("%s flags %d container %d: %d streams, %d Ok, %d errors" % (label, flags, container, len(items), n_ok, n_err))
    assert not bad, (label, flags, len(bad), bad[:8])
    return len(items), n_ok, n_err


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_path_every_stream(path, flags, monkeypatch):
    """All of CASES and the random sweep through one path at a time (batches of at most 48: the span path takes at most 64 long
    streams a call), RFC-conformant and reference-strict."""
    choose(monkeypatch, path)
    eng = engine()
    n, n_ok, n_err = check(eng, directed_items() + random_items(), flags, label=path)
    assert n_ok >= len(S.VALID) // 2 and n_err >= len(S.INVALID)


def test_long_streams_take_the_span_path_with_no_knob_set(monkeypatch):
    """Families 5 (thousands of tiny blocks) and 8 (big random streams) are longer than 128 KiB compressed: the library cuts them
    by its own rule -- the profile shows the span kernels --, one stream a call and all of them in one."""
    choose(monkeypatch, None)
    eng = engine()
    assert len(S.LARGE) >= 4
    for names in [[n] for n in S.LARGE] + [S.LARGE]:
        eng.profile_reset()
        eng.profile_enable(True)
        try:
            check(eng, directed_items(names), label="default " + ",".join(names))
        finally:
            prof = eng.profile_read()
            eng.profile_enable(False)
        assert "k_inflate_span" in prof and "k_span_scan" in prof, (names, prof)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_output_slots_full_short_and_spare(path, monkeypatch):
    """The valid lut_edge and deep15 streams (their output is a multiple of 8 bytes) in slots that are exactly full, 8 bytes short
    (the oracle's status for those) and 8 bytes spare, as test_fast_round_edges does with zlib's streams."""
    choose(monkeypatch, path)
    eng = engine()
    names = [n for n in S.VALID if n.startswith(("lut_edge_", "deep15_"))]
    assert len(names) >= 9
    items = []
    for n in names:
        stream, want = S.CASES[n]
        assert len(want) % 8 == 0, n
        for cap in (len(want), len(want) - 8, len(want) + 8):
            items.append(("%s cap %+d" % (n, cap - len(want)), stream, want, cap))
            assert (oracle(stream, O.RAW, 0, cap)[0] == "Ok") == (cap >= len(want)), n
    check(eng, items, label=path + " slots")


def gzip_wrap(stream, data, crc_xor=0, size_add=0):
    return (bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 3]) + stream + ((pyzlib.crc32(data) ^ crc_xor) & 0xFFFFFFFF).to_bytes(4, "little")
            + ((len(data) + size_add) & 0xFFFFFFFF).to_bytes(4, "little"))


def zlib_wrap(stream, data, sum_xor=0):
    return bytes([0x78, 0x9C]) + stream + ((pyzlib.adler32(data) ^ sum_xor) & 0xFFFFFFFF).to_bytes(4, "big")


@pytest.mark.parametrize("path", [None, "k_inflate_par", "spans-symbols"], ids=["default", "k_inflate_par", "spans-symbols"])
def test_wrapped_as_gzip_and_zlib(path, monkeypatch):
    """Every valid stream as a gzip member and as a zlib stream -- header and footer written here from the generator's expansion --
    and each of them once more with a wrong footer: the checksum kernels on outputs they have not seen."""
    choose(monkeypatch, path)
    eng = engine()
    valid = directed_items(S.VALID) + random_items()[:64]
    gz, zl = [], []
    for k, (name, stream, want, cap) in enumerate(valid):
        gz.append((name, gzip_wrap(stream, want), want, cap))
        gz.append((name + " wrong footer", gzip_wrap(stream, want, crc_xor=1 << (k % 32)) if k % 2 else gzip_wrap(stream, want, size_add=1),
                   want, cap))
        zl.append((name, zlib_wrap(stream, want), want, cap))
        zl.append((name + " wrong footer", zlib_wrap(stream, want, sum_xor=1 << (k % 32)), want, cap))
    for container, items, wrong in ((O.GZIP, gz, ("WrongGzipChecksum", "WrongGzipSize")), (O.ZLIB, zl, ("WrongZlibChecksum",))):
        for k, it in enumerate(items):  # the oracle's verdicts are what the test means them to be
            assert oracle(it[1], container, 0, (it[3] + 7) & ~7)[0] in (wrong if k % 2 else ("Ok",)), it[0]
        n, n_ok, n_err = check(eng, items, container=container, label=str(path))
        assert n_ok == n_err == len(valid)


@pytest.mark.parametrize("flags", [0, 1])
def test_one_mixed_batch(flags, monkeypatch):
    """All valid cases, all invalid cases and 64 random streams in a single call: error streams and long slow-path streams next
    to each other in one launch."""
    choose(monkeypatch, None)
    eng = engine()
    items = directed_items() + random_items()[:64]
    random.Random(9).shuffle(items)
    n, n_ok, n_err = check(eng, items, flags, batch=len(items), label="mixed")
    assert n == len(S.CASES) + 64 and n_err >= len(S.INVALID)
