"""Cases of compressing records against preset dictionaries (flate_hip_compress_batch_dict) and what they must compress
to.  The reference has no dictionaries; its Compressor keeps the LZ77 history across a sync flush and a flush ends on a
byte boundary, so with T the last min(len, 32768) bytes of the dictionary the stream of record R is what a raw reference
compressor writes for   write(T); flush(); write(R); finish()   from the end of the flush marker on (include/flate_hip.h).
expected() says so with tests/_oracle.py; tests/test_dict_compress_cases_cpu.py holds the expectations against stdlib
zlib, tests/test_gpu_compress_dict.py runs every case on the GPU."""
import collections

import numpy as np

import _oracle as O
from flate_amd import synth

LEVELS = (4, 6, 9)
CONTAINERS = (O.RAW, O.ZLIB)
WINDOW = 32768
MAX_STREAM = 65535  # tail + record

Case = collections.namedtuple("Case", "name zdict rec")  # zdict None: the record has no dictionary

TEXT = synth.text(synth.SEED_TEXT, 200000).tobytes()


def noise(seed, n):
    """bytes in which nothing repeats by plan"""
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def tail(d):
    return d[len(d) - WINDOW:] if len(d) > WINDOW else d


_RAW = {}


def raw_expected(d, rec, level):
    """(stream bytes, token log) of `rec` against dictionary `d`, raw container: the reference from the flush on"""
    key = (d, rec, level)
    if key not in _RAW:
        z = O.Deflate(O.RAW, level, log_tokens=True)
        z.write(tail(d))
        z.flush()
        at, ntok = len(z.output()), len(z.tokens())
        assert z.output()[-4:] == b"\x00\x00\xff\xff"
        z.write(rec)
        z.finish()
        _RAW[key] = (z.output()[at:], z.tokens()[ntok:])
        z.close()
    return _RAW[key]


def expected(d, rec, level, container):
    """the bytes flate_hip_compress_batch_dict must write for `rec` with dictionary `d` (None: without one)"""
    if d is None:
        return O.compress(rec, container, level)
    body = raw_expected(d, rec, level)[0]
    if container == O.RAW:
        return body
    assert container == O.ZLIB
    return b"\x78\xbb" + O.adler32(d).to_bytes(4, "big") + body + O.adler32(rec).to_bytes(4, "big")


def expected_tokens(d, rec, level):
    return raw_expected(d, rec, level)[1]


# ---------------------------------------------------------------- the shapes: a rotor over (D, N)
# D: the empty dictionary, the lengths around the three positions a flush keeps out of the hash table and the four bytes a
# hash needs, the tokenizer's segment sizes (48, 64), a maximal match, sub-pass B's base (16320), the window; one
# dictionary longer than the window.  N: the shortest records, and those that end at sub-pass A's end (49152), a maximal
# match beyond it, and at the limit.
DICT_LENS = (0, 1, 2, 3, 4, 5, 47, 48, 49, 63, 64, 65, 258, 4095, 16319, 16320, 16321, 32767, 32768, 40000)
SMALL_N = (0, 1, 3, 4, 300)
ENDS = (49151, 49152, 49153, 49152 + 258, 65535)  # D + N


def _shapes():
    out = []
    for i, dl in enumerate(DICT_LENS):
        # (text the record continues and repeats: matches reach into the dictionary from everywhere)
        d = TEXT[3000 + 7 * i: 3000 + 7 * i + dl]
        D = min(dl, WINDOW)
        for j, n in enumerate((SMALL_N[i % 5], SMALL_N[(i + 2) % 5], ENDS[i % 5] - D, ENDS[(i + 3) % 5] - D)):
            at = 3000 + 7 * i + max(dl - 2000 - 100 * j, 0)  # the record begins inside the dictionary's last 2000 bytes
            out.append(Case("shape_d%d_n%d" % (dl, n), d, TEXT[at: at + n]))
    return out


# ---------------------------------------------------------------- planted cases
def straddle(k):
    """(c) an 8-byte string that starts k bytes before the dictionary's end and appears again 20 bytes into the record"""
    s = noise(100 + k, 8)
    d = noise(200 + k, 300 - k) + s[:k]
    rec = s[k:] + noise(300 + k, 20 - (8 - k)) + s + noise(400 + k, 30)
    return Case("straddle_k%d" % k, d, rec)


def _planted():
    out = []
    # (a) the record is a 258-byte prefix of T: distance exactly 32768 (position 0 of T is the chain's null)
    t = noise(1, 600) + TEXT[50000: 50000 + WINDOW - 600]
    out.append(Case("far_prefix_258", t, t[:258]))
    out.append(Case("far_prefix_from_1", t, b"#" + t[1:259] + b"#"))
    out.append(Case("far_prefix_long_dict", noise(2, 5000) + t, t[:258] + t[1000:1300]))
    # (b) a match whose source starts in T and runs on into the record; a run that overlaps itself across the seam
    d = noise(3, 500)
    u = noise(4, 12)
    out.append(Case("source_runs_past_seam", d, u + d[-8:] + u + d[-8:] + u))
    out.append(Case("run_from_last_byte", noise(5, 400) + b"z", b"z" * 700 + noise(6, 5)))
    out.append(Case("run_from_five_bytes", noise(7, 400) + b"zzzzz", b"z" * 700 + noise(8, 5)))
    # (c)
    out += [straddle(k) for k in (1, 2, 3, 4)]
    # (d) one repeated byte
    out.append(Case("same_byte_both", b"a" * 1000, b"a" * 2000))
    out.append(Case("same_byte_window", b"a" * WINDOW, b"a" * (MAX_STREAM - WINDOW)))
    out.append(Case("same_byte_dict_text_rec", b"a" * 5000, TEXT[9000:12000]))
    out.append(Case("same_byte_dict_other_byte_rec", b"a" * 300, b"b" * 300))
    # (e) a lazy chain at the record's first positions: each position's match in T is longer than the one before it
    j = [noise(20 + i, 9) for i in range(4)]
    s = noise(9, 16)
    d = j[0] + s[0:4] + j[1] + s[1:7] + j[2] + s[2:11] + j[3] + s[3:16] + noise(10, 40)
    out.append(Case("lazy_chain_at_start", d, s + noise(11, 20)))
    # (f) nothing of the record is in T
    out.append(Case("no_match_noise", noise(12, 4096), noise(13, 3000)))
    out.append(Case("no_match_text", noise(14, WINDOW), TEXT[120000:124096]))
    return out


CASES = _shapes() + _planted()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert all(min(len(c.zdict), WINDOW) + len(c.rec) <= MAX_STREAM for c in CASES)

# incompressible records of every length in the list: the slot size (flate_hip_compress_bound + 4)
BOUND_N = sorted(set(SMALL_N) | {e - min(d, WINDOW) for e in ENDS for d in (0, 4095, WINDOW)} | {MAX_STREAM - WINDOW, 4096, 32768})


def mixed_batch():
    """streams with dictionary 0, with dictionary 1, with none and with the empty dictionary, in one call:
    (records, dicts, dict_of)"""
    dicts = [TEXT[20000:20000 + WINDOW], TEXT[70000:70000 + 5000], b""]
    recs, of = [], []
    for i in range(24):
        of.append((0, 1, None, 2)[i % 4])
        n = (200, 4096, 70000, 0, 1, 30000, 65535, 300)[i % 8]
        if of[-1] is not None:
            n = min(n, MAX_STREAM - len(dicts[of[-1]]))
        base = (20000, 70000, 100000, 40000)[i % 4]
        recs.append(TEXT[base + 131 * i: base + 131 * i + n])
    return recs, dicts, of
