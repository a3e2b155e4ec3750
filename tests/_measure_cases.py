"""Inputs for the tokenizer's MEASURE: the exact common prefix of a position p and a chain candidate q (test infrastructure; pure
numpy, no GPU import).  k_lz_parse measures 16 bytes an iteration from the aligned dwords that hold them, a shift a side, and
counts the bytes of the last iteration from the lowest differing bit; what can go wrong depends on the match length against 8
and 16, on the alignment of p and of q in their dwords and on (p - q) % 16, and on where the window ends.  The planted lists of
tests/_planted.py hold lengths 4, 5, 33 and 258 only.  Here every case is ONE match of L bytes, fenced on all four sides:

  background  bytes 128..255 from a Generator seeded by the case's name
  source      L bytes of 0..127 at q, 0x80 before it, 0x7e behind it
  copy        the same L bytes at p = q + d, 0x81 before it, 0x7f behind it
              (without the two bytes in front, 0.7 % of random cases start their match a byte early)

so that the oracle's token list holds ("M", d, L) at p at every level (tests/test_measure_cases_cpu.py asserts it for every case;
tests/test_gpu_measure_cases.py compares the GPU's bytes).

  small_cases()  one small input per case, q = 64 + ph: L in SMALL_L, ph in 0..15, d in SMALL_D (every third of them for L > 20;
                 a d below L + 1 is raised by 16 * ((L + 16) // 16): source and copy stay apart, (p - q) % 16 keeps its value);
                 40 bytes of background behind the copy's fence
  end_cases()    the copy runs to the input's last byte (N = p + L, d = L + 24): L in END_L, ph in 0, 3, .., 15; behind the source
                 come background bytes (after 0x7e), or 20 zero bytes -- what the window's padding behind the input holds, so a
                 measure that reads past the end finds the two sides equal there
  subb_cases()   the same event in sub-pass B's re-based window: a 52 KiB background chunk, p = 51456 + ph, d = 1000
"""
import functools
import zlib
from typing import NamedTuple

import numpy as np

LEVELS = (4, 6, 7, 9)
SMALL_L = tuple(range(4, 41)) + (47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258)
SMALL_D = tuple(range(1, 18)) + (31, 32, 33, 1000)
END_L = tuple(range(4, 36)) + (257, 258)
END_PH = tuple(range(0, 16, 3))
SUBB_L = (7, 8, 9, 15, 16, 17, 23, 24, 25)
SUBB_N = 52 * 1024
SUBB_P = 51456
SUBB_D = 1000
N_SMALL = 17 * 16 * 21 + 33 * 16 * 7   # 9408 (x 4 levels: 37632)
N_END = len(END_L) * len(END_PH) * 2   # 408 (x 4 levels: 1632)
N_SUBB = len(SUBB_L) * 16              # 144


class Case(NamedTuple):
    name: str
    data: bytes
    p: int      # where the copy starts
    want: tuple  # ("M", distance, length): the token the oracle's list holds at p


def _rng(name):
    return np.random.default_rng([0x4D454153, zlib.crc32(name.encode())])


def _plant(buf, rng, q, d, L):
    """source at q, copy at q + d, the four fences (a fence that falls outside the buffer is left out: the input ends there)"""
    p = q + d
    buf[q:q + L] = rng.integers(0, 128, L, dtype=np.uint8)
    buf[p:p + L] = buf[q:q + L]
    buf[q - 1] = 0x80
    buf[p - 1] = 0x81
    buf[q + L] = 0x7E
    if p + L < len(buf):
        buf[p + L] = 0x7F
    return p


def small_d(L, d):
    return d if d >= L + 1 else d + 16 * ((L + 16) // 16)


@functools.lru_cache(None)
def small_cases():
    out = []
    for L in SMALL_L:
        for ph in range(16):
            for d0 in (SMALL_D if L <= 20 else SMALL_D[::3]):
                d = small_d(L, d0)
                name = "small/L%d_ph%d_d%d" % (L, ph, d0)
                rng = _rng(name)
                q = 64 + ph
                buf = rng.integers(128, 256, q + d + L + 1 + 40, dtype=np.uint8)
                p = _plant(buf, rng, q, d, L)
                out.append(Case(name, buf.tobytes(), p, ("M", d, L)))
    return tuple(out)


@functools.lru_cache(None)
def end_cases():
    out = []
    for L in END_L:
        for ph in END_PH:
            for form in ("bg", "zero"):
                name = "end/L%d_ph%d_%s" % (L, ph, form)
                rng = _rng(name)
                q, d = 64 + ph, L + 24
                buf = rng.integers(128, 256, q + d + L, dtype=np.uint8)
                p = _plant(buf, rng, q, d, L)
                if form == "zero":
                    buf[q + L:q + L + 20] = 0
                out.append(Case(name, buf.tobytes(), p, ("M", d, L)))
    return tuple(out)


@functools.lru_cache(None)
def subb_cases():
    out = []
    for L in SUBB_L:
        for ph in range(16):
            name = "subb/L%d_ph%d" % (L, ph)
            rng = _rng(name)
            buf = rng.integers(128, 256, SUBB_N, dtype=np.uint8)
            p = _plant(buf, rng, SUBB_P + ph - SUBB_D, SUBB_D, L)
            out.append(Case(name, buf.tobytes(), p, ("M", SUBB_D, L)))
    return tuple(out)


GROUPS = {"small": small_cases, "end": end_cases, "subb": subb_cases}
