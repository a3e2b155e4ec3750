"""CPU tests of the host arithmetic of the resumable deflater (flate_amd/csrc/deflater_plan.h, through
tests/cpu_shim/deflater_shim.cpp): the blocks a stream cut into feeds turns into are the blocks of the one-shot call
and of the sync-flush call, feed for feed the reference has written no block that the deflater has not, and the
output bound holds for the stored blocks."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libdeflater_shim.so")
BLOCK = 65535
MORE, FLUSH, FINISH = 0, 1, 2


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(SHIM_DIR, "deflater_shim.cpp")
    deps = [src] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in ("deflater_plan.h", "flate_layout.h")]
    if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=undefined", "-fno-sanitize-recover",
                        "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
    lib = C.CDLL(SHIM_SO)
    lib.shim_dfl_blocks.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.shim_dfl_checksum_units.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]
    lib.shim_dfl_out_bound.argtypes = [C.c_uint32, C.c_uint32]
    lib.shim_dfl_out_bound.restype = C.c_uint64
    return lib


def feeds(shim, steps):
    """steps: (piece length, op).  Returns the blocks as absolute (start, len, flags) and per step the number of
    blocks emitted so far."""
    bl, pos, blocks, counts = 0, 0, [], []
    for n, op in steps:
        buf = np.zeros(3 * (n // BLOCK + 8), dtype=np.uint32)
        keep = C.c_uint32(0)
        k = shim.shim_dfl_blocks(bl, n, op, buf.ctypes.data, buf.size // 3, C.byref(keep))
        start = pos - bl  # absolute position of the staged input
        for j in range(k):
            s, ln, fl = (int(x) for x in buf[3 * j: 3 * j + 3])
            blocks.append((start + s if fl != 2 else -1, ln, fl))
        assert keep.value < BLOCK
        pos += n
        bl = keep.value
        counts.append(len(blocks))
    return blocks, counts


def one_shot(total, flush_points=()):
    """the block list of compress_flush (flate_hip.hip, `piece`) / of compress_batch without flush points"""
    out, prev = [], 0

    def piece(start, end, last):
        p = start
        while end - p >= BLOCK:
            out.append((p, BLOCK, 0))
            p += BLOCK
        out.append((p, end - p, 1 if last else 0))
        if not last:
            out.append((-1, 0, 2))

    for f in flush_points:
        piece(prev, f, False)
        prev = f
    piece(prev, total, True)
    return out


def schedule(rnd, total, n_cuts, flushes=0):
    pts = sorted(rnd.randrange(total + 1) for _ in range(n_cuts))
    fl = set(rnd.sample(range(len(pts)), min(flushes, len(pts)))) if pts else set()
    steps, prev = [], 0
    for j, p in enumerate(pts):
        steps.append((p - prev, FLUSH if j in fl else MORE))
        prev = p
    steps.append((total - prev, FINISH))
    return steps


def test_cut_anywhere_gives_the_one_shot_blocks(shim):
    rnd = random.Random(1)
    for total in [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 5 * BLOCK + 7, 1 << 20]:
        for n_cuts in (0, 1, 2, 7, 40):
            for _ in range(5):
                blocks, _ = feeds(shim, schedule(rnd, total, n_cuts))
                assert blocks == one_shot(total), (total, n_cuts)


def test_flush_feeds_give_the_compress_flush_blocks(shim):
    rnd = random.Random(2)
    for total in [0, 1000, BLOCK, 3 * BLOCK + 5, 700000]:
        for _ in range(20):
            steps = schedule(rnd, total, rnd.randrange(1, 8), flushes=rnd.randrange(1, 4))
            if rnd.random() < 0.3:
                steps.insert(rnd.randrange(len(steps)), (0, FLUSH))  # flush twice / at 0
            fpos, acc = [], 0
            for n, op in steps:
                acc += n
                if op == FLUSH:
                    fpos.append(acc)
            blocks, _ = feeds(shim, steps)
            assert blocks == one_shot(total, fpos), (total, steps)


@pytest.mark.parametrize("mode", [O.STORE, O.HUFFMAN])
def test_never_behind_the_reference_writer(shim, mode):
    """after every MORE feed the deflater has emitted at least the blocks the reference's SimpleCompressor has written
    (store-only: a block is 5 + 65535 bytes of the reference's output), and the reference's output is a prefix of the
    one-shot stream"""
    rnd = random.Random(3 + mode)
    data = bytes(rnd.getrandbits(8) for _ in range(5 * BLOCK + 999))
    full = O.compress(data, O.RAW, mode)
    for _ in range(6):
        steps = schedule(rnd, len(data), rnd.randrange(1, 12))
        _, counts = feeds(shim, steps)
        o = O.Deflate(O.RAW, mode)
        pos = 0
        for (n, op), k in zip(steps[:-1], counts):
            o.write(data[pos:pos + n])
            pos += n
            ref = o.output()
            assert full.startswith(ref)
            assert k == pos // BLOCK  # every full buffer is out
            if mode == O.STORE:
                assert k >= len(ref) // (BLOCK + 5), (pos, k, len(ref))


def test_checksum_units_cover_the_piece(shim):
    for bl, n in [(0, 0), (5, 0), (0, 1), (100, BLOCK), (BLOCK - 1, 3 * BLOCK + 2)]:
        buf = np.zeros(2 * (n // BLOCK + 2), dtype=np.uint32)
        k = shim.shim_dfl_checksum_units(bl, n, buf.ctypes.data, buf.size // 2)
        units = [(int(buf[2 * j]), int(buf[2 * j + 1])) for j in range(k)]
        assert sum(u[1] for u in units) == n and all(0 < u[1] <= BLOCK for u in units)
        pos = bl
        for s, ln in units:
            assert s == pos
            pos += ln


def test_output_bound_holds_for_stored_blocks(shim):
    # store-only output of a feed: 5 bytes per block plus the data, the header, the footer and the carried byte
    for bl, n in [(0, 0), (0, 1), (BLOCK - 1, 1), (0, 10 * BLOCK), (1234, 777777)]:
        L = bl + n
        worst = L + 5 * (L // BLOCK + 2) + 10 + 8 + 1
        assert shim.shim_dfl_out_bound(bl, n) >= worst
