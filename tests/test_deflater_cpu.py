"""CPU tests of the host side of the resumable deflater (flate_amd/csrc/deflater_plan.h, through
tests/cpu_shim/deflater_shim.cpp): the blocks a stream cut into feeds turns into are the blocks of the one-shot call
and of the sync-flush call, feed for feed the reference has written no block that the deflater has not, and the
output bound holds for the stored blocks.  Then a feed's own decisions: the check of the caller's tables, every stream's
route, the layout of the active streams and the settle rule, each with expected values worked out by hand from the rules
as deflater_plan.h and include/flate_hip.h state them, and a host model of whole sessions over all of them."""
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
    deps = [src] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in ("deflater_plan.h", "flate_layout.h", "flate_common.h")]
    if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=undefined", "-fno-sanitize-recover",
                        "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
    lib = C.CDLL(SHIM_SO)
    lib.shim_dfl_blocks.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.shim_dfl_checksum_units.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]
    lib.shim_dfl_out_bound.argtypes = [C.c_uint32, C.c_uint32]
    lib.shim_dfl_out_bound.restype = C.c_uint64
    u32, u64, i, p = C.c_uint32, C.c_uint64, C.c_int, C.c_void_p
    lib.shim_dfl_max_piece.restype = u64
    lib.shim_dfl_feed_ok.argtypes = [p, p, p, u32, i]
    lib.shim_dfl_route.argtypes = [p, u64, i, u64, p]
    lib.shim_dfl_stage_slices.argtypes = [u64]
    lib.shim_dfl_stage_slices.restype = u32
    lib.shim_dfl_lay_out.argtypes = [p, u32, p, u32, p, p, i, p, p, p, p, u64, p]
    lib.shim_dfl_settle.argtypes = [p, u32, u32, u32, u64, u64, u64, p]
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


# ---------------------------------------------------------------- one feed's decisions
# statuses (include/flate_hip.h) and what a route is (deflater_plan.h, fl_dfl_route_kind)
OK, NEED_INPUT, NEED_OUTPUT = 0, 104, 105
DRAIN, FINISHED, SKIPPED, ACTIVE = 0, 1, 2, 3
MAX_PIECE = 0xfff00000 - 65536


def u64(v):
    return np.ascontiguousarray(np.array(list(v), dtype=np.uint64))


def feed_ok(shim, hin, hout, ops, have_in=True):
    a, b, c = u64(hin), u64(hout), np.ascontiguousarray(np.array(ops, dtype=np.uint8))
    assert len(hin) == len(hout) == len(ops) + 1
    return bool(shim.shim_dfl_feed_ok(a.ctypes.data, b.ctypes.data, c.ctypes.data, len(ops), int(have_in)))


def route(shim, mirror, piece, op, slot):
    """mirror: (bl, hdr_done, finished, pend_len, pend_pos) -> (kind, from, give, status, mirror afterwards)"""
    m, out = u64(mirror), np.zeros(3, np.uint64)
    kind = shim.shim_dfl_route(m.ctypes.data, piece, op, slot, out.ctypes.data)
    return kind, int(out[0]), int(out[1]), int(out[2]), tuple(int(x) for x in m)


def settle(shim, mirror, n, keep, finish, out_cap, produced, slot):
    """-> (ok, give, pend, consumed, status, mirror afterwards)"""
    m, out = u64(mirror), np.zeros(4, np.uint64)
    ok = shim.shim_dfl_settle(m.ctypes.data, n, keep, int(finish), out_cap, produced, slot, out.ctypes.data)
    return (bool(ok),) + tuple(int(x) for x in out) + (tuple(int(x) for x in m),)


def lay_out(shim, mirrors, act, hin, ops, dev):
    """-> (jobs, chunks, blocks, units, totals): lists of tuples as tests/cpu_shim/deflater_shim.cpp lays them out"""
    n, nj = len(mirrors), len(act)
    cap = sum((hin[i + 1] - hin[i]) // BLOCK + 4 for i in range(n))
    m = u64(x for row in mirrors for x in row)
    a = np.ascontiguousarray(np.array(act, dtype=np.uint32))
    h, o = u64(hin), np.ascontiguousarray(np.array(ops, dtype=np.uint8))
    jobs, chunks = np.zeros((max(nj, 1), 9), np.uint64), np.zeros((max(nj, 1), 8), np.uint64)
    blocks, units, totals = np.zeros((cap, 4), np.uint64), np.zeros((cap, 4), np.uint64), np.zeros(6, np.uint64)
    assert shim.shim_dfl_lay_out(m.ctypes.data, n, a.ctypes.data, nj, h.ctypes.data, o.ctypes.data, int(dev), jobs.ctypes.data,
                                 chunks.ctypes.data, blocks.ctypes.data, units.ctypes.data, cap, totals.ctypes.data) == 1
    t = [int(x) for x in totals]
    assert t[4] <= cap and t[5] <= cap
    rows = lambda arr, k: [tuple(int(x) for x in r) for r in arr[:k]]
    assert all(c[7] == 1 for c in rows(chunks, nj))     # nothing but the fields below is set
    return rows(jobs, nj), [c[:7] for c in rows(chunks, nj)], rows(blocks, t[4]), rows(units, t[5]), t[:4]


def test_the_piece_limit_is_the_documented_one(shim):
    assert shim.shim_dfl_max_piece() == MAX_PIECE == 0xffef0000     # include/flate_hip.h: "at most 0xffef0000 bytes"


def test_feed_check(shim):
    hin, hout, ops = [5, 5, 9, 20], [0, 0, 7, 7], [MORE, FLUSH, FINISH]
    assert feed_ok(shim, hin, hout, ops)
    assert not feed_ok(shim, [5, 5, 4, 20], hout, ops)              # input offsets go back
    assert not feed_ok(shim, hin, [0, 0, 7, 6], ops)                # output offsets go back
    assert not feed_ok(shim, hin, hout, [MORE, 3, FINISH])          # an op above FINISH
    assert not feed_ok(shim, hin, hout, [MORE, FLUSH, 255])
    assert not feed_ok(shim, hin, hout, ops, have_in=False)         # input bytes and no buffer
    assert feed_ok(shim, [5, 5, 5, 5], hout, ops, have_in=False)    # no input bytes: no buffer needed
    assert feed_ok(shim, [7, 7 + MAX_PIECE], [0, 0], [MORE])        # a piece at the limit
    assert not feed_ok(shim, [7, 8 + MAX_PIECE], [0, 0], [MORE])    # one byte more
    assert feed_ok(shim, [3], [4], [])


def test_route_draining(shim):
    pending = (10, 1, 0, 100, 20)       # 80 bytes left
    # partly drained: the slot is filled, NEED_OUTPUT, the position moves on
    assert route(shim, pending, 500, FINISH, 30) == (DRAIN, 20, 30, NEED_OUTPUT, (10, 1, 0, 100, 50))
    # exactly drained (and a larger slot gives no more than is left): NEED_INPUT, nothing pending any more
    assert route(shim, pending, 500, FINISH, 80) == (DRAIN, 20, 80, NEED_INPUT, (10, 1, 0, 0, 0))
    assert route(shim, pending, 0, MORE, 1000) == (DRAIN, 20, 80, NEED_INPUT, (10, 1, 0, 0, 0))
    assert route(shim, pending, 0, MORE, 79) == (DRAIN, 20, 79, NEED_OUTPUT, (10, 1, 0, 100, 99))
    # ... of a finished stream: its final status
    assert route(shim, (0, 1, 1, 100, 20), 0, MORE, 80) == (DRAIN, 20, 80, OK, (0, 1, 1, 0, 0))
    assert route(shim, (0, 1, 1, 100, 20), 0, MORE, 79) == (DRAIN, 20, 79, NEED_OUTPUT, (0, 1, 1, 100, 99))
    # a slot of 0 while pending: nothing moves, and the stream is not skipped
    assert route(shim, pending, 0, MORE, 0) == (DRAIN, 20, 0, NEED_OUTPUT, pending)
    assert route(shim, pending, 9, FLUSH, 0) == (DRAIN, 20, 0, NEED_OUTPUT, pending)


def test_route_without_pending_output(shim):
    done, fresh = (0, 1, 1, 0, 0), (7, 1, 0, 0, 0)
    for piece, op, slot in [(5, FINISH, 100), (0, MORE, 0), (0, FLUSH, 9)]:
        assert route(shim, done, piece, op, slot) == (FINISHED, 0, 0, OK, done)
    assert route(shim, fresh, 0, MORE, 0) == (SKIPPED, 0, 0, NEED_INPUT, fresh)
    assert route(shim, fresh, 0, MORE, 1)[0] == ACTIVE          # an empty MORE with a slot is a feed
    assert route(shim, fresh, 1, MORE, 0)[0] == ACTIVE
    assert route(shim, fresh, 0, FLUSH, 0)[0] == ACTIVE         # FLUSH and FINISH of nothing write blocks
    assert route(shim, fresh, 0, FINISH, 0)[0] == ACTIVE
    assert route(shim, (0, 0, 0, 0, 0), 0, FINISH, 0) == (ACTIVE, 0, 0, NEED_INPUT, (0, 0, 0, 0, 0))    # routing leaves it alone
    # a position that has reached the length is not pending (reset and a whole drain leave 0, 0)
    assert route(shim, (7, 1, 0, 5, 5), 0, MORE, 0)[0] == SKIPPED


def test_stage_slices(shim):
    # min(1024, ceil(max_units / 256))
    assert [shim.shim_dfl_stage_slices(u) for u in (1, 256, 257, 1024 * 256, 1024 * 256 + 1, 1 << 40)] == [1, 1, 2, 1024, 1024, 1024]


# five streams, 0, 2 and 4 take their piece: 3 + 5 bytes (below 16), 100 + 130970 = 2 * 65535, 65534 + 2
LAY_MIRRORS = [(3, 0, 0, 0, 0), (9, 1, 0, 50, 10), (100, 1, 0, 0, 0), (0, 1, 1, 0, 0), (65534, 1, 0, 0, 0)]
LAY_HIN = [1000, 1005, 1012, 131982, 131982, 131984]
LAY_OPS = [MORE, MORE, FLUSH, MORE, FINISH]
LAY_ACT = [0, 2, 4]


@pytest.mark.parametrize("dev", [False, True])
def test_layout_of_three_active_streams_out_of_five(shim, dev):
    jobs, chunks, blocks, units, (win_n, out_n, max_units, slices) = lay_out(shim, LAY_MIRRORS, LAY_ACT, LAY_HIN, LAY_OPS, dev)
    src = [1000, 1012, 131982] if dev else [0, 12, 130982]      # absolute / from the first staged byte
    #        src_off, stream, bl, n, keep, ck_first, ck_n, hdr, finish
    assert jobs == [(src[0], 0, 3, 5, 8, 0, 1, 1, 0),           # MORE of 8 bytes: no block, all kept; the header is due
                    (src[1], 2, 100, 130970, 0, 1, 2, 0, 0),
                    (src[2], 4, 65534, 2, 0, 3, 1, 0, 1)]
    # out_cap = L + 5 * (L // 65535 + 3) + 35: 8 + 15 + 35, 131070 + 25 + 35, 65536 + 20 + 35
    # in_off: 0, + 16 + 16, + 131072 + 16; out_off: 0, + 64, + 131136
    #          in_off, in_len, out_off, out_cap, first_block, n_blocks, unfinished
    assert chunks == [(0, 8, 0, 58, 0, 0, 1),
                      (32, 131070, 64, 131130, 0, 4, 1),
                      (131120, 65536, 131200, 65591, 4, 2, 0)]
    assert (win_n, out_n) == (131120 + 65536 + 16, 131200 + 65600)
    assert blocks == [(0, 65535, 0, 1), (65535, 65535, 0, 1), (131070, 0, 0, 1), (0, 0, 2, 1),     # two full, the flush's two
                      (0, 65535, 0, 2), (65535, 1, 1, 2)]                                          # one full, the final one
    assert units == [(3, 5, 0, 0), (100, 65535, 0, 1), (65635, 65435, 0, 1), (65534, 2, 0, 2)]
    assert (max_units, slices) == (8192, 32)        # (131070 + 15) // 16, ceil(8192 / 256)


@pytest.mark.parametrize("dev", [False, True])
def test_layout_regions_and_tables_agree(shim, dev):
    jobs, chunks, blocks, units, (win_n, out_n, _, _) = lay_out(shim, LAY_MIRRORS, LAY_ACT, LAY_HIN, LAY_OPS, dev)
    in_end = out_end = 0
    for j, (jb, c) in enumerate(zip(jobs, chunks)):
        in_off, in_len, out_off, out_cap, first, nb, _ = c
        assert in_off % 16 == 0 and out_off % 16 == 0
        assert in_off >= in_end and out_off >= out_end          # disjoint, in order
        in_end, out_end = in_off + (in_len + 15) // 16 * 16 + 16, out_off + out_cap
        assert in_end <= win_n or j + 1 < len(jobs)
        # the blocks and the kept bytes are fl_dfl_blocks' for the stream's buffer and piece
        buf, keep = np.zeros(3 * 8, dtype=np.uint32), C.c_uint32(0)
        k = shim.shim_dfl_blocks(jb[2], jb[3], LAY_OPS[jb[1]], buf.ctypes.data, 8, C.byref(keep))
        assert (nb, jb[4]) == (k, keep.value)
        assert [b[:3] for b in blocks[first:first + nb]] == [tuple(int(x) for x in buf[3 * t:3 * t + 3]) for t in range(k)]
        assert all(b[3] == j for b in blocks[first:first + nb])         # the tables lead back to the job
        assert all(u[3] == j for u in units[jb[5]:jb[5] + jb[6]])
        assert sum(u[1] for u in units[jb[5]:jb[5] + jb[6]]) == jb[3]
    assert in_end == win_n and out_end <= out_n
    assert sorted(range(len(blocks)), key=lambda k: blocks[k][3]) == list(range(len(blocks)))       # job after job
    assert sum(c[5] for c in chunks) == len(blocks) and sum(jb[6] for jb in jobs) == len(units)


def test_layout_of_no_active_stream_forgets_an_earlier_one(shim):
    # (the shim hands fl_dfl_lay_out a record that is not empty)
    assert lay_out(shim, LAY_MIRRORS, [], LAY_HIN, LAY_OPS, False) == ([], [], [], [], [0, 0, 1, 1])


def test_settle(shim):
    m = (100, 0, 0, 0, 0)
    # everything fits: NEED_INPUT, the piece is taken, the mirror holds the kept bytes and the header is out
    assert settle(shim, m, 500, 7, False, 1000, 300, 300) == (True, 300, 0, 500, NEED_INPUT, (7, 1, 0, 0, 0))
    assert settle(shim, m, 500, 0, True, 1000, 300, 4000) == (True, 300, 0, 500, OK, (0, 1, 1, 0, 0))
    # a byte too many: the slot is filled, the rest pends from its first byte
    assert settle(shim, m, 500, 7, False, 1000, 301, 300) == (True, 300, 1, 500, NEED_OUTPUT, (7, 1, 0, 1, 0))
    assert settle(shim, m, 500, 0, True, 1000, 1000, 0) == (True, 0, 1000, 500, NEED_OUTPUT, (0, 1, 1, 1000, 0))
    # nothing produced (a MORE feed below a block): nothing pends, whatever the slot
    assert settle(shim, m, 5, 105, False, 1000, 0, 0) == (True, 0, 0, 5, NEED_INPUT, (105, 1, 0, 0, 0))
    # more than the bound: refused, nothing moves
    assert settle(shim, m, 500, 7, True, 1000, 1001, 5000) == (False, 0, 0, 0, NEED_INPUT, m)


def test_host_model_of_whole_sessions(shim):
    """Random sessions through routing, layout and settle, the kernels replaced by a made-up number of produced bytes per
    job (0 .. out_cap): every produced byte is handed out once and in order, a piece is taken whole or not at all, a
    finished stream takes nothing, the statuses are those of include/flate_hip.h, and the blocks of all feeds are the
    one-shot call's."""
    rnd = random.Random(11)
    for session in range(40):
        n = rnd.randrange(1, 6)
        scheds = []
        for _ in range(n):
            total = rnd.choice([0, 1, 15, BLOCK - 1, BLOCK, BLOCK + 1, rnd.randrange(400000)])
            scheds.append(schedule(rnd, total, rnd.randrange(0, 6), flushes=rnd.randrange(0, 3)))
        mirrors = [(0, 0, 0, 0, 0)] * n
        step, taken, made = [0] * n, [0] * n, [0] * n       # schedule position, input bytes taken, output bytes produced
        pend = [[] for _ in range(n)]                       # the pending bytes, by their position in the stream's output
        got = [[] for _ in range(n)]
        blocks = [[] for _ in range(n)]
        final = [False] * n
        for feed in range(10000):
            if all(final):
                break
            after = [s[step[i]] if step[i] < len(s) else (rnd.choice([0, 3]), rnd.choice([MORE, FINISH])) for i, s in enumerate(scheds)]
            slots = [rnd.choice([0, 1, 7, 258, 70000, 1 << 20]) for _ in range(n)]
            hin = [rnd.randrange(1000)]
            for ln, _ in after:
                hin.append(hin[-1] + ln)
            ops = [op for _, op in after]
            act, consumed, status = [], [0] * n, [None] * n
            for i in range(n):
                was = mirrors[i]
                kind, frm, give, status[i], mirrors[i] = route(shim, was, after[i][0], ops[i], slots[i])
                assert give <= slots[i]
                if kind == DRAIN:
                    assert pend[i] and frm == was[4] and give == min(slots[i], was[3] - was[4])
                    got[i] += pend[i][frm:frm + give]
                    if frm + give == len(pend[i]):
                        pend[i] = []
                else:
                    assert not pend[i] and give == 0 and mirrors[i] == was
                    assert kind == (FINISHED if was[2] else SKIPPED if after[i] == (0, MORE) and slots[i] == 0 else ACTIVE)
                if kind == ACTIVE:
                    act.append(i)
            jobs, chunks, blks, _, _ = lay_out(shim, mirrors, act, hin, ops, bool(feed & 1))
            for j, i in enumerate(act):
                assert step[i] < len(scheds[i])             # a finished stream is never active
                ln, op = after[i]
                out_cap, first, nb = chunks[j][3], chunks[j][4], chunks[j][5]
                assert settle(shim, mirrors[i], ln, jobs[j][4], op == FINISH, out_cap, out_cap + 1, slots[i])[0] is False
                p = rnd.choice([0, out_cap, rnd.randrange(out_cap + 1)])
                ok, give, left, consumed[i], status[i], mirrors[i] = settle(shim, mirrors[i], ln, jobs[j][4], op == FINISH, out_cap, p, slots[i])
                assert ok and give == min(p, slots[i]) and left == p - give and consumed[i] == ln
                new = list(range(made[i], made[i] + p))
                made[i] += p
                got[i] += new[:give]
                pend[i] = new[give:]
                base = taken[i] - jobs[j][2]                # where the staged input starts in the stream
                blocks[i] += [(base + b[0] if b[2] != 2 else -1, b[1], b[2]) for b in blks[first:first + nb]]
                taken[i] += ln
                step[i] += 1
                assert mirrors[i][0] == jobs[j][4] < BLOCK and mirrors[i][1] == 1 and mirrors[i][2] == (op == FINISH)
            for i in range(n):
                done = step[i] == len(scheds[i])
                assert status[i] == (NEED_OUTPUT if pend[i] else OK if done else NEED_INPUT), (session, feed, i)
                assert mirrors[i][3:] == (0, 0) if not pend[i] else mirrors[i][3] == len(pend[i]) > mirrors[i][4]
                if i not in act:
                    assert consumed[i] == 0
                final[i] = done and not pend[i]
        assert all(final), session
        for i in range(n):
            assert got[i] == list(range(made[i])), (session, i)
            fpos, acc = [], 0
            for ln, op in scheds[i]:
                acc += ln
                if op == FLUSH:
                    fpos.append(acc)
            assert taken[i] == acc and blocks[i] == one_shot(acc, fpos), (session, i)
