"""GPU tests of the resumable deflater (flate_hip_deflater_*, kernels_deflater.h): huffman-only and store-only streams fed
piece by piece give, whatever the cut, the bytes of the one-shot flate_hip_compress_batch of the whole input (or of
flate_hip_compress_flush with the same flush points) and of the oracle's SimpleCompressor."""
import io
import os
import random
import subprocess
import sys
import zlib as pyzlib

import numpy as np
import pytest

import _oracle as O
from conftest import golden
from gpu_util import engine
from test_gpu_inflater import splits

pytestmark = pytest.mark.gpu

NEED_INPUT, NEED_OUTPUT = 104, 105
MORE, FLUSH, FINISH = 0, 1, 2
MODES = [O.STORE, O.HUFFMAN]
CONTAINERS = [O.RAW, O.GZIP, O.ZLIB]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text(n, seed=1):
    from flate_amd import synth
    return synth.text(seed, n).tobytes()


def _inputs():
    rnd = random.Random(7)
    return {
        "rfc1951": golden("rfc1951.txt"),
        "text": _text(1 << 20),
        "zeros": bytes(1 << 20),
        "random": bytes(rnd.getrandbits(8) for _ in range(200 << 10)),
        "slide": golden("slide", "text250k.bin"),
    }


def run(eng, container, mode, schedules, caps=None, flags=0):
    """One deflater over len(schedules) streams.  schedules[i]: list of (piece bytes, op).  Every feed gives every stream
    its current step (a stream whose schedule is over is skipped); a step that was not taken (consumed 0) is sent again.
    Returns (outputs, final statuses, per-stream list of the output delivered after each taken step)."""
    n = len(schedules)
    d = eng.deflater(n, container, mode, flags)
    outs = [bytearray() for _ in range(n)]
    marks = [[] for _ in range(n)]
    pos = [0] * n
    final = [None] * n
    try:
        for _ in range(100000):
            if all(final[i] is not None for i in range(n)):
                break
            pieces, ops, cap = [], [], []
            for i in range(n):
                if final[i] is not None:
                    pieces.append(None), ops.append(MORE), cap.append(0)
                else:
                    p, o = schedules[i][pos[i]]
                    pieces.append(p), ops.append(o), cap.append(None if caps is None else caps[i])
            o, st, cons = d.feed(pieces, op=ops, caps=cap)
            for i in range(n):
                if final[i] is not None:
                    assert o[i] == b"" and cons[i] == 0
                    continue
                outs[i] += o[i]
                p, op = schedules[i][pos[i]]
                assert cons[i] in (0, len(p)), (i, cons[i], len(p))
                if cons[i] == 0 and len(p):
                    raise AssertionError("a piece was not taken without pending output (stream %d, status %d)" % (i, st[i]))
                # the step was taken: drain what it left over (empty MORE pieces take nothing) before moving on
                while st[i] == NEED_OUTPUT:
                    pieces2, ops2, cap2 = [None] * n, [MORE] * n, [0] * n
                    pieces2[i] = b""
                    cap2[i] = None if caps is None else caps[i]
                    if cap2[i] == 0:
                        break
                    o2, st2, cons2 = d.feed(pieces2, op=ops2, caps=cap2)
                    assert cons2[i] == 0
                    # a drain delivers min(slot, pending); NEED_OUTPUT only while bytes are left
                    assert o2[i] and (st2[i] != NEED_OUTPUT or len(o2[i]) == cap2[i]), (st2[i], len(o2[i]))
                    outs[i] += o2[i]
                    st[i] = st2[i]
                marks[i].append(len(outs[i]))
                pos[i] += 1
                if op == FINISH:
                    assert st[i] in (0, 102), st[i]
                    final[i] = st[i]
                else:
                    assert st[i] == NEED_INPUT, st[i]
    finally:
        d.close()
    return [bytes(x) for x in outs], final, marks


def cut(data, points, last=FINISH):
    pts = [0] + sorted(points) + [len(data)]
    steps = [(data[a:b], MORE) for a, b in zip(pts[:-1], pts[1:])]
    steps[-1] = (steps[-1][0], last)
    return steps


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("container", CONTAINERS)
def test_two_feeds_every_cut_of_small_inputs(mode, container):
    eng = engine()
    for data in (b"", b"a", golden("rfc1951.txt")[:12000]):
        want, wst = eng.compress_many([data], container, mode)
        assert wst == [0] and want[0] == O.compress(data, container, mode)
        ks = splits(len(data))
        got, st, _ = run(eng, container, mode, [cut(data, [k]) for k in ks])
        assert st == [0] * len(ks)
        for k, g in zip(ks, got):
            assert g == want[0], (len(data), k)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("container", CONTAINERS)
def test_cuts_at_and_around_block_boundaries(mode, container):
    eng = engine()
    rnd = random.Random(container * 10 + mode)
    for name, data in _inputs().items():
        want, wst = eng.compress_many([data], container, mode)
        assert wst == [0] and want[0] == O.compress(data, container, mode), name
        ks = set()
        for b in range(0, len(data) + 1, 65535):
            ks |= {b + e for e in (-258, -7, -1, 0, 1, 7, 258) if 0 <= b + e <= len(data)}
        ks = sorted(ks)
        scheds = [cut(data, [k]) for k in ks]
        # seeded random schedules, some of many small pieces
        for _ in range(6):
            m = rnd.choice([2, 5, 17, 60])
            scheds.append(cut(data, [rnd.randrange(len(data) + 1) for _ in range(m)]))
        got, st, _ = run(eng, container, mode, scheds)
        assert st == [0] * len(scheds)
        for j, g in enumerate(got):
            assert g == want[0], (name, j)


@pytest.mark.parametrize("mode", MODES)
def test_one_byte_pieces_across_a_block(mode):
    eng = engine()
    data = _text(65535 + 300, seed=3)
    pts = list(range(65535 - 200, 65535 + 200))
    got, st, _ = run(eng, O.GZIP, mode, [cut(data, pts)])
    assert st == [0] and got[0] == O.compress(data, O.GZIP, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("container", CONTAINERS)
def test_batch_of_72_streams_with_own_schedules(mode, container):
    eng = engine()
    rnd = random.Random(100 + mode * 3 + container)
    base = _text(3 << 20, seed=5)
    datas = []
    for i in range(72):
        kind = i % 4
        ln = rnd.choice([0, 1, 1000, 65535, 65536, 200000, 400000])
        if kind == 0:
            d = base[rnd.randrange(len(base) - ln):][:ln]
        elif kind == 1:
            d = bytes(ln)
        elif kind == 2:
            d = rnd.randbytes(ln)
        else:
            d = (base[:ln // 2] + rnd.randbytes(ln - ln // 2))
        datas.append(d)
    scheds = [cut(d, [rnd.randrange(len(d) + 1) for _ in range(rnd.randrange(0, 9))]) for d in datas]
    # empty MORE steps with an empty slot in between are skips
    got, st, _ = run(eng, container, mode, scheds)
    want, wst = eng.compress_many(datas, container, mode)
    assert st == [0] * len(datas) and wst == [0] * len(datas)
    for i in range(len(datas)):
        assert got[i] == want[i], i
    for i in range(0, len(datas), 9):
        assert got[i] == O.compress(datas[i], container, mode), i


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("container", CONTAINERS)
def test_flush_feeds_match_compress_flush_and_the_oracle(mode, container):
    eng = engine()
    rnd = random.Random(mode * 7 + container)
    data = _text(700000, seed=9)
    cases = [[0], [0, 0], [1000, 1000], [65534, 65535, 65536], [131070], [rnd.randrange(len(data)) for _ in range(5)],
             [len(data)]]
    for fl in cases:
        fl = sorted(fl)
        pts = sorted(set(fl) | {rnd.randrange(len(data)) for _ in range(4)})
        steps, prev = [], 0
        for p in pts:
            steps.append((data[prev:p], FLUSH if p in fl else MORE))
            prev = p
        # equal flush points: flush called twice
        for p in fl:
            if fl.count(p) > 1:
                steps.insert([i for i, s in enumerate(steps) if s[1] == FLUSH][0] + 1, (b"", FLUSH))
                break
        steps.append((data[prev:], FINISH))
        fpos, acc = [], 0
        for p, op in steps:
            acc += len(p)
            if op == FLUSH:
                fpos.append(acc)
        got, st, marks = run(eng, container, mode, [steps])
        want, wst = eng.compress_flush(data, fpos, True, container, mode)
        o = O.Deflate(container, mode)
        for p, op in steps:
            o.write(p)
            if op == FLUSH:
                o.flush()
        o.finish()
        assert st == [0] and wst == 0
        assert got[0] == want == o.output(), fpos
        # after a FLUSH feed, the output so far is compress_flush up to and including that marker
        for j, (p, op) in enumerate(steps):
            if op == FLUSH:
                upto = sum(len(s[0]) for s in steps[:j + 1])
                nfl = sum(1 for s in steps[:j + 1] if s[1] == FLUSH)
                pre, pst = eng.compress_flush(data[:upto], fpos[:nfl], False, container, mode)
                assert got[0][:marks[0][j]] == pre, (fpos, j)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("container", CONTAINERS)
def test_progress_after_each_more_feed(mode, container):
    eng = engine()
    rnd = random.Random(31 + mode + container)
    data = _text(600000, seed=11)
    pts = sorted(rnd.randrange(len(data)) for _ in range(12))
    steps = cut(data, pts)
    got, st, marks = run(eng, container, mode, [steps])
    assert st == [0]
    o = O.Deflate(container, mode)
    for j, (p, op) in enumerate(steps[:-1]):
        o.write(p)
        ref = o.output()
        assert marks[0][j] >= len(ref), (j, marks[0][j], len(ref))
        assert got[0][:len(ref)] == ref
    o.write(steps[-1][0])
    o.finish()
    assert got[0] == o.output()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("slot", [0, 1, 7, 258, 65536])
def test_small_slots_drain_pending_output(mode, slot):
    eng = engine()
    data = _text(300000, seed=13)
    steps = cut(data, [1000, 70000, 200000])
    want = O.compress(data, O.GZIP, mode)
    if slot == 0:
        # a zero slot never delivers: the first feed takes the piece, the next ones drain nothing and take nothing
        d = eng.deflater(1, O.GZIP, mode)
        try:
            o, st, c = d.feed([steps[0][0]], op=MORE, caps=0)
            assert o == [b""] and c == [len(steps[0][0])] and st == [NEED_OUTPUT]
            o, st, c = d.feed([steps[1][0]], op=MORE, caps=0)
            assert o == [b""] and c == [0] and st == [NEED_OUTPUT]
            o, st, c = d.feed([steps[1][0]], op=MORE, caps=1 << 20)
            assert c == [0] and st == [NEED_INPUT] and want.startswith(o[0]) and o[0]  # all delivered, piece not taken
            o2, st, c = d.feed([steps[1][0]], op=MORE, caps=1 << 20)
            assert c == [len(steps[1][0])] and st == [NEED_INPUT] and want.startswith(o[0] + o2[0])
        finally:
            d.close()
        return
    got, st, _ = run(eng, O.GZIP, mode, [steps], caps=[slot])
    assert st == [0] and got[0] == want


@pytest.mark.parametrize("mode", MODES)
def test_finished_stream_takes_nothing_and_reset_starts_a_member(mode):
    import gzip as pygzip
    eng = engine()
    a, b = _text(100000, seed=17), _text(70000, seed=19)
    d = eng.deflater(1, O.GZIP, mode)
    try:
        o1, st, c = d.feed([a], op=FINISH)
        assert st == [0] and c == [len(a)]
        o, st, c = d.feed([b"xyz"], op=MORE)
        assert o == [b""] and st == [0] and c == [0]
        d.reset([0])
        o2a, st, c = d.feed([b[:5000]], op=MORE)
        assert st == [NEED_INPUT] and c == [5000]
        o2b, st, c = d.feed([b[5000:]], op=FINISH)
        assert st == [0]
    finally:
        d.close()
    stream = o1[0] + o2a[0] + o2b[0]
    assert pygzip.decompress(stream) == a + b
    assert o1[0] == O.compress(a, O.GZIP, mode) and o2a[0] + o2b[0] == O.compress(b, O.GZIP, mode)


def test_levels_4_to_9_are_refused():
    from flate_amd._capi import FlateHipError
    eng = engine()
    for level in (4, 6, 9):
        with pytest.raises(FlateHipError):
            eng.deflater(1, O.GZIP, level)


@pytest.mark.parametrize("mode", MODES)
def test_device_memory_feeds(mode):
    import torch
    eng = engine()
    rnd = random.Random(41 + mode)
    datas = [_text(rnd.randrange(1, 300000), seed=50 + i) for i in range(20)] + [b"", bytes(200000)]
    n = len(datas)
    d = eng.deflater(n, O.ZLIB, mode)
    cuts = [sorted(rnd.randrange(len(x) + 1) for _ in range(2)) for x in datas]
    outs = [bytearray() for _ in range(n)]
    dev = torch.device("cuda:0")
    try:
        for step in range(3):
            pieces = []
            for i, x in enumerate(datas):
                pts = [0] + cuts[i] + [len(x)]
                pieces.append(x[pts[step]:pts[step + 1]])
            blob = b"".join(pieces)
            t_in = torch.tensor(list(blob) if len(blob) < 4096 else np.frombuffer(blob, dtype=np.uint8).copy(),
                                dtype=torch.uint8, device=dev) if blob else torch.zeros(1, dtype=torch.uint8, device=dev)
            in_off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum([len(p) for p in pieces], out=in_off[1:])
            caps = [len(p) + 70000 for p in pieces]
            out_off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(caps, out=out_off[1:])
            t_in_off = torch.tensor(in_off, device=dev)
            t_out_off = torch.tensor(out_off, device=dev)
            t_op = torch.full((n,), FINISH if step == 2 else MORE, dtype=torch.uint8, device=dev)
            t_out = torch.zeros(int(out_off[-1]) + 4, dtype=torch.uint8, device=dev)
            t_len = torch.zeros(n, dtype=torch.int64, device=dev)
            t_cons = torch.zeros(n, dtype=torch.int64, device=dev)
            t_st = torch.zeros(n, dtype=torch.int32, device=dev)
            eng.deflater_feed_device(d, t_in.data_ptr(), t_in_off.data_ptr(), t_op.data_ptr(), t_out.data_ptr(),
                                     t_out_off.data_ptr(), t_len.data_ptr(), t_cons.data_ptr(), t_st.data_ptr())
            torch.cuda.synchronize()
            ho = t_out.cpu().numpy()
            ln, cons, st = t_len.cpu().tolist(), t_cons.cpu().tolist(), t_st.cpu().tolist()
            for i in range(n):
                assert cons[i] == len(pieces[i]), (step, i)
                assert st[i] == (0 if step == 2 else NEED_INPUT), (step, i, st[i])
                outs[i] += ho[out_off[i]: out_off[i] + ln[i]].tobytes()
    finally:
        d.close()
    want, _ = eng.compress_many(datas, O.ZLIB, mode)
    for i in range(n):
        assert bytes(outs[i]) == want[i], i
        assert pyzlib.decompress(bytes(outs[i])) == datas[i]


def _raw_feed(eng, d, device, blob, in_off, ops, out_off):
    """flate_hip_deflater_feed as it is, on host or device memory -> (return code, outputs, statuses, consumed)"""
    from flate_amd._capi import MEM_DEVICE, MEM_HOST
    n = len(ops)
    arrs = [np.frombuffer(blob, dtype=np.uint8).copy(), np.array(in_off, dtype=np.uint64), np.array(ops, dtype=np.uint8),
            np.zeros(max(out_off), dtype=np.uint8), np.array(out_off, dtype=np.uint64), np.zeros(n, dtype=np.uint64),
            np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int32)]
    if device:
        import torch
        ts = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0") for a in arrs]
        rc = eng._L.flate_hip_deflater_feed(eng._h, d._d, *[t.data_ptr() for t in ts], MEM_DEVICE)
        torch.cuda.synchronize()
        out, _, ln, cons, st = [t.cpu().numpy() for t in ts[3:]]
    else:
        rc = eng._L.flate_hip_deflater_feed(eng._h, d._d, *[a.ctypes.data for a in arrs], MEM_HOST)
        out, _, ln, cons, st = arrs[3:]
    return rc, [out[int(out_off[i]): int(out_off[i]) + int(ln[i])].tobytes() for i in range(n)], st.tolist(), cons.tolist()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_refused_feed_touches_nothing(mode, device):
    """three streams that each cross a block; between two valid feeds, a feed with an op above FINISH and a feed whose
    offsets go back are refused as a whole, and the streams still come out as the one-shot call's"""
    from flate_amd._capi import E_INVALID_ARG
    eng = engine()
    datas = [_text(70000, seed=60 + i) for i in range(3)]
    want, _ = eng.compress_many(datas, O.GZIP, mode)
    cut = 30000
    first, rest = b"".join(x[:cut] for x in datas), b"".join(x[cut:] for x in datas)
    off1, off2 = [0, cut, 2 * cut, 3 * cut], [0, 40000, 80000, 120000]
    slots = [0, 80000, 160000, 240000]
    d = eng.deflater(3, O.GZIP, mode)
    try:
        rc, outs, st, cons = _raw_feed(eng, d, device, first, off1, [MORE] * 3, slots)
        assert rc == 0 and st == [NEED_INPUT] * 3 and cons == [cut] * 3
        assert _raw_feed(eng, d, device, rest, off2, [FINISH, 3, FINISH], slots)[0] == E_INVALID_ARG
        assert _raw_feed(eng, d, device, rest, [0, 80000, 40000, 120000], [FINISH] * 3, slots)[0] == E_INVALID_ARG
        rc, outs2, st, cons = _raw_feed(eng, d, device, rest, off2, [FINISH] * 3, slots)
        assert rc == 0 and st == [0] * 3 and cons == [40000] * 3
    finally:
        d.close()
    for i in range(3):
        assert outs[i] + outs2[i] == want[i], i


@pytest.mark.parametrize("mode", [O.HUFFMAN, O.STORE])
def test_gzip_stream_beyond_4_gib(mode):
    """4.5 GiB in 64 MiB device pieces, each stamped with its index: zlib inflates every piece back and checks CRC-32
    and ISIZE (the length mod 2^32) itself; the deflater's device memory does not grow after the first feeds."""
    import torch
    eng = engine()
    piece = 64 << 20
    n_pieces = 72  # 4.5 GiB
    dev = torch.device("cuda:0")
    base = np.frombuffer(_text(piece, seed=23), dtype=np.uint8).copy()
    t_base = torch.from_numpy(base).to(dev)
    d = eng.deflater(1, O.GZIP, mode)
    cap = piece + piece // 8 + (1 << 20)
    t_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    t_out_off = torch.tensor([0, cap], dtype=torch.int64, device=dev)
    t_in_off = torch.tensor([0, piece], dtype=torch.int64, device=dev)
    t_len = torch.zeros(1, dtype=torch.int64, device=dev)
    t_cons = torch.zeros(1, dtype=torch.int64, device=dev)
    t_st = torch.zeros(1, dtype=torch.int32, device=dev)
    inf = pyzlib.decompressobj(31)
    mem = {}
    back, tail = 0, b""
    base_rest = base[8:].tobytes()
    try:
        for k in range(n_pieces):
            t_in = t_base.clone()
            t_in[:8] = torch.tensor(list(k.to_bytes(8, "little")), dtype=torch.uint8, device=dev)
            t_op = torch.tensor([FINISH if k == n_pieces - 1 else MORE], dtype=torch.uint8, device=dev)
            eng.deflater_feed_device(d, t_in.data_ptr(), t_in_off.data_ptr(), t_op.data_ptr(), t_out.data_ptr(),
                                     t_out_off.data_ptr(), t_len.data_ptr(), t_cons.data_ptr(), t_st.data_ptr())
            torch.cuda.synchronize()
            assert t_cons.item() == piece and t_st.item() == (0 if k == n_pieces - 1 else NEED_INPUT), k
            chunk = t_out[: t_len.item()].cpu().numpy().tobytes()
            got = tail + inf.decompress(chunk)
            while len(got) >= piece:
                assert got[:8] == back.to_bytes(8, "little") and got[8:piece] == base_rest, back
                got = got[piece:]
                back += 1
            tail = got
            mem[k] = eng.device_bytes()
            del t_in
        assert inf.eof and inf.unused_data == b""
    finally:
        d.close()
    assert back == n_pieces and tail == b""
    assert mem[n_pieces - 1] <= mem[4] + (1 << 20), (mem[4], mem[n_pieces - 1])
    # the one-shot path refuses a stream of this size
    assert piece * n_pieces > 0xfffffff0


def test_python_facade_piece_equals_whole(tmp_path):
    from flate_amd import gzip as fgzip
    rnd = random.Random(61)
    data = _text(5 << 20, seed=29)
    for mod in (fgzip.huffman, fgzip.store):
        plain, pieced = io.BytesIO(), io.BytesIO()
        a = mod.compressor(plain)
        b = mod.compressor(pieced, piece=1 << 20)
        p = 0
        while p < len(data):
            k = rnd.choice([1, 100, 70000, 1 << 20, 3 << 20])
            a.write(data[p:p + k])
            b.write(data[p:p + k])
            p += k
            if rnd.random() < 0.2:
                a.flush()
                b.flush()
        a.finish()
        b.finish()
        assert pieced.getvalue() == plain.getvalue()
        assert pyzlib.decompress(pieced.getvalue(), 31) == data


def test_python_facade_compress_reads_bounded_pieces():
    from flate_amd import zlib as fzlib

    class Reader:
        def __init__(self, data):
            self.data, self.pos, self.biggest = data, 0, 0

        def read(self, n=-1):
            n = len(self.data) - self.pos if n is None or n < 0 else n
            self.biggest = max(self.biggest, n)
            b = self.data[self.pos:self.pos + n]
            self.pos += len(b)
            return b

    data = _text(3 << 20, seed=37)
    r, w = Reader(data), io.BytesIO()
    fzlib.huffman.compress(r, w, piece=256 << 10)
    assert r.biggest <= 256 << 10
    assert w.getvalue() == O.compress(data, O.ZLIB, O.HUFFMAN)


def test_gzip_tool_piece_round_trips(tmp_path):
    src = tmp_path / "in.bin"
    data = _text(3 << 20, seed=43)
    src.write_bytes(data)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gzip.py"), "--piece", str(1 << 20), "--huffman",
                    str(src)], check=True)
    gz = tmp_path / "in.bin.gz"
    assert gz.read_bytes() == O.compress(data, O.GZIP, O.HUFFMAN)
    src.unlink()
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gunzip.py"), str(gz)], check=True)
    assert src.read_bytes() == data
