"""Host-buffer batches at production shapes, at the DEFAULT sub-batch knobs: many small records, many passes, the pass
boundaries of the schedule (tests/_pass_plan.py, flate_amd/csrc/pass_plan.h), and what a handle keeps on the device
afterwards.  Host batches with pinned buffers (or pageable ones of 8 MiB and more: pinned mirrors) and planned device
batches of more than one pass alternate their passes between two compute streams; their workspace is two slices of the
largest pass, so it must not grow with the batch.  Every stream is compared with the oracle (a sample that holds every
pass boundary where the oracle is too slow for all of them) and with a call that takes another way: device memory, or
FLATE_HIP_ONE_COMPUTE_STREAM=1."""
import contextlib
import os

import numpy as np
import pytest

import _oracle as O
import _pass_plan as P

pytestmark = pytest.mark.gpu

REC = 100                 # bytes a record
RECORDS_BYTES = 64 << 20  # 671089 records
MAX_CHUNK = 65535


@pytest.fixture(scope="module")
def texts():
    from flate_amd import synth
    return {"text": synth.text(synth.SEED_TEXT + 21, RECORDS_BYTES),
            "silesia": synth.silesia_like(synth.SEED_TEXT + 22, RECORDS_BYTES)}


@contextlib.contextmanager
def knob(name, value):
    """a FLATE_HIP_* knob for the calls inside (an Engine reads its knobs again when it sees them change)"""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def fresh_engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flate_amd import Engine
    eng = Engine(0)
    eng._sync_env()
    return eng


@pytest.fixture
def engines():
    """fresh handles, closed whatever way the test ends (a handle keeps its workspace until then)"""
    made = []

    def make():
        made.append(fresh_engine())
        return made[-1]
    yield make
    for eng in made:
        eng.close()


def offsets(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(sizes, dtype=np.uint64), out=off[1:])
    return off


def slots(eng, sizes, container, mode):
    caps = np.array([(eng.compress_bound(int(s), container, mode) + 7) & ~7 for s in np.unique(sizes)], dtype=np.uint64)
    cap_of = dict(zip(np.unique(sizes).tolist(), caps.tolist()))
    return offsets([cap_of[int(s)] for s in sizes])


def host_batch(eng, data, off, out_off, container, mode, pin_in=False, pin_out=False):
    """flate_hip_compress_batch on host buffers: pageable numpy arrays or pinned torch tensors.  Returns the output
    buffer (slots at out_off, zeros beyond what a stream produced) and the lengths."""
    import torch
    from flate_amd import _capi
    n = len(off) - 1
    if pin_in:
        h_in = torch.empty(len(data) + 8, dtype=torch.uint8).pin_memory()
        h_in[: len(data)] = torch.from_numpy(data)
        in_ptr, keep_in = h_in.data_ptr(), h_in
    else:
        keep_in = np.ascontiguousarray(data)
        in_ptr = keep_in.ctypes.data
    if pin_out:
        h_out = torch.zeros(int(out_off[-1]) + 8, dtype=torch.uint8).pin_memory()
        out_ptr, out = h_out.data_ptr(), h_out.numpy()
    else:
        out = np.zeros(int(out_off[-1]) + 8, dtype=np.uint8)
        out_ptr = out.ctypes.data
    out_len = np.zeros(n, dtype=np.uint64)
    status = np.full(n, 77, dtype=np.int32)
    rc = eng._L.flate_hip_compress_batch(eng._h, in_ptr, off.ctypes.data, n, container, mode, out_ptr,
                                         out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data, _capi.MEM_HOST)
    eng._check(rc, "flate_hip_compress_batch")
    assert not status.any(), np.flatnonzero(status)[:10]
    del keep_in
    return (out.copy() if pin_out else out), out_len


def device_batch(eng, data, off, out_off, container, mode):
    import torch
    dev = torch.device("cuda", 0)
    n = len(off) - 1
    d_in = torch.from_numpy(np.concatenate([data, np.zeros(8, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_oo = torch.from_numpy(out_off.view(np.int64)).to(dev)
    d_out = torch.zeros(int(out_off[-1]) + 8, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(n, dtype=torch.int64, device=dev)
    d_st = torch.full((n,), 77, dtype=torch.int32, device=dev)
    eng.compress_device(d_in.data_ptr(), d_off.data_ptr(), n, container, mode, d_out.data_ptr(), d_oo.data_ptr(),
                        d_len.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    return d_out.cpu().numpy(), d_len.cpu().numpy().astype(np.uint64)


def stream(out, out_off, out_len, i):
    a = int(out_off[i])
    return out[a: a + int(out_len[i])].tobytes()


def boundary_sample(n, extra=200, seed=0, **sched):
    """the first and last chunk of every pass of the schedule, and a few more"""
    passes, _ = P.schedule(n, **sched)
    idx = {c0 for c0, _, _ in passes} | {c0 + nc - 1 for c0, nc, _ in passes}
    idx |= set(np.random.default_rng(seed).integers(0, n, extra).tolist())
    return sorted(idx)


def pack(out, out_off, out_len):
    """the streams back to back, and their offsets"""
    lens = out_len.astype(np.int64)
    c_off = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(lens, out=c_off[1:].view(np.int64))
    starts = np.repeat(out_off[:-1].astype(np.int64) - c_off[:-1].astype(np.int64), lens)
    return out[np.arange(int(c_off[-1]), dtype=np.int64) + starts], c_off


def host_inflate(eng, packed, c_off, want_off, container):
    from flate_amd import _capi
    n = len(c_off) - 1
    blob = np.concatenate([packed, np.zeros(8, dtype=np.uint8)])
    out = np.zeros(int(want_off[-1]) + 8, dtype=np.uint8)
    out_len = np.zeros(n, dtype=np.uint64)
    status = np.full(n, 77, dtype=np.int32)
    consumed = np.zeros(n, dtype=np.uint64)
    rc = eng._L.flate_hip_decompress_batch(eng._h, blob.ctypes.data, c_off.ctypes.data, n, container, 0, out.ctypes.data,
                                           want_off.ctypes.data, out_len.ctypes.data, status.ctypes.data,
                                           consumed.ctypes.data, _capi.MEM_HOST)
    eng._check(rc, "flate_hip_decompress_batch")
    return out, out_len, status, consumed


def ceiling(largest, mode):
    """what two slices of `largest` chunks may hold: the LZ workspace and two block slots a chunk, each buffer grown by
    1/8 and 256 bytes (ensure), and room for the few small buffers of a call"""
    per = P.lz_chunk_bytes(mode) + 2 * P.block_bytes()
    return 2 * largest * per * 9 // 8 + 64 * 1024


@pytest.mark.parametrize("source,mode", [("text", 6), ("text", 9), ("silesia", 6), ("silesia", 9)])
def test_many_small_records_from_host_memory(engines, texts, source, mode):
    """64 MiB of 100-byte records (671089 chunks) from pageable memory: pinned mirrors, 656 sub-batches on two compute
    streams.  Sized as one slice per chunk this asked for hundreds of GiB (FLATE_HIP_E_ALLOC); every stream equals the
    oracle on a sample that holds every pass boundary and the device-memory call everywhere, and the whole batch
    inflates back from host memory."""
    data = texts[source]
    n = (len(data) + REC - 1) // REC
    sizes = np.full(n, REC, dtype=np.int64)
    sizes[-1] = len(data) - REC * (n - 1)
    off = offsets(sizes)
    eng = engines()
    ref = engines()
    sample = boundary_sample(n, extra=300, seed=mode)
    for container in (O.RAW, O.GZIP, O.ZLIB):
        out_off = slots(eng, sizes, container, mode)
        out, out_len = host_batch(eng, data, off, out_off, container, mode)
        with knob("FLATE_HIP_MAX_PASS_CHUNKS", "4096"):  # (the device-memory reference: modest HBM on a shared card)
            d_out, d_len = device_batch(ref, data, off, out_off, container, mode)
        assert np.array_equal(out_len, d_len)
        assert np.array_equal(out[: int(out_off[-1])], d_out[: int(out_off[-1])])
        for i in sample:
            want = O.compress(data[int(off[i]): int(off[i + 1])].tobytes(), container, mode)
            assert stream(out, out_off, out_len, i) == want, (container, i)
        packed, c_off = pack(out, out_off, out_len)
        back, b_len, b_st, b_cons = host_inflate(eng, packed, c_off, off, container)
        assert not b_st.any() and np.array_equal(b_len, sizes.astype(np.uint64))
        assert np.array_equal(b_cons, np.diff(c_off))
        assert np.array_equal(back[: len(data)], data)
    eng.close()
    ref.close()


@pytest.mark.parametrize("mode", [6, 9])
def test_workspace_does_not_grow_with_the_batch(engines, texts, mode):
    """What a handle keeps after a host batch of 65535-byte chunks is two slices of the largest pass: after 3073 or
    16385 chunks (1 GiB) no more than after 2559 -- 1024 + 1535, the largest merged tail there is -- and no more than
    the constants allow."""
    tile = texts["text"][: 64 * MAX_CHUNK]
    _, largest = P.schedule(2559)
    assert largest == 1535
    held = {}
    for n in (2559, 3 * 1024 + 1, 16385):
        data = np.tile(tile, (n + 63) // 64)[: n * MAX_CHUNK]
        off = offsets(np.full(n, MAX_CHUNK))
        eng = engines()
        out_off = slots(eng, np.full(n, MAX_CHUNK), O.GZIP, mode)
        out, out_len = host_batch(eng, data, off, out_off, O.GZIP, mode)  # pageable, 64 MiB or more: pinned mirrors
        held[n] = eng.workspace_bytes()
        for i in (0, n // 2, n - 1):
            assert stream(out, out_off, out_len, i) == O.compress(data[int(off[i]): int(off[i + 1])].tobytes(), O.GZIP, mode)
        eng.close()
        del data, out
    assert held[3073] <= held[2559] and held[16385] <= held[2559], held
    assert 2 * largest * P.lz_chunk_bytes(mode) <= held[2559] <= ceiling(largest, mode), held


def boundary_batch(n, texts, seed):
    """ragged chunks (most 4-20 KB: more than 8 MiB for every n here) with an empty chunk, a 65535-byte chunk and an
    incompressible one at the first and last chunk of the passes"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(4096, 20000, n)
    passes, _ = P.schedule(n)
    kinds = np.zeros(n, dtype=np.int64)  # 0 text, 1 noise
    for k, (c0, nc, _) in enumerate(passes):
        first, last = c0, c0 + nc - 1
        sizes[first], kinds[first] = ((0, 0), (MAX_CHUNK, 1), (MAX_CHUNK, 0))[k % 3]
        sizes[last], kinds[last] = ((MAX_CHUNK, 0), (0, 0), (int(rng.integers(1, MAX_CHUNK)), 1))[k % 3]
    off = offsets(sizes)
    text = texts["text"]
    data = np.empty(int(off[-1]), dtype=np.uint8)
    pos = 0
    for i in range(n):
        a, b = int(off[i]), int(off[i + 1])
        if kinds[i]:
            data[a:b] = rng.integers(0, 256, b - a, dtype=np.uint8)
        else:
            data[a:b] = text[pos: pos + b - a]
            pos = (pos + b - a) % (len(text) - 2 * MAX_CHUNK)
    return sizes, off, data


@pytest.mark.parametrize("mode", [4, 6, 9])
def test_pass_boundaries_of_the_host_path(engines, texts, mode):
    """n around the schedule's edges (one sub-batch, the merged tail, the ramp) for pinned input and output, pageable
    input and output (pinned mirrors) and pinned input with pageable output: the same streams as one compute stream
    (FLATE_HIP_ONE_COMPUTE_STREAM=1), and the oracle's at every pass boundary.  Containers 0, 1 and 2 in turn."""
    eng = engines()
    for j, n in enumerate((1024, 1025, 1535, 1536, 1537, 3071, 3072, 3073, 4097)):
        container = (j + mode) % 3
        sizes, off, data = boundary_batch(n, texts, seed=n * 10 + mode)
        assert len(data) > 8 << 20
        out_off = slots(eng, sizes, container, mode)
        with knob("FLATE_HIP_ONE_COMPUTE_STREAM", "1"):
            eng._sync_env()
            one, one_len = host_batch(eng, data, off, out_off, container, mode, pin_in=True, pin_out=True)
        eng._sync_env()
        for pin_in, pin_out in ((True, True), (False, False), (True, False)):
            out, out_len = host_batch(eng, data, off, out_off, container, mode, pin_in, pin_out)
            assert np.array_equal(out_len, one_len), (n, pin_in, pin_out)
            assert np.array_equal(out[: int(out_off[-1])], one[: int(out_off[-1])]), (n, pin_in, pin_out)
        for i in boundary_sample(n, extra=8, seed=n):
            want = O.compress(data[int(off[i]): int(off[i + 1])].tobytes(), container, mode)
            assert stream(one, out_off, one_len, i) == want, (n, container, i)
    eng.close()


@pytest.mark.parametrize("mode,container", [(6, O.GZIP), (9, O.RAW)])
def test_planned_batches_of_many_passes(engines, texts, mode, container):
    """671089 records planned once (FLATE_HIP_MAX_PASS_CHUNKS=4096: 164 passes on two streams) and enqueued three times:
    the oracle's bytes at every pass boundary each time, the same bytes every time, and the handle keeps no more than
    two slices of 4096 chunks."""
    import torch
    data = texts["text"]
    n = (len(data) + REC - 1) // REC
    sizes = np.full(n, REC, dtype=np.int64)
    sizes[-1] = len(data) - REC * (n - 1)
    off = offsets(sizes)
    with knob("FLATE_HIP_MAX_PASS_CHUNKS", "4096"):  # (the handle keeps it: compress_planned reads no knobs again)
        eng = engines()
        out_off = slots(eng, sizes, container, mode)
        plan = eng.plan_compress(off, out_off, container, mode)
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(np.concatenate([data, np.zeros(8, dtype=np.uint8)])).to(dev)
    sample = boundary_sample(n, extra=200, seed=mode, pinned=False, planned=True, max_pass=4096)
    want = {i: O.compress(data[int(off[i]): int(off[i + 1])].tobytes(), container, mode) for i in sample}
    first = None
    for rep in range(3):
        d_out = torch.full((int(out_off[-1]) + 8,), 0xA5, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(n, dtype=torch.int64, device=dev)
        d_st = torch.full((n,), 77, dtype=torch.int32, device=dev)
        eng.compress_planned(plan, d_in.data_ptr(), d_out.data_ptr(), d_len.data_ptr(), d_st.data_ptr())
        torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any(), rep
        out, out_len = d_out.cpu().numpy(), d_len.cpu().numpy().astype(np.uint64)
        for i in sample:
            assert stream(out, out_off, out_len, i) == want[i], (rep, i)
        packed, _ = pack(out, out_off, out_len)
        if first is None:
            first = (packed, out_len)
        assert np.array_equal(out_len, first[1]) and np.array_equal(packed, first[0]), rep
        assert eng.workspace_bytes() <= ceiling(4096, mode), rep
    # ... and it only enqueues (include/flate_hip.h): behind a kernel that keeps the stream busy, two calls with set_sync(0)
    # return before that kernel ends -- a host wait for the second compute stream would wait for it -- with the same bytes
    side = torch.cuda.Stream(device=dev)
    eng.set_stream(side.cuda_stream)
    eng.set_sync(False)
    outs = [torch.full((int(out_off[-1]) + 8,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(2)]
    lens = [torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(2)]
    sts = [torch.full((n,), 77, dtype=torch.int32, device=dev) for _ in range(2)]
    with torch.cuda.stream(side):
        torch.cuda._sleep(1 << 28)
        for k in range(2):
            eng.compress_planned(plan, d_in.data_ptr(), outs[k].data_ptr(), lens[k].data_ptr(), sts[k].data_ptr())
        done = torch.cuda.Event()
        done.record(side)
    still_running = not done.query()
    torch.cuda.synchronize()
    eng.set_sync(True)
    eng.set_stream(0)
    assert still_running, "compress_planned of many passes waited for the GPU"
    for k in range(2):
        assert not sts[k].cpu().numpy().any(), k
        out_len = lens[k].cpu().numpy().astype(np.uint64)
        packed, _ = pack(outs[k].cpu().numpy(), out_off, out_len)
        assert np.array_equal(out_len, first[1]) and np.array_equal(packed, first[0]), k
    eng.plan_destroy(plan)
    eng.close()


@pytest.mark.parametrize("mode", [6, 9])
def test_one_handle_big_small_big(engines, texts, mode):
    """A big host batch, a smaller one, a bigger one of other data, on one handle: each the bytes of the same batch on a
    fresh handle -- a slice that kept a token count, a flag or a histogram of the call before would show here."""
    batches = []
    for k, (n, lo, hi) in enumerate(((5000, 1000, 10000), (1600, 0, 4000), (9000, 1000, 9000))):
        rng = np.random.default_rng(100 + k)
        sizes = rng.integers(lo, hi, n)
        sizes[rng.integers(0, n, n // 50)] = MAX_CHUNK
        sizes[rng.integers(0, n, n // 50)] = 0
        off = offsets(sizes)
        src = texts["silesia" if k == 2 else "text"]
        start = int(rng.integers(0, len(src) - int(off[-1])))
        batches.append((sizes, off, src[start: start + int(off[-1])].copy(), O.GZIP if k != 1 else O.ZLIB))
    eng = engines()
    got = []
    for sizes, off, data, container in batches:
        out_off = slots(eng, sizes, container, mode)
        got.append((out_off,) + host_batch(eng, data, off, out_off, container, mode, pin_in=True, pin_out=True))
    eng.close()
    for (sizes, off, data, container), (out_off, out, out_len) in zip(batches, got):
        ref = engines()
        r_out, r_len = host_batch(ref, data, off, out_off, container, mode, pin_in=True, pin_out=True)
        ref.close()
        assert np.array_equal(out_len, r_len) and np.array_equal(out[: int(out_off[-1])], r_out[: int(out_off[-1])])
        for i in boundary_sample(len(sizes), extra=5, seed=len(sizes)):
            assert stream(out, out_off, out_len, i) == O.compress(data[int(off[i]): int(off[i + 1])].tobytes(), container, mode)
