#!/usr/bin/env python3
"""Which HIP calls and kernels the inflate entry points make, in order: thirteen small calls that between them take every
way through decompress_core, flate_hip_decompress_batch_dict, flate_hip_decompressed_sizes, flate_hip_decompress_members
and flate_hip_decompress_ranges (with flate_hip_index_build's walk in front of it), for comparing two builds of the library
(a change to its host code should leave both lists as they are).

  rocprofv3 --hip-runtime-trace --kernel-trace -f csv -d DIR -- python tools/inflate_calls.py run
  python tools/inflate_calls.py list DIR > calls.txt        (once per build; then diff the two files)

`run` and `list` work as those of tools/compress_calls.py do (every call three times between two pairs of device
synchronisations; `list` is that tool's, with this one's names)."""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compress_calls  # noqa: E402

NAMES = ["device batch, long streams: spans", "device batch, streams of 32 KiB and more: k_inflate_par",
         "pageable batch, tight slots: dense copy-out", "pageable batch, slots of 16 x the size: packed copy-out",
         "pinned in and out, three sub-batches", "dict batch, host memory", "dict batch, device memory",
         "sizes, long streams: spans", "sizes, short streams", "members by scan", "members by walk (zlib)",
         "members, more candidates than allowed: walk", "index build and ranges in two passes, host memory"]
REPEATS = compress_calls.REPEATS


def deflate(data, wbits, zdict=None):
    c = zlib.compressobj(6, zlib.DEFLATED, wbits, zdict=zdict) if zdict is not None else zlib.compressobj(6, zlib.DEFLATED, wbits)
    return c.compress(data) + c.flush()


def run():
    os.environ.setdefault("FLATE_HIP_PRELOAD_TORCH_HIP", "1")  # one HIP runtime per process (flate_amd/_capi.py)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from flate_amd import Engine, synth, _capi
    eng, L = Engine(0), _capi.lib()
    text = synth.text(synth.SEED_TEXT, 8 << 20).tobytes()

    missed = []  # calls that went another way than their name says (the listing is then of no use: said at the end)

    def took(ok, paths):
        if not ok:
            missed.append(str(paths))

    def offsets(sizes):
        off = np.zeros(len(sizes) + 1, dtype=np.uint64)
        np.cumsum(np.array(sizes, dtype=np.uint64), out=off[1:])
        return off

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    def device_call(plain, knobs, path):
        """a raw batch on device memory; path: the entry of Engine.inflate_paths() that must have counted"""
        streams = [deflate(p, -15) for p in plain]
        slots = [(len(p) + 7) & ~7 for p in plain]
        d_in, d_inoff, d_outoff = dev(np.frombuffer(b"".join(streams), np.uint8)), dev(offsets([len(s) for s in streams])), dev(offsets(slots))
        d_out = torch.zeros(sum(slots) + 8, dtype=torch.uint8, device="cuda:0")
        d_len = torch.zeros(len(plain), dtype=torch.int64, device="cuda:0")
        d_st = torch.zeros(len(plain), dtype=torch.int32, device="cuda:0")

        def call():
            eng.decompress_device(d_in.data_ptr(), d_inoff.data_ptr(), len(plain), 0, 0, d_out.data_ptr(), d_outoff.data_ptr(),
                                  d_len.data_ptr(), d_st.data_ptr())
            torch.cuda.synchronize()
            assert not d_st.any().item() and d_len.tolist() == [len(p) for p in plain]
            took(eng.inflate_paths()[path] > 0, eng.inflate_paths())
        return call, knobs, [d_in, d_inoff, d_outoff, d_out, d_len, d_st]

    def pageable_call(plain, factor):
        streams = [deflate(p, 31) for p in plain]

        def call():
            res, st, _ = eng.decompress_many(streams, 1, 0, caps=[factor * len(p) for p in plain])
            assert not any(st) and res == plain
        return call, {}, []

    def pinned_call(plain, knobs):
        streams = [deflate(p, 31) for p in plain]
        slots = [(len(p) + 7) & ~7 for p in plain]
        in_off, out_off = offsets([len(s) for s in streams]), offsets(slots)
        src = torch.from_numpy(np.frombuffer(b"".join(streams), np.uint8).copy()).pin_memory()
        dst = torch.zeros(int(out_off[-1]) + 8, dtype=torch.uint8).pin_memory()
        out_len, status = np.zeros(len(plain), dtype=np.uint64), np.zeros(len(plain), dtype=np.int32)

        def call():
            rc = L.flate_hip_decompress_batch(eng._h, src.data_ptr(), in_off.ctypes.data, len(plain), 1, 0, dst.data_ptr(),
                                              out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data, None, _capi.MEM_HOST)
            assert rc == 0 and not status.any() and [int(x) for x in out_len] == [len(p) for p in plain]
        return call, knobs, [src, dst]

    zdict = text[:20000]
    dict_plain = [text[30000 + 3000 * i: 30000 + 3000 * (i + 1)] for i in range(12)]
    dict_streams = [deflate(p, -15, zdict) for p in dict_plain]

    def dict_host_call():
        def call():
            res, st, _ = eng.decompress_many_dict(dict_streams, [zdict], None, 0, 0, caps=[4096] * len(dict_plain))
            assert not any(st) and res == dict_plain
        return call, {}, []

    def dict_device_call():
        n = len(dict_plain)
        d_in, d_inoff = dev(np.frombuffer(b"".join(dict_streams), np.uint8)), dev(offsets([len(s) for s in dict_streams]))
        d_outoff, d_dict, d_doff = dev(offsets([4096] * n)), dev(np.frombuffer(zdict, np.uint8)), dev(offsets([len(zdict)]))
        d_out = torch.zeros(4096 * n + 8, dtype=torch.uint8, device="cuda:0")
        d_len = torch.zeros(n, dtype=torch.int64, device="cuda:0")
        d_cons = torch.zeros(n, dtype=torch.int64, device="cuda:0")
        d_st = torch.zeros(n, dtype=torch.int32, device="cuda:0")

        def call():
            eng.decompress_dict_device(d_in.data_ptr(), d_inoff.data_ptr(), n, 0, 0, d_out.data_ptr(), d_outoff.data_ptr(), d_len.data_ptr(),
                                       d_st.data_ptr(), d_cons.data_ptr(), d_dict.data_ptr(), d_doff.data_ptr(), 1, None)
            torch.cuda.synchronize()
            assert not d_st.any().item() and d_len.tolist() == [len(p) for p in dict_plain]
        return call, {}, [d_in, d_inoff, d_outoff, d_dict, d_doff, d_out, d_len, d_cons, d_st]

    def sizes_call(plain, path):
        streams = [deflate(p, 31) for p in plain]

        def call():
            sizes, st, _ = eng.decompressed_sizes(streams, 1)
            assert not any(st) and sizes == [len(p) for p in plain]
            took(eng.size_paths()[path] > 0, eng.size_paths())
        return call, {}, []

    def members_call(wbits, container, knobs, path):
        plain = [text[100000 * i: 100000 * i + 60000] for i in range(6)]
        streams = [b"".join(deflate(p[a:a + 20000], wbits) for a in range(0, len(p), 20000)) for p in plain]

        def call():
            res, st, _, members = eng.decompress_members(streams, container, 0, caps=[65536] * len(plain))
            assert not any(st) and res == plain and members == [3] * len(plain)
            took(eng.member_paths()[path] == len(plain), eng.member_paths())
        return call, knobs, []

    def ranges_call():
        plain = [text[: 4 << 20], text[4 << 20: (4 << 20) + 300000]]
        streams = [deflate(p, 31) for p in plain]
        ranges = [(1, 5, 1000), (0, 100, 1 << 20), (0, (2 << 20) + 300000, 900000)]   # 1 MiB and a little | what does not fit behind it

        def call():
            ix, res, st, _ = eng.build_index(streams, 1)
            assert not any(st) and res == plain
            got, rst = ix.read_ranges(ranges)
            assert not any(rst) and got == [plain[s][b:b + n] for s, b, n in ranges]
            took(eng.index_passes() == 2, eng.index_passes())
            ix.close()
        return call, {"FLATE_HIP_INDEX_PASS_BYTES": str(3 << 19)}, []

    six = [text[70000 * i: 70000 * i + n] for i, n in enumerate((70000, 1234, 4097, 517, 800, 12345))]
    calls = [
        device_call([text[: 4 << 20], text[4 << 20:]], {}, "span_done"),
        device_call([text[200000 * i: 200000 * (i + 1)] for i in range(8)], {"FLATE_HIP_INFLATE_SPANS": "0"}, "par_done"),
        pageable_call(six, 1),
        pageable_call(six, 16),
        pinned_call([text[5000 * i: 5000 * i + 300 + 200 * i] for i in range(20)], {"FLATE_HIP_HOST_PASS_CHUNKS": "2"}),   # 7 + 7 + 6 streams
        dict_host_call(),
        dict_device_call(),
        sizes_call([text[: 4 << 20], text[4 << 20:]], 0),
        sizes_call(six, 1),
        members_call(31, 1, {}, 0),
        members_call(15, 2, {}, 1),
        members_call(31, 1, {"FLATE_HIP_MEMBER_CANDIDATES": "0"}, 1),
        ranges_call(),
    ]
    assert len(calls) == len(NAMES)
    for call, knobs, _keep in calls:
        os.environ.update(knobs)
        eng._sync_env()
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            torch.cuda.synchronize()
            call()
            torch.cuda.synchronize()
            torch.cuda.synchronize()
        for k in knobs:
            del os.environ[k]
    print("inflate_calls: %d calls x %d done" % (len(calls), REPEATS))
    if missed:
        sys.exit("inflate_calls: a call did not go the way it is named for: " + "; ".join(missed))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        compress_calls.listing(sys.argv[2], NAMES)
    else:
        sys.exit(__doc__)
