#!/usr/bin/env python3
"""Which HIP calls and kernels the compress entry points make, in order: five small calls that between them take every
way through compress_impl and seven whole-stream calls that take every way through compress_stream_pass (windows
ungrouped, grouped with a fix launch, given up to the tiles; tiles with the direct and the grouped stitch; the windows
of levels 8-9; a flush call at level 9), for comparing two builds of the library (a change to its host code should
leave both lists as they are).

  rocprofv3 --hip-runtime-trace --kernel-trace -f csv -d DIR -- python tools/compress_calls.py run
  python tools/compress_calls.py list DIR > calls.txt        (once per build; then diff the two files)

`run`: every call is made three times (the first allocates) between two pairs of device synchronisations, which `list`
finds again in the trace.  `list`: per call the HIP API names in the order they were called, and the kernels with their
grids in the order they were launched (by the correlation id of the launch: on two compute streams the order in which
they START is not fixed).  Addresses and times are left out."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pinned in and out, three sub-batches", "pageable, just above 8 MiB", "planned device batch of two passes",
         "flush call at level 6", "pinned, short inputs and one of 65536 bytes",
         "300 streams of 70000 bytes, level 6: windows, a workgroup per stream", "one 6 MiB stream, level 6, groups of 4 windows: one fix launch",
         "3 MiB and 5 MiB of zeros round an x, groups of 4: given up to the tiles", "1 MiB on the tiles: direct stitch",
         "9 MiB on the tiles: grouped stitch", "300 KiB, level 9, groups of 2 windows", "flush call at level 9"]
REPEATS = 3


def run():
    os.environ.setdefault("FLATE_HIP_PRELOAD_TORCH_HIP", "1")  # one HIP runtime per process (flate_amd/_capi.py)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from flate_amd import Engine, synth, _capi
    eng, L = Engine(0), _capi.lib()

    def layout(lens, mode=6):
        off = np.zeros(len(lens) + 1, dtype=np.uint64)
        np.cumsum(np.array(lens, dtype=np.uint64), out=off[1:])
        caps = np.array([(eng.compress_bound(int(x), 0, mode) + 7) & ~7 for x in lens], dtype=np.uint64)
        oo = np.zeros(len(lens) + 1, dtype=np.uint64)
        np.cumsum(caps, out=oo[1:])
        return off, oo

    def host_call(lens, pinned, knobs):
        off, oo = layout(lens)
        data = synth.text(synth.SEED_TEXT, int(off[-1]))
        out = np.zeros(int(oo[-1]) + 8, dtype=np.uint8)
        keep = [data, out]
        if pinned:
            keep = [torch.from_numpy(data).pin_memory(), torch.from_numpy(out).pin_memory()]
            src, dst = keep[0].data_ptr(), keep[1].data_ptr()
        else:
            src, dst = data.ctypes.data, out.ctypes.data
        out_len, status = np.zeros(len(lens), dtype=np.uint64), np.zeros(len(lens), dtype=np.int32)

        def call():
            rc = L.flate_hip_compress_batch(eng._h, src, off.ctypes.data, len(lens), 0, 6, dst, oo.ctypes.data,
                                            out_len.ctypes.data, status.ctypes.data, _capi.MEM_HOST)
            assert rc == 0 and not status.any() and out_len.all()
        return call, knobs, keep

    def planned_call():
        lens = [65535] * 40
        off, oo = layout(lens)
        d_in = torch.from_numpy(synth.text(synth.SEED_TEXT, int(off[-1]))).cuda()
        d_out = torch.zeros(int(oo[-1]) + 8, dtype=torch.uint8, device="cuda:0")
        d_len = torch.zeros(len(lens), dtype=torch.int64, device="cuda:0")
        d_st = torch.zeros(len(lens), dtype=torch.int32, device="cuda:0")
        knobs = {"FLATE_HIP_MAX_PASS_CHUNKS": "24"}     # 24 + 16 chunks
        state = {}

        def call():
            if "plan" not in state:
                state["plan"] = eng.plan_compress(off, oo, 0, 6)
            for _ in range(2):
                eng.compress_planned(state["plan"], d_in.data_ptr(), d_out.data_ptr(), d_len.data_ptr(), d_st.data_ptr())
            torch.cuda.synchronize()
            assert not d_st.any().item() and d_len.all().item()
        return call, knobs, [d_in, d_out, d_len, d_st]

    def flush_call(level=6):
        text = synth.text(synth.SEED_TEXT, 4 * 65535 + 1234).tobytes()

        def call():
            out, st = eng.compress_flush(text, [70000, 200000], True, 1, level)
            assert st == 0 and out
        return call, {}, []

    def stream_call(datas, level, knobs):   # whole-stream passes: every input longer than 65535 bytes
        def call():
            outs, st = eng.compress_many(datas, 0, level)
            assert not any(st) and all(outs)
        return call, knobs, []

    text = synth.text(synth.SEED_TEXT, 9 << 20).tobytes()
    groups_of_4 = {"FLATE_HIP_STREAM_WINDOWS": "1", "FLATE_HIP_STREAM_GROUP": "4"}

    calls = [
        host_call([65535] * 40, True, {"FLATE_HIP_HOST_PASS_CHUNKS": "16"}),      # 16 + 16 + 8 chunks
        host_call([65535] * 130, False, {"FLATE_HIP_HOST_PASS_CHUNKS": "64"}),     # 8.1 MiB: the mirrors, 64 + 66 chunks
        planned_call(),
        flush_call(),
        host_call([3000] * 20 + [65536] + [65535] * 20, True, {}),
        stream_call([text[70000 * i: 70000 * (i + 1)] for i in range(100)] * 3, 6, {}),
        stream_call([text[: 6 << 20]], 6, groups_of_4),
        stream_call([bytes(3 << 20) + b"x" + bytes(5 << 20)], 6, groups_of_4),   # periodic: a window's stitch does not settle
        stream_call([text[: 1 << 20]], 6, {"FLATE_HIP_STREAM_WINDOWS": "0"}),
        stream_call([text], 6, {"FLATE_HIP_STREAM_WINDOWS": "0"}),                # 288 segments in one piece
        stream_call([text[: 300 << 10]], 9, {"FLATE_HIP_STREAM_WINDOWS": "1", "FLATE_HIP_STREAM_GROUP": "2"}),
        flush_call(9),
    ]
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
    print("compress_calls: %d calls x %d done" % (len(calls), REPEATS))


def rows(d, pattern):
    out = []
    for f in glob.glob(os.path.join(d, "**", pattern), recursive=True):
        out += list(csv.DictReader(open(f)))
    return out


def listing(d, call_names=NAMES):
    """call_names: what the calls of the run are called, in order (tools/inflate_calls.py lists its own run with this)"""
    api = sorted(rows(d, "*hip_api_trace.csv"), key=lambda r: (int(r["Start_Timestamp"]), int(r["Correlation_Id"])))
    main_thread = max(set(r["Thread_Id"] for r in api), key=lambda t: sum(1 for r in api if r["Thread_Id"] == t))
    api = [r for r in api if r["Thread_Id"] == main_thread]
    kern = {}
    for r in rows(d, "*kernel_trace.csv"):
        grid = "x".join(r.get("Grid_Size_" + a, r.get("Grid_Size", "?")) for a in "XYZ")
        wg = "x".join(r.get("Workgroup_Size_" + a, r.get("Workgroup_Size", "?")) for a in "XYZ")
        kern.setdefault(int(r["Correlation_Id"]), []).append("%s grid %s block %s" % (r["Kernel_Name"].split("(")[0], grid, wg))
    # a call lies between two pairs of hipDeviceSynchronize (torch asks for the device around each of them)
    quiet = ("hipGetDevice", "hipSetDevice", "hipGetLastError", "hipPeekAtLastError", "hipGetDeviceCount")
    names = [r["Function"] for r in api]
    sync = [i for i, n in enumerate(names) if n == "hipDeviceSynchronize"]
    pairs = [(a, b) for a, b in zip(sync, sync[1:]) if all(n in quiet for n in names[a + 1:b])]
    spans = [(p[1] + 1, q[0]) for p, q in zip(pairs, pairs[1:])]
    spans = [(a, b) for a, b in spans if any(n not in quiet for n in names[a:b])]
    assert len(spans) == len(call_names) * REPEATS, (len(spans), len(sync), sorted(set(names)))
    for k, (a, b) in enumerate(spans):
        print("==== call %d (%s), repeat %d: %d HIP calls" % (k // REPEATS, call_names[k // REPEATS], k % REPEATS, b - a))
        launched = []
        for r in api[a:b]:
            print("  " + r["Function"])
            launched += sorted(kern.get(int(r["Correlation_Id"]), []))  # (a memset may be two fill kernels: in no fixed order)
        print("  ---- %d kernels" % len(launched))
        for s in launched:
            print("  " + s)


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        listing(sys.argv[2])
    else:
        sys.exit(__doc__)
