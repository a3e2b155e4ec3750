"""ctypes binding of tests/cpu_shim/stream_plan_shim.cpp: the host decisions of a whole-stream pass
(flate_amd/csrc/stream_plan.h) as the library computes them -- window and group tables, the windows / tiles verdict,
the wexit layout, the fix-launch verdict, the stitch tables, the workspace sizes."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libstream_plan_shim.so")
MAX_PASS_CHUNKS = 32768     # FLATE_HIP_MAX_PASS_CHUNKS default (flate_hip.hip, fl_knobs): the tile limit
SETTLED, AGAIN, GIVE_UP = 0, 1, 2   # fl_fix
FIX_FIRST = 0xffffffff              # FL_FIX_FIRST: the read behind the first launch
# fl_ws_buf, in its order
BUFS = ("tiles segs pieces fpts zones nsorted cflag S desc tokens marks entry segtok tokbase bound ntok "
        "wchunks swins links wexit NC rec jmp exitmap sgroups sgroup0 gmap gentry").split()
COMMON, WINDOWS, TILES, STITCH = 0, 1, 2, 3

_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "stream_plan_shim.cpp")
        deps = [src] + [os.path.join(ROOT, "flate_amd", "csrc", h)
                        for h in ("stream_plan.h", "stream_tables.h", "flate_layout.h", "flate_common.h")]
        if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=undefined", "-fno-sanitize-recover",
                            "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        u32, u64, i, p = C.c_uint32, C.c_uint64, C.c_int, C.c_void_p
        L.shim_stream_fix_max.restype = C.c_uint
        L.shim_bulk_min_chain.restype = C.c_uint
        L.shim_stream_deep_walk.argtypes = [u32]
        L.shim_stream_windows_allowed.argtypes = [i, i, i, u32]
        L.shim_stream_windows.argtypes = [p, u32, u32, u32, i, p, u64, p, u64, p]
        L.shim_stream_windows.restype = None
        L.shim_stream_estimate.argtypes = [p, u32, u32, u32, i, i, u64, p, p]
        L.shim_wexit_offsets.argtypes = [u32, u32, p]
        L.shim_wexit_offsets.restype = None
        L.shim_fix_verdict.argtypes = [u32, u32, u32]
        L.shim_stitch_plan.argtypes = [p, u32, p, u32, p, p]
        L.shim_stitch_plan.restype = None
        L.shim_stream_ws.argtypes = [i, p, u32, u32, p, i, p]
        L.shim_stream_links_bytes.argtypes = [u32]
        L.shim_stream_links_bytes.restype = u64
        L.shim_stream_rec_bytes.argtypes = [u64]
        L.shim_stream_rec_bytes.restype = u64
        _lib = L
    return _lib


def n_slides(n):
    """how often the reference slides its window over a stream of n bytes (stream_tables.h, add_stream_chunk)"""
    return (n - 65536) // 32768 + 1 if n >= 65536 else 0


def _streams(streams):
    """streams: lengths, or (in_off, in_len, flush_off, n_flush) tuples"""
    rows = []
    for s in streams:
        in_off, in_len, flush_off, n_flush = s if isinstance(s, tuple) else (0, s, 0, 0)
        rows.append([in_off, in_len, n_slides(in_len), flush_off, n_flush])
    return np.array(rows, dtype=np.uint64).reshape(len(rows), 5)


def windows(streams, n_cu, deep_walk=False, group_knob=0):
    """(wins, groups, meta): wins rows of (in_off, in_len, pad_, piece0, flush_off, n_flush), groups rows of
    (chunk, win0, nwin, wfirst, prev), meta a dict"""
    L, s = lib(), _streams(streams)
    meta = np.zeros(7, dtype=np.uint64)
    L.shim_stream_windows(s.ctypes.data, len(s), group_knob, n_cu, int(deep_walk), None, 0, None, 0, meta.ctypes.data)
    nw, ng = int(meta[0]), int(meta[1])
    wins = np.zeros((max(nw, 1), 6), dtype=np.uint64)
    groups = np.zeros((max(ng, 1), 5), dtype=np.uint32)
    L.shim_stream_windows(s.ctypes.data, len(s), group_knob, n_cu, int(deep_walk), wins.ctypes.data, nw, groups.ctypes.data, ng,
                          meta.ctypes.data)
    names = ("nw", "ng", "grouped", "G", "max_win", "bytes", "slots")
    return ([tuple(int(x) for x in r) for r in wins[:nw]], [tuple(int(x) for x in r) for r in groups[:ng]],
            {k: int(v) for k, v in zip(names, meta)})


def estimate(streams, n_cu, deep_walk=False, windows_knob=-1, group_knob=0, tile_limit=MAX_PASS_CHUNKS):
    """(windows?, est_new, est_old, round_cap) of a pass that may take the windows"""
    s = _streams(streams)
    est = np.zeros(2, dtype=np.float64)
    cap = C.c_uint32(0)
    w = lib().shim_stream_estimate(s.ctypes.data, len(s), group_knob, n_cu, int(deep_walk), windows_knob, tile_limit,
                                   est.ctypes.data, C.byref(cap))
    return bool(w), float(est[0]), float(est[1]), int(cap.value)


def wexit_offsets(nw, ng):
    out = np.zeros(5, dtype=np.uint64)
    lib().shim_wexit_offsets(nw, ng, out.ctypes.data)
    return dict(zip(("wexit", "gexit", "gentry", "dirty", "words"), (int(x) for x in out)))


def fix_verdict(it, flag, ng):
    return int(lib().shim_fix_verdict(it, flag, ng))


def stitch_plan(n_seg):
    """(max_seg, direct, [(piece, g), ...], group0) for pieces of n_seg[i] segments"""
    a = np.array(n_seg, dtype=np.uint32)
    meta = np.zeros(4, dtype=np.uint32)
    cap = int(sum((int(x) + 63) // 64 for x in n_seg)) + 1
    groups = np.zeros((cap, 2), dtype=np.uint32)
    group0 = np.zeros(len(a) + 1, dtype=np.uint32)
    lib().shim_stitch_plan(a.ctypes.data, len(a), groups.ctypes.data, cap, group0.ctypes.data, meta.ctypes.data)
    assert meta[2] <= cap
    return (int(meta[0]), bool(meta[1]), [tuple(int(x) for x in r) for r in groups[:int(meta[2])]],
            [int(x) for x in group0[:int(meta[3])]])


def workspace(shape, npos=0, ntiles=0, nfpts=0, nzones=0, tile_limit=MAX_PASS_CHUNKS, nseg=0, npc=0, nb=0, deep_walk=False, a=0, b=0):
    """[(buffer name, bytes), ...] in the order the driver reserves them, and tiles_per_launch"""
    dims = np.array([npos, ntiles, nfpts, nzones, tile_limit, nseg, npc, nb, int(deep_walk)], dtype=np.uint64)
    out = np.zeros((16, 2), dtype=np.uint64)
    tpl = np.zeros(1, dtype=np.uint64)
    n = lib().shim_stream_ws(shape, dims.ctypes.data, a, b, out.ctypes.data, 16, tpl.ctypes.data)
    return [(BUFS[int(r[0])], int(r[1])) for r in out[:n]], int(tpl[0])
