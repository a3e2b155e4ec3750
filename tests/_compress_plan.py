"""ctypes binding of tests/cpu_shim/compress_plan_shim.cpp: compress_impl's host decisions (flate_amd/csrc/pass_plan.h)
as the library takes them -- the chunk table, the walk that cuts a batch into passes, a pass's block tables, the
two-stream rule with its slices, the rectangle rows.  Used by tests/test_compress_plan_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from _pass_plan import HOST_PASS_CHUNKS, MAX_PASS_CHUNKS, ROOT, SHIM_DIR

SHIM_SO = os.path.join(SHIM_DIR, "libcompress_plan_shim.so")
FL_BLOCK_BYTES = 65535      # flate_layout.h
FL_CHUNK_STRIDE = 65536
FL_SEG = 32768
MAX_LZ_CHUNK = 65535        # FLATE_HIP_MAX_LZ_CHUNK (include/flate_hip.h)

# fl_chunk (flate_layout.h)
CHUNK = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("out_cap", "<u8"), ("pos_off", "<u8"), ("in_len", "<u4"),
                  ("first_block", "<u4"), ("n_blocks", "<u4"), ("skip", "<u4"), ("piece0", "<u4"), ("n_piece", "<u4"),
                  ("flush_off", "<u4"), ("n_flush", "<u4"), ("zone_off", "<u4"), ("n_slides", "<u4"),
                  ("unfinished", "<u4"), ("pad_", "<u4")])

_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "compress_plan_shim.cpp")
        deps = [src, os.path.join(ROOT, "include", "flate_hip.h")] + [
            os.path.join(ROOT, "flate_amd", "csrc", h)
            for h in ("pass_plan.h", "stream_tables.h", "flate_layout.h", "flate_common.h")]
        if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=undefined", "-fno-sanitize-recover",
                            "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        u64, u32, i, p = C.c_uint64, C.c_uint32, C.c_int, C.c_void_p
        L.shim_sizeof_chunk.restype = C.c_uint
        L.shim_chunk_table.argtypes = [p, p, u32, u64, u64, i, i, i, p]
        L.shim_pass_walk.argtypes = [p, u64, u64, u64, i, i, i, i, i, u64, p, i]
        L.shim_pass_tables.argtypes = [p, u32, i, i, i, p, u32, i, p, u32, p, p, u32, p, p]
        L.shim_pass_tables.restype = u32
        L.shim_batch_blocks.argtypes = [p, u32, i]
        L.shim_batch_blocks.restype = u64
        L.shim_two_eligible.argtypes = [p, u64, u64, u64, i, i, i, i, u64, i, i, i]
        L.shim_two_from_plan.argtypes = [p, p, u32, p, i, p, p]
        L.shim_two_from_schedule.argtypes = [u64, u64, u64, i, i, i, p, i, p, p]
        L.shim_rect_rows.argtypes = [p, u32, i, p]
        assert L.shim_sizeof_chunk() == CHUNK.itemsize
        _lib = L
    return _lib


def _u32(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.uint32))


def _u64(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.uint64))


def _triples(buf, k):
    return [tuple(int(x) for x in buf[3 * j: 3 * j + 3]) for j in range(k)]


def chunk_table(hin, hout, in_shift=0, out_shift=0, mode=6, flush=None):
    """(ok, records): flush = None, or the FlushSpec's `finish`"""
    hin, hout = _u64(hin), _u64(hout)
    n = len(hin) - 1
    out = np.zeros(max(n, 1), dtype=CHUNK)
    ok = lib().shim_chunk_table(hin.ctypes.data, hout.ctypes.data, n, in_shift, out_shift, mode, int(flush is not None),
                                int(bool(flush)), out.ctypes.data)
    return bool(ok), out[:n]


def walk(in_len, n=None, host=HOST_PASS_CHUNKS, max_pass=MAX_PASS_CHUNKS, pinned=True, ramp=True, planned=False, mode=6,
         flush=False, stream_bytes=4096 << 20, raw=False):
    """[(c0, nc, whole_stream), ...] (raw: as an array of that shape): in_len = the inputs' lengths, or None with n chunks
    (no chunk table)"""
    if in_len is not None:
        arr = _u32(in_len)
        n, ptr = len(arr), arr.ctypes.data
    else:
        ptr = None
    args = (ptr, n, host, max_pass, int(pinned), int(ramp), int(planned), mode, int(flush), stream_bytes)
    k = lib().shim_pass_walk(*args, None, 0)
    assert k >= 0
    buf = np.zeros(3 * max(k, 1), dtype=np.uint64)
    assert lib().shim_pass_walk(*args, buf.ctypes.data, k) == k
    return buf[:3 * k].reshape(k, 3) if raw else _triples(buf, k)


def chunks_of(in_len):
    c = np.zeros(len(in_len), dtype=CHUNK)
    c["in_len"] = in_len
    return c


def pass_tables(chunks, stream=False, mode=6, flush=None, finish=True):
    """fills `chunks` (a CHUNK array: one pass) in place; flush = None, or the flush points.
    Returns (nb, blk_chunk, sblocks as (start, len, flags), (tiles, pieces, segs, flush points))"""
    L = lib()
    fpos = _u64(flush if flush is not None else [])
    cap = 1 << 16
    blk, sb = np.zeros(cap, dtype=np.uint32), np.zeros(3 * cap, dtype=np.uint32)
    n_blk, n_sb = C.c_uint32(0), C.c_uint32(0)
    st = np.zeros(4, dtype=np.uint32)
    nb = L.shim_pass_tables(chunks.ctypes.data, len(chunks), int(stream), mode, int(flush is not None), fpos.ctypes.data,
                            len(fpos), int(finish), blk.ctypes.data, cap, C.byref(n_blk), sb.ctypes.data, cap,
                            C.byref(n_sb), st.ctypes.data)
    assert n_blk.value <= cap and n_sb.value <= cap
    return int(nb), [int(x) for x in blk[:n_blk.value]], _triples(sb, n_sb.value), tuple(int(x) for x in st)


def batch_blocks(in_len, mode):
    arr = _u32(in_len)
    return int(lib().shim_batch_blocks(arr.ctypes.data, len(arr), mode))


def two_eligible(in_len, pinned_passes, planned_passes, mode, flush=False, one_stream=False, host=HOST_PASS_CHUNKS,
                 max_pass=MAX_PASS_CHUNKS):
    arr = _u32(in_len)
    return bool(lib().shim_two_eligible(arr.ctypes.data, len(arr), host, max_pass, int(pinned_passes), 1,
                                        int(planned_passes > 0), int(pinned_passes), planned_passes, mode, int(flush),
                                        int(one_stream)))


def two_from_plan(passes):
    """passes: [(nc, nb), ...] -> (on, schedule, slice_nc, slice_nb)"""
    nc, nb = _u32([a for a, _ in passes]), _u32([b for _, b in passes])
    buf, sl, on = np.zeros(3 * max(len(passes), 1), dtype=np.uint64), np.zeros(2, dtype=np.uint64), C.c_int(0)
    k = lib().shim_two_from_plan(nc.ctypes.data, nb.ctypes.data, len(passes), buf.ctypes.data, len(passes),
                                 sl.ctypes.data, C.byref(on))
    return bool(on.value), _triples(buf, k), int(sl[0]), int(sl[1])


def two_from_schedule(n, host=HOST_PASS_CHUNKS, max_pass=MAX_PASS_CHUNKS, pinned=True, ramp=True, planned=False):
    cap = n + 1
    buf, sl, on = np.zeros(3 * cap, dtype=np.uint64), np.zeros(2, dtype=np.uint64), C.c_int(0)
    k = lib().shim_two_from_schedule(n, host, max_pass, int(pinned), int(ramp), int(planned), buf.ctypes.data, cap,
                                     sl.ctypes.data, C.byref(on))
    return bool(on.value), _triples(buf, k), int(sl[0]), int(sl[1])


def rect_rows(slot, knob):
    """slot: the nc + 1 offsets of a pass's output slots -> (urows, pitch, half)"""
    arr = _u64(slot)
    out = np.zeros(3, dtype=np.uint64)
    lib().shim_rect_rows(arr.ctypes.data, len(arr) - 1, knob, out.ctypes.data)
    return tuple(int(x) for x in out)
