"""ctypes binding of tests/cpu_shim/dict_compress_plan_shim.cpp: the host decisions of flate_hip_compress_batch_dict
(flate_amd/csrc/dict_compress_plan.h) as the library computes them -- argument checks, every stream's dictionary tail
and the too-long verdict, the passes of a batch, the staging layout and the tables of a pass of staged streams."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libdict_compress_plan_shim.so")
NONE = 0xffffffff
E_UNSUPPORTED = -5
CHUNK, STREAM, STAGED = 0, 1, 2  # fl_dictc_kind_t
HEADERS = ("dict_compress_plan.h", "dict_plan.h", "pass_plan.h", "stream_tables.h", "flate_layout.h", "flate_common.h")

_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "dict_compress_plan_shim.cpp")
        deps = [src, os.path.join(ROOT, "include", "flate_hip.h")] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in HEADERS]
        if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        u32, u64, i, p = C.c_uint32, C.c_uint64, C.c_int, C.c_void_p
        L.shim_dictc_const.argtypes = [i]
        L.shim_dictc_const.restype = u32
        L.shim_dictc_args_ok.argtypes = [i, i, p, u32, p, i, u32]
        L.shim_dictc_streams.argtypes = [p, u32, p, u32, p, p, p, p]
        L.shim_dictc_passes.argtypes = [p, p, u32, p, p, i, u64, u64, u32, p, u32]
        L.shim_dictc_passes.restype = u32
        L.shim_dictc_stage.argtypes = [p, p, u32, p, p, i, p, p, p]
        L.shim_dictc_stage.restype = u64
        _lib = L
    return _lib


def const(name):
    return int(lib().shim_dictc_const(("max_stream", "pass_streams", "stage_tail", "sizeof_job", "sizeof_chunk").index(name)))


def _off(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.array(lens, dtype=np.uint64))
    return off


def _of(dict_of):
    return None if dict_of is None else np.array([NONE if d is None else d for d in dict_of], dtype=np.uint32)


def args_ok(container, mode, dict_lens, dict_of, n_chunks):
    doff, of = _off(dict_lens), _of(dict_of)
    return bool(lib().shim_dictc_args_ok(container, mode, doff.ctypes.data, len(dict_lens), None if of is None else of.ctypes.data,
                                         int(of is not None), n_chunks))


def streams(rec_lens, dict_lens, dict_of, dict_base=0):
    """(verdict, [(dict or None, hist, t_start), ...])"""
    n = len(rec_lens)
    hin, doff, of = _off(rec_lens), _off(dict_lens) + np.uint64(dict_base), _of(dict_of)
    d, h, t = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    rc = lib().shim_dictc_streams(hin.ctypes.data, n, doff.ctypes.data, len(dict_lens), None if of is None else of.ctypes.data,
                                  d.ctypes.data, h.ctypes.data, t.ctypes.data)
    return rc, [(None if int(a) == NONE else int(a), int(b), int(c)) for a, b, c in zip(d, h, t)]


def passes(rec_lens, hists, mode=6, max_pass_chunks=32768, stream_pass_bytes=4096 << 20, pass_streams=2048):
    """[(nc, kind), ...]; hists: per stream its history length, or None (no dictionary)"""
    n = len(rec_lens)
    hin, hout = _off(rec_lens), _off([l + 64 for l in rec_lens])
    d = np.array([NONE if h is None else 0 for h in hists], np.uint32)
    h = np.array([0 if h is None else h for h in hists], np.uint32)
    out = np.zeros((n + 1, 2), np.uint32)
    k = lib().shim_dictc_passes(hin.ctypes.data, hout.ctypes.data, n, d.ctypes.data, h.ctypes.data, mode, max_pass_chunks,
                                stream_pass_bytes, pass_streams, out.ctypes.data, n + 1)
    assert k != NONE and k <= n
    return [(int(a), int(b)) for a, b in out[:k]]


STAGE_COLS = ("dst", "in_off", "in_len", "out_off", "out_cap", "n_blocks", "n_piece", "n_flush", "piece_start", "piece_end", "tgt0")


def stage(rec_lens, hists, container, caps=None, in_base=0, out_base=0):
    """(staging bytes, blocks of the pass, workspace bytes, [dict of STAGE_COLS per stream]) of one pass of staged streams"""
    n = len(rec_lens)
    hin = _off(rec_lens) + np.uint64(in_base)
    hout = _off(caps if caps is not None else [l + 64 for l in rec_lens]) + np.uint64(out_base)
    d, h = np.zeros(n, np.uint32), np.array(hists, np.uint32)
    rows = np.zeros((max(n, 1), 11), np.uint64)
    nb, ws = C.c_uint32(0), C.c_uint64(0)
    b = lib().shim_dictc_stage(hin.ctypes.data, hout.ctypes.data, n, d.ctypes.data, h.ctypes.data, container, rows.ctypes.data,
                               C.byref(nb), C.byref(ws))
    assert b != 0xffffffffffffffff
    return int(b), int(nb.value), int(ws.value), [dict(zip(STAGE_COLS, (int(x) for x in r))) for r in rows[:n]]
