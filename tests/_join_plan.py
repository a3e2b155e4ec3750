"""ctypes binding of tests/cpu_shim/join_plan_shim.cpp: the host decisions of flate_hip_compress_joined
(flate_amd/csrc/join_plan.h) as the library computes them -- argument checks, the pieces of a stream, the streams and piece
tables of a call, the bound, the scratch slots, the marker's length."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libjoin_plan_shim.so")
HEADERS = ("join_plan.h", "flate_common.h")
CONSTS = ("max_piece", "marker_max", "slot_align", "slot_spare", "max_pieces", "sizeof_stream")
STREAM_COLS = ("in_off", "n", "out_off", "out_cap", "piece0", "n_pieces")

_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "join_plan_shim.cpp")
        deps = [src, os.path.join(ROOT, "include", "flate_hip.h")] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in HEADERS]
        if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        u32, u64, i, p = C.c_uint32, C.c_uint64, C.c_int, C.c_void_p
        L.shim_join_const.argtypes = [i]
        L.shim_join_const.restype = u64
        L.shim_join_args_ok.argtypes = [u32, i, i]
        L.shim_join_piece_bytes.argtypes = [u32]
        L.shim_join_piece_bytes.restype = u32
        L.shim_join_marker_bytes.argtypes = [u32]
        L.shim_join_marker_bytes.restype = u32
        L.shim_join_raw_bound.argtypes = [u64]
        L.shim_join_raw_bound.restype = u64
        L.shim_join_bound.argtypes = [u64, u32, i]
        L.shim_join_bound.restype = u64
        L.shim_join_slot_bytes.argtypes = [u32]
        L.shim_join_slot_bytes.restype = u64
        L.shim_join_piece_count.argtypes = [u64, u32]
        L.shim_join_piece_count.restype = u64
        L.shim_join_layout.argtypes = [p, p, u32, u32, u64, u64, p]
        L.shim_join_layout.restype = u64
        L.shim_join_piece_of.argtypes = [u64, u64, u32, u64, p]
        L.shim_join_tables.argtypes = [p, p, u32, u32, u64, p, p, p]
        L.shim_join_tables.restype = u64
        _lib = L
    return _lib


def const(name):
    return int(lib().shim_join_const(CONSTS.index(name)))


def args_ok(piece_bytes, container, mode):
    return bool(lib().shim_join_args_ok(piece_bytes, container, mode))


def piece_bytes(piece):
    return int(lib().shim_join_piece_bytes(piece))


def marker_bytes(residue):
    return int(lib().shim_join_marker_bytes(residue))


def raw_bound(n):
    return int(lib().shim_join_raw_bound(n))


def bound(n, piece, container):
    return int(lib().shim_join_bound(n, piece, container))


def slot_bytes(n):
    return int(lib().shim_join_slot_bytes(n))


def piece_count(n, piece):
    return int(lib().shim_join_piece_count(n, piece))


def _off(lens, base=0):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.array(lens, dtype=np.uint64))
    return off + np.uint64(base)


def layout(lens, caps, piece, in_base=0, out_base=0, in_shift=0, out_shift=0):
    """(pieces of the call, [dict of STREAM_COLS per stream])"""
    n = len(lens)
    hin, hout = _off(lens, in_base), _off(caps, out_base)
    rows = np.zeros((max(n, 1), 6), np.uint64)
    total = lib().shim_join_layout(hin.ctypes.data, hout.ctypes.data, n, piece, in_shift, out_shift, rows.ctypes.data)
    return int(total), [dict(zip(STREAM_COLS, (int(x) for x in r))) for r in rows[:n]]


def piece_of(in_off, n, piece, k):
    """(in_off, in_len, last) of piece k of a stream of n bytes"""
    out = np.zeros(3, np.uint64)
    lib().shim_join_piece_of(in_off, n, piece, k, out.ctypes.data)
    return int(out[0]), int(out[1]), bool(out[2])


def tables(lens, piece, in_base=0):
    """(scratch bytes, piece -> stream, the pieces' input offsets, their scratch slots) of a call"""
    n = len(lens)
    total, _ = layout(lens, [0] * n, piece, in_base)
    hin, hout = _off(lens, in_base), _off([0] * n)
    ps, pin, pslot = np.zeros(total, np.uint32), np.zeros(total + 1, np.uint64), np.zeros(total + 1, np.uint64)
    b = lib().shim_join_tables(hin.ctypes.data, hout.ctypes.data, n, piece, total, ps.ctypes.data, pin.ctypes.data, pslot.ctypes.data)
    assert b != 0xffffffffffffffff
    return int(b), [int(x) for x in ps], [int(x) for x in pin], [int(x) for x in pslot]
