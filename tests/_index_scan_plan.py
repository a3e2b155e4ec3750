"""ctypes binding of tests/cpu_shim/index_scan_plan_shim.cpp: the host decision of flate_hip_index_scan
(flate_amd/csrc/index_scan_plan.h) as the library computes it -- the lists the device walkers hand over for one stream, to
the stream's points."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libindex_scan_plan_shim.so")
HEADERS = ("index_scan_plan.h", "index_plan.h", "size_plan.h")

_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "index_scan_plan_shim.cpp")
        deps = [src] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in HEADERS]
        if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        u64, p = C.c_uint64, C.c_void_p
        L.shim_ixs_max_entries.argtypes = [u64, u64]
        L.shim_ixs_max_entries.restype = u64
        L.shim_ixs_walk_entries.argtypes = [u64, u64]
        L.shim_ixs_walk_entries.restype = u64
        L.shim_ixs_copy_whole.argtypes = []
        L.shim_ixs_copy_whole.restype = u64
        L.shim_ixs_points.argtypes = [u64, p, p, p, p, p, p, u64, u64, p, u64]
        L.shim_ixs_points.restype = C.c_int64
        _lib = L
    return _lib


def max_entries(out_len, spacing):
    return int(lib().shim_ixs_max_entries(out_len, spacing))


def walk_entries(max_points, in_bits):
    """room a walk's list gets: max_points = 1 + out_len // spacing of the walk, in_bits = its length in the stream"""
    return int(lib().shim_ixs_walk_entries(max_points, in_bits))


def copy_whole():
    """with room for at most this many entries in a call the lists are copied back as they are, else packed first"""
    return int(lib().shim_ixs_copy_whole())


def points(walks, size, spacing):
    """walks: [dict(entries=[(in_bit, out_pos, need)], out_len, last_mark, has_mark, first)] of one stream in stream order
    -> [(in_bit, out_pos)], or None when the lists are refused ("disagrees with its probe")"""
    u64 = lambda a: np.ascontiguousarray(np.array(list(a) + [0], np.uint64))
    u32 = lambda a: np.ascontiguousarray(np.array(list(a) + [0], np.uint32))
    n = u64(len(w["entries"]) for w in walks)
    ol, lm = u64(w["out_len"] for w in walks), u64(w["last_mark"] for w in walks)
    hm, fi = u32(int(w["has_mark"]) for w in walks), u32(int(w["first"]) for w in walks)
    ent = u64(v for w in walks for e in w["entries"] for v in e)
    room = sum(len(w["entries"]) for w in walks) + 1
    pts = np.zeros((room, 2), np.uint64)
    got = int(lib().shim_ixs_points(len(walks), n.ctypes.data, ol.ctypes.data, lm.ctypes.data, hm.ctypes.data, fi.ctypes.data,
                                    ent.ctypes.data, size, spacing, pts.ctypes.data, room))
    assert got != -2, "a refusal left points behind"
    if got < 0:
        return None
    assert got <= room
    return [(int(b), int(p)) for b, p in pts[:got]]
