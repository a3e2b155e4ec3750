"""The CPU build of the serial block planner (tests/cpu_shim/planner_shim.cpp: flate_amd/csrc/flate_common.h, the exact
source one GPU lane per block executes) and a Python model of the bit packers on top of it.  No GPU.
Shared by test_planner_cpu.py and test_block_synth_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libplanner_shim.so")
NO_INPUT = 0xFFFFFFFF


class Plan(C.Structure):
    _fields_ = [("type", C.c_uint32), ("size_bits", C.c_uint32), ("hdr_nbits", C.c_uint32),
                ("final_block", C.c_uint32), ("in_start", C.c_uint32), ("in_len", C.c_uint32),
                ("tok_start", C.c_uint32), ("tok_count", C.c_uint32), ("valid", C.c_uint32),
                ("no_input", C.c_uint32), ("q1_gap", C.c_uint32), ("pad_", C.c_uint32), ("bit_off", C.c_uint64), ("hdr", C.c_uint8 * 640),
                ("lit", C.c_uint16 * (2 * 286)), ("dist", C.c_uint16 * (2 * 30))]


_shim = None


def load_shim():
    """Build (when stale) and load the CPU build of the planner."""
    global _shim
    if _shim is not None:
        return _shim
    src = os.path.join(SHIM_DIR, "planner_shim.cpp")
    deps = [src] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in ("flate_common.h", "flate_layout.h", "stream_tables.h")]
    if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=undefined", "-fno-sanitize-recover",
                        "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
    lib = C.CDLL(SHIM_SO)
    lib.shim_plan_block.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.shim_huff_generate.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.shim_tables.argtypes = [C.c_void_p] * 6
    lib.shim_set_pm.argtypes = [C.c_int]
    assert lib.shim_plan_sizeof() == C.sizeof(Plan)
    _shim = lib
    return lib


class BitSink:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, nb):
        self.acc |= int(v) << self.n
        self.n += int(nb)
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def put_many(self, v, nb):
        """put(v[i], nb[i]) for every i, in order (numpy: a block has up to 65535 items)."""
        v = np.asarray(v, np.uint64)
        nb = np.asarray(nb, np.int64)
        if not v.size:
            return
        off = self.n + np.cumsum(nb) - nb
        total = self.n + int(nb.sum())
        bits = np.zeros(total + 8, np.uint8)
        for j in range(self.n):
            bits[j] = (self.acc >> j) & 1
        for j in range(int(nb.max())):
            m = nb > j
            bits[off[m] + j] = (v[m] >> np.uint64(j)) & np.uint64(1)
        whole = total // 8
        self.out += np.packbits(bits[:8 * whole], bitorder="little").tobytes()
        self.n = total - 8 * whole
        self.acc = int(np.packbits(bits[8 * whole:8 * whole + 8], bitorder="little")[0])

    def align(self):
        if self.n:
            self.out.append(self.acc & 0xFF)
        self.acc, self.n = 0, 0


def tables(lib):
    li = np.zeros(256, np.uint8); le = np.zeros(29, np.uint8); lb = np.zeros(29, np.uint8)
    dc = np.zeros(32768, np.uint8); de = np.zeros(30, np.uint8); db = np.zeros(30, np.uint16)
    lib.shim_tables(li.ctypes.data, le.ctypes.data, lb.ctypes.data, dc.ctypes.data, de.ctypes.data, db.ctypes.data)
    return li, le, lb, dc, de, db


def token_items(tokens, lc, dcodes, tabs):
    """(value, bit count) of every token's item, as the encode kernels assemble it: length code, length extra bits,
    distance code, distance extra bits (block_writer.zig:492-520)."""
    li, le, lb, dc, de, db = tabs
    t = np.asarray(tokens, np.uint32).astype(np.int64)
    m = ((t >> 23) & 1) == 1
    ll = (t >> 15) & 0xFF
    v = lc[ll, 0].astype(np.uint64)
    n = lc[ll, 1].astype(np.int64)
    if m.any():
        ml = ll[m]
        idx = li[ml].astype(np.int64)
        mv = lc[257 + idx, 0].astype(np.uint64)
        mn = lc[257 + idx, 1].astype(np.int64)
        mv |= (ml - lb[idx]).astype(np.uint64) << mn.astype(np.uint64)
        mn += le[idx]
        d = t[m] & 0x7FFF
        c = dc[d].astype(np.int64)
        mv |= dcodes[c, 0].astype(np.uint64) << mn.astype(np.uint64)
        mn += dcodes[c, 1]
        mv |= (d - db[c]).astype(np.uint64) << mn.astype(np.uint64)
        mn += de[c]
        v[m] = mv
        n[m] = mn
    return v, n


def plan_histogram(lib, mode, lit, dist, in_len=NO_INPUT, eof=0):
    """The planner on a histogram (lit WITHOUT the end-of-block count).  mode 0: BlockWriter.write, 1: huffman-only,
    2: BlockWriter.dynamicBlock."""
    l16 = np.zeros(286, np.uint16)
    d16 = np.zeros(30, np.uint16)
    l16[:] = np.asarray(lit)[:286]
    d16[:] = np.asarray(dist)[:30]
    plan = Plan()
    lib.shim_plan_block(mode, l16.ctypes.data, d16.ctypes.data, in_len, int(eof), C.addressof(plan))
    return plan


def dynamic_estimate_bits(lib, lit, dist):
    """BlockWriter.write's size estimate of the dynamic candidate for a block that can be stored: the emitted dynamic
    block plus the phantom distance symbol the estimate counts when the block has no match."""
    plan = plan_histogram(lib, 2, lit, dist)
    return plan.size_bits + (plan.dist[1] if not np.asarray(dist).any() else 0)


def encode_block(lib, mode, tokens, input_bytes, eof, dyn=False, widths=None):
    """Assemble the block bytes the way the encode kernel does: planner output + codes.
    widths (a dict): gets 'hdr' (bit count of every header item), 'sym' (of every token / input byte), 'symv' (their
    values) and 'eob'."""
    tabs = li, le, lb, dc, de, db = tables(lib)
    lit = np.zeros(286, np.uint16)
    dist = np.zeros(30, np.uint16)
    if mode == 0:
        t = np.asarray(tokens, np.uint32).astype(np.int64)
        m = ((t >> 23) & 1) == 1
        lit[:256] = np.bincount((t[~m] >> 15) & 0xFF, minlength=256)
        lit[257:] = np.bincount(li[(t[m] >> 15) & 0xFF], minlength=29)
        dist[:] = np.bincount(dc[t[m] & 0x7FFF], minlength=30)
    else:
        h = np.bincount(np.frombuffer(input_bytes, np.uint8), minlength=256)
        lit[:256] = h
    in_len = NO_INPUT if input_bytes is None else len(input_bytes)
    plan = Plan()
    lib.shim_plan_block(2 if dyn else mode, lit.ctypes.data, dist.ctypes.data, in_len, int(eof), C.addressof(plan))
    s = BitSink()
    if plan.type == 0:  # stored
        s.put(1 if eof else 0, 3)
        s.align()
        s.put(len(input_bytes), 16)
        s.put((~len(input_bytes)) & 0xFFFF, 16)
        s.out += input_bytes
        return bytes(s.out), plan
    hdr = bytes(plan.hdr)
    for i in range(plan.hdr_nbits // 8):
        s.put(hdr[i], 8)
    if plan.hdr_nbits % 8:
        s.put(hdr[plan.hdr_nbits // 8] & ((1 << (plan.hdr_nbits % 8)) - 1), plan.hdr_nbits % 8)
    lc = np.array(plan.lit, np.uint16).reshape(286, 2)
    dcodes = np.array(plan.dist, np.uint16).reshape(30, 2)
    if mode == 0:
        v, n = token_items(tokens, lc, dcodes, tabs)
    else:
        b = np.frombuffer(input_bytes, np.uint8)
        v, n = lc[b, 0], lc[b, 1].astype(np.int64)
    s.put_many(v, n)
    s.put(lc[256][0], lc[256][1])
    nbits = len(s.out) * 8 + s.n
    assert nbits == plan.size_bits, (nbits, plan.size_bits)
    s.align()
    if widths is not None:
        widths["hdr"] = np.array([8] * (plan.hdr_nbits // 8) + ([plan.hdr_nbits % 8] if plan.hdr_nbits % 8 else []), np.int64)
        widths["sym"] = n
        widths["symv"] = np.asarray(v, np.uint64)
        widths["eob"] = int(lc[256][1])
    return bytes(s.out), plan
