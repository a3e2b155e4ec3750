"""Inflate with preset dictionaries, the part that needs no GPU: the inputs of tests/test_gpu_inflate_dict.py
(tests/_dict_cases.py) against stdlib zlib, the host-side decisions of flate_amd/csrc/dict_plan.h through a shim
(tests/cpu_shim/dict_plan_shim.cpp, built here the way tests/test_span_plan_cpu.py builds its own), and the new names of
the C ABI and its Python mirror."""
import ctypes as C
import inspect
import os
import subprocess
import zlib

import numpy as np
import pytest

import _dict_cases as dc
from conftest import ROOT

SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libdict_plan_shim.so")
DEPS = [os.path.join(ROOT, "flate_amd", "csrc", "dict_plan.h")]
NONE = 0xffffffff
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "dict_plan_shim.cpp")
        fresh = os.path.exists(SHIM_SO) and os.path.getmtime(SHIM_SO) >= max(os.path.getmtime(d) for d in [src] + DEPS)
        if not fresh:
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        L.shim_dict_const.restype = C.c_uint32
        L.shim_dict_args_ok.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_uint32]
        L.shim_dict_table.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
        _lib = L
    return _lib


# ---------------------------------------------------------------- the inputs

def test_the_families_are_all_there():
    names = set(dc.NAMES)
    nz = len(dc.LEVELS) * 2 * (len(dc.DICT_LENS) * len(dc.RECORD_LENS) + 1)
    assert sum(n.startswith("Z_") for n in names) == nz == 510
    assert dc.DICT_LENS == (1, 2, 257, 1788, 1789, 2047, 2048, 2049, 32508, 32509, 32767, 32768, 32769, 40000)
    assert dc.RECORD_LENS == (0, 1, 3, 200, 4096, 70000)
    s = [n for n in names if n.startswith("S_")]
    assert len(s) % 2 == 0 and all((n[:-6] + "_dyn" in names) for n in s if n.endswith("_fixed"))
    assert sum(n.startswith("H_") for n in names) == 13


def test_every_valid_case_is_what_zlib_inflates_it_to():
    for c in dc.CASES:
        if c.status == 0:
            assert dc.zlib_inflate(c) == c.out, c.name
            assert c.consumed == len(c.stream), c.name


def test_zlib_refuses_every_invalid_case():
    bad = [c for c in dc.CASES if c.status != 0]
    assert sorted(set(c.status for c in bad)) == [1, 6, 11, 106, 107]
    for c in bad:
        assert dc.zlib_inflate(c) is None, c.name


def test_family_z_streams_need_their_dictionary():
    """A Family Z stream of a record of 200 bytes or more does not inflate without its dictionary: the inputs really reach
    into it.  (zlib streams say so in their header; raw streams fail at the first match that reaches in front of the stream.)
    The exception, with its reason, is at _dict_cases.NEEDS_DICT_MIN: zlib never emits a match into a dictionary of 1 or 2
    bytes, whatever the record, so the RAW streams of those two dictionaries inflate without them; matches into such
    dictionaries are synthesized (S_p0_dict_of_1_byte, S_p0_dict_of_2_bytes)."""
    seen = 0
    for c in dc.CASES:
        if not c.name.startswith("Z_") or len(c.out) < 200 or len(c.zdict) == 0:
            continue
        if c.container == 0 and len(c.zdict) < dc.NEEDS_DICT_MIN:
            continue
        seen += 1
        with pytest.raises(zlib.error):
            o = zlib.decompressobj(-15 if c.container == 0 else 15)
            o.decompress(c.stream)
            assert o.eof
    assert seen == len(dc.LEVELS) * (2 * len(dc.DICT_LENS) - 2) * 3
    for form in ("fixed", "dyn"):  # ... and the synthesized ones do need theirs
        for name in ("S_p0_dict_of_1_byte_", "S_p0_dict_of_2_bytes_"):
            with pytest.raises(zlib.error):
                zlib.decompressobj(-15).decompress(dc.BY_NAME[name + form].stream)


def test_invalid_match_cases_expect_the_bytes_in_front_of_the_match():
    for form in ("fixed", "dyn"):
        assert dc.BY_NAME["S_p0_dist_hist_plus1_" + form].out == b""
        assert dc.BY_NAME["S_p3_dist_hist_plus4_" + form].out == b"ABC"
        assert dc.BY_NAME["S_d32768_wp1_dict32766_" + form].out == b"Z"
        c = dc.BY_NAME["S_d32768_wp0_dict40000_" + form]
        assert c.out[:258] == c.zdict[40000 - 32768:40000 - 32768 + 258]
        c = dc.BY_NAME["S_d32768_wp1_dict32767_" + form]
        assert c.out[1:259] == c.zdict[:258]


def test_dynamic_forms_fit_the_lookup_tables():
    assert max(dc.LL) <= 10 and max(dc.DL) <= 8 and min(dc.LL) >= 1 and min(dc.DL) >= 1


# ---------------------------------------------------------------- dict_plan.h

def args_ok(container, dict_off, dict_of, n_chunks):
    off = np.ascontiguousarray(np.array(dict_off, np.uint64))
    of = None if dict_of is None else np.ascontiguousarray(np.array(list(dict_of) + [0], np.uint32))
    return bool(lib().shim_dict_args_ok(container, off.ctypes.data, len(dict_off) - 1, None if of is None else of.ctypes.data,
                                        0 if of is None else 1, n_chunks))


def test_shim_constants():
    assert [lib().shim_dict_const(i) for i in range(3)] == [32768, NONE, 24]


def test_args_containers():
    assert args_ok(0, [0, 10], None, 3) and args_ok(2, [0, 10], None, 3)
    assert not args_ok(1, [0, 10], None, 3)  # gzip has no dictionaries
    assert not args_ok(3, [0, 10], None, 3) and not args_ok(-1, [0, 10], None, 3)


def test_args_offsets_ascend():
    assert args_ok(0, [0, 0, 0], [0, 1], 2)  # empty dictionaries
    assert args_ok(0, [5, 7, 7, 100], [2, 1, 0], 3)
    assert not args_ok(0, [5, 4], None, 1)
    assert not args_ok(0, [0, 10, 9], [0], 1)


def test_args_dict_of():
    assert args_ok(0, [0, 10, 20], [0, 1, NONE, 1], 4)
    assert not args_ok(0, [0, 10, 20], [0, 2], 2)        # index out of range
    assert not args_ok(0, [0, 10, 20], [0, NONE - 1], 2)
    assert not args_ok(0, [0, 10, 20], None, 2)          # NULL only with exactly one dictionary
    assert not args_ok(0, [0], None, 2)
    assert args_ok(0, [0], [NONE, NONE], 2)              # no dictionaries at all: every stream says "none"
    assert not args_ok(0, [0], [0], 1)


def test_table_tail_and_hist_len():
    lens = [0, 1, 32767, 32768, 32769, 40000, 5]
    off = np.zeros(len(lens) + 1, np.uint64)
    off[0] = 7
    off[1:] = 7 + np.cumsum(lens)
    n = len(lens)
    start, end, hist, adler = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.ones(n, np.uint32)
    lib().shim_dict_table(off.ctypes.data, n, start.ctypes.data, end.ctypes.data, hist.ctypes.data, adler.ctypes.data)
    assert [int(x) for x in start] == [int(x) for x in off[:-1]]
    assert [int(x) for x in end] == [int(x) for x in off[1:]]
    assert [int(x) for x in hist] == [0, 1, 32767, 32768, 32768, 32768, 5]
    assert [int(e) - int(h) for e, h in zip(end, hist)] == [int(off[i + 1]) - min(lens[i], 32768) for i in range(n)]  # tail start
    assert not adler.any()  # the device fills it


def test_dict_plan_under_sanitizers():
    """tests/host_cpp/test_dict_plan.cpp: a program of its own, built with AddressSanitizer and UBSan, that checks the argument
    rules and the table over random and hostile offset tables held in exactly-sized heap arrays."""
    src = os.path.join(ROOT, "tests", "host_cpp", "test_dict_plan.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_dict_plan")
    if not (os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(d) for d in [src] + DEPS)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", exe, src],
                       check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "dict_plan ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- names

def test_new_symbols_and_status_names():
    from flate_amd import _capi
    L = _capi.lib()
    for s in ("flate_hip_decompress_batch_dict", "flate_hip_inflater_set_dictionary"):
        assert s in _capi.SYMBOLS and hasattr(L, s), s
    assert _capi.status_name(106) == "NeedDict" and _capi.status_name(107) == "WrongDict"
    assert (_capi.ST_NEED_DICT, _capi.ST_WRONG_DICT, _capi.INFLATER_NEED_DICT, _capi.DICT_NONE) == (106, 107, 2, NONE)
    hdr = open(os.path.join(ROOT, "include", "flate_hip.h")).read()
    for text in ("FLATE_HIP_ST_NEED_DICT = 106", "FLATE_HIP_ST_WRONG_DICT = 107", "FLATE_HIP_INFLATER_NEED_DICT = 2",
                 "one wave"):
        assert text in hdr, text


def test_python_surface():
    from flate_amd import api, flate, gzip, zlib as fzlib
    from flate_amd.engine import Engine, Inflater
    assert api.NeedDict.status == 106 and api.WrongDict.status == 107
    assert issubclass(api.NeedDict, api.FlateError) and issubclass(api.WrongDict, api.FlateError)
    assert api._ERRORS[106] is api.NeedDict and api._ERRORS[107] is api.WrongDict
    for mod in (flate, fzlib, gzip):
        for fn in (mod.decompress, mod.decompressor):
            p = inspect.signature(fn).parameters["zdict"]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert list(inspect.signature(Engine.decompress_many_dict).parameters)[1:] == ["streams", "dicts", "dict_of", "container",
                                                                                   "flags", "caps"]
    assert hasattr(Engine, "decompress_dict_device") and hasattr(Inflater, "set_dictionary")
    # gzip has no preset dictionaries: refused before anything touches a device
    with pytest.raises(ValueError):
        gzip.decompressor(b"", zdict=b"abc")
    with pytest.raises(ValueError):
        gzip.decompressor(b"", piece=4096, zdict=b"abc")
