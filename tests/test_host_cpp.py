"""The C++ host façade (flate_amd/host/flate.hpp) mirrors the reference's public interface
(flate.zig:9-71).  CPU: it compiles and links against the C-ABI library.  GPU: the reference's
"public interface" test (flate.zig:356-481) runs through it."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host_cpp", "test_facade.cpp")
BIN = os.path.join(ROOT, "tests", "host_cpp", "test_facade")


def _build():
    from flate_amd import _capi
    assert os.path.exists(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", BIN, SRC, "-L" + os.path.dirname(_capi.LIB_PATH),
                    "-lflate_hip", "-Wl,-rpath," + os.path.dirname(_capi.LIB_PATH)], check=True)


def test_facade_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


def test_pass_plan_under_the_sanitizers():
    """tests/host_cpp/test_pass_plan.cpp: a program of its own, built with AddressSanitizer and UBSan, that walks a few
    thousand random and hostile batches (empty ones, offsets that do not grow, flush points beyond the input, nearly 2^32
    chunks) through compress_impl's chunk table, pass walk and table builder (flate_amd/csrc/pass_plan.h).  It checks that
    the passes cover the batch exactly once and that a pass's block count is the length of its block table; what the
    calls decide is tests/test_compress_plan_cpu.py's business."""
    src = os.path.join(ROOT, "tests", "host_cpp", "test_pass_plan.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_pass_plan")
    deps = [src, os.path.join(ROOT, "include", "flate_hip.h")] + [
        os.path.join(ROOT, "flate_amd", "csrc", h) for h in ("pass_plan.h", "stream_tables.h", "flate_layout.h", "flate_common.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", exe, src],
                       check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout


def test_stream_plan_under_the_sanitizers():
    """tests/host_cpp/test_stream_plan.cpp: a program of its own, built with AddressSanitizer and UBSan, that pushes random
    and hostile whole-stream passes (zero-length streams, a stream at the length limit, thousands of tiny streams, groups of
    one window, flush points on top of each other) through every rule of flate_amd/csrc/stream_plan.h.  It checks that the
    groups partition every stream's windows in order, that no window looks beyond its stream, that the stitch groups cover
    every segment once, that the regions of the wexit buffer do not overlap and that the fix loop ends; what the rules
    decide is tests/test_stream_plan_cpu.py's business."""
    src = os.path.join(ROOT, "tests", "host_cpp", "test_stream_plan.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_stream_plan")
    deps = [src] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in ("stream_plan.h", "stream_tables.h", "flate_layout.h", "flate_common.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", exe, src],
                       check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout


def test_inflate_plan_under_the_sanitizers():
    """tests/host_cpp/test_inflate_plan.cpp: a program of its own, built with AddressSanitizer and UBSan, that pushes random
    and hostile inputs (empty streams, streams at and beyond the length limit, nearly 2^32 streams, member tables with an
    empty stream, a first start that is not 0, starts that go backwards or lie beyond their stream) through every rule of
    flate_amd/csrc/inflate_plan.h and through the host's side of flate_amd/csrc/member_plan.h.  It checks that the sub-batches
    partition [0, n), that the members of an accepted table are a contiguous ascending cover of the input range and of the
    slots, that a refused table names the stream that was spoilt, that a table's capacity is never below what it holds, and
    that the tables a host feed of the resumable inflater stages describe the caller's pieces and slots from 0;
    what the rules decide is the business of tests/test_inflate_plan_cpu.py and tests/test_members_cpu.py."""
    src = os.path.join(ROOT, "tests", "host_cpp", "test_inflate_plan.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_inflate_plan")
    deps = [src] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in ("inflate_plan.h", "member_plan.h", "flate_layout.h", "flate_common.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", exe, src],
                       check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout


def test_deflater_plan_under_the_sanitizers():
    """tests/host_cpp/test_deflater_plan.cpp: a program of its own, built with AddressSanitizer and UBSan, that hands the feed
    check of flate_amd/csrc/deflater_plan.h hostile tables (offsets near 2^64, offsets that go back, ops 3..255, pieces at the
    limit and one byte above it), lays out what it accepts, and drives routing, layout and settle through random valid
    sessions.  It checks that a table is accepted exactly when it may be, that every index of a layout is inside its table
    and its staged regions are aligned and disjoint, and that every produced byte is handed out once; what the rules decide
    is tests/test_deflater_cpu.py's business."""
    src = os.path.join(ROOT, "tests", "host_cpp", "test_deflater_plan.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_deflater_plan")
    deps = [src] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in ("deflater_plan.h", "flate_layout.h", "flate_common.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", exe, src],
                       check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout


@pytest.mark.gpu
def test_facade_public_interface_on_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade ok" in r.stdout
