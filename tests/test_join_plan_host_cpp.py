"""flate_amd/csrc/join_plan.h, the host decisions of flate_hip_compress_joined, under the sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_join_plan_under_the_sanitizers():
    """tests/host_cpp/test_join_plan.cpp: a program of its own, built with AddressSanitizer and UBSan, that walks a few
    thousand random and hostile batches (empty streams, streams of exactly k pieces and one byte off, pieces of one byte,
    offsets beyond 2^32, streams of more pieces than a call may have) through the stream table, the piece tables, the
    scratch slots and the bound.  It checks that the pieces cover every stream exactly once and in order, that the tables
    agree with fl_join_piece_of, that the slots are aligned and hold bound, marker and spare bytes, and that the closed
    form of the bound is the sum over the pieces; what the calls decide is tests/test_join_plan_cpu.py's business."""
    src = os.path.join(ROOT, "tests", "host_cpp", "test_join_plan.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_join_plan")
    deps = [src, os.path.join(ROOT, "include", "flate_hip.h")] + [
        os.path.join(ROOT, "flate_amd", "csrc", h) for h in ("join_plan.h", "flate_common.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", exe, src],
                       check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout
