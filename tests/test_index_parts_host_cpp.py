"""flate_amd/csrc/index_parts_plan.h, the host decisions of the fresh seek index, under the sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_index_parts_plan_under_the_sanitizers():
    """tests/host_cpp/test_index_parts_plan.cpp: a program of its own, built with AddressSanitizer and UBSan, that writes the
    version-2 blobs of a few hundred random fresh indexes and runs a few thousand truncated, bit-flipped and field-mutated
    copies of them, each in a heap array of exactly its size, through the validator: every one is refused, or accepted with
    all the invariants true that the part decoder relies on (counts inside the blob, ascending points inside their streams,
    no window anywhere).  It also cuts hostile ranges -- begins near 2^64, begin + len past it, slots too small, begins and
    ends on points and beside them -- and checks every part table against the definition.  What the calls decide is
    tests/test_index_parts_plan_cpu.py's business."""
    src = os.path.join(ROOT, "tests", "host_cpp", "test_index_parts_plan.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_index_parts_plan")
    deps = [src] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in ("index_parts_plan.h", "index_plan.h", "size_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", exe, src],
                       check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout
