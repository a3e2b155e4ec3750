"""flate_amd/csrc/index_scan_plan.h, the host decision of flate_hip_index_scan, under the sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_index_scan_plan_under_the_sanitizers():
    """tests/host_cpp/test_index_scan_plan.cpp: a program of its own, built with AddressSanitizer and UBSan, that runs a few
    thousand valid lists of the scan walkers -- some with every position lifted to just below 2^64 -- through the decision
    and compares the points with a quadratic restatement of the rule, and tens of thousands of hostile ones (positions,
    lengths and needs near 2^64, lists without their start, walks that overlap, one field of a good pair of walks replaced):
    every one is refused with nothing appended, or accepted with everything true that the version-2 blob's validator asks
    of a stream's points.  What the decision decides is tests/test_index_scan_plan_cpu.py's business."""
    src = os.path.join(ROOT, "tests", "host_cpp", "test_index_scan_plan.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_index_scan_plan")
    deps = [src] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in ("index_scan_plan.h", "index_plan.h", "size_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", exe, src],
                       check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout
