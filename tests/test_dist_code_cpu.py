"""fl_dist_code_p256 (flate_amd/csrc/flate_common.h: the distance code from a float's exponent, what k_lz_emit and
k_encode_wave use) against fl_dist_code (what the planner and k_encode use) for every distance, on the CPU."""
import os
import subprocess

from conftest import ROOT

SRC = r"""
#include <stdio.h>
#include "flate_common.h"
int main() {
    int bad = 0;
    for (uint32_t d = 0; d < FL_MAX_DIST; d++)
        if (fl_dist_code_p256(d) != fl_dist_code(d) + 256u) {
            if (!bad) printf("first difference at d = %u: %u, %u\n", d, fl_dist_code_p256(d), fl_dist_code(d) + 256u);
            bad++;
        }
    printf("%d differences\n", bad);
    return bad != 0;
}
"""


def test_float_distance_code_equals_the_table_form_for_every_distance(tmp_path):
    src, exe = tmp_path / "dist_code.cpp", tmp_path / "dist_code"
    src.write_text(SRC)
    for opt in ("-O0", "-O2"):
        subprocess.run(["g++", opt, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "flate_amd", "csrc"), "-o", str(exe),
                        str(src)], check=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "0 differences", (opt, r.stdout)
