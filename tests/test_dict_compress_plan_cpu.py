"""CPU tests of flate_amd/csrc/dict_compress_plan.h, the host decisions of flate_hip_compress_batch_dict, through
tests/cpu_shim/dict_compress_plan_shim.cpp -- and the stand-alone program that walks the header under the sanitizers."""
import os
import subprocess

import pytest

import _dict_compress_plan as P

ROOT = P.ROOT


def test_constants():
    assert P.const("max_stream") == 65535
    assert P.const("pass_streams") == 2048
    assert P.const("sizeof_job") == 40


def test_argument_errors():
    for mode in (4, 5, 6, 7, 8, 9):
        assert P.args_ok(0, mode, [10], None, 3)
        assert P.args_ok(2, mode, [10], None, 3)
    for mode in (-1, 0, 1, 2, 3, 10):
        assert not P.args_ok(0, mode, [10], None, 3)
    assert not P.args_ok(1, 6, [10], None, 3)            # gzip
    assert not P.args_ok(3, 6, [10], None, 3)
    assert not P.args_ok(0, 6, [10, 20], None, 3)        # dict_of == NULL with two dictionaries
    assert not P.args_ok(0, 6, [], None, 3)              # ... and with none
    assert P.args_ok(0, 6, [10, 20], [0, 1, None], 3)
    assert not P.args_ok(0, 6, [10, 20], [0, 2, None], 3)  # index out of range
    assert P.args_ok(0, 6, [], [None, None], 2)
    assert P.args_ok(2, 6, [0], [0, 0], 2)               # the empty dictionary is one


def test_tail_start_and_history_length():
    rc, s = P.streams([10, 20, 30, 40, 0], [0, 5, 32768, 40000], [0, 1, 2, 3, None], dict_base=100)
    assert rc == 0
    assert s[0] == (0, 0, 100)
    assert s[1] == (1, 5, 100)
    assert s[2] == (2, 32768, 105)
    assert s[3] == (3, 32768, 105 + 32768 + 40000 - 32768)  # the last 32768 bytes
    assert s[4] == (None, 0, 0)
    rc, s = P.streams([7, 8], [300], None)                  # dict_of == NULL: everyone uses dictionary 0
    assert rc == 0 and s == [(0, 300, 0), (0, 300, 0)]


def test_too_long_verdict_at_65535_and_65536():
    for d, D in ((0, 0), (1, 1), (4095, 4095), (32768, 32768), (40000, 32768)):
        assert P.streams([65535 - D], [d], None)[0] == 0
        assert P.streams([65536 - D], [d], None)[0] == P.E_UNSUPPORTED
        assert P.streams([5, 65536 - D, 5], [d], [0, 0, 0])[0] == P.E_UNSUPPORTED
        assert P.streams([5, 65536 - D, 5], [d], [0, None, 0])[0] == 0   # without a dictionary any length goes
    assert P.streams([1 << 20], [10], [None])[0] == 0


def test_passes_are_runs_of_one_kind():
    H = 32768
    # chunk, chunk | staged x3 | stream (a long input without a dictionary) | chunk | staged (the empty dictionary)
    lens = [100, 65535, 200, 300, 0, 65536, 5, 50]
    hist = [None, None, H, 5, H, None, None, 0]
    assert P.passes(lens, hist) == [(2, P.CHUNK), (3, P.STAGED), (1, P.STREAM), (1, P.CHUNK), (1, P.STAGED)]
    # at most pass_streams staged streams a pass, whatever their size
    assert P.passes([10] * 10, [H] * 10, pass_streams=4) == [(4, P.STAGED), (4, P.STAGED), (2, P.STAGED)]
    assert P.passes([10] * 5000, [H] * 5000) == [(2048, P.STAGED), (2048, P.STAGED), (904, P.STAGED)]
    # ... and at most stream_pass_bytes staged bytes (history included); the first stream is always taken
    assert P.passes([1000] * 6, [1000] * 6, stream_pass_bytes=4000) == [(2, P.STAGED)] * 3
    assert P.passes([1000] * 3, [1000] * 3, stream_pass_bytes=10) == [(1, P.STAGED)] * 3
    # chunk passes end at FLATE_HIP_MAX_PASS_CHUNKS
    assert P.passes([10] * 7, [None] * 7, max_pass_chunks=3) == [(3, P.CHUNK), (3, P.CHUNK), (1, P.CHUNK)]


@pytest.mark.parametrize("container", [0, 2])
def test_staged_offsets_and_tables(container):
    lens = [0, 1, 300, 65535, 0, 15, 16, 17, 32767, 200]
    hist = [0, 32768, 5, 0, 32768, 1, 16, 15, 32768, 32768]
    caps = [3, 64, 400, 70000, 4, 64, 64, 64, 33000, 5]
    bytes_, nb, ws, rows = P.stage(lens, hist, container, caps, in_base=77, out_base=1000)
    end = 0
    out_at = 1000
    for n, h, cap, r in zip(lens, hist, caps, rows):
        assert r["dst"] % 16 == 0 and r["dst"] >= end          # aligned, not overlapping
        end = r["dst"] + ((n + h + 15) & ~15)
        assert r["in_off"] == r["dst"] and r["in_len"] == n + h  # the staged stream is the pass's input
        assert r["n_piece"] == 1 and (r["piece_start"], r["piece_end"]) == (h, n + h)  # no piece for the history
        assert r["n_flush"] == (1 if h else 0) and r["tgt0"] == h
        assert r["n_blocks"] == n // 32768 + 1                  # the record's blocks alone: no marker
        shift = 4 if container == 2 else 0
        assert r["out_off"] == out_at + shift and r["out_cap"] == max(cap - shift, 0)
        out_at += cap
    assert bytes_ >= end + P.const("stage_tail")
    assert nb == sum(n // 32768 + 1 for n in lens)
    assert ws == bytes_ + len(lens) * (P.const("sizeof_job") + P.const("sizeof_chunk"))


def test_staging_is_bounded_per_pass():
    """16384 records against a 32 KiB dictionary are staged 2048 at a time: 2048 x (32768 + 200 rounded up + 16) bytes"""
    assert P.passes([200] * 16384, [32768] * 16384) == [(2048, P.STAGED)] * 8
    bytes_, _, ws, _ = P.stage([200] * 2048, [32768] * 2048, 0)
    assert bytes_ == 2048 * (32976 + 16) + P.const("stage_tail") and ws < 70 << 20


def test_dict_compress_plan_under_the_sanitizers():
    """tests/host_cpp/test_dict_compress_plan.cpp: a program of its own, built with AddressSanitizer and UBSan"""
    src = os.path.join(ROOT, "tests", "host_cpp", "test_dict_compress_plan.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_dict_compress_plan")
    deps = [src, os.path.join(ROOT, "include", "flate_hip.h")] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in P.HEADERS]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", exe, src],
                       check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout
