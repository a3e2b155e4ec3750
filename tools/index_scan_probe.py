"""The scan index on device memory (DESIGN.md §5 "Seek index"): what flate_hip_index_scan costs beside the size probe it
starts with and beside flate_hip_index_build, what its index weighs, and what reading through it gives beside the windowed
index over the same stream.

    python tools/index_scan_probe.py [--bytes 67108864] [--calls 7] [--ranges 4096] [--out profiles/index_scan.txt | --out -]

Two gzip streams of the same synth.text:
  Z  made by stdlib zlib at level 6 with Z_FULL_FLUSH every 128 KiB
  J  the library's own joined stream (flate_hip_compress_joined, level 6, 65535-byte pieces)
and for each of them, in this one process:
  (a) flate_hip_decompressed_sizes
  (b) flate_hip_index_scan at 1 MiB spacing, and at spacing 1 for the ranges below; points and blob bytes
  (c) flate_hip_index_build at 1 MiB and at 64 KiB spacing; points and blob bytes
  (d) flate_hip_decompress_batch of the whole stream
  (e) --ranges random 64 KiB ranges in one flate_hip_decompress_ranges call through the scan index at spacing 1
  (f) the same ranges through (c)'s windowed index at 64 KiB
  (h) the whole stream as ONE range through the scan index at spacing 1
Expected: (b) costs less than (c) -- no decode, no window copies --, and the ranges behave as README's seekable row: (e) is
not slower than (f), (h) is not slower than (d).  A missed expectation is printed as MISSED.
Every figure is the median of --calls calls after two warm-up calls; the calls wait for the handle's stream.  Every step
runs under an alarm of its own (--step-seconds): a step that does not end takes the process down with it.  The output goes
to --out (-: to standard output), the command as its first line.
"""
import argparse
import os
import signal
import statistics
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("FLATE_HIP_PRELOAD_TORCH_HIP", "1")

PIECE = 65535
GZIP = 1
LEVEL = 6
FLUSH_EVERY = 128 << 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=64 << 20)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "index_scan.txt"))
    args = ap.parse_args()
    out = sys.stdout if args.out == "-" else open(args.out, "w")

    def say(line):
        out.write(line + "\n")
        out.flush()

    say(("python tools/index_scan_probe.py " + " ".join(sys.argv[1:])).strip())
    import torch
    from flate_amd import Engine, synth
    assert torch.cuda.is_available(), "index_scan_probe needs a GPU"
    eng = Engine(0)
    n = args.bytes
    text = synth.text(synth.SEED_TEXT + 7, n)
    t_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()

    def dev(a, dtype=np.int64):
        return torch.from_numpy(np.array(a, dtype=dtype)).cuda()

    def step(call):
        """one GPU step under its own time limit (SIGALRM's default action ends the process)"""
        signal.alarm(args.step_seconds)
        try:
            return call()
        finally:
            signal.alarm(0)

    def timed(call):
        def run():
            call()
            call()
            ts = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
            return statistics.median(ts), min(ts), max(ts)
        return step(run)

    def ms(t):
        return "median %.3f ms (min %.3f, max %.3f)" % (t[0] * 1e3, t[1] * 1e3, t[2] * 1e3)

    def profile(call):
        def run():
            eng.profile_enable(True)
            eng.profile_reset()
            call()
            for k, (t, cnt) in sorted(eng.profile_read().items()):
                if cnt:
                    say("    %-20s %9.3f ms  %d launches" % (k, t, cnt))
            eng.profile_enable(False)
        step(run)

    # ---- the two streams
    co = zlib.compressobj(LEVEL, zlib.DEFLATED, 31)
    raw = text.tobytes()
    z = b"".join(co.compress(raw[a:a + FLUSH_EVERY]) + co.flush(zlib.Z_FULL_FLUSH) for a in range(0, n, FLUSH_EVERY)) + co.flush()
    del raw
    cap = (eng.joined_bound(n, PIECE, GZIP, LEVEL) + 7) & ~7
    t_j = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    t_jlen, t_jst = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    t_inoff, t_capoff = dev([0, n]), dev([0, cap])
    torch.cuda.synchronize()
    step(lambda: (eng.compress_joined_device(t_text.data_ptr(), t_inoff.data_ptr(), 1, PIECE, GZIP, LEVEL, t_j.data_ptr(), t_capoff.data_ptr(),
                                             t_jlen.data_ptr(), t_jst.data_ptr()), torch.cuda.synchronize()))
    assert int(t_jst[0]) == 0
    streams = (("Z", "stdlib zlib level %d, Z_FULL_FLUSH every %d bytes" % (LEVEL, FLUSH_EVERY), torch.from_numpy(np.frombuffer(z + bytes(64), np.uint8).copy()).cuda(), len(z)),
               ("J", "flate_hip_compress_joined level %d, %d-byte pieces" % (LEVEL, PIECE), t_j, int(t_jlen[0])))

    ocap = (n + 64 + 7) & ~7
    t_ooff = dev([0, ocap])
    t_out = torch.zeros(ocap + 64, dtype=torch.uint8, device="cuda")
    t_len, t_cons = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    t_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(11)
    begins = [int(x) for x in rng.integers(0, n - 65536, args.ranges)]
    lens = [65536] * len(begins)
    missed = []

    for tag, what, t_z, z_len in streams:
        say("---- stream %s: %d bytes of text as one gzip stream (%s), %d bytes compressed" % (tag, n, what, z_len))
        t_zoff = dev([0, z_len])
        torch.cuda.synchronize()

        def sizes():
            eng.decompressed_sizes_device(t_z.data_ptr(), t_zoff.data_ptr(), 1, GZIP, 0, t_len.data_ptr(), t_st.data_ptr(), t_cons.data_ptr())
            torch.cuda.synchronize()

        def scan(spacing):
            return eng.scan_index_device(t_z.data_ptr(), t_zoff.data_ptr(), 1, GZIP, 0, t_len.data_ptr(), t_st.data_ptr(), t_cons.data_ptr(), spacing)

        def build(spacing):
            return eng.index_build_device(t_z.data_ptr(), t_zoff.data_ptr(), 1, GZIP, 0, t_out.data_ptr(), t_ooff.data_ptr(), t_len.data_ptr(),
                                          t_st.data_ptr(), t_cons.data_ptr(), spacing)

        def decompress():
            eng.decompress_device(t_z.data_ptr(), t_zoff.data_ptr(), 1, GZIP, 0, t_out.data_ptr(), t_ooff.data_ptr(), t_len.data_ptr(),
                                  t_st.data_ptr(), t_cons.data_ptr())
            torch.cuda.synchronize()

        a = timed(sizes)
        assert int(t_st[0]) == 0 and int(t_len[0]) == n
        say("(a) flate_hip_decompressed_sizes: %s, paths chain | whole %s" % (ms(a), eng.size_paths()))
        scanned, built, bt, ct = {}, {}, {}, {}
        for spacing in (1 << 20, 1):
            bt[spacing] = timed(lambda: eng.index_destroy(scan(spacing)))
            ix = scanned[spacing] = step(lambda: scan(spacing))
            assert int(t_st[0]) == 0 and int(t_len[0]) == n
            say("(b) flate_hip_index_scan, spacing %d: %s (%.3f ms over (a)), walks spans | whole %s; %d points, blob %d bytes = %.4f %% of the "
                "compressed stream; no device memory" % (spacing, ms(bt[spacing]), (bt[spacing][0] - a[0]) * 1e3, eng.index_paths(),
                                                         eng.index_info(ix, 0)[2], len(eng.index_export(ix)), 100.0 * len(eng.index_export(ix)) / z_len))
        profile(lambda: eng.index_destroy(scan(1 << 20)))
        d = timed(decompress)
        assert int(t_st[0]) == 0 and int(t_len[0]) == n and bool((t_out[:n] == t_text).all())
        say("(d) flate_hip_decompress_batch of the whole stream: %s, output %.2f GB/s" % (ms(d), n / d[0] / 1e9))
        for spacing in (1 << 20, 64 << 10):
            ct[spacing] = timed(lambda: eng.index_destroy(build(spacing)))
            ix = built[spacing] = step(lambda: build(spacing))
            blob = len(step(lambda: eng.index_export(ix)))
            say("(c) flate_hip_index_build, spacing %d: %s (%.3f ms over (d)); %d points, blob %d bytes = %.2f %% of the compressed stream"
                % (spacing, ms(ct[spacing]), (ct[spacing][0] - d[0]) * 1e3, eng.index_info(ix, 0)[2], blob, 100.0 * blob / z_len))
        profile(lambda: eng.index_destroy(build(1 << 20)))

        def ranges_call(ix, begins, lens, check):
            m = len(begins)
            ooff = np.zeros(m + 1, np.int64)
            ooff[1:] = np.cumsum(lens)
            t_rs, t_rb, t_rl, t_oo = dev(np.zeros(m), np.int32), dev(begins), dev(lens), dev(ooff)
            t_o = torch.zeros(int(ooff[-1]) + 64, dtype=torch.uint8, device="cuda")
            t_l, t_s = torch.zeros(m, dtype=torch.int64, device="cuda"), torch.zeros(m, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def call():
                rc = eng.decompress_ranges_device(ix, t_z.data_ptr(), t_zoff.data_ptr(), 1, m, t_rs.data_ptr(), t_rb.data_ptr(), t_rl.data_ptr(),
                                                  t_o.data_ptr(), t_oo.data_ptr(), t_l.data_ptr(), t_s.data_ptr())
                assert rc == 0, rc
                torch.cuda.synchronize()
            t = timed(call)
            assert int(t_s.abs().sum()) == 0 and int(t_l.sum()) == int(ooff[-1])
            for j in check:
                assert bool((t_o[int(ooff[j]):int(ooff[j + 1])] == t_text[begins[j]:begins[j] + lens[j]]).all()), j
            return t, int(ooff[-1])

        e, total = ranges_call(scanned[1], begins, lens, range(0, len(begins), 97))
        say("(e) %d random ranges of 65536 bytes through the scan index, spacing 1: %s, output %.2f GB/s, parts direct | scratch %s, %d passes"
            % (len(begins), ms(e), total / e[0] / 1e9, eng.index_parts(), eng.index_passes()))
        f, total = ranges_call(built[64 << 10], begins, lens, range(0, len(begins), 97))
        say("(f) the same ranges through the windowed index, spacing 65536: %s, output %.2f GB/s, %d passes"
            % (ms(f), total / f[0] / 1e9, eng.index_passes()))
        h, total = ranges_call(scanned[1], [0], [n], [0])
        say("(h) the whole stream as ONE range through the scan index, spacing 1: %s, output %.2f GB/s, parts direct | scratch %s"
            % (ms(h), n / h[0] / 1e9, eng.index_parts()))
        for ix in list(scanned.values()) + list(built.values()):
            eng.index_destroy(ix)
        verdicts = (("the scan costs less than the build at 1 MiB", bt[1 << 20][0] < ct[1 << 20][0], bt[1 << 20][0], ct[1 << 20][0]),
                    ("ranges through the scan index are not slower than through the windowed one", e[0] <= f[0], e[0], f[0]),
                    ("the whole stream as one range is not slower than flate_hip_decompress_batch", h[0] <= d[0], h[0], d[0]))
        for text_, ok, x, y in verdicts:
            say("expected, stream %s: %s: %.3f ms against %.3f ms: %s" % (tag, text_, x * 1e3, y * 1e3, "met" if ok else "MISSED"))
            if not ok:
                missed.append((tag, text_))
    say("summary: %d of 6 expectations missed%s" % (len(missed), "".join("; %s: %s" % m for m in missed)))
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
