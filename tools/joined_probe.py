"""Joined compress beside the two paths it stands between, on device memory (DESIGN.md §4b'''').

    python tools/joined_probe.py [--mib 256] [--calls 7] > profiles/joined.txt

synth.text, level 6; input GB/s = input bytes over the median call (a warm-up call first, one process):
  (a) flate_hip_compress_batch, raw, 65535-byte chunks: the floor -- the pieces and nothing else
  (b) the same bytes joined as ONE gzip stream, flate_hip_compress_joined
  (c) the same bytes through flate_hip_compress_batch as one gzip stream: the whole-stream path it competes with
  (d) 64 streams of 4 MiB joined (gzip)
Every row: the compressed bytes -- what dropping the history costs in ratio is (b) against (c) --, and the kernel times
(flate_hip_profile_*) of one call.  (b) and (d) are inflated by stdlib zlib.  The last lines: the handle's workspace after
(b) alone, in a handle of its own.
"""
import argparse
import os
import statistics
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("FLATE_HIP_PRELOAD_TORCH_HIP", "1")

PIECE = 65535
GZIP, RAW = 1, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--calls", type=int, default=7)
    args = ap.parse_args()
    print("python tools/joined_probe.py " + " ".join(sys.argv[1:]))
    import torch
    from flate_amd import Engine, synth
    assert torch.cuda.is_available(), "joined_probe needs a GPU"
    eng = Engine(0)
    level = 6
    total = args.mib << 20
    text = synth.text(synth.SEED_TEXT, total)
    t_in = torch.from_numpy(np.ascontiguousarray(text)).cuda()

    def dev(a):
        return torch.from_numpy(np.array(a, dtype=np.int64)).cuda()

    def measure(label, in_off, caps, joined, container, check):
        n = len(caps)
        out_off = np.zeros(n + 1, np.int64)
        out_off[1:] = np.cumsum(caps)
        t_inoff, t_outoff = dev(in_off), dev(out_off)
        t_out = torch.zeros(int(out_off[-1]) + 64, dtype=torch.uint8, device="cuda")
        t_len = torch.zeros(n, dtype=torch.int64, device="cuda")
        t_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def call(e=eng):
            if joined:
                e.compress_joined_device(t_in.data_ptr(), t_inoff.data_ptr(), n, PIECE, container, level, t_out.data_ptr(),
                                         t_outoff.data_ptr(), t_len.data_ptr(), t_st.data_ptr())
            else:
                e.compress_device(t_in.data_ptr(), t_inoff.data_ptr(), n, container, level, t_out.data_ptr(), t_outoff.data_ptr(),
                                  t_len.data_ptr(), t_st.data_ptr())
        call()  # warm-up; the calls wait for the handle's stream (set_sync 1)
        assert int(t_st.abs().sum()) == 0, t_st.cpu().numpy()[:8]
        ln = t_len.cpu().numpy()
        if check:
            for i in sorted({0, n - 1}):
                z = t_out[int(out_off[i]): int(out_off[i]) + int(ln[i])].cpu().numpy().tobytes()
                assert zlib.decompress(z, 31) == text[int(in_off[i]): int(in_off[i + 1])].tobytes(), (label, i)
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        print("%s: %d streams, level %d, %d -> %d bytes (ratio %.4f), median of %d calls %.3f ms (min %.3f, max %.3f), input %.2f GB/s"
              % (label, n, level, total, int(ln.sum()), total / float(ln.sum()), args.calls, med * 1e3, min(ts) * 1e3, max(ts) * 1e3,
                 total / med / 1e9))
        eng.profile_enable(True)
        eng.profile_reset()
        call()
        for k, (ms, cnt) in sorted(eng.profile_read().items()):
            if cnt:
                print("    %-16s %8.3f ms  %d launches" % (k, ms, cnt))
        eng.profile_enable(False)
        return med, call

    chunk_off = np.minimum(np.arange(0, total + PIECE, PIECE, dtype=np.int64), total)
    if chunk_off[-1] == chunk_off[-2]:
        chunk_off = chunk_off[:-1]
    chunk_caps = [(eng.compress_bound(int(b - a), RAW, level) + 7) & ~7 for a, b in zip(chunk_off[:-1], chunk_off[1:])]
    a, _ = measure("(a) flate_hip_compress_batch, raw, 65535-byte chunks", chunk_off, chunk_caps, False, RAW, False)
    one_off = np.array([0, total], np.int64)
    b, call_b = measure("(b) flate_hip_compress_joined, one gzip stream", one_off, [(eng.joined_bound(total, PIECE, GZIP, level) + 7) & ~7], True, GZIP, True)
    c, _ = measure("(c) flate_hip_compress_batch, one gzip stream (whole-stream path)", one_off, [(eng.compress_bound(total, GZIP, level) + 7) & ~7],
                   False, GZIP, False)
    per = total // 64
    many_off = np.arange(65, dtype=np.int64) * per
    d, _ = measure("(d) flate_hip_compress_joined, 64 gzip streams of %d bytes" % per, many_off,
                   [(eng.joined_bound(per, PIECE, GZIP, level) + 7) & ~7] * 64, True, GZIP, True)
    gbs = [total / x / 1e9 for x in (a, b, c, d)]
    print("summary: (a) %.2f GB/s  (b) %.2f GB/s  (c) %.2f GB/s  (d) %.2f GB/s  median (b) / median (a) %.3f (expected within 1.15)"
          % (gbs[0], gbs[1], gbs[2], gbs[3], b / a))
    fresh = Engine(0)
    call_b(fresh)
    print("workspace of a handle after (b) alone: %.1f MiB, of which the pieces' scratch slots and tables about %.1f MiB"
          % (fresh.workspace_bytes() / 1048576.0, (total * 1.0205 + (total / PIECE + 1) * 206) / 1048576.0))


if __name__ == "__main__":
    main()
