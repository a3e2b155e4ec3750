"""Seekable compress on device memory (DESIGN.md §5 "Seek index"): what the fresh index of
flate_hip_compress_joined_indexed costs to get and to keep, and what reading through it gives, beside the windowed index
of flate_hip_index_build over the same stream.

    python tools/seekable_probe.py [--bytes 177244160] [--calls 7] [--ranges 4096] > profiles/seekable.txt

One stream of synth.text, gzip, level 6, joined from 65535-byte pieces:
  (a) flate_hip_compress_joined: the baseline for (b)
  (b) flate_hip_compress_joined_indexed at spacing 1 (every piece a point) and at 1 MiB: the index should cost one small
      copy and one wait
  (c) flate_hip_index_build on that stream at 64 KiB and 1 MiB spacing, with the blob's size
  (d) the fresh index of (b), with the blob's size
  (e) --ranges random 64 KiB ranges in one flate_hip_decompress_ranges call through the fresh index at spacing 1
  (f) the same ranges through (c)'s windowed index at 64 KiB
  (g) flate_hip_decompress_batch of the whole stream
  (h) the whole stream as ONE range through the fresh index at spacing 1
  (i) the floor: the pieces as independent raw streams through flate_hip_decompress_batch
Every figure is the median of --calls calls after two warm-up calls; the calls wait for the handle's stream.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("FLATE_HIP_PRELOAD_TORCH_HIP", "1")

PIECE = 65535
GZIP, RAW = 1, 0
LEVEL = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=177_244_160)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--ranges", type=int, default=4096)
    args = ap.parse_args()
    print("python tools/seekable_probe.py " + " ".join(sys.argv[1:]))
    import torch
    from flate_amd import Engine, synth
    assert torch.cuda.is_available(), "seekable_probe needs a GPU"
    eng = Engine(0)
    n = args.bytes
    text = synth.text(synth.SEED_TEXT + 7, n)
    t_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()

    def dev(a, dtype=np.int64):
        return torch.from_numpy(np.array(a, dtype=dtype)).cuda()

    def timed(call):
        call()
        call()
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts)

    def ms(t):
        return "median %.3f ms (min %.3f, max %.3f)" % (t[0] * 1e3, t[1] * 1e3, t[2] * 1e3)

    def profile(call):
        eng.profile_enable(True)
        eng.profile_reset()
        call()
        for k, (t, cnt) in sorted(eng.profile_read().items()):
            if cnt:
                print("    %-20s %9.3f ms  %d launches" % (k, t, cnt))
        eng.profile_enable(False)

    # ---- (a), (b), (d): the stream and its fresh index
    cap = (eng.joined_bound(n, PIECE, GZIP, LEVEL) + 7) & ~7
    t_inoff, t_outoff = dev([0, n]), dev([0, cap])
    t_z = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    t_zlen, t_zst = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def joined():
        eng.compress_joined_device(t_text.data_ptr(), t_inoff.data_ptr(), 1, PIECE, GZIP, LEVEL, t_z.data_ptr(), t_outoff.data_ptr(),
                                   t_zlen.data_ptr(), t_zst.data_ptr())

    def indexed(spacing):
        return eng.compress_joined_indexed_device(t_text.data_ptr(), t_inoff.data_ptr(), 1, PIECE, GZIP, LEVEL, t_z.data_ptr(),
                                                  t_outoff.data_ptr(), t_zlen.data_ptr(), t_zst.data_ptr(), spacing=spacing)

    a = timed(joined)
    z_len = int(t_zlen[0])
    assert int(t_zst[0]) == 0
    print("stream: %d bytes of text, gzip level %d joined from %d-byte pieces, %d bytes compressed" % (n, LEVEL, PIECE, z_len))
    print("(a) flate_hip_compress_joined: %s, input %.2f GB/s" % (ms(a), n / a[0] / 1e9))
    fresh, bt, ct = {}, {}, {}
    for spacing in (1, 1 << 20):
        b = bt[spacing] = timed(lambda: eng.index_destroy(indexed(spacing)))
        ix = indexed(spacing)
        assert int(t_zst[0]) == 0 and int(t_zlen[0]) == z_len
        npts, blob = eng.index_info(ix, 0)[2], len(eng.index_export(ix))
        fresh[spacing] = ix
        print("(b) flate_hip_compress_joined_indexed, spacing %d: %s, input %.2f GB/s: %.3f ms over (a)"
              % (spacing, ms(b), n / b[0] / 1e9, (b[0] - a[0]) * 1e3))
        print("(d) the fresh index, spacing %d: %d points, blob %d bytes = %.4f %% of the compressed stream, %.4f %% of its output; "
              "no device memory" % (spacing, npts, blob, 100.0 * blob / z_len, 100.0 * blob / n))
    profile(lambda: eng.index_destroy(indexed(1)))

    # ---- (g), (c): decode and build over the packed stream
    t_zoff = dev([0, z_len])
    ocap = (n + 64 + 7) & ~7
    t_ooff = dev([0, ocap])
    t_out = torch.zeros(ocap + 64, dtype=torch.uint8, device="cuda")
    t_len, t_cons = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    t_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def decompress():
        eng.decompress_device(t_z.data_ptr(), t_zoff.data_ptr(), 1, GZIP, 0, t_out.data_ptr(), t_ooff.data_ptr(), t_len.data_ptr(),
                              t_st.data_ptr(), t_cons.data_ptr())

    def build(spacing):
        return eng.index_build_device(t_z.data_ptr(), t_zoff.data_ptr(), 1, GZIP, 0, t_out.data_ptr(), t_ooff.data_ptr(), t_len.data_ptr(),
                                      t_st.data_ptr(), t_cons.data_ptr(), spacing)

    g = timed(decompress)
    assert int(t_st[0]) == 0 and int(t_len[0]) == n and bool((t_out[:n] == t_text).all())
    print("(g) flate_hip_decompress_batch of the whole stream: %s, output %.2f GB/s, paths %s" % (ms(g), n / g[0] / 1e9, eng.inflate_paths()))
    windowed = {}
    for spacing in (64 << 10, 1 << 20):
        c = ct[spacing] = timed(lambda: eng.index_destroy(build(spacing)))
        ix = build(spacing)
        npts, blob = eng.index_info(ix, 0)[2], len(eng.index_export(ix))
        windowed[spacing] = ix
        print("(c) flate_hip_index_build, spacing %d: %s (%.3f ms over (g)); %d points, blob %d bytes = %.2f %% of the compressed "
              "stream, %.3f %% of its output" % (spacing, ms(c), (c[0] - g[0]) * 1e3, npts, blob, 100.0 * blob / z_len, 100.0 * blob / n))

    # ---- (e), (f), (h): ranges
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
        t = timed(call)
        assert int(t_s.abs().sum()) == 0 and int(t_l.sum()) == int(ooff[-1])
        for j in check:
            assert bool((t_o[int(ooff[j]):int(ooff[j + 1])] == t_text[begins[j]:begins[j] + lens[j]]).all()), j
        return t, int(ooff[-1]), call

    rng = np.random.default_rng(11)
    begins = [int(x) for x in rng.integers(0, n - 65536, args.ranges)]
    lens = [65536] * len(begins)
    e, total, call_e = ranges_call(fresh[1], begins, lens, range(0, len(begins), 97))
    print("(e) %d random ranges of 65536 bytes through the fresh index, spacing 1: %s, output %.2f GB/s, parts direct | scratch %s, "
          "%d passes" % (len(begins), ms(e), total / e[0] / 1e9, eng.index_parts(), eng.index_passes()))
    profile(call_e)
    f, total, call_f = ranges_call(windowed[64 << 10], begins, lens, range(0, len(begins), 97))
    print("(f) the same ranges through the windowed index, spacing 65536: %s, output %.2f GB/s, %d passes"
          % (ms(f), total / f[0] / 1e9, eng.index_passes()))
    profile(call_f)
    h, total, call_h = ranges_call(fresh[1], [0], [n], [0])
    print("(h) the whole stream as ONE range through the fresh index, spacing 1: %s, output %.2f GB/s, parts direct | scratch %s"
          % (ms(h), n / h[0] / 1e9, eng.index_parts()))
    profile(call_h)
    for ix in list(fresh.values()) + list(windowed.values()):
        eng.index_destroy(ix)

    # ---- (i): the pieces as independent raw streams
    chunk_off = np.minimum(np.arange(0, n + PIECE, PIECE, dtype=np.int64), n)
    if chunk_off[-1] == chunk_off[-2]:
        chunk_off = chunk_off[:-1]
    k = len(chunk_off) - 1
    caps = [(eng.compress_bound(int(q - p), RAW, LEVEL) + 7) & ~7 for p, q in zip(chunk_off[:-1], chunk_off[1:])]
    slot = np.zeros(k + 1, np.int64)
    slot[1:] = np.cumsum(caps)
    t_coff, t_slot = dev(chunk_off), dev(slot)
    t_c = torch.zeros(int(slot[-1]) + 64, dtype=torch.uint8, device="cuda")
    t_clen, t_cst = torch.zeros(k, dtype=torch.int64, device="cuda"), torch.zeros(k, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.compress_device(t_text.data_ptr(), t_coff.data_ptr(), k, RAW, LEVEL, t_c.data_ptr(), t_slot.data_ptr(), t_clen.data_ptr(), t_cst.data_ptr())
    torch.cuda.synchronize()
    assert int(t_cst.abs().sum()) == 0
    # (each stream's input slot ends where the next begins: the decoder is told the slot, and stops at the final block)
    ocaps = [(int(q - p) + 64 + 7) & ~7 for p, q in zip(chunk_off[:-1], chunk_off[1:])]
    oslot = np.zeros(k + 1, np.int64)
    oslot[1:] = np.cumsum(ocaps)
    t_oslot = dev(oslot)
    t_o = torch.zeros(int(oslot[-1]) + 64, dtype=torch.uint8, device="cuda")
    t_l, t_cn = torch.zeros(k, dtype=torch.int64, device="cuda"), torch.zeros(k, dtype=torch.int64, device="cuda")
    t_s = torch.zeros(k, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def pieces():
        eng.decompress_device(t_c.data_ptr(), t_slot.data_ptr(), k, RAW, 0, t_o.data_ptr(), t_oslot.data_ptr(), t_l.data_ptr(), t_s.data_ptr(),
                              t_cn.data_ptr())
    i = timed(pieces)
    assert int(t_s.abs().sum()) == 0 and int(t_l.sum()) == n
    print("(i) the floor: %d pieces as independent raw streams through flate_hip_decompress_batch: %s, output %.2f GB/s, paths %s"
          % (k, ms(i), n / i[0] / 1e9, eng.inflate_paths()))
    print("summary: index for free? (b) - (a) = %.3f ms at spacing 1 against (c) - (g) = %.3f ms at 64 KiB; blob fresh | windowed above.  "
          "ranges: (e) %.3f ms against (f) %.3f ms: %s.  whole stream: (h) %.3f ms against (g) %.3f ms: %s; floor (i) %.3f ms"
          % ((bt[1][0] - a[0]) * 1e3, (ct[64 << 10][0] - g[0]) * 1e3, e[0] * 1e3, f[0] * 1e3, "met" if e[0] <= f[0] else "MISSED", h[0] * 1e3, g[0] * 1e3,
             "met" if h[0] <= g[0] else "MISSED", i[0] * 1e3))


if __name__ == "__main__":
    main()
