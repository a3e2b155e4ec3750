"""The seek index on device memory (DESIGN.md §5 "Seek index"): what building it costs and what reading through it gives.

    python tools/index_probe.py [--bytes 177244160] [--calls 7] [--ranges 4096] > profiles/index.txt

One gzip level-6 stream of synth.text (the 177 MB shape bench.py's one-stream inflate uses), made by this engine:
  (a) flate_hip_index_build (spacing 1 MiB) against flate_hip_decompress_batch of the same stream, same process: the
      difference is the walk and the window copies; the points and the blob's size as a share of the stream
  (b) --ranges random 64 KiB ranges in one flate_hip_decompress_ranges call, at spacing 256 KiB, 1 MiB and 4 MiB, against
      the only way to those bytes without an index: flate_hip_decompress_batch of the whole stream (then slices)
  (c) the whole stream as consecutive point-to-point ranges in one call, against flate_hip_decompress_batch (span path)
  (d) 128 streams of 1 MiB of text each: build against decompress
Every figure is the median of --calls calls after a warm-up; the calls wait for the handle's stream.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("FLATE_HIP_PRELOAD_TORCH_HIP", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=177_244_160)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--ranges", type=int, default=4096)
    args = ap.parse_args()
    print("python tools/index_probe.py " + " ".join(sys.argv[1:]))
    import torch
    from flate_amd import Engine, synth
    assert torch.cuda.is_available(), "index_probe needs a GPU"
    eng = Engine(0)

    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()  # (a copy: frombuffer arrays are read-only)

    def timed(call):
        call()
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts)

    class Batch:
        def __init__(self, plains):
            self.plains, self.n = plains, len(plains)
            streams, st = eng.compress_many(plains, 1, 6)
            assert not any(st)
            self.comp = sum(len(z) for z in streams)
            self.size = sum(len(p) for p in plains)
            off = np.zeros(self.n + 1, np.int64)
            off[1:] = np.cumsum([len(z) for z in streams])
            caps = [(len(p) + 64 + 7) & ~7 for p in plains]
            ooff = np.zeros(self.n + 1, np.int64)
            ooff[1:] = np.cumsum(caps)
            self.t_in, self.t_inoff, self.t_outoff = dev(np.frombuffer(b"".join(streams) + b"\0", np.uint8)), dev(off), dev(ooff)
            self.t_out = torch.zeros(int(ooff[-1]) + 64, dtype=torch.uint8, device="cuda")
            self.t_len = torch.zeros(self.n, dtype=torch.int64, device="cuda")
            self.t_cons = torch.zeros(self.n, dtype=torch.int64, device="cuda")
            self.t_st = torch.zeros(self.n, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

        def decompress(self):
            eng.decompress_device(self.t_in.data_ptr(), self.t_inoff.data_ptr(), self.n, 1, 0, self.t_out.data_ptr(), self.t_outoff.data_ptr(),
                                  self.t_len.data_ptr(), self.t_st.data_ptr(), self.t_cons.data_ptr())

        def build(self, spacing):
            return eng.index_build_device(self.t_in.data_ptr(), self.t_inoff.data_ptr(), self.n, 1, 0, self.t_out.data_ptr(),
                                          self.t_outoff.data_ptr(), self.t_len.data_ptr(), self.t_st.data_ptr(), self.t_cons.data_ptr(), spacing)

        def build_once(self, spacing):
            eng.index_destroy(self.build(spacing))

    def ranges_call(b, ix, begins, lens, check):
        m = len(begins)
        ooff = np.zeros(m + 1, np.int64)
        ooff[1:] = np.cumsum(lens)
        t_rs, t_rb, t_rl, t_oo = dev(np.zeros(m, np.int32)), dev(np.array(begins, np.int64)), dev(np.array(lens, np.int64)), dev(ooff)
        t_o = torch.zeros(int(ooff[-1]) + 64, dtype=torch.uint8, device="cuda")
        t_l, t_s = torch.zeros(m, dtype=torch.int64, device="cuda"), torch.zeros(m, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def call():
            rc = eng.decompress_ranges_device(ix, b.t_in.data_ptr(), b.t_inoff.data_ptr(), 1, m, t_rs.data_ptr(), t_rb.data_ptr(),
                                              t_rl.data_ptr(), t_o.data_ptr(), t_oo.data_ptr(), t_l.data_ptr(), t_s.data_ptr())
            assert rc == 0, rc
        t = timed(call)
        assert int(t_s.abs().sum()) == 0 and int(t_l.sum()) == int(ooff[-1])
        out = t_o.cpu().numpy()
        for j in check:
            assert out[int(ooff[j]):int(ooff[j + 1])].tobytes() == b.plains[0][begins[j]:begins[j] + lens[j]], j
        return t, int(ooff[-1]), eng.index_passes()

    # ---- (a)
    text = bytes(synth.text(synth.SEED_TEXT + 7, args.bytes))
    one = Batch([text])
    n = one.size
    d_med, d_min, d_max = timed(one.decompress)
    assert int(one.t_st[0]) == 0 and int(one.t_len[0]) == n
    print("stream: %d bytes of text, gzip level 6, %d bytes compressed" % (n, one.comp))
    print("(a) flate_hip_decompress_batch: median of %d calls %.3f ms (min %.3f, max %.3f), output %.2f GB/s, paths %s"
          % (args.calls, d_med * 1e3, d_min * 1e3, d_max * 1e3, n / d_med / 1e9, eng.inflate_paths()))
    for spacing in (1 << 20,):
        b_med, b_min, b_max = timed(lambda: one.build_once(spacing))
        ix = one.build(spacing)
        npts, blob = eng.index_info(ix, 0)[2], len(eng.index_export(ix))
        eng.index_destroy(ix)
        print("(a) flate_hip_index_build, spacing %d: median %.3f ms (min %.3f, max %.3f): %.3f ms over decompress (the walk and the "
              "window copies); %d points, blob %d bytes = %.2f %% of the compressed stream, %.3f %% of its output"
              % (spacing, b_med * 1e3, b_min * 1e3, b_max * 1e3, (b_med - d_med) * 1e3, npts, blob, 100.0 * blob / one.comp, 100.0 * blob / n))
    eng.profile_enable(True)
    eng.profile_reset()
    one.build_once(1 << 20)
    for k, (ms, cnt) in sorted(eng.profile_read().items()):
        if cnt:
            print("    %-20s %9.3f ms  %d launches" % (k, ms, cnt))
    eng.profile_enable(False)

    # ---- (b), (c)
    rng = np.random.default_rng(11)
    begins = [int(x) for x in rng.integers(0, n - 65536, args.ranges)]
    for spacing in (256 << 10, 1 << 20, 4 << 20):
        ix = one.build(spacing)
        pts = eng.index_points(ix, 0)
        (med, lo, hi), total, passes = ranges_call(one, ix, begins, [65536] * len(begins), (0, len(begins) // 2, len(begins) - 1))
        print("(b) spacing %7d: %d points, blob %d bytes; %d ranges of 65536 bytes in one call: median %.3f ms (min %.3f, max %.3f), "
              "output %.2f GB/s, %d passes; the whole stream by flate_hip_decompress_batch: %.3f ms"
              % (spacing, len(pts), len(eng.index_export(ix)), len(begins), med * 1e3, lo * 1e3, hi * 1e3, total / med / 1e9, passes, d_med * 1e3))
        if spacing == 1 << 20:
            pos = [p for _, p in pts] + [n]
            (med, lo, hi), total, passes = ranges_call(one, ix, pos[:-1], [b - a for a, b in zip(pos, pos[1:])], (0, len(pts) - 1))
            assert total == n
            print("(c) the whole stream as %d point-to-point ranges in one call: median %.3f ms (min %.3f, max %.3f), output %.2f GB/s, "
                  "%d passes; flate_hip_decompress_batch: %.3f ms, %.2f GB/s"
                  % (len(pts), med * 1e3, lo * 1e3, hi * 1e3, total / med / 1e9, passes, d_med * 1e3, n / d_med / 1e9))
            # the same ranges with room for all of them in one pass: what the passes cost
            os.environ["FLATE_HIP_INDEX_PASS_BYTES"] = str(8 << 30)
            (med, lo, hi), total, passes = ranges_call(one, ix, begins, [65536] * len(begins), (0, len(begins) - 1))
            del os.environ["FLATE_HIP_INDEX_PASS_BYTES"]
            print("(b) spacing %7d with FLATE_HIP_INDEX_PASS_BYTES=%d: median %.3f ms (min %.3f, max %.3f), output %.2f GB/s, %d passes, "
                  "workspace %d bytes" % (spacing, 8 << 30, med * 1e3, lo * 1e3, hi * 1e3, total / med / 1e9, passes, eng.workspace_bytes()))
        eng.index_destroy(ix)
    del one

    # ---- (d)
    many = Batch([bytes(synth.text(synth.SEED_TEXT + 100 + i, 1 << 20)) for i in range(128)])
    d_med, d_min, d_max = timed(many.decompress)
    b_med, b_min, b_max = timed(lambda: many.build_once(1 << 20))
    print("(d) 128 streams of 1 MiB: flate_hip_decompress_batch median %.3f ms (min %.3f, max %.3f), %.2f GB/s; flate_hip_index_build "
          "median %.3f ms (min %.3f, max %.3f), %.2f GB/s"
          % (d_med * 1e3, d_min * 1e3, d_max * 1e3, many.size / d_med / 1e9, b_med * 1e3, b_min * 1e3, b_max * 1e3, many.size / b_med / 1e9))


if __name__ == "__main__":
    main()
