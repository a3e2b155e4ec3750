#!/usr/bin/env python3
"""Resumable compress vs the one-shot batch, huffman-only gzip, device memory throughout (MEM_DEVICE, one
wait per run), best of `reps`: 1 GiB of synth.text as ONE stream, compressed by flate_hip_compress_batch and by a
deflater fed 16 / 64 / 256 MiB pieces; then 64 streams of 16 MiB in 1 / 4 / 16 feeds.  Every run's output is checked
against the one-shot bytes.  Prints one JSON line per measurement.  The piece rows also give the slowest and the median feed.  usage: deflater_probe.py [reps [MiB,MiB,..]]
(the second argument picks the piece sizes of the one-stream case and skips the rest)"""
import os
os.environ.setdefault("FLATE_HIP_PRELOAD_TORCH_HIP", "1")
import json
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from flate_amd import Engine, synth  # noqa: E402

GZIP, HUFFMAN, MORE, FINISH = 1, 1, 0, 2


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    eng = Engine(0)
    dev = torch.device("cuda", 0)

    def t(v):
        return torch.tensor(v, dtype=torch.int64, device=dev)

    def one_shot(d_in, sizes):
        n = len(sizes)
        caps = [eng.compress_bound(s, GZIP, HUFFMAN) for s in sizes]
        in_off, out_off = t([0] + list(np.cumsum(sizes))), t([0] + list(np.cumsum(caps)))
        d_out = torch.empty(sum(caps), dtype=torch.uint8, device=dev)
        d_len, d_st = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        best = 1e9
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.compress_device(d_in.data_ptr(), in_off.data_ptr(), n, GZIP, HUFFMAN, d_out.data_ptr(), out_off.data_ptr(),
                                d_len.data_ptr(), d_st.data_ptr())
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        lens = d_len.cpu().tolist()
        offs = out_off.cpu().tolist()
        return best, [d_out[offs[i]: offs[i] + lens[i]].cpu().numpy().tobytes() for i in range(n)]

    def pieced(d_in, sizes, feeds):
        """every stream in `feeds` equal pieces, all streams in each feed"""
        n = len(sizes)
        starts = np.concatenate([[0], np.cumsum(sizes)])
        best, outs, feed_ms = 1e9, None, []
        for _ in range(reps):
            d = eng.deflater(n, GZIP, HUFFMAN)
            got = [bytearray() for _ in range(n)]
            plan = []
            for f in range(feeds):
                a = [int(starts[i] + sizes[i] * f // feeds) for i in range(n)]
                b = [int(starts[i] + sizes[i] * (f + 1) // feeds) for i in range(n)]
                caps = [eng.compress_bound(b[i] - a[i], GZIP, HUFFMAN) for i in range(n)]
                # the pieces lie in the input back to back only when there is one stream; else gather them
                if n == 1:
                    src = d_in[a[0]:b[0]]
                    in_off = t([0, b[0] - a[0]])
                else:
                    src = torch.cat([d_in[a[i]:b[i]] for i in range(n)])
                    in_off = t([0] + list(np.cumsum([b[i] - a[i] for i in range(n)])))
                plan.append((src, in_off, t([0] + list(np.cumsum(caps))), sum(caps),
                             torch.full((n,), FINISH if f == feeds - 1 else MORE, dtype=torch.uint8, device=dev)))
            d_out = torch.empty(max(p[3] for p in plan), dtype=torch.uint8, device=dev)
            d_len, d_cons = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
            d_st = torch.empty(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            el, fm = 0.0, []
            for src, in_off, out_off, _, op in plan:
                t0 = time.perf_counter()
                eng.deflater_feed_device(d, src.data_ptr(), in_off.data_ptr(), op.data_ptr(), d_out.data_ptr(),
                                         out_off.data_ptr(), d_len.data_ptr(), d_cons.data_ptr(), d_st.data_ptr())
                torch.cuda.synchronize()
                el += time.perf_counter() - t0
                fm.append((time.perf_counter() - t0) * 1e3)
                lens, offs = d_len.cpu().tolist(), out_off.cpu().tolist()
                for i in range(n):
                    got[i] += d_out[offs[i]: offs[i] + lens[i]].cpu().numpy().tobytes()
            d.close()
            if el < best:
                feed_ms = sorted(fm)
            best, outs = min(best, el), [bytes(g) for g in got]
        return best, outs, feed_ms

    one = 1 << 30
    text = np.frombuffer(synth.text(synth.SEED_TEXT, one).tobytes(), dtype=np.uint8).copy()
    d_in = torch.from_numpy(text).to(dev)
    base_s, base_out = one_shot(d_in, [one])
    print(json.dumps({"case": "1 GiB one stream", "feed": "one-shot", "GB/s": round(one / base_s / 1e9, 2)}), flush=True)
    only = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else None
    for mib in only or (256, 64, 16):
        s, outs, fm = pieced(d_in, [one], one // (mib << 20))
        assert outs == base_out, mib
        print(json.dumps({"case": "1 GiB one stream", "feed": "%d MiB pieces" % mib, "GB/s": round(one / s / 1e9, 2),
                          "of_one_shot": round(base_s / s, 3), "feed_ms_max": round(fm[-1], 2),
                          "feed_ms_median": round(fm[len(fm) // 2], 2)}), flush=True)
    if only:
        return
    sizes = [16 << 20] * 64
    base_s, base_out = one_shot(d_in, sizes)
    print(json.dumps({"case": "64 x 16 MiB", "feed": "one-shot", "GB/s": round(one / base_s / 1e9, 2)}), flush=True)
    for feeds in (1, 4, 16):
        s, outs, fm = pieced(d_in, sizes, feeds)
        assert outs == base_out, feeds
        print(json.dumps({"case": "64 x 16 MiB", "feed": "%d feeds" % feeds, "GB/s": round(one / s / 1e9, 2),
                          "of_one_shot": round(base_s / s, 3), "feed_ms_max": round(fm[-1], 2),
                          "feed_ms_median": round(fm[len(fm) // 2], 2)}), flush=True)


if __name__ == "__main__":
    main()
