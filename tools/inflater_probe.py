#!/usr/bin/env python3
"""Resumable inflate vs the one-shot batch: the config-2 batch (16385 level-6 streams of 65535 bytes, 1 GiB)
decoded by flate_hip_decompress_batch and by an inflater fed each stream in 1, 2, 4 and 16 equal pieces, alternated in
one process, device memory throughout (MEM_DEVICE, set_sync(0), one wait per run).  Then one long stream fed in 1 MiB
pieces.  Prints one JSON line per measurement.  usage: inflater_probe.py [reps]"""
import os
os.environ.setdefault("FLATE_HIP_PRELOAD_TORCH_HIP", "1")
import json
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from flate_amd import Engine, synth  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    eng = Engine(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    n, size = 16385, 65535
    text = synth.text(synth.SEED_TEXT, n * size).tobytes()
    chunks = [text[i * size:(i + 1) * size] for i in range(n)]
    comp, s = eng.compress_many(chunks, 0, 6)
    assert s == [0] * n
    total_out = n * size
    slot = 1 << 16
    lens = np.array([len(c) for c in comp], dtype=np.int64)
    with torch.cuda.stream(st):
        d_in = torch.from_numpy(np.frombuffer(b"".join(comp), dtype=np.uint8).copy()).to(dev)
        base = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        base[1:] = torch.from_numpy(np.cumsum(lens)).to(dev)
        d_lens = torch.from_numpy(lens).to(dev)
        out_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * slot
        d_out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        d_len = torch.empty(n, dtype=torch.int64, device=dev)
        d_cons = torch.empty(n, dtype=torch.int64, device=dev)
        d_st = torch.empty(n, dtype=torch.int32, device=dev)
        fin0 = torch.zeros(n, dtype=torch.uint8, device=dev)
        fin1 = torch.ones(n, dtype=torch.uint8, device=dev)
        # feed k of K: bytes [len * k / K, len * (k + 1) / K) of every stream, as offsets into the one input buffer
        feeds = {}
        for K in (1, 2, 4, 16):
            offs = []
            for k in range(K + 1):
                cut = base[:-1] + (d_lens * k) // K
                offs.append(cut)
            # piece k of stream i = in[offs[k][i], offs[k+1][i]): the offsets of one feed are not one ascending list, so
            # every feed gets its own compacted input
            lst = []
            for k in range(K):
                a, b = offs[k], offs[k + 1]
                plen = b - a
                off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
                off[1:] = torch.cumsum(plen, 0)
                idx = torch.repeat_interleave(a - off[:-1], plen) + torch.arange(int(off[-1]), device=dev)
                lst.append((d_in[idx].contiguous(), off))
            feeds[K] = lst
    eng.set_stream(st.cuda_stream)
    eng.set_sync(0)

    def one_shot():
        eng.decompress_device(d_in.data_ptr(), base.data_ptr(), n, 0, 0, d_out.data_ptr(), out_off.data_ptr(),
                              d_len.data_ptr(), d_st.data_ptr(), d_cons.data_ptr())

    def inflater(K, inf):
        inf.reset(range(n))
        for k, (buf, off) in enumerate(feeds[K]):
            # (output of every feed into the same slots: only the time is measured here; the tests check the bytes)
            eng.inflater_feed_device(inf, buf.data_ptr(), off.data_ptr(), (fin1 if k == K - 1 else fin0).data_ptr(),
                                     d_out.data_ptr(), out_off.data_ptr(), d_len.data_ptr(), d_cons.data_ptr(),
                                     d_st.data_ptr())

    inf = eng.inflater(n, 0)
    runs = [("one_shot", None)] + [("inflater_%d" % K, K) for K in (1, 2, 4, 16)]
    times = {name: [] for name, _ in runs}
    for rep in range(reps + 1):
        for name, K in runs:
            st.synchronize()
            t0 = time.perf_counter()
            one_shot() if K is None else inflater(K, inf)
            st.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                times[name].append(dt)
            sts = d_st.cpu().numpy()
            assert (sts == 0).all(), (name, np.unique(sts))
    for name, _ in runs:
        best = min(times[name])
        print(json.dumps({"probe": "inflater", "run": name, "ms": round(best * 1e3, 2),
                          "GBps": round(total_out / best / 1e9, 2), "streams": n}))
    inf.close()
    eng.set_sync(1)
    eng.set_stream(0)

    # one long stream in 1 MiB pieces (host memory, the bounded decompressor's way)
    one = synth.text(synth.SEED_TEXT + 5, 256 << 20).tobytes()
    c1, s = eng.compress_many([one], 0, 6)
    assert s == [0]
    inf = eng.inflater(1, 0)
    data, pos, out_n, t0 = c1[0], 0, 0, time.perf_counter()
    status = 104
    while status in (104, 105):
        piece = data[pos:pos + (1 << 20)]
        o, s, c = inf.feed([piece], final=pos + len(piece) >= len(data), caps=4 << 20)
        pos += c[0]
        out_n += len(o[0])
        status = s[0]
    dt = time.perf_counter() - t0
    assert status == 0 and out_n == len(one)
    print(json.dumps({"probe": "inflater", "run": "one_stream_1MiB_pieces", "ms": round(dt * 1e3, 1),
                      "GBps": round(out_n / dt / 1e9, 3), "bytes": out_n}))
    inf.close()


if __name__ == "__main__":
    main()
