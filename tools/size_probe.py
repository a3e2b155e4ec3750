#!/usr/bin/env python3
"""The size probe against the decoder ("Size probe"): flate_hip_decompressed_sizes and
flate_hip_decompress_batch on the same streams, device memory throughout, alternated in one process; after a warm-up
call of each, the min / median / max of `reps` calls (each call ends with a wait).  Three inputs: the headline's 16385
level-6 streams of 65535 bytes of text, one gzip level-6 stream of 177,244,160 bytes of text, 128 gzip level-6 members
of 1 MiB of the Silesia-like buffer.  The sizes are checked against the decoder's.  Prints one JSON line per input.
usage: size_probe.py [reps >= 7]"""
import os
os.environ.setdefault("FLATE_HIP_PRELOAD_TORCH_HIP", "1")
import json
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from flate_amd import Engine, synth  # noqa: E402


def measure(eng, name, comp, container, out_sizes, reps):
    dev = torch.device("cuda", 0)
    n = len(comp)
    lens = np.array([len(c) for c in comp], dtype=np.int64)
    d_in = torch.from_numpy(np.frombuffer(b"".join(comp), dtype=np.uint8).copy()).to(dev)
    in_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    in_off[1:] = torch.from_numpy(np.cumsum(lens)).to(dev)
    slots = np.array([(z + 8 + 7) & ~7 for z in out_sizes], dtype=np.int64)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    out_off[1:] = torch.from_numpy(np.cumsum(slots)).to(dev)
    d_out = torch.empty(int(slots.sum()) + 8, dtype=torch.uint8, device=dev)
    d_len, d_sizes = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
    d_cons, d_cons2 = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
    d_st, d_st2 = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))

    def decode():
        eng.decompress_device(d_in.data_ptr(), in_off.data_ptr(), n, container, 0, d_out.data_ptr(), out_off.data_ptr(),
                              d_len.data_ptr(), d_st.data_ptr(), d_cons.data_ptr())

    def probe():
        eng.decompressed_sizes_device(d_in.data_ptr(), in_off.data_ptr(), n, container, 0, d_sizes.data_ptr(),
                                      d_st2.data_ptr(), d_cons2.data_ptr())

    times = {"decompress_batch": [], "decompressed_sizes": []}
    for rep in range(reps + 1):
        for key, fn in (("decompress_batch", decode), ("decompressed_sizes", probe)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:  # (the first call of each is the warm-up)
                times[key].append((time.perf_counter() - t0) * 1e3)
    assert d_st.cpu().tolist() == [0] * n and d_st2.cpu().tolist() == [0] * n
    assert torch.equal(d_len, d_sizes) and d_sizes.cpu().tolist() == list(out_sizes) and torch.equal(d_cons, d_cons2)
    row = {"input": name, "streams": n, "compressed_bytes": int(lens.sum()), "output_bytes": int(sum(out_sizes)), "reps": reps,
           "size_paths": eng.size_paths()}
    for key, t in times.items():
        row[key + "_ms"] = {"min": round(min(t), 3), "median": round(statistics.median(t), 3), "max": round(max(t), 3)}
    row["probe_not_slower"] = row["decompressed_sizes_ms"]["median"] <= row["decompress_batch_ms"]["median"]
    print(json.dumps(row), flush=True)


def main():
    reps = max(7, int(sys.argv[1])) if len(sys.argv) > 1 else 7
    eng = Engine(0)
    n, size = 16385, 65535
    text = synth.text(synth.SEED_TEXT, n * size).tobytes()
    chunks = [text[i * size:(i + 1) * size] for i in range(n)]
    comp, st = eng.compress_many(chunks, 0, 6)
    assert st == [0] * n
    measure(eng, "16385 level-6 streams of 65535 B of text", comp, 0, [size] * n, reps)
    del text, chunks, comp
    one = synth.text(synth.SEED_TEXT + 7, 177_244_160).tobytes()
    comp, st = eng.compress_many([one], 1, 6)
    assert st == [0]
    measure(eng, "one gzip level-6 stream of 177,244,160 B of text", comp, 1, [len(one)], reps)
    del one, comp
    m, sz = 128, 1 << 20
    sil = synth.silesia_like(synth.SEED_SILESIA + 1, m * sz).tobytes()
    comp, st = eng.compress_many([sil[i * sz:(i + 1) * sz] for i in range(m)], 1, 6)
    assert st == [0] * m
    measure(eng, "128 gzip level-6 members of 1 MiB (Silesia-like)", comp, 1, [sz] * m, reps)


if __name__ == "__main__":
    main()
