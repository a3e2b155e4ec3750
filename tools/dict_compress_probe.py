"""Compress against preset dictionaries beside the plain batch compressor, on device memory (DESIGN.md §5 "Preset
dictionaries: compress").

    python tools/dict_compress_probe.py [--records 16384] [--calls 7] > profiles/dict_compress.txt

Records of synth.text, raw container; input GB/s = record bytes over the median call:
  (a) 4096-byte records without a dictionary, level 6, flate_hip_compress_batch  -- the yardstick, existing code, same build
  (b) the same records against one shared 32 KiB dictionary, level 6, flate_hip_compress_batch_dict
  (c) as (b) with 200-byte records
  (d) as (b) at level 9
Every row: the compressed bytes, and the kernel times (flate_hip_profile_*) of one call -- k_dict_stage, the staging
kernel, and k_lz_parse among them: the dictionary is copied, not parsed.  Samples of (b), (c), (d) are inflated by stdlib
zlib with the dictionary.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=16384)
    ap.add_argument("--calls", type=int, default=7)
    args = ap.parse_args()
    print("python tools/dict_compress_probe.py " + " ".join(sys.argv[1:]))
    import torch
    from flate_amd import Engine, synth
    assert torch.cuda.is_available(), "dict_compress_probe needs a GPU"
    eng = Engine(0)
    n = args.records
    text = bytes(synth.text(synth.SEED_TEXT, 32768 + n * 4096))
    zdict, body = text[:32768], text[32768:]

    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()

    def measure(label, rlen, with_dict, level):
        recs = [body[i * 4096: i * 4096 + rlen] for i in range(n)]
        cap = (eng.compress_bound(rlen, 0, level) + 4 + 7) & ~7
        t_in = dev(np.frombuffer(b"".join(recs), np.uint8))
        t_inoff = dev(np.arange(n + 1, dtype=np.int64) * rlen)
        t_outoff = dev(np.arange(n + 1, dtype=np.int64) * cap)
        t_out = torch.zeros(n * cap + 64, dtype=torch.uint8, device="cuda")
        t_len = torch.zeros(n, dtype=torch.int64, device="cuda")
        t_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        t_dict, t_doff = dev(np.frombuffer(zdict, np.uint8)), dev(np.array([0, len(zdict)], np.int64))
        torch.cuda.synchronize()

        def call():
            if with_dict:
                rc = eng.compress_dict_device(t_in.data_ptr(), t_inoff.data_ptr(), n, 0, level, t_out.data_ptr(), t_outoff.data_ptr(),
                                              t_len.data_ptr(), t_st.data_ptr(), t_dict.data_ptr(), t_doff.data_ptr(), 1, None)
                assert rc == 0, rc
            else:
                eng.compress_device(t_in.data_ptr(), t_inoff.data_ptr(), n, 0, level, t_out.data_ptr(), t_outoff.data_ptr(),
                                    t_len.data_ptr(), t_st.data_ptr())
        call()  # warm-up; the calls wait for the handle's stream (set_sync 1)
        assert int(t_st.abs().sum()) == 0
        out, ln = t_out.cpu().numpy(), t_len.cpu().numpy()
        for i in (0, n // 2, n - 1):
            o = zlib.decompressobj(-15, zdict=zdict) if with_dict else zlib.decompressobj(-15)
            assert o.decompress(out[i * cap: i * cap + int(ln[i])].tobytes()) == recs[i] and o.eof
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        print("%s: %d records of %d bytes, level %d, %d -> %d bytes, median of %d calls %.3f ms (min %.3f, max %.3f), input %.2f GB/s"
              % (label, n, rlen, level, n * rlen, int(ln.sum()), args.calls, med * 1e3, min(ts) * 1e3, max(ts) * 1e3, n * rlen / med / 1e9))
        eng.profile_enable(True)
        eng.profile_reset()
        call()
        for k, (ms, cnt) in sorted(eng.profile_read().items()):
            if cnt:
                print("    %-16s %8.3f ms  %d launches" % (k, ms, cnt))
        eng.profile_enable(False)
        return n * rlen / med / 1e9

    a = measure("(a) no dictionary, flate_hip_compress_batch", 4096, False, 6)
    b = measure("(b) one 32 KiB dictionary, flate_hip_compress_batch_dict", 4096, True, 6)
    c = measure("(c) one 32 KiB dictionary, flate_hip_compress_batch_dict", 200, True, 6)
    d = measure("(d) one 32 KiB dictionary, flate_hip_compress_batch_dict", 4096, True, 9)
    print("summary: (a) %.2f GB/s  (b) %.2f GB/s  (c) %.2f GB/s  (d) %.2f GB/s  (b)/(a) %.3f" % (a, b, c, d, b / a))
    ws = eng.workspace_bytes() if hasattr(eng, "workspace_bytes") else None
    if ws is not None:
        print("workspace held by the handle after the four rows: %.1f MiB" % (ws / 1048576.0))


if __name__ == "__main__":
    main()
