"""Inflate with preset dictionaries against the plain batch inflater, on device memory (DESIGN.md §5 "Preset dictionaries").

    python tools/dict_probe.py [--records 16384] [--calls 7] [--profile] > profiles/dict_inflate.txt

Records of synth.text, level 6, raw, compressed by stdlib zlib; output GB/s = decompressed bytes over the median call:
  (a) 4096-byte records without a dictionary, flate_hip_decompress_batch       -- the yardstick, existing code, same build
  (b) the same records against one shared 32 KiB dictionary, flate_hip_decompress_batch_dict
  (c) as (b) with 200-byte records
--profile adds the kernel times (flate_hip_profile_*) of one call each and, counted on the host over the probe's own
streams, the share of match tokens whose distance exceeds the small ring's near_max (1788): the far-copy branch.
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


def deflate(data, zdict):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, 0, zdict) if zdict is not None else zlib.compressobj(6, zlib.DEFLATED, -15, 9, 0)
    return c.compress(data) + c.flush()


def far_share(streams, zdict, near_max=1788):
    """(match tokens, of them with distance > near_max) of raw streams, by a plain bit-level walk of their blocks"""
    LB = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    LE = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
    DB = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
          12289, 16385, 24577]
    DE = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
    ORD = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

    def table(lens):
        code, t = 0, {}
        for b in range(1, 16):
            for s, l in enumerate(lens):
                if l == b:
                    t[(b, code)] = s
                    code += 1
            code <<= 1
        return t

    FIXL = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
    FIXD = table([5] * 30)
    matches = far = 0
    for z in streams:
        v, pos = int.from_bytes(z, "little"), 0

        def bits(n):
            nonlocal pos
            r = (v >> pos) & ((1 << n) - 1)
            pos += n
            return r

        def sym(t):
            code = 0
            for b in range(1, 16):
                code = (code << 1) | bits(1)
                if (b, code) in t:
                    return t[(b, code)]
            raise ValueError("bad code")

        while True:
            final, btype = bits(1), bits(2)
            if btype == 0:
                pos = (pos + 7) & ~7
                n = bits(16)
                bits(16)
                pos += 8 * n
            else:
                if btype == 1:
                    tl, td = FIXL, FIXD
                else:
                    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                    cl = [0] * 19
                    for i in range(hclen):
                        cl[ORD[i]] = bits(3)
                    tc, lens = table(cl), []
                    while len(lens) < hlit + hdist:
                        s = sym(tc)
                        if s < 16:
                            lens.append(s)
                        elif s == 16:
                            lens += [lens[-1]] * (3 + bits(2))
                        elif s == 17:
                            lens += [0] * (3 + bits(3))
                        else:
                            lens += [0] * (11 + bits(7))
                    tl, td = table(lens[:hlit]), table(lens[hlit:])
                while True:
                    s = sym(tl)
                    if s == 256:
                        break
                    if s > 256:
                        bits(LE[s - 257])
                        d = sym(td)
                        dist = DB[d] + bits(DE[d])
                        matches += 1
                        far += dist > near_max
            if final:
                break
    return matches, far


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=16384)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    print("python tools/dict_probe.py " + " ".join(sys.argv[1:]))
    import torch
    from flate_amd import Engine, synth
    assert torch.cuda.is_available(), "dict_probe needs a GPU"
    eng = Engine(0)
    n = args.records
    text = bytes(synth.text(synth.SEED_TEXT, 32768 + n * 4096))
    zdict, body = text[:32768], text[32768:]

    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()

    def measure(label, rlen, with_dict):
        recs = [body[i * 4096: i * 4096 + rlen] for i in range(n)]
        streams = [deflate(r, zdict if with_dict else None) for r in recs]
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(z) for z in streams])
        cap = (rlen + 15) & ~7
        t_in, t_inoff = dev(np.frombuffer(b"".join(streams), np.uint8)), dev(off)
        t_outoff = dev(np.arange(n + 1, dtype=np.int64) * cap)
        t_out = torch.zeros(n * cap + 64, dtype=torch.uint8, device="cuda")
        t_len, t_cons = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
        t_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        t_dict, t_doff = dev(np.frombuffer(zdict, np.uint8)), dev(np.array([0, len(zdict)], np.int64))
        torch.cuda.synchronize()

        def call():
            if with_dict:
                eng.decompress_dict_device(t_in.data_ptr(), t_inoff.data_ptr(), n, 0, 0, t_out.data_ptr(), t_outoff.data_ptr(),
                                           t_len.data_ptr(), t_st.data_ptr(), t_cons.data_ptr(), t_dict.data_ptr(),
                                           t_doff.data_ptr(), 1, None)
            else:
                eng.decompress_device(t_in.data_ptr(), t_inoff.data_ptr(), n, 0, 0, t_out.data_ptr(), t_outoff.data_ptr(),
                                      t_len.data_ptr(), t_st.data_ptr(), t_cons.data_ptr())
        call()  # warm-up; the calls wait for the handle's stream (set_sync 1)
        assert int(t_st.abs().sum()) == 0 and int(t_len.sum()) == n * rlen
        out = t_out.cpu().numpy()
        for i in (0, n // 2, n - 1):
            assert out[i * cap: i * cap + rlen].tobytes() == recs[i]
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        print("%s: %d records of %d bytes, %d -> %d bytes, median of %d calls %.3f ms (min %.3f, max %.3f), output %.2f GB/s"
              % (label, n, rlen, int(off[-1]), n * rlen, args.calls, med * 1e3, min(ts) * 1e3, max(ts) * 1e3, n * rlen / med / 1e9))
        if args.profile:
            eng.profile_enable(True)
            eng.profile_reset()
            call()
            for k, (ms, cnt) in sorted(eng.profile_read().items()):
                if cnt:
                    print("    %-16s %8.3f ms  %d launches" % (k, ms, cnt))
            eng.profile_enable(False)
            m, f = far_share(streams[:: max(1, n // 256)], zdict)
            print("    match tokens with distance > 1788 (far copies of the small ring): %d of %d (%.1f %%)" % (f, m, 100.0 * f / max(m, 1)))
        return n * rlen / med / 1e9

    a = measure("(a) no dictionary, flate_hip_decompress_batch", 4096, False)
    b = measure("(b) one 32 KiB dictionary, flate_hip_decompress_batch_dict", 4096, True)
    c = measure("(c) one 32 KiB dictionary, flate_hip_decompress_batch_dict", 200, True)
    print("summary: (a) %.2f GB/s  (b) %.2f GB/s  (c) %.2f GB/s  (b)/(a) %.2f" % (a, b, c, b / a))


if __name__ == "__main__":
    main()
