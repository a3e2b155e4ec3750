"""One decompress_batch call on tests/_big_member.py's member, in a process of its own (test infrastructure; the parent gives it
a time limit): `python _big_inflate_job.py CONTAINER GROUPS`, the FLATE_HIP_* knobs from the environment.  Prints one JSON line:
status, out_len, whether every output byte is 'a' (checked in slices), the seconds of the call, the path counts."""
import ctypes as C
import json
import os
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
os.environ.setdefault("FLATE_HIP_PRELOAD_TORCH_HIP", "1")

import _big_member as B  # noqa: E402


def adler_of_a(n):
    """Adler-32 of b"a" * n from the definition: a = 1 + 97 n, b = n + 97 n (n + 1) / 2  (mod 65521)"""
    return ((1 + 97 * n) % 65521) | (((n + 97 * n * (n + 1) // 2) % 65521) << 16)


def member(container, groups):
    raw = b"".join(B.raw_chunks(groups))
    n = B.output_size(groups)
    if container == 1:
        return B.GZ_HEADER + raw + B.crc_of_output(groups).to_bytes(4, "little") + (n & 0xFFFFFFFF).to_bytes(4, "little")
    assert adler_of_a(70001) == zlib.adler32(b"a" * 70001)
    return bytes([0x78, 0x9C]) + raw + adler_of_a(n).to_bytes(4, "big")


def main():
    container, groups = int(sys.argv[1]), int(sys.argv[2])
    from flate_amd import Engine
    from flate_amd._capi import MEM_HOST
    eng = Engine(0)
    eng._sync_env()
    stream = member(container, groups)
    n = B.output_size(groups)
    cap = (n + 64 + 7) & ~7  # explicit: ISIZE is the length mod 2^32
    blob = np.frombuffer(stream, dtype=np.uint8)
    in_off = np.array([0, len(stream)], dtype=np.uint64)
    out_off = np.array([0, cap], dtype=np.uint64)
    out = np.zeros(cap + 8, dtype=np.uint8)
    out_len, status, consumed = np.zeros(1, dtype=np.uint64), np.full(1, -99, dtype=np.int32), np.zeros(1, dtype=np.uint64)
    t0 = time.time()
    rc = eng._L.flate_hip_decompress_batch(eng._h, blob.ctypes.data, in_off.ctypes.data, 1, container, 0, out.ctypes.data,
                                           out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data, consumed.ctypes.data,
                                           MEM_HOST)
    dt = time.time() - t0
    eng._check(rc, "flate_hip_decompress_batch")
    got = int(out_len[0])
    all_a = all(bool((out[k:min(k + (1 << 28), got)] == 97).all()) for k in range(0, got, 1 << 28)) and not out[got:].any()
    print(json.dumps({"status": int(status[0]), "out_len": got, "want_len": n, "all_a": bool(all_a), "consumed": int(consumed[0]),
                      "stream_bytes": len(stream), "seconds": round(dt, 3), "paths": eng.inflate_paths()}))


if __name__ == "__main__":
    main()
