#!/usr/bin/env python3
"""Concatenated members three ways ("Members"): (i) flate_hip_decompress_members, (ii) the loop a caller
wrote before it -- flate_hip_decompress_batch on the first member of what is left of every file, its consumed count read
back, again -- and (iii) the floor, flate_hip_decompress_batch handed the true member offsets.  Device memory throughout,
one process; after a warm-up call of each, the median of `reps` calls (each ends with a wait).  Inputs: (a) one gzip file
of 4096 level-6 members of 65535 bytes of text, (b) 128 level-6 members of 1 MiB of the Silesia-like buffer as one file,
(c) 64 files of 64 of (a)'s members.  In (ii) a single file's call is given 4 x its largest member from the current
position on (a caller who knows a bound; the rest of a 100 MB file per call would be cut into spans every time).  The
outputs of the three are compared.  Then the kernels of (i) by flate_hip_profile_read.  One JSON line per input.
usage: multi_member_probe.py [reps >= 7] [inputs, e.g. ac]"""
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

GZIP = 1
KERNELS = ("k_member_scan", "k_inflate_size", "k_member_chain", "k_member_pack", "k_member_fold", "k_member_walk", "k_inflate",
           "k_inflate_par", "k_span_scan", "k_inflate_span")


def i64(a, dev):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)


def measure(eng, name, files, member_out, reps):
    """files: list of lists of members (bytes); member_out: output bytes of every member"""
    dev = torch.device("cuda", 0)
    nf = len(files)
    flat = [m for f in files for m in f]
    nm = len(flat)
    mlen = np.array([len(m) for m in flat], dtype=np.int64)
    file_len = np.array([sum(len(m) for m in f) for f in files], dtype=np.int64)
    file_out = np.array([len(f) * member_out for f in files], dtype=np.int64)
    file_off = np.concatenate([[0], np.cumsum(file_len)])
    fout_off = np.concatenate([[0], np.cumsum(file_out)])
    total_out = int(fout_off[-1])
    d_in = torch.from_numpy(np.frombuffer(b"".join(flat), dtype=np.uint8).copy()).to(dev)
    outs = [torch.zeros(total_out + 8, dtype=torch.uint8, device=dev) for _ in range(3)]
    window = 4 * int(mlen.max())

    # (i) the new call
    f_inoff, f_outoff = i64(file_off, dev), i64(fout_off, dev)
    f_len, f_used = (torch.zeros(nf, dtype=torch.int64, device=dev) for _ in range(2))
    f_st, f_mem = (torch.zeros(nf, dtype=torch.int32, device=dev) for _ in range(2))

    def members():
        eng.decompress_members_device(d_in.data_ptr(), f_inoff.data_ptr(), nf, GZIP, 0, outs[0].data_ptr(), f_outoff.data_ptr(),
                                      f_len.data_ptr(), f_st.data_ptr(), f_used.data_ptr(), f_mem.data_ptr())

    # (ii) the loop: one call per round of members, consumed read back
    l_inoff, l_outoff = (torch.zeros(nf + 1, dtype=torch.int64, device=dev) for _ in range(2))
    l_len, l_used = (torch.zeros(nf, dtype=torch.int64, device=dev) for _ in range(2))
    l_st = torch.zeros(nf, dtype=torch.int32, device=dev)
    calls = [0]

    def loop():
        pos, produced = np.zeros(nf, dtype=np.int64), np.zeros(nf, dtype=np.int64)
        live = np.ones(nf, dtype=bool)
        calls[0] = 0
        while live.any():
            # (streams are a contiguous partition: a file that is done keeps an empty stream)
            a = np.concatenate([file_off[:-1] + pos, file_off[-1:]])
            if nf == 1:
                a[1] = min(a[0] + window, a[1])
            o = np.concatenate([fout_off[:-1] + produced, fout_off[-1:]])
            l_inoff.copy_(torch.from_numpy(a))
            l_outoff.copy_(torch.from_numpy(o))
            eng.decompress_device(d_in.data_ptr(), l_inoff.data_ptr(), nf, GZIP, 0, outs[1].data_ptr(), l_outoff.data_ptr(),
                                  l_len.data_ptr(), l_st.data_ptr(), l_used.data_ptr())
            calls[0] += 1
            st, n_out, used = l_st.cpu().numpy(), l_len.cpu().numpy(), l_used.cpu().numpy()
            assert (st[live] == 0).all(), st
            pos[live] += used[live]
            produced[live] += n_out[live]
            live &= pos < file_len
            assert live.all() or not live.any()  # (files of equal member counts: no file idles while others go on)

    # (iii) the floor: the true member offsets
    m_inoff = i64(np.concatenate([[0], np.cumsum(mlen)]), dev)
    m_outoff = i64(np.arange(nm + 1, dtype=np.int64) * member_out, dev)
    m_len, m_used = (torch.zeros(nm, dtype=torch.int64, device=dev) for _ in range(2))
    m_st = torch.zeros(nm, dtype=torch.int32, device=dev)

    def floor():
        eng.decompress_device(d_in.data_ptr(), m_inoff.data_ptr(), nm, GZIP, 0, outs[2].data_ptr(), m_outoff.data_ptr(),
                              m_len.data_ptr(), m_st.data_ptr(), m_used.data_ptr())

    ways = (("members", members), ("loop", loop), ("floor", floor))
    times = {k: [] for k, _ in ways}
    for rep in range(reps + 1):
        for key, fn in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:  # (the first call of each is the warm-up)
                times[key].append((time.perf_counter() - t0) * 1e3)
    assert f_st.cpu().tolist() == [0] * nf and m_st.cpu().tolist() == [0] * nm
    assert f_mem.cpu().tolist() == [len(f) for f in files] and f_len.cpu().tolist() == file_out.tolist()
    assert f_used.cpu().tolist() == file_len.tolist()
    assert torch.equal(outs[0][:total_out], outs[2][:total_out]) and torch.equal(outs[1][:total_out], outs[2][:total_out])
    paths = eng.member_paths()
    eng.profile_enable(True)
    eng.profile_reset()
    members()
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile_enable(False)
    row = {"input": name, "files": nf, "members": nm, "compressed_bytes": int(mlen.sum()), "output_bytes": total_out,
           "reps": reps, "member_paths": paths, "loop_calls": calls[0], "loop_window_bytes": window if nf == 1 else None}
    med = {}
    for key, t in times.items():
        med[key] = statistics.median(t)
        row[key + "_ms"] = {"min": round(min(t), 3), "median": round(med[key], 3), "max": round(max(t), 3)}
    row["members_over_floor"] = round(med["members"] / med["floor"], 2)
    row["loop_over_members"] = round(med["loop"] / med["members"], 2)
    row["kernel_ms_of_one_members_call"] = {k: round(prof[k][0], 3) for k in KERNELS if k in prof and prof[k][1]}
    print(json.dumps(row), flush=True)


def main():
    reps = max(7, int(sys.argv[1])) if len(sys.argv) > 1 else 7
    which = sys.argv[2] if len(sys.argv) > 2 else "abc"
    eng = Engine(0)
    if "a" in which or "c" in which:
        n, size = 4096, 65535
        text = synth.text(synth.SEED_TEXT, n * size).tobytes()
        comp, st = eng.compress_many([text[i * size:(i + 1) * size] for i in range(n)], GZIP, 6)
        assert st == [0] * n
        del text
        if "a" in which:
            measure(eng, "(a) one file of 4096 level-6 members of 65535 B of text", [comp], size, reps)
        if "c" in which:
            measure(eng, "(c) 64 files of 64 such members", [comp[i * 64:(i + 1) * 64] for i in range(64)], size, reps)
        del comp
    if "b" in which:
        m, sz = 128, 1 << 20
        sil = synth.silesia_like(synth.SEED_SILESIA + 1, m * sz).tobytes()
        comp, st = eng.compress_many([sil[i * sz:(i + 1) * sz] for i in range(m)], GZIP, 6)
        assert st == [0] * m
        measure(eng, "(b) one file of 128 level-6 members of 1 MiB (Silesia-like)", [comp], sz, reps)


if __name__ == "__main__":
    main()
