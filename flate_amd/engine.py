"""Engine: one handle of the HIP DEFLATE engine on one device (one process per GPU).

Host-buffer entry points (`compress_many`, `decompress_many`) take / return Python
bytes; device entry points take raw device pointers (e.g. torch tensors'
`data_ptr()`), keep everything resident in HBM and run on the caller's stream.
"""
import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import FlateHipError, MEM_DEVICE, MEM_HOST


class Engine:
    def __init__(self, device=0):
        self._L = _capi.lib()
        self._h = C.c_void_p()
        rc = self._L.flate_hip_create(int(device), C.byref(self._h))
        if rc != 0:
            import sys
            hint = ""
            if "torch" in sys.modules and os.environ.get("FLATE_HIP_PRELOAD_TORCH_HIP", "0") in ("", "0"):
                # (two HIP runtimes in one process: the second to come up finds no device -- flate_amd/_capi.py)
                hint = ("; this process also runs PyTorch, which ships its own libamdhip64: import torch BEFORE flate_amd, "
                        "or set FLATE_HIP_PRELOAD_TORCH_HIP=1 before importing flate_amd, so that both use one runtime")
            raise FlateHipError("flate_hip_create(device=%d) failed with %d: no usable MI355X / HIP device "
                                "(there is no CPU fallback)%s" % (device, rc, hint))
        self.device = device

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.flate_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            err = self._L.flate_hip_last_error(self._h).decode()
            raise FlateHipError("%s failed with %d (%s)" % (what, rc, err))

    # ---- configuration ----
    _KNOBS = ("FLATE_HIP_MAX_PASS_CHUNKS", "FLATE_HIP_HOST_PASS_CHUNKS", "FLATE_HIP_MAX_STREAM_PASS_MIB",
              "FLATE_HIP_INFLATE_SPANS", "FLATE_HIP_SPAN_DEBUG", "FLATE_HIP_SPAN_TWIN", "FLATE_HIP_NO_PIN_MIRROR",
              "FLATE_HIP_NO_RAMP", "FLATE_HIP_INFLATE_PAR", "FLATE_HIP_INFLATE_RING", "FLATE_HIP_RECT", "FLATE_HIP_STREAM_WINDOWS", "FLATE_HIP_SIMPLE_CK_INLINE", "FLATE_HIP_STREAM_GROUP", "FLATE_HIP_SPAN_TWO_RUNS", "FLATE_HIP_MEMSET_INLINE", "FLATE_HIP_ONE_COMPUTE_STREAM",
              "FLATE_HIP_MEMBER_SCAN", "FLATE_HIP_MEMBER_CANDIDATES", "FLATE_HIP_INDEX_PASS_BYTES")

    def _sync_env(self):
        """The library reads its FLATE_HIP_* tuning variables once, when the handle is made.  Tests and probes change them
        between calls of one engine: when this process's view of them has changed, the handle is told to read them again."""
        now = tuple(os.environ.get(k) for k in self._KNOBS)
        if now != getattr(self, "_knob_state", None):
            if getattr(self, "_knob_state", None) is not None or any(v is not None for v in now):
                self._L.flate_hip_debug_reload_env(self._h)
            self._knob_state = now

    def set_stream(self, stream_ptr):
        self._L.flate_hip_set_stream(self._h, C.c_void_p(stream_ptr or 0))

    def set_sync(self, flag):
        self._L.flate_hip_set_sync(self._h, int(bool(flag)))

    def set_flags(self, flags):
        """_capi.DEFLATE_REPAIR_Q1: levels 4..9 hand every block the bytes its tokens cover (streams that always inflate
        to their input; they differ from the reference's only where the reference's own stream is broken: status 102)."""
        self._check(self._L.flate_hip_set_flags(self._h, int(flags)), "flate_hip_set_flags")

    def compress_bound(self, n, container=0, mode=6):
        return self._L.flate_hip_compress_bound(int(n), container, mode)

    # ---- host buffers ----
    def compress_many(self, chunks, container=0, mode=6):
        """chunks: sequence of bytes-like.  Returns (list of bytes, list of status codes)."""
        self._sync_env()
        n = len(chunks)
        if n == 0:
            return [], []
        lens = np.array([len(c) for c in chunks], dtype=np.uint64)
        in_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(lens, out=in_off[1:])
        blob = np.frombuffer(b"".join(bytes(c) for c in chunks), dtype=np.uint8)
        if blob.size == 0:
            blob = np.zeros(1, dtype=np.uint8)
        caps = np.array([(self.compress_bound(int(l), container, mode) + 7) & ~7 for l in lens], dtype=np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(caps, out=out_off[1:])
        out = np.zeros(int(out_off[-1]) + 8, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        rc = self._L.flate_hip_compress_batch(self._h, blob.ctypes.data, in_off.ctypes.data, n, container, mode,
                                              out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data,
                                              status.ctypes.data, MEM_HOST)
        self._check(rc, "flate_hip_compress_batch")
        res = [out[int(out_off[i]): int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
        return res, [int(s) for s in status]

    def compress_flush(self, data, flush_points, finish=True, container=0, mode=6):
        """One stream with sync-flush points (Compressor.write / flush / finish, deflate.zig:335-367).
        Returns (bytes, status)."""
        self._sync_env()
        blob = np.frombuffer(bytes(data), dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
        fp = np.array(list(flush_points), dtype=np.uint64)
        cap = (self.compress_bound(len(data), container, mode) + 64 * (len(fp) + 1) + 7) & ~7
        out = np.zeros(cap + 8, dtype=np.uint8)
        out_len = np.zeros(1, dtype=np.uint64)
        status = np.zeros(1, dtype=np.int32)
        rc = self._L.flate_hip_compress_flush(self._h, blob.ctypes.data, len(data), fp.ctypes.data if len(fp) else None,
                                              len(fp), 1 if finish else 0, container, mode, out.ctypes.data, cap,
                                              out_len.ctypes.data, status.ctypes.data, MEM_HOST)
        self._check(rc, "flate_hip_compress_flush")
        return out[: int(out_len[0])].tobytes(), int(status[0])

    def checksum(self, data, container):
        """CRC-32 (container 1) / Adler-32 (container 2) of a host buffer, by the checksum kernels."""
        blob = np.frombuffer(bytes(data), dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
        v = np.zeros(1, dtype=np.uint32)
        rc = self._L.flate_hip_checksum(self._h, blob.ctypes.data, len(data), container, v.ctypes.data)
        self._check(rc, "flate_hip_checksum")
        return int(v[0])

    def checksum_combine(self, container, a, b, len_b):
        return int(self._L.flate_hip_checksum_combine(container, a, b, len_b))

    def _host_input(self, streams):
        """(blob, in_off) of a host batch"""
        n = len(streams)
        lens = np.array([len(c) for c in streams], dtype=np.uint64)
        in_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(lens, out=in_off[1:])
        blob = np.frombuffer(b"".join(bytes(c) for c in streams), dtype=np.uint8)
        if blob.size == 0:
            blob = np.zeros(1, dtype=np.uint8)
        return blob, in_off

    def decompressed_sizes(self, streams, container=0, flags=0):
        """How many bytes each stream inflates to, without inflating it (flate_hip_decompressed_sizes): no output is
        allocated or written.  The footer is read but not compared, so a stream with a wrong checksum reports 0.
        Returns (list of sizes -- exact where the status is 0 --, list of status codes, list of consumed input bytes)."""
        self._sync_env()
        n = len(streams)
        if n == 0:
            return [], [], []
        blob, in_off = self._host_input(streams)
        sizes = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        consumed = np.zeros(n, dtype=np.uint64)
        rc = self._L.flate_hip_decompressed_sizes(self._h, blob.ctypes.data, in_off.ctypes.data, n, container, flags,
                                                  sizes.ctypes.data, status.ctypes.data, consumed.ctypes.data, MEM_HOST)
        self._check(rc, "flate_hip_decompressed_sizes")
        return [int(x) for x in sizes], [int(x) for x in status], [int(x) for x in consumed]

    def decompress_members(self, streams, container=0, flags=0, caps=None):
        """Every member of each stream, concatenated (flate_hip_decompress_members): what a caller gets who decodes a
        stream member by member with decompress_many and its consumed count, in one call.  caps: output capacity per
        stream (default: 1100 output bytes per input byte).
        Returns (list of bytes -- the members in front of the first failing one --, list of status codes, list of
        consumed input bytes, list of member counts)."""
        self._sync_env()
        n = len(streams)
        if n == 0:
            return [], [], [], []
        blob, in_off = self._host_input(streams)
        if caps is None:
            caps = [max(1 << 16, len(c) * 1100 + 1024) for c in streams]
        caps = np.array([int(c) for c in caps], dtype=np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(caps, out=out_off[1:])
        out = np.zeros(int(out_off[-1]) + 8, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        consumed = np.zeros(n, dtype=np.uint64)
        members = np.zeros(n, dtype=np.uint32)
        rc = self._L.flate_hip_decompress_members(self._h, blob.ctypes.data, in_off.ctypes.data, n, container, flags,
                                                  out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data,
                                                  status.ctypes.data, consumed.ctypes.data, members.ctypes.data, MEM_HOST)
        self._check(rc, "flate_hip_decompress_members")
        res = [out[int(out_off[i]): int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
        return res, [int(s) for s in status], [int(c) for c in consumed], [int(m) for m in members]

    def decompress_members_device(self, in_ptr, in_off_ptr, n_streams, container, flags, out_ptr, out_off_ptr, out_len_ptr,
                                  status_ptr, consumed_ptr=None, n_members_ptr=None):
        """flate_hip_decompress_members on device memory (n + 1 offsets; n lengths / statuses / consumed / member counts)."""
        self._sync_env()
        rc = self._L.flate_hip_decompress_members(self._h, in_ptr, in_off_ptr, n_streams, container, flags, out_ptr,
                                                  out_off_ptr, out_len_ptr, status_ptr, consumed_ptr, n_members_ptr,
                                                  MEM_DEVICE)
        self._check(rc, "flate_hip_decompress_members")

    # ---- the seek index ----
    def build_index(self, streams, container=0, flags=0, spacing=None, caps=None):
        """Decode the streams as decompress_many does and keep a seek index over them (flate_hip_index_build): for every
        stream the block starts nearest behind each multiple of `spacing` output bytes (default 1 MiB), each with the 32 KiB
        in front of it.  caps: output capacity per stream (default: the size probe's answer).
        Returns (Index, list of bytes, list of status codes, list of consumed input bytes); a stream whose status is not 0
        has no points."""
        self._sync_env()
        n = len(streams)
        blob, in_off = self._host_input(streams)
        if caps is None:
            caps = self._measured_caps(streams, container, flags, [max(1 << 16, len(c) * 1100 + 1024) for c in streams]) if n else []
        caps = np.array([(int(c) + 7) & ~7 for c in caps], dtype=np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(caps, out=out_off[1:])
        out = np.zeros(int(out_off[-1]) + 8, dtype=np.uint8)
        out_len = np.zeros(max(n, 1), dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.int32)
        consumed = np.zeros(max(n, 1), dtype=np.uint64)
        ix = C.c_void_p()
        rc = self._L.flate_hip_index_build(self._h, blob.ctypes.data, in_off.ctypes.data, n, container, flags, out.ctypes.data,
                                           out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data, consumed.ctypes.data,
                                           MEM_HOST, int(spacing or 0), C.byref(ix))
        self._check(rc, "flate_hip_index_build")
        res = [out[int(out_off[i]): int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
        return Index(self, ix, blob, in_off, n), res, [int(s) for s in status[:n]], [int(c) for c in consumed[:n]]

    def scan_index(self, streams, container=0, flags=0, spacing=None):
        """A fresh seek index over streams written elsewhere, found without decoding them (flate_hip_index_scan): the size
        probe runs, then every good stream is walked for its flush markers -- a point is block 0 or a marker-following
        block start that the spacing rule keeps (default 1 MiB) and behind which no match reaches in front of it.
        Returns (Index, list of sizes, list of status codes, list of consumed input bytes), the last three as
        decompressed_sizes gives them; a stream whose status is not 0 has no points."""
        self._sync_env()
        n = len(streams)
        blob, in_off = self._host_input(streams)
        sizes = np.zeros(max(n, 1), dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.int32)
        consumed = np.zeros(max(n, 1), dtype=np.uint64)
        ix = C.c_void_p()
        rc = self._L.flate_hip_index_scan(self._h, blob.ctypes.data, in_off.ctypes.data, n, container, flags, sizes.ctypes.data,
                                          status.ctypes.data, consumed.ctypes.data, MEM_HOST, int(spacing or 0), C.byref(ix))
        self._check(rc, "flate_hip_index_scan")
        return (Index(self, ix, blob, in_off, n), [int(x) for x in sizes[:n]], [int(s) for s in status[:n]],
                [int(c) for c in consumed[:n]])

    def index_from_bytes(self, blob, streams):
        """An Index from what Index.to_bytes() returned and the streams it was built from (flate_hip_index_import): the blob
        is validated, the streams only by their lengths -- nothing tells bytes that have changed but still decode."""
        raw = np.frombuffer(bytes(blob), dtype=np.uint8)
        ix = C.c_void_p()
        rc = self._L.flate_hip_index_import(self._h, raw.ctypes.data if raw.size else None, raw.size, C.byref(ix))
        self._check(rc, "flate_hip_index_import")
        data, in_off = self._host_input(streams)
        return Index(self, ix, data, in_off, len(streams))

    def index_build_device(self, in_ptr, in_off_ptr, n_streams, container, flags, out_ptr, out_off_ptr, out_len_ptr, status_ptr,
                           consumed_ptr=None, spacing=0, memkind=MEM_DEVICE):
        """flate_hip_index_build on raw pointers (device memory unless memkind says otherwise); returns the index handle for
        index_* / decompress_ranges_device, to be given to index_destroy."""
        self._sync_env()
        ix = C.c_void_p()
        rc = self._L.flate_hip_index_build(self._h, in_ptr, in_off_ptr, n_streams, container, flags, out_ptr, out_off_ptr,
                                           out_len_ptr, status_ptr, consumed_ptr, memkind, int(spacing), C.byref(ix))
        self._check(rc, "flate_hip_index_build")
        return ix

    def scan_index_device(self, in_ptr, in_off_ptr, n_streams, container, flags, sizes_ptr, status_ptr, consumed_ptr=None,
                          spacing=0, memkind=MEM_DEVICE):
        """flate_hip_index_scan on raw pointers (device memory unless memkind says otherwise); returns the handle of the
        fresh index for index_* / decompress_ranges_device, to be given to index_destroy.  The host waits for the stream."""
        self._sync_env()
        ix = C.c_void_p()
        rc = self._L.flate_hip_index_scan(self._h, in_ptr, in_off_ptr, n_streams, container, flags, sizes_ptr, status_ptr,
                                          consumed_ptr, memkind, int(spacing), C.byref(ix))
        self._check(rc, "flate_hip_index_scan")
        return ix

    def index_destroy(self, ix):
        self._check(self._L.flate_hip_index_destroy(self._h, ix), "flate_hip_index_destroy")

    def index_info(self, ix, stream):
        """(size, status, number of points) of one stream of an index"""
        size, st, npts = C.c_uint64(), C.c_int32(), C.c_uint64()
        rc = self._L.flate_hip_index_stream_info(self._h, ix, stream, C.addressof(size), C.addressof(st), C.addressof(npts))
        self._check(rc, "flate_hip_index_stream_info")
        return int(size.value), int(st.value), int(npts.value)

    def index_points(self, ix, stream):
        """[(in_bit, out_pos)] of one stream of an index"""
        n = self.index_info(ix, stream)[2]
        bit, pos = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        got = self._L.flate_hip_index_points(self._h, ix, stream, bit.ctypes.data, pos.ctypes.data, n)
        if got != n:
            raise FlateHipError("flate_hip_index_points returned %d, %d points expected" % (got, n))
        return [(int(b), int(p)) for b, p in zip(bit[:n], pos[:n])]

    def index_export(self, ix):
        size = C.c_uint64()
        self._check(self._L.flate_hip_index_export_size(self._h, ix, C.addressof(size)), "flate_hip_index_export_size")
        blob = np.zeros(int(size.value), dtype=np.uint8)
        self._check(self._L.flate_hip_index_export(self._h, ix, blob.ctypes.data, blob.size), "flate_hip_index_export")
        return blob.tobytes()

    def index_import(self, blob):
        """the index handle of a blob; raises FlateHipError (code -2) for anything index_export did not write"""
        raw = np.frombuffer(bytes(blob), dtype=np.uint8)
        ix = C.c_void_p()
        rc = self._L.flate_hip_index_import(self._h, raw.ctypes.data if raw.size else None, raw.size, C.byref(ix))
        self._check(rc, "flate_hip_index_import")
        return ix

    def decompress_ranges_device(self, ix, in_ptr, in_off_ptr, n_streams, n_ranges, range_stream_ptr, range_begin_ptr,
                                 range_len_ptr, out_ptr, out_off_ptr, out_len_ptr, status_ptr, memkind=MEM_DEVICE):
        """flate_hip_decompress_ranges on raw pointers; returns the call's return code (0, or an argument error)"""
        self._sync_env()
        return self._L.flate_hip_decompress_ranges(self._h, ix, in_ptr, in_off_ptr, n_streams, n_ranges, range_stream_ptr,
                                                   range_begin_ptr, range_len_ptr, out_ptr, out_off_ptr, out_len_ptr, status_ptr,
                                                   memkind)

    def index_paths(self):
        """(good streams of the last index build or scan walked span by span, walked whole by one wave)
        (flate_hip_debug_index_paths)"""
        v = np.zeros(2, dtype=np.uint64)
        self._check(self._L.flate_hip_debug_index_paths(self._h, v.ctypes.data), "flate_hip_debug_index_paths")
        return int(v[0]), int(v[1])

    def index_passes(self):
        """passes the last decompress_ranges call took (flate_hip_debug_index_passes)"""
        v = C.c_uint64()
        self._check(self._L.flate_hip_debug_index_passes(self._h, C.addressof(v)), "flate_hip_debug_index_passes")
        return int(v.value)

    def index_parts(self):
        """(parts decoded straight into a slot, parts decoded through scratch) of the last decompress_ranges call on a
        fresh index (flate_hip_debug_index_parts)"""
        v = np.zeros(2, dtype=np.uint64)
        self._check(self._L.flate_hip_debug_index_parts(self._h, v.ctypes.data), "flate_hip_debug_index_parts")
        return int(v[0]), int(v[1])

    def member_paths(self):
        """How the last decompress_members call found its members: (streams by the scan for candidates, streams walked,
        candidates probed that lie on no chain) (flate_hip_debug_member_paths)."""
        v = np.zeros(3, dtype=np.uint64)
        self._check(self._L.flate_hip_debug_member_paths(self._h, v.ctypes.data), "flate_hip_debug_member_paths")
        return int(v[0]), int(v[1]), int(v[2])

    def _measured_caps(self, streams, container, flags, worst):
        """slots from the size probe: the stream's size + 8 where the probe's status is 0, the worst case elsewhere"""
        sizes, st, _ = self.decompressed_sizes(streams, container, flags)
        return [sizes[i] + 8 if st[i] == 0 else worst[i] for i in range(len(streams))]

    def decompress_many(self, streams, container=0, flags=0, caps=None, measure=False):
        """streams: sequence of bytes-like.  caps: output capacity per stream.  Default: for gzip the ISIZE
        field of the stream's last 8 bytes (container.zig:92-96) plus slack, and whatever then reports
        OutputTooSmall (more members behind the first, a damaged footer) is decoded again with the worst
        case of 1100 output bytes per input byte; raw / zlib streams get the worst case at once.
        measure=True (with caps=None): the slots come from the size probe instead of the worst case -- a stream's
        exact size + 8 where the probe's status is 0; for gzip only the streams whose ISIZE guess came back
        OutputTooSmall are probed, before their second decode.
        Returns (list of bytes, list of status codes, list of consumed input bytes)."""
        self._sync_env()
        n = len(streams)
        if n == 0:
            return [], [], []
        if caps is None and container == 1:  # gzip
            worst = [max(1 << 16, len(c) * 1100 + 1024) for c in streams]
            guess = [min(w, int.from_bytes(bytes(c[-4:]), "little") + 64) if len(c) >= 18 else w
                     for c, w in zip(streams, worst)]
            res, st, cons = self.decompress_many(streams, container, flags, guess)
            redo = [i for i in range(n) if st[i] == 100 and guess[i] < worst[i]]  # FLATE_HIP_ST_OUTPUT_TOO_SMALL
            if redo:
                again = [streams[i] for i in redo]
                caps2 = [worst[i] for i in redo]
                if measure:
                    caps2 = self._measured_caps(again, container, flags, caps2)
                r2, s2, c2 = self.decompress_many(again, container, flags, caps2)
                for k, i in enumerate(redo):
                    res[i], st[i], cons[i] = r2[k], s2[k], c2[k]
            return res, st, cons
        lens = np.array([len(c) for c in streams], dtype=np.uint64)
        in_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(lens, out=in_off[1:])
        blob = np.frombuffer(b"".join(bytes(c) for c in streams), dtype=np.uint8)
        if blob.size == 0:
            blob = np.zeros(1, dtype=np.uint8)
        if caps is None:
            caps = [max(1 << 16, int(l) * 1100 + 1024) for l in lens]
            if measure:
                caps = self._measured_caps(streams, container, flags, caps)
        caps = np.array([(int(c) + 7) & ~7 for c in caps], dtype=np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(caps, out=out_off[1:])
        out = np.zeros(int(out_off[-1]) + 8, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        consumed = np.zeros(n, dtype=np.uint64)
        rc = self._L.flate_hip_decompress_batch(self._h, blob.ctypes.data, in_off.ctypes.data, n, container, flags,
                                                out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data,
                                                status.ctypes.data, consumed.ctypes.data, MEM_HOST)
        self._check(rc, "flate_hip_decompress_batch")
        res = [out[int(out_off[i]): int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
        return res, [int(s) for s in status], [int(c) for c in consumed]

    def decompress_many_dict(self, streams, dicts, dict_of=None, container=0, flags=0, caps=None):
        """Streams compressed against preset dictionaries (flate_hip_decompress_batch_dict; raw or zlib).  dicts: sequence
        of bytes-like.  dict_of: per stream the index of its dictionary or None (it has none); default None: there is
        exactly one dictionary and every stream uses it.  caps: output capacity per stream (default: the worst case of
        1100 output bytes per input byte).  Returns (list of bytes, list of status codes, list of consumed input bytes)."""
        self._sync_env()
        if container == _capi.GZIP:
            raise ValueError("gzip has no preset dictionaries")
        n = len(streams)
        if dict_of is None and len(dicts) != 1:
            raise ValueError("dict_of may be left out only with exactly one dictionary")
        if n == 0:
            return [], [], []
        blob, in_off = self._host_input(streams)
        dblob, d_off = self._host_input(dicts)
        of = None
        if dict_of is not None:
            if len(dict_of) != n:
                raise ValueError("dict_of wants one entry per stream")
            of = np.array([_capi.DICT_NONE if d is None else int(d) for d in dict_of], dtype=np.uint32)
        if caps is None:
            caps = [max(1 << 16, len(c) * 1100 + 1024) for c in streams]
        caps = np.array([int(c) for c in caps], dtype=np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(caps, out=out_off[1:])
        out = np.zeros(int(out_off[-1]) + 8, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        consumed = np.zeros(n, dtype=np.uint64)
        rc = self._L.flate_hip_decompress_batch_dict(self._h, blob.ctypes.data, in_off.ctypes.data, n, container, flags,
                                                     out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data,
                                                     status.ctypes.data, consumed.ctypes.data, MEM_HOST, dblob.ctypes.data,
                                                     d_off.ctypes.data, len(dicts), None if of is None else of.ctypes.data)
        self._check(rc, "flate_hip_decompress_batch_dict")
        res = [out[int(out_off[i]): int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
        return res, [int(s) for s in status], [int(c) for c in consumed]

    def compress_many_dict(self, chunks, dicts, dict_of=None, container=0, mode=6, caps=None):
        """Records compressed against preset dictionaries (flate_hip_compress_batch_dict; raw or zlib, levels 4..9): the
        streams decompress_many_dict and zlib.decompressobj(wbits, zdict=...) inflate.  dicts: sequence of bytes-like.
        dict_of: per record the index of its dictionary or None (it has none); default None: there is exactly one
        dictionary and every record uses it.  The last min(len, 32768) bytes of a dictionary and the record may be 65535
        bytes together; a longer one raises FlateHipError (FLATE_HIP_E_UNSUPPORTED).  caps: slot size per record
        (default: compress_bound + 4).  Returns (list of bytes, list of status codes)."""
        self._sync_env()
        if container == _capi.GZIP:
            raise ValueError("gzip has no preset dictionaries")
        n = len(chunks)
        if dict_of is None and len(dicts) != 1:
            raise ValueError("dict_of may be left out only with exactly one dictionary")
        if n == 0:
            return [], []
        blob, in_off = self._host_input(chunks)
        dblob, d_off = self._host_input(dicts)
        of = None
        if dict_of is not None:
            if len(dict_of) != n:
                raise ValueError("dict_of wants one entry per record")
            of = np.array([_capi.DICT_NONE if d is None else int(d) for d in dict_of], dtype=np.uint32)
        if caps is None:
            caps = [(self.compress_bound(len(c), container, mode) + 4 + 7) & ~7 for c in chunks]
        caps = np.array([int(c) for c in caps], dtype=np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(caps, out=out_off[1:])
        out = np.zeros(int(out_off[-1]) + 8, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        rc = self._L.flate_hip_compress_batch_dict(self._h, blob.ctypes.data, in_off.ctypes.data, n, container, mode,
                                                   out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data,
                                                   status.ctypes.data, MEM_HOST, dblob.ctypes.data, d_off.ctypes.data,
                                                   len(dicts), None if of is None else of.ctypes.data)
        self._check(rc, "flate_hip_compress_batch_dict")
        res = [out[int(out_off[i]): int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
        return res, [int(s) for s in status]

    def joined_bound(self, n, piece=65535, container=0, mode=6):
        return int(self._L.flate_hip_joined_bound(int(n), int(piece), container, mode))

    def compress_joined(self, streams, container, mode, piece=65535, caps=None, index_spacing=None):
        """Every input as ONE gzip / zlib / raw stream of independent pieces of `piece` bytes (flate_hip_compress_joined;
        levels 4..9, piece 1..65535): the pieces are compressed with no history at the rate of the chunk path and joined
        with sync-flush markers, one header and one footer around them -- any inflater reads the result.  caps: slot
        size per stream (default: joined_bound).  Returns (list of bytes, list of status codes).  index_spacing (a
        number of bytes; 0: 1 MiB): flate_hip_compress_joined_indexed runs, and the handle of the fresh seek index over
        the streams is returned as a third value, to be given to index_destroy (or to an Index)."""
        self._sync_env()
        if not 1 <= int(piece) <= _capi.JOIN_MAX_PIECE:
            raise ValueError("piece must be 1..%d" % _capi.JOIN_MAX_PIECE)
        n = len(streams)
        if n == 0 and index_spacing is None:
            return [], []
        blob, in_off = self._host_input(streams)
        if caps is None:
            caps = [(self.joined_bound(len(c), piece, container, mode) + 7) & ~7 for c in streams]
        caps = np.array([int(c) for c in caps], dtype=np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(caps, out=out_off[1:])
        out = np.zeros(int(out_off[-1]) + 8, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        ix = C.c_void_p()
        if index_spacing is None:
            rc = self._L.flate_hip_compress_joined(self._h, blob.ctypes.data, in_off.ctypes.data, n, int(piece), container, mode,
                                                   out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data,
                                                   status.ctypes.data, MEM_HOST)
            self._check(rc, "flate_hip_compress_joined")
        else:
            rc = self._L.flate_hip_compress_joined_indexed(self._h, blob.ctypes.data, in_off.ctypes.data, n, int(piece), container,
                                                           mode, out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data,
                                                           status.ctypes.data, MEM_HOST, int(index_spacing), C.byref(ix))
            self._check(rc, "flate_hip_compress_joined_indexed")
        res = [out[int(out_off[i]): int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
        if index_spacing is None:
            return res, [int(s) for s in status]
        return res, [int(s) for s in status], ix

    # ---- device buffers (raw pointers; everything already in HBM) ----
    def compress_joined_device(self, in_ptr, in_off_ptr, n_streams, piece, container, mode, out_ptr, out_off_ptr,
                               out_len_ptr, status_ptr):
        self._sync_env()
        rc = self._L.flate_hip_compress_joined(self._h, in_ptr, in_off_ptr, n_streams, int(piece), container, mode, out_ptr,
                                               out_off_ptr, out_len_ptr, status_ptr, MEM_DEVICE)
        self._check(rc, "flate_hip_compress_joined")

    def compress_joined_indexed_device(self, in_ptr, in_off_ptr, n_streams, piece, container, mode, out_ptr, out_off_ptr,
                                       out_len_ptr, status_ptr, spacing=0, memkind=MEM_DEVICE):
        """flate_hip_compress_joined_indexed on raw pointers; returns the handle of the fresh index, to be given to
        index_destroy.  The host waits for the stream."""
        self._sync_env()
        ix = C.c_void_p()
        rc = self._L.flate_hip_compress_joined_indexed(self._h, in_ptr, in_off_ptr, n_streams, int(piece), container, mode,
                                                       out_ptr, out_off_ptr, out_len_ptr, status_ptr, memkind, int(spacing),
                                                       C.byref(ix))
        self._check(rc, "flate_hip_compress_joined_indexed")
        return ix

    def compress_device(self, in_ptr, in_off_ptr, n_chunks, container, mode, out_ptr, out_off_ptr, out_len_ptr,
                        status_ptr):
        self._sync_env()
        rc = self._L.flate_hip_compress_batch(self._h, in_ptr, in_off_ptr, n_chunks, container, mode, out_ptr,
                                              out_off_ptr, out_len_ptr, status_ptr, MEM_DEVICE)
        self._check(rc, "flate_hip_compress_batch")

    def plan_compress(self, in_off, out_off, container, mode):
        """Plan a device batch whose layout repeats (host offset arrays, n + 1 entries each); returns a
        handle for compress_planned / plan_destroy."""
        self._sync_env()
        a = np.ascontiguousarray(in_off, dtype=np.uint64)
        b = np.ascontiguousarray(out_off, dtype=np.uint64)
        plan = C.c_void_p()
        rc = self._L.flate_hip_plan_compress(self._h, a.ctypes.data, b.ctypes.data, a.size - 1, container, mode,
                                             C.byref(plan))
        self._check(rc, "flate_hip_plan_compress")
        return plan

    def compress_planned(self, plan, in_ptr, out_ptr, out_len_ptr, status_ptr):
        """Enqueue one planned batch: kernels only, nothing touches the host."""
        rc = self._L.flate_hip_compress_planned(self._h, plan, in_ptr, out_ptr, out_len_ptr, status_ptr)
        self._check(rc, "flate_hip_compress_planned")

    def plan_destroy(self, plan):
        self._L.flate_hip_plan_destroy(self._h, plan)

    def decompress_device(self, in_ptr, in_off_ptr, n_chunks, container, flags, out_ptr, out_off_ptr, out_len_ptr,
                          status_ptr, consumed_ptr=None):
        self._sync_env()
        rc = self._L.flate_hip_decompress_batch(self._h, in_ptr, in_off_ptr, n_chunks, container, flags, out_ptr,
                                                out_off_ptr, out_len_ptr, status_ptr, consumed_ptr, MEM_DEVICE)
        self._check(rc, "flate_hip_decompress_batch")

    def decompress_dict_device(self, in_ptr, in_off_ptr, n_chunks, container, flags, out_ptr, out_off_ptr, out_len_ptr,
                               status_ptr, consumed_ptr, dict_ptr, dict_off_ptr, n_dicts, dict_of_ptr=None):
        """flate_hip_decompress_batch_dict on device memory (n_dicts + 1 dictionary offsets; dict_of: n_chunks uint32 or
        None with one dictionary)."""
        self._sync_env()
        rc = self._L.flate_hip_decompress_batch_dict(self._h, in_ptr, in_off_ptr, n_chunks, container, flags, out_ptr,
                                                     out_off_ptr, out_len_ptr, status_ptr, consumed_ptr, MEM_DEVICE,
                                                     dict_ptr, dict_off_ptr, n_dicts, dict_of_ptr)
        self._check(rc, "flate_hip_decompress_batch_dict")

    def compress_dict_device(self, in_ptr, in_off_ptr, n_chunks, container, mode, out_ptr, out_off_ptr, out_len_ptr,
                             status_ptr, dict_ptr, dict_off_ptr, n_dicts, dict_of_ptr=None):
        """flate_hip_compress_batch_dict on device memory (n_dicts + 1 dictionary offsets; dict_of: n_chunks uint32 or
        None with one dictionary).  Returns the call's return code where it is FLATE_HIP_E_INVALID_ARG or
        FLATE_HIP_E_UNSUPPORTED -- the call has done nothing then --, raises on every other failure."""
        self._sync_env()
        rc = self._L.flate_hip_compress_batch_dict(self._h, in_ptr, in_off_ptr, n_chunks, container, mode, out_ptr,
                                                   out_off_ptr, out_len_ptr, status_ptr, MEM_DEVICE, dict_ptr,
                                                   dict_off_ptr, n_dicts, dict_of_ptr)
        if rc in (_capi.E_INVALID_ARG, _capi.E_UNSUPPORTED):
            return rc
        self._check(rc, "flate_hip_compress_batch_dict")
        return 0

    def decompressed_sizes_device(self, in_ptr, in_off_ptr, n_chunks, container, flags, sizes_ptr, status_ptr,
                                  consumed_ptr=None):
        """The size probe on device memory (n + 1 offsets, n sizes / statuses / consumed): enqueued on the handle's
        stream unless the batch has long streams that are cut (flate_hip_decompressed_sizes)."""
        self._sync_env()
        rc = self._L.flate_hip_decompressed_sizes(self._h, in_ptr, in_off_ptr, n_chunks, container, flags, sizes_ptr,
                                                  status_ptr, consumed_ptr, MEM_DEVICE)
        self._check(rc, "flate_hip_decompressed_sizes")

    def size_paths(self):
        """How the last size probe got its sizes: (streams summed over a closed chain of spans, streams counted whole
        by one wave) (flate_hip_debug_size_paths)."""
        v = np.zeros(2, dtype=np.uint64)
        self._check(self._L.flate_hip_debug_size_paths(self._h, v.ctypes.data), "flate_hip_debug_size_paths")
        return int(v[0]), int(v[1])

    def inflater(self, n, container, flags=0):
        """n resumable stream decoders (flate_hip_inflater_*): feed each its input piece by piece, in bounded memory."""
        return Inflater(self, n, container, flags)

    def inflater_feed_device(self, inflater, in_ptr, in_off_ptr, final_ptr, out_ptr, out_off_ptr, out_len_ptr,
                             consumed_ptr, status_ptr):
        """One feed of an inflater on device memory (n + 1 offsets, n final flags / lengths / statuses): enqueued on the
        handle's stream, the kernel reads the offsets itself; set_sync decides about the final wait."""
        rc = self._L.flate_hip_inflater_feed(self._h, inflater._s, in_ptr, in_off_ptr, final_ptr, out_ptr, out_off_ptr,
                                             out_len_ptr, consumed_ptr, status_ptr, MEM_DEVICE)
        self._check(rc, "flate_hip_inflater_feed")

    def deflater(self, n, container, mode, flags=0):
        """n resumable compressors (flate_hip_deflater_*, modes 0 and 1): feed each its input piece by piece, in bounded
        memory."""
        return Deflater(self, n, container, mode, flags)

    def deflater_feed_device(self, deflater, in_ptr, in_off_ptr, op_ptr, out_ptr, out_off_ptr, out_len_ptr,
                             consumed_ptr, status_ptr):
        """One feed of a deflater on device memory (n + 1 offsets, n ops / lengths / statuses).  The feed reads the
        offsets and ops back and waits for its kernels."""
        rc = self._L.flate_hip_deflater_feed(self._h, deflater._d, in_ptr, in_off_ptr, op_ptr, out_ptr, out_off_ptr,
                                             out_len_ptr, consumed_ptr, status_ptr, MEM_DEVICE)
        self._check(rc, "flate_hip_deflater_feed")

    def device_bytes(self):
        """Device bytes the handle's deflaters hold (state, buffers, feed workspace, pending output)."""
        v = C.c_uint64(0)
        self._check(self._L.flate_hip_debug_device_bytes(self._h, C.byref(v)), "flate_hip_debug_device_bytes")
        return int(v.value)

    def workspace_bytes(self):
        """Device bytes the handle keeps as workspace of its passes (not the staged copies of a batch's data, not its chunk
        tables, not the deflaters')."""
        v = C.c_uint64(0)
        self._check(self._L.flate_hip_debug_workspace_bytes(self._h, C.byref(v)), "flate_hip_debug_workspace_bytes")
        return int(v.value)

    def inflate_paths(self):
        """Which path finished the streams of the last decompress call: {"span_done", "span_handed_on", "par_done",
        "par_handed_on"} (flate_hip_debug_inflate_paths); every stream in neither *_done was decoded by k_inflate."""
        v = np.zeros(4, dtype=np.uint64)
        self._check(self._L.flate_hip_debug_inflate_paths(self._h, v.ctypes.data), "flate_hip_debug_inflate_paths")
        return dict(zip(("span_done", "span_handed_on", "par_done", "par_handed_on"), (int(x) for x in v)))

    def gather_streams_device(self, out_ptr, out_off_ptr, out_len_ptr, n_chunks, dst_ptr, dst_off_ptr):
        """Pack the produced streams back to back in device memory (dst_off gets n_chunks + 1 entries)."""
        rc = self._L.flate_hip_gather_streams(self._h, out_ptr, out_off_ptr, out_len_ptr, n_chunks, dst_ptr,
                                              dst_off_ptr)
        self._check(rc, "flate_hip_gather_streams")

    # ---- measurement / test seams ----
    def profile_enable(self, flag=True):
        self._L.flate_hip_profile_enable(self._h, int(bool(flag)))

    def profile_reset(self):
        self._L.flate_hip_profile_reset(self._h)

    def profile_read(self):
        """{kernel name: (total_ms, launches)}"""
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        cnt = (C.c_uint64 * cap)()
        n = self._L.flate_hip_profile_read(self._h, names, ms, cnt, cap)
        return {names[i].decode(): (ms[i], int(cnt[i])) for i in range(max(n, 0))}

    def phase_cycles(self):
        """Shader-clock timestamps of workgroup 0's phases in the last tokenizer launch (tuning aid)."""
        buf = np.zeros(160, dtype=np.uint64)
        self._L.flate_hip_debug_phase_cycles(self._h, buf.ctypes.data, 160)
        return buf

    def debug_write_block(self, tokens, input_bytes, eof, dynamic_only=False):
        """One block from a token list through the device planner / offset scan / bit packer
        (input_bytes None = the Zig null).  Returns the block's bytes."""
        tok = np.ascontiguousarray(tokens, dtype=np.uint32)
        inp = None if input_bytes is None else np.frombuffer(bytes(input_bytes), dtype=np.uint8)
        cap = 8 * tok.size + (0 if inp is None else inp.size) + 1024
        out = np.zeros(cap + 8, dtype=np.uint8)
        out_len = np.zeros(1, dtype=np.uint64)
        keep = np.zeros(1, dtype=np.uint8)  # a non-NULL pointer for an empty input
        rc = self._L.flate_hip_debug_write_block(
            self._h, tok.ctypes.data if tok.size else None, tok.size,
            None if inp is None else (inp.ctypes.data if inp.size else keep.ctypes.data),
            0 if inp is None else inp.size, int(bool(eof)), int(bool(dynamic_only)), out.ctypes.data, cap,
            out_len.ctypes.data)
        self._check(rc, "flate_hip_debug_write_block")
        return out[: int(out_len[0])].tobytes()

    @staticmethod
    def debug_block_bound(n_tokens, input_len):
        """Bytes that hold any block of n_tokens tokens (48 bits each at most) or its stored form, and the 8 spare
        bytes debug_write_blocks asks for behind it."""
        return 6 * int(n_tokens) + int(input_len) + 700

    def debug_write_blocks(self, blocks, encoder=0, paired=False, dynamic_only=False, slot_starts=None):
        """n blocks, each (tokens, input_bytes or None, eof), in ONE launch of the device planner / offset scan and
        the bit packer `encoder` names (0: k_encode<true>, 1: k_encode_wave); paired: the chunk path's layout of two plan
        slots a chunk (include/flate_hip.h).  slot_starts: byte offset of every block's output slot (ascending, any
        residue mod 4, debug_block_bound apart at least); default: slot i at residue i mod 4.  Returns the blocks' bytes."""
        n = len(blocks)
        toks = [np.ascontiguousarray(b[0], dtype=np.uint32) for b in blocks]
        inps = [np.zeros(0, np.uint8) if b[1] is None else np.frombuffer(bytes(b[1]), dtype=np.uint8) for b in blocks]
        has = np.array([b[1] is not None for b in blocks], dtype=np.uint8)
        eof = np.array([bool(b[2]) for b in blocks], dtype=np.uint8)
        tok_off = np.zeros(n + 1, dtype=np.uint64)
        tok_off[1:] = np.cumsum([t.size for t in toks])
        in_off = np.zeros(n + 1, dtype=np.uint64)
        in_off[1:] = np.cumsum([a.size for a in inps])
        tok_all = np.concatenate(toks + [np.zeros(1, np.uint32)])
        in_all = np.concatenate(inps + [np.zeros(1, np.uint8)])
        caps = np.array([self.debug_block_bound(t.size, a.size) for t, a in zip(toks, inps)], dtype=np.uint64)
        if slot_starts is None:
            slot_starts, at = [], 0
            for i in range(n):
                at = (at + 3) // 4 * 4 + i % 4
                slot_starts.append(at)
                at += int(caps[i])
        starts = np.array(slot_starts, dtype=np.uint64)
        ends = starts + caps
        if n > 1 and (starts[1:] < ends[:-1]).any():
            raise ValueError("debug_write_blocks: output slots overlap")
        out_cap = (int(ends.max()) + 3) // 4 * 4
        out = np.zeros(out_cap, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint64)
        rc = self._L.flate_hip_debug_write_blocks(
            self._h, n, tok_all.ctypes.data, tok_off.ctypes.data, in_all.ctypes.data, in_off.ctypes.data,
            has.ctypes.data, eof.ctypes.data, int(bool(dynamic_only)), int(encoder), int(bool(paired)),
            out.ctypes.data, out_cap, starts.ctypes.data, caps.ctypes.data, out_len.ctypes.data)
        self._check(rc, "flate_hip_debug_write_blocks")
        return [out[int(s): int(s) + int(m)].tobytes() for s, m in zip(starts, out_len)]

    def debug_tokens(self, chunk):
        """Token list the tokenizer kernels produced for `chunk` of the last level 4..9 call."""
        buf = np.zeros(65536, dtype=np.uint32)
        n = self._L.flate_hip_debug_tokens(self._h, int(chunk), buf.ctypes.data, buf.size)
        if n > buf.size:  # whole-stream pass: the count comes back even when the buffer is short
            buf = np.zeros(n, dtype=np.uint32)
            n = self._L.flate_hip_debug_tokens(self._h, int(chunk), buf.ctypes.data, buf.size)
        if n < 0:
            raise FlateHipError("flate_hip_debug_tokens failed with %d" % n)
        return buf[:n].copy()


class Inflater:
    """n independent stream decoders whose state stays on the device between feeds (include/flate_hip.h)."""

    def __init__(self, engine, n, container, flags=0):
        self._eng, self.n, self.container = engine, int(n), container
        self._s = C.c_void_p()
        engine._check(engine._L.flate_hip_inflater_create(engine._h, self.n, container, int(flags), C.byref(self._s)),
                      "flate_hip_inflater_create")

    def feed(self, pieces, final=None, caps=None):
        """pieces: n bytes-like, or None = skip that stream (empty piece, not final, no slot).  final: a bool for all or
        one per stream (default False).  caps: output slot per stream (default max(64 KiB, 8 x the piece); at least 258).
        Returns (list of output bytes, list of statuses, list of consumed input bytes)."""
        n = self.n
        if len(pieces) != n:
            raise ValueError("feed() wants %d pieces" % n)
        if final is None or isinstance(final, (bool, int)):
            final = [bool(final)] * n
        if caps is None or isinstance(caps, int):
            caps = [caps] * n
        skip = [p is None for p in pieces]
        data = [b"" if p is None else bytes(p) for p in pieces]
        fin = np.array([0 if skip[i] else int(bool(final[i])) for i in range(n)], dtype=np.uint8)
        cap = np.array([0 if skip[i] else (caps[i] if caps[i] is not None else max(1 << 16, 8 * len(data[i])))
                        for i in range(n)], dtype=np.uint64)
        in_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.array([len(d) for d in data], dtype=np.uint64), out=in_off[1:])
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(cap, out=out_off[1:])
        blob = np.frombuffer(b"".join(data), dtype=np.uint8) if in_off[-1] else np.zeros(1, dtype=np.uint8)
        out = np.zeros(max(int(out_off[-1]), 1), dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint64)
        consumed = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        L = self._eng._L
        rc = L.flate_hip_inflater_feed(self._eng._h, self._s, blob.ctypes.data, in_off.ctypes.data, fin.ctypes.data,
                                       out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data, consumed.ctypes.data,
                                       status.ctypes.data, MEM_HOST)
        self._eng._check(rc, "flate_hip_inflater_feed")
        outs = [out[int(out_off[i]): int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
        return outs, [int(v) for v in status], [int(v) for v in consumed]

    def set_dictionary(self, indices, zdict):
        """Give these streams one preset dictionary (flate_hip_inflater_set_dictionary).  Only a stream that has absorbed
        nothing since create / reset takes it.  Returns the list of booleans: applied or not, one per index."""
        w = np.ascontiguousarray(list(indices), dtype=np.uint32)
        if w.size == 0:
            return []
        d = np.frombuffer(bytes(zdict), dtype=np.uint8) if len(zdict) else np.zeros(1, dtype=np.uint8)
        applied = np.zeros(w.size, dtype=np.uint8)
        rc = self._eng._L.flate_hip_inflater_set_dictionary(self._eng._h, self._s, w.ctypes.data, w.size, d.ctypes.data,
                                                            len(zdict), MEM_HOST, applied.ctypes.data)
        self._eng._check(rc, "flate_hip_inflater_set_dictionary")
        return [bool(a) for a in applied]

    def reset(self, indices):
        """Start a new member on these streams (Inflate.reset, inflate.zig:301-309).  Drops a preset dictionary."""
        w = np.ascontiguousarray(list(indices), dtype=np.uint32)
        rc = self._eng._L.flate_hip_inflater_reset(self._eng._h, self._s, w.ctypes.data if w.size else None, w.size)
        self._eng._check(rc, "flate_hip_inflater_reset")

    def close(self):
        if getattr(self, "_s", None) and self._s.value and self._eng._h.value:
            self._eng._L.flate_hip_inflater_destroy(self._eng._h, self._s)
        self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Deflater:
    """n independent huffman-only / store-only compressors whose state stays on the device between feeds
    (include/flate_hip.h)."""

    def __init__(self, engine, n, container, mode, flags=0):
        self._eng, self.n, self.container, self.mode = engine, int(n), container, mode
        self._d = C.c_void_p()
        engine._check(engine._L.flate_hip_deflater_create(engine._h, self.n, container, int(mode), int(flags),
                                                          C.byref(self._d)), "flate_hip_deflater_create")

    def feed(self, pieces, op=0, caps=None):
        """pieces: n bytes-like, or None = an empty piece.  op: FEED_MORE / FEED_FLUSH / FEED_FINISH for all, or one per
        stream.  caps: output slot per stream (default: room for everything the piece can produce).
        Returns (list of output bytes, list of statuses, list of consumed input bytes)."""
        n = self.n
        if len(pieces) != n:
            raise ValueError("feed() wants %d pieces" % n)
        if isinstance(op, int):
            op = [op] * n
        if caps is None or isinstance(caps, int):
            caps = [caps] * n
        data = [b"" if p is None else bytes(p) for p in pieces]
        ops = np.array([int(o) for o in op], dtype=np.uint8)
        cap = np.array([caps[i] if caps[i] is not None else len(data[i]) + 5 * (len(data[i]) // 65535) + (1 << 17)
                        for i in range(n)], dtype=np.uint64)
        in_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.array([len(d) for d in data], dtype=np.uint64), out=in_off[1:])
        out_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(cap, out=out_off[1:])
        blob = np.frombuffer(b"".join(data), dtype=np.uint8) if in_off[-1] else np.zeros(1, dtype=np.uint8)
        out = np.zeros(max(int(out_off[-1]), 1), dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint64)
        consumed = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.int32)
        rc = self._eng._L.flate_hip_deflater_feed(self._eng._h, self._d, blob.ctypes.data, in_off.ctypes.data,
                                                  ops.ctypes.data, out.ctypes.data, out_off.ctypes.data,
                                                  out_len.ctypes.data, consumed.ctypes.data, status.ctypes.data,
                                                  MEM_HOST)
        self._eng._check(rc, "flate_hip_deflater_feed")
        outs = [out[int(out_off[i]): int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
        return outs, [int(v) for v in status], [int(v) for v in consumed]

    def reset(self, indices):
        """Start a new stream (a new gzip / zlib member) on these streams."""
        w = np.ascontiguousarray(list(indices), dtype=np.uint32)
        rc = self._eng._L.flate_hip_deflater_reset(self._eng._h, self._d, w.ctypes.data if w.size else None, w.size)
        self._eng._check(rc, "flate_hip_deflater_reset")

    def close(self):
        if getattr(self, "_d", None) and self._d.value and self._eng._h.value:
            self._eng._L.flate_hip_deflater_destroy(self._eng._h, self._d)
        self._d = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Index:
    """A seek index over a batch of streams (Engine.build_index / Engine.index_from_bytes) together with the streams' bytes,
    which every read needs.  The bytes stay in host memory; a read stages only the part of them its ranges can consume, from
    a range's point to the first point behind its end."""

    def __init__(self, engine, handle, blob, in_off, n):
        self._e, self._ix, self._blob, self._in_off, self.n = engine, handle, blob, in_off, n

    def info(self, stream=0):
        """(size, status, number of points) of a stream"""
        return self._e.index_info(self._ix, stream)

    def points(self, stream=0):
        """[(in_bit, out_pos)] of a stream"""
        return self._e.index_points(self._ix, stream)

    def read_ranges(self, ranges):
        """ranges: [(stream, begin, length)] -> (list of bytes, list of status codes); a range is clipped to its stream's
        size (flate_hip_decompress_ranges)."""
        m = len(ranges)
        if m == 0:
            return [], []
        sizes = {}
        for s, _, _ in ranges:
            if s not in sizes:
                sizes[s] = self.info(s)[0]
        rs = np.array([r[0] for r in ranges], dtype=np.uint32)
        rb = np.array([min(int(r[1]), (1 << 64) - 1) for r in ranges], dtype=np.uint64)
        rl = np.array([min(int(r[2]), (1 << 64) - 1) for r in ranges], dtype=np.uint64)
        caps = np.array([max(0, min(int(r[2]), sizes[r[0]] - min(int(r[1]), sizes[r[0]]))) for r in ranges], dtype=np.uint64)
        out_off = np.zeros(m + 1, dtype=np.uint64)
        np.cumsum(caps, out=out_off[1:])
        out = np.zeros(int(out_off[-1]) + 8, dtype=np.uint8)
        out_len = np.zeros(m, dtype=np.uint64)
        status = np.zeros(m, dtype=np.int32)
        rc = self._e.decompress_ranges_device(self._ix, self._blob.ctypes.data, self._in_off.ctypes.data, self.n, m, rs.ctypes.data,
                                              rb.ctypes.data, rl.ctypes.data, out.ctypes.data, out_off.ctypes.data,
                                              out_len.ctypes.data, status.ctypes.data, MEM_HOST)
        self._e._check(rc, "flate_hip_decompress_ranges")
        return ([out[int(out_off[j]): int(out_off[j]) + int(out_len[j])].tobytes() for j in range(m)], [int(s) for s in status])

    def to_bytes(self):
        """the index as one self-contained blob (flate_hip_index_export; the streams' bytes are not in it)"""
        return self._e.index_export(self._ix)

    def close(self):
        if self._ix is not None and getattr(self._e, "_h", None) and self._e._h.value:
            self._e.index_destroy(self._ix)
        self._ix = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default = None


def default_engine():
    global _default
    if _default is None:
        _default = Engine(0)
    return _default
