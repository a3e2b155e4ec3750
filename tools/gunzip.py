#!/usr/bin/env python3
"""gunzip [--piece N | --members | --index FILE [--range BEGIN:LEN] | --scan-index FILE [--spacing N]] <file>.gz: writes <file> with the MI355X engine -- the reference's bin/gunzip.zig:25-27
(`gzip.decompress(br.reader(), output_file.writer())`; refuses names without the .gz suffix, :15-19).
Concatenated members are decoded one after the other (Inflate.reset, inflate.zig:301-309).  With --piece N the file is
read N bytes at a time and decoded by the resumable inflater: memory stays bounded whatever the file's size.  With
--members the file is read whole and all its members are found and decoded in one GPU call (gzip.decompress_members).
With --index FILE the first member is decoded and a seek index over it is written to FILE beside the normal output
(gzip.build_index), or read from FILE when it exists; with --range BEGIN:LEN only those bytes of the output are decoded,
from the index, and written to stdout.  With --scan-index FILE nothing is decoded and no output file is written: the first
member is walked for its full-flush points (gzip.scan_index; pigz -i and Z_FULL_FLUSH leave such points, one is kept every
N output bytes or so, default 1 MiB) and the window-free index is written to FILE, which --index FILE --range reads as it
reads its own."""
import os
os.environ.setdefault("FLATE_HIP_PRELOAD_TORCH_HIP", "1")  # one HIP runtime per process: torch, imported later, brings its own (flate_amd/_capi.py)
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    piece = None
    if len(argv) == 3 and argv[0] == "--piece" and argv[1].isdigit() and int(argv[1]) > 0:
        piece, argv = int(argv[1]), argv[2:]
    members = False
    if len(argv) == 2 and argv[0] == "--members":
        members, argv = True, argv[1:]
    index = rng = None
    if len(argv) >= 3 and argv[0] == "--index" and piece is None and not members:
        index, argv = argv[1], argv[2:]
        if len(argv) == 3 and argv[0] == "--range":
            b, _, n = argv[1].partition(":")
            if not (b.isdigit() and n.isdigit()):
                argv = []
            else:
                rng, argv = (int(b), int(n)), argv[2:]
    scan = spacing = None
    if len(argv) >= 3 and argv[0] == "--scan-index" and piece is None and not members and index is None:
        scan, argv = argv[1], argv[2:]
        if len(argv) == 3 and argv[0] == "--spacing":
            if argv[1].isdigit() and int(argv[1]) > 0:
                spacing, argv = int(argv[1]), argv[2:]
            else:
                argv = []
    if len(argv) != 1:
        print("usage: gunzip.py [--piece N | --members | --index FILE [--range BEGIN:LEN] | --scan-index FILE [--spacing N]] <file>.gz",
              file=sys.stderr)
        return 2
    name = argv[0]
    if not name.endswith(".gz"):
        print("not a .gz file", file=sys.stderr)
        return 1
    from flate_amd import gzip
    if scan is not None:
        return scan_index(gzip, name, scan, spacing)
    if index is not None and (rng is not None or not os.path.exists(index)):
        return with_index(gzip, name, index, rng)
    # (an index that is there already has nothing to give a full decode: the normal path below)
    # decoded into a temporary file beside the target: an archive that fails to decode leaves an existing
    # file of that name as it was (and no partial output behind)
    out_name, tmp_name = name[:-3], name[:-3] + ".gunzip-tmp"
    try:
        with open(name, "rb") as src, open(tmp_name, "wb") as dst:
            if members:
                dst.write(gzip.decompress_members(src))
            else:
                d = gzip.decompressor(src) if piece is None else gzip.decompressor(src, piece=piece)
                d.decompress(dst)
                while d.more_input():  # further members of the same file
                    d.reset()
                    d.decompress(dst)
        os.replace(tmp_name, out_name)
    except BaseException:
        if os.path.exists(tmp_name):
            os.unlink(tmp_name)
        raise
    return 0


def scan_index(gzip, name, index, spacing):
    """--scan-index: the index of the file's full-flush points, written to `index`; the file is not decoded"""
    with open(name, "rb") as src:
        ix = gzip.scan_index(src.read(), spacing)
    with open(index + ".gunzip-tmp", "wb") as f:
        f.write(ix.to_bytes())
    os.replace(index + ".gunzip-tmp", index)
    print("%d points over %d bytes" % (len(ix.points()), ix.size), file=sys.stderr)
    return 0


def with_index(gzip, name, index, rng):
    """--index: the index is read from `index` when it is there (then a range is asked for), else built while the file is
    decoded and written there"""
    with open(name, "rb") as src:
        data = src.read()
    whole = None
    if os.path.exists(index):
        with open(index, "rb") as f:
            ix = gzip.index_from_bytes(f.read(), data)
    else:
        from flate_amd import api, default_engine
        raw, outs, st, _ = default_engine().build_index([data], 1)
        api.raise_for_status(st[0])
        ix, whole = api.StreamIndex(raw), outs[0]
        with open(index + ".gunzip-tmp", "wb") as f:
            f.write(ix.to_bytes())
        os.replace(index + ".gunzip-tmp", index)
    if rng is not None:
        sys.stdout.buffer.write(ix.read_at(*rng))
        return 0
    tmp_name = name[:-3] + ".gunzip-tmp"
    with open(tmp_name, "wb") as dst:
        dst.write(whole)
    os.replace(tmp_name, name[:-3])
    return 0


if __name__ == "__main__":
    sys.exit(main())
