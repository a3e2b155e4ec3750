#!/usr/bin/env python3
"""gzip <file>: writes <file>.gz with the MI355X engine -- the reference's bin/gzip.zig:20
(`gzip.compress(input_file.reader(), output_file.writer(), .{})`, comparable to `gzip -kfn`).
Options beyond the reference's tool: -l LEVEL (4..9), --huffman, --store, and --piece N (with --huffman or --store):
bounded memory -- the file is read N bytes at a time and compressed by a resumable compressor as it arrives;
--joined [N] (levels 4..9): one gzip stream of independent pieces of N bytes (1..65535, default 65535) at the rate of the
batched chunk path, as pigz -i writes it -- a file of any length, a little larger than the whole-stream output;
--index FILE [--spacing S] (with --joined): also writes a seek index over the .gz to FILE -- piece starts every S bytes or
so (default 1 MiB), no windows -- which gunzip.py --index FILE --range B:N reads."""
import argparse
import os
os.environ.setdefault("FLATE_HIP_PRELOAD_TORCH_HIP", "1")  # one HIP runtime per process: torch, imported later, brings its own (flate_amd/_capi.py)
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("input_file")
    ap.add_argument("-l", dest="level", type=int, default=6, choices=range(4, 10))
    ap.add_argument("--huffman", action="store_true")
    ap.add_argument("--store", action="store_true")
    ap.add_argument("--piece", type=int, default=None)
    ap.add_argument("--joined", type=int, nargs="?", const=65535, default=None, metavar="N")
    ap.add_argument("--index", default=None, metavar="FILE")
    ap.add_argument("--spacing", type=int, default=None, metavar="S")
    a = ap.parse_args(argv)
    if a.index is not None and a.joined is None:
        ap.error("--index FILE needs --joined")
    if a.spacing is not None and (a.index is None or a.spacing < 1):
        ap.error("--spacing S needs --index FILE and S >= 1")
    if a.joined is not None and (a.huffman or a.store or a.piece is not None or not 1 <= a.joined <= 65535):
        ap.error("--joined [N] needs 1 <= N <= 65535 and takes none of --huffman, --store, --piece")
    if a.piece is not None and (a.piece < 1 or not (a.huffman or a.store)):
        ap.error("--piece N needs N >= 1 and --huffman or --store (levels 4..9 are not resumable)")
    from flate_amd import gzip
    with open(a.input_file, "rb") as src, open(a.input_file + ".gz", "wb") as dst:
        if a.huffman:
            gzip.huffman.compress(src, dst, piece=a.piece)
        elif a.store:
            gzip.store.compress(src, dst, piece=a.piece)
        elif a.joined is not None:
            blob = gzip.compress(src, dst, gzip.Options(level=a.level), joined=a.joined,
                                 index=None if a.index is None else (True if a.spacing is None else a.spacing))
            if blob is not None:
                with open(a.index, "wb") as f:
                    f.write(blob)
        else:
            gzip.compress(src, dst, gzip.Options(level=a.level))
    return 0


if __name__ == "__main__":
    sys.exit(main())
