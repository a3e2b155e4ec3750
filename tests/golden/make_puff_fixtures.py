#!/usr/bin/env python3
"""Regenerate tests/golden/puff_verdicts.json: the reference's differential inflater (bin/puff/puff.c, built into
oracle/_ref by `make -C oracle` where the reference tree is) run on every stream the tests hand it.

Each entry is DATA -- "<sha-256 of the stream>/<output capacity>": [puff's return code, sha-256 of its output when the
code is 0, else null] -- so the tests that compare against puff.c run wherever oracle/_ref cannot be built
(tests/_oracle.py: puff_verdict).  Where oracle/_ref is built the tests ask puff.c itself and check it against this file.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))

import _oracle as O  # noqa: E402


def streams():
    """(stream, cap) of every puff.c call in the suite."""
    import test_gpu_compress as gc
    import test_gpu_inflate as gi
    import test_oracle_inflate_pins as pins
    import _deflate_synth as synth
    from _inflate_edge_cases import CASES

    def golden(*parts):
        with open(os.path.join(HERE, *parts), "rb") as f:
            return f.read()

    for name, _, _ in pins.FUZZ:
        yield golden("fuzz", name + ".input"), None
    yield O.compress(golden("rfc1951.txt")[20395:20395 + 1662], O.RAW, 6), None  # test_q6_cross_boundary_repeat
    for data in pins.random_stream_inputs():
        for mode in pins.RANDOM_STREAM_MODES:
            yield O.compress(data, O.RAW, mode), len(data) + 16
    for _, s in sorted(CASES.items()):
        yield s, 80000
    for _, (s, want) in sorted(synth.CASES.items()):  # test_synth_directed_cases_agree_with_every_reference
        yield s, pins.synth_cap(want)
    for s, want in synth.random_streams(pins.SYNTH_SEED, pins.SYNTH_STORED):  # (the sweep's other seeds: only where puff.c is built)
        yield s, pins.synth_cap(want)
    for c in gi.puff_mutants()[1]:
        yield c, 1 << 17
    for level in (4, 6, 9):  # test_q1_streams_are_reported_and_repairable: the repaired raw streams
        for d in gc._q1_inputs(level).values():
            yield O.compress(d, O.RAW, level, repair_q1=True), None


def main():
    if not O.puff_available():
        sys.exit("oracle/_ref/libpuff.so is not built (make -C oracle, with the reference tree present)")
    out = {}
    for s, cap in streams():
        rc, got = O.puff(s, cap)
        out[O.puff_key(s, cap)] = [rc, O.digest(got) if rc == 0 else None]
    path = os.path.join(HERE, "puff_verdicts.json")
    with open(path, "w") as f:
        f.write("{\n%s\n}\n" % ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(out.items())))
    print("%d verdicts -> %s" % (len(out), path))


if __name__ == "__main__":
    main()
