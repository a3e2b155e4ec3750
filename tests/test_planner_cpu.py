"""CPU check of the serial block planner (flate_amd/csrc/flate_common.h) -- the exact
source that one GPU lane per block executes -- against the oracle and the reference's
golden block vectors (block_writer.zig:599-706).  No GPU."""
import json
import os

import numpy as np
import pytest

import _oracle as O
from _planner_shim import encode_block, load_shim, tables
from conftest import GOLDEN, golden


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def test_tables_match_oracle(shim):
    li, le, lb, dc, de, db = tables(shim)
    for v in range(256):
        assert 257 + int(li[v]) == O.lib().fo_length_code(v)
    for d in range(32768):
        assert dc[d] == O.lib().fo_distance_code(d)
    for i in range(29):
        assert le[i] == O.lib().fo_length_extra_bits(257 + i)
    for i in range(30):
        assert de[i] == O.lib().fo_distance_extra_bits(i)
    assert list(lb) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 112,
                        128, 160, 192, 224, 255]
    assert list(db[:6]) == [0, 1, 2, 3, 4, 6] and db[29] == 0x6000 and db[28] == 0x4000


@pytest.fixture(params=[0, 1], ids=["lazy-loop", "package-merge"])
def pm(request, shim):
    """Both forms of the Huffman bit counts: the reference's lazy loop and the package-merge form the GPU runs."""
    shim.shim_set_pm(request.param)
    yield request.param
    shim.shim_set_pm(0)


def test_package_merge_equals_the_lazy_loop(shim):
    """huffman_encoder.zig:122-247 as package-merge (flate_common.h fl_huff_bit_counts_pm) against the loop
    itself, on frequency sets that stress ties, the length limit and totals of exactly 65536 (Q3's 65535-leaves)."""
    rng = np.random.default_rng(23)
    n_cases = 0
    for it in range(1600):
        kind = it % 8
        n = int(rng.integers(3, 287))
        f = np.zeros(286, np.int64)
        if kind == 0:
            f = rng.integers(0, 50, 286)
        elif kind == 1:
            f = (rng.pareto(1.0, 286) * 20).clip(0, 60000).astype(np.int64)
        elif kind == 2:
            a, b = 1, 1
            for i in range(min(n, 23)):
                f[i] = a
                a, b = b, a + b
        elif kind == 3:
            w = rng.dirichlet(np.ones(n) * 0.3)
            f[:n] = np.floor(w * 65536).astype(np.int64)
            f[0] += 65536 - f.sum()
        elif kind == 4:
            f[:n] = rng.integers(1, 4, n)
        elif kind == 5:
            f[:n] = (2.0 ** rng.integers(0, 12, n)).astype(np.int64)
        elif kind == 6:
            f[:n] = 1
            f[rng.integers(0, n)] = 65535 - n
        else:
            f = rng.integers(0, 2000, 286) * (rng.random(286) < 0.4)
        f = np.clip(f, 0, 65535)
        while f.sum() > 65536:
            f = (f + 1) // 2 * (f > 0)
        rng.shuffle(f)
        for sub, mb in ((f, 15), (f[:30], 15), (f[:19], 7)):
            sub = np.ascontiguousarray(sub, dtype=np.uint16)
            res = []
            for form in (0, 1):
                shim.shim_set_pm(form)
                cs = np.zeros(sub.size, np.uint16)
                ls = np.zeros(sub.size, np.uint16)
                shim.shim_huff_generate(sub.ctypes.data, sub.size, mb, cs.ctypes.data, ls.ctypes.data)
                res.append((cs, ls))
            shim.shim_set_pm(0)
            assert (res[0][0] == res[1][0]).all() and (res[0][1] == res[1][1]).all()
            n_cases += 1
    assert n_cases == 4800


def test_huffman_generate_matches_oracle(shim, pm):
    rng = np.random.default_rng(7)
    cases = []
    for n, mb in ((286, 15), (30, 15), (19, 7)):
        for trial in range(150):
            kind = trial % 6
            if kind == 0:
                f = rng.integers(0, 50, n)
            elif kind == 1:
                f = (rng.pareto(0.6, n) * 3).astype(np.int64)
            elif kind == 2:  # fibonacci-like: forces the length limit
                f = np.zeros(n, np.int64)
                a, b = 1, 1
                for i in range(min(n, 22)):
                    f[rng.integers(0, n)] = a
                    a, b = b, a + b
            elif kind == 3:
                f = rng.integers(0, 3, n)
            elif kind == 4:
                f = np.zeros(n, np.int64)
                k = int(rng.integers(0, 5))
                f[rng.choice(n, k, replace=False)] = rng.integers(1, 1000, k)
            else:
                f = rng.integers(0, 65535, n) * (rng.random(n) < 0.3)
            f = np.clip(f, 0, 65535)
            # keep the total within what a block can hold (<= 65536 symbols)
            while f.sum() > 65536:
                f = f // 2
            cases.append((f.astype(np.uint16), mb))
    for f, mb in cases:
        co, lo = O.huffman_generate(f, mb)
        cs = np.zeros(f.size, np.uint16)
        ls = np.zeros(f.size, np.uint16)
        shim.shim_huff_generate(f.ctypes.data, f.size, mb, cs.ctypes.data, ls.ctypes.data)
        assert (lo == ls).all() and (co == cs).all()


def _cases():
    with open(os.path.join(GOLDEN, "block_writer_tokens.json")) as f:
        cases = json.load(f)
    for c in cases:
        c["tok"] = np.array([O.tok_lit(t[0]) if len(t) == 1 else O.tok_match(t[0], t[1])
                             for t in c["tokens"]], dtype=np.uint32)
    return cases


@pytest.mark.parametrize("fn", ["wb", "dyn"])
def test_planner_reproduces_block_writer_goldens(shim, pm, fn):
    n = 0
    for c in _cases():
        for with_input in (True, False):
            if with_input and not (c["input"] and c["want"]):
                continue
            inp = golden("block_writer", c["input"]) if with_input else None
            name = (c["want"] if with_input else c["want_no_input"]).replace("{s}", fn)
            want = golden("block_writer", name)
            got, plan = encode_block(shim, 0, c["tok"], inp, False, fn == "dyn")
            assert got == want, name
            got, plan = encode_block(shim, 0, c["tok"], inp, True, fn == "dyn")
            assert got[0] & 1 and bytes([got[0] & 0xFE]) + got[1:] == want
            n += 1
    assert n == 17


def test_planner_reproduces_huffman_block_goldens(shim, pm):
    names = [c["input"] for c in _cases() if c["input"]] + ["huffman-rand-max.input"]
    for name in names:
        inp = golden("block_writer", name)
        want = golden("block_writer", name.replace(".input", ".huff.expect"))
        got, plan = encode_block(shim, 1, None, inp, False)
        assert got == want, name


def test_planner_matches_oracle_on_random_blocks(shim, pm):
    rng = np.random.default_rng(11)
    for trial in range(60):
        n = int(rng.integers(0, 3000))
        kind = trial % 4
        if kind == 0:
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif kind == 1:
            data = rng.integers(97, 101, n, dtype=np.uint8).tobytes()
        elif kind == 2:
            data = (b"the quick brown fox jumps over the lazy dog " * (n // 40 + 1))[:n]
        else:
            data = bytes(n)
        toks = O.tokenize(data, 6)
        for eof in (False, True):
            want = O.block_write("wb", toks, eof, data)
            got, _ = encode_block(shim, 0, toks, data, eof)
            assert got == want
            want = O.block_write("huff", toks, eof, data)
            got, _ = encode_block(shim, 1, None, data, eof)
            assert got == want
