"""CPU tests of the pass schedule of a chunk-path batch (flate_amd/csrc/pass_plan.h, through
tests/cpu_shim/pass_plan_shim.cpp): the passes cover the batch in order, none is empty, none is larger than the slice
the two-stream path sizes its workspace by, passes k and k + 2 share a stream, and the ramp and the merged tail of the
host-buffer path are what compress_impl promises.  The largest pass is what a handle keeps on the device (two slices of
it), so a schedule that grew with the batch would be a footprint that grows with the batch."""
import random

import pytest

import _pass_plan as P

DEFAULT = (P.HOST_PASS_CHUNKS, P.MAX_PASS_CHUNKS)
# (host sub-batch limit, max_pass_chunks): the defaults, small limits, and a max_pass_chunks that caps the merged tail
CONFIGS = [DEFAULT, (1, 32768), (5, 32768), (128, 32768), (128, 5), (1024, 1100), (1024, 4096)]


def model(n, host, max_pass, pinned, ramp, planned):
    """the rule written out plainly: sub-batches of L = min(host, max_pass) on the pinned path (max_pass otherwise);
    a pinned pass that starts with fewer than L + L // 2 chunks left takes them all (up to max_pass); with n >= 3 L the
    first two pinned passes are max(64, L / 4) and max(64, L / 2), never above L"""
    pin = pinned and not planned
    L = min(host, max_pass) if pin else max_pass
    out, c0 = [], 0
    while c0 < n:
        k = len(out)
        left = n - c0
        if pin and ramp and n >= 3 * L and k < 2:
            cap = min(L, max(64, L >> (2 - k)))
        elif pin and left < L + L // 2:
            cap = min(max_pass, left)
        else:
            cap = L
        nc = min(cap, left)
        out.append((c0, nc, k & 1))
        c0 += nc
    return out


def limit(host, max_pass, pinned=True, planned=False):
    return min(host, max_pass) if pinned and not planned else max_pass


def top(L, most, small):
    """how far n goes: every pass is checked one by one, so with a limit of 1 or 5 chunks the range is shorter (3 L and
    1.5 L, where the rules change, are far inside it)"""
    return most if L >= 100 else small


def check(n, host, max_pass, pinned=True, ramp=True, planned=False):
    passes, largest = P.schedule(n, host, max_pass, pinned, ramp, planned)
    assert passes == model(n, host, max_pass, pinned, ramp, planned), (n, host, max_pass, pinned, ramp, planned)
    # contiguous cover of [0, n), nothing empty
    assert passes[0][0] == 0
    for (a, na, _), (b, _, _) in zip(passes, passes[1:]):
        assert b == a + na
    assert passes[-1][0] + passes[-1][1] == n
    assert all(nc > 0 for _, nc, _ in passes)
    # the slice: no pass above it, and it is a pass (not more than needed)
    assert largest == max(nc for _, nc, _ in passes)
    pin = pinned and not planned
    L = min(host, max_pass) if pin else max_pass
    # what the slice can be at most: a merged tail of less than 1.5 sub-batches, whatever n is
    assert largest <= max(L, min(max_pass, L + L // 2 - 1)) if pin else largest <= max_pass
    # streams alternate: k and k + 2 on one stream (and one workspace slice), k and k + 1 never
    for k in range(len(passes)):
        assert passes[k][2] == k & 1
        if k + 2 < len(passes):
            assert passes[k][2] == passes[k + 2][2]
    return passes, largest


@pytest.mark.parametrize("host,max_pass", CONFIGS)
@pytest.mark.parametrize("pinned,ramp,planned", [(True, True, False), (True, False, False), (False, True, False),
                                                 (False, True, True)])
def test_every_n_up_to_5000(host, max_pass, pinned, ramp, planned):
    for n in range(1, top(limit(host, max_pass, pinned, planned), 5000, 1000) + 1):
        check(n, host, max_pass, pinned, ramp, planned)


@pytest.mark.parametrize("host,max_pass", CONFIGS)
def test_sample_up_to_a_million(host, max_pass):
    rng = random.Random(host * 7919 + max_pass)
    for pinned, ramp, planned in [(True, True, False), (True, False, False), (False, True, True)]:
        hi = top(limit(host, max_pass, pinned, planned), 10 ** 6, 20000)
        ns = {hi, hi - 1, min(hi, 671089), min(hi, 16385)} | {rng.randrange(5001, hi + 1) for _ in range(40)}
        for n in sorted(ns):
            check(n, host, max_pass, pinned, ramp, planned)


def test_default_boundaries_by_hand():
    """the default host path (1024 a sub-batch, 32768 a pass at most), written out"""
    want = {
        1: [1],
        1024: [1024],                      # n = L: one pass
        1025: [1025],                      # L + 1: the tail merges into one pass
        1535: [1535],                      # 1.5 L - 1: still one pass -- the largest pass there is
        1536: [1024, 512],                 # 1.5 L: a sub-batch and half of one
        1537: [1024, 513],                 # 1.5 L + 1
        2559: [1024, 1535],                # the merged tail at its largest
        2560: [1024, 1024, 512],
        3071: [1024, 1024, 1023],          # 3 L - 1: no ramp
        3072: [256, 512, 1024, 1280],      # 3 L: the ramp, then the tail merges
        3073: [256, 512, 1024, 1281],      # 3 L + 1
        4097: [256, 512, 1024, 1024, 1281],
        16385: [256, 512] + [1024] * 14 + [1281],
    }
    for n, sizes in want.items():
        passes, largest = check(n, *DEFAULT)
        assert [nc for _, nc, _ in passes] == sizes, n
        assert largest == max(sizes)
    assert check(2559, *DEFAULT)[1] == 1535


@pytest.mark.parametrize("L", [1, 5, 128, 1024])
def test_boundaries_at_every_limit(L):
    """n = L, L + 1, 1.5 L +- 1, 3 L - 1, 3 L, 3 L + 1 at sub-batch limit L: the ramp starts exactly at 3 L and the
    tail merges exactly below 1.5 L"""
    half = L + L // 2
    for n in sorted({L, L + 1, half - 1, half, half + 1, 3 * L - 1, 3 * L, 3 * L + 1} - {0}):
        passes, _ = check(n, L, P.MAX_PASS_CHUNKS)
        sizes = [nc for _, nc, _ in passes]
        ramped = n >= 3 * L
        if ramped:
            assert sizes[:2] == [min(L, max(64, L // 4)), min(L, max(64, L // 2))], (L, n, sizes)
        # every pass that starts with 1.5 L or more left is one sub-batch; the first with fewer takes the rest
        c0 = 0
        for k, nc in enumerate(sizes):
            left = n - c0
            if ramped and k < 2:
                pass
            elif left < half:
                assert nc == left and k == len(sizes) - 1, (L, n, sizes)
            else:
                assert nc == L, (L, n, sizes)
            c0 += nc
        # without the ramp the same batch has no small first passes
        passes, _ = check(n, L, P.MAX_PASS_CHUNKS, ramp=False)
        assert all(nc >= min(L, n) or k == len(passes) - 1 for k, (_, nc, _) in enumerate(passes))


def test_device_and_planned_batches_cut_at_max_pass_chunks():
    for max_pass in (5, 4096, 32768):
        for n in (1, max_pass - 1, max_pass, max_pass + 1, 671089):
            if n < 1:
                continue
            for planned in (False, True):
                passes, largest = check(n, P.HOST_PASS_CHUNKS, max_pass, pinned=False, planned=planned)
                assert [nc for _, nc, _ in passes[:-1]] == [max_pass] * (len(passes) - 1)
                assert largest == min(n, max_pass)


def test_workspace_bytes_per_chunk_and_block():
    """the constants the two-stream slices are sized by: 64 KiB positions a chunk -- 2-byte chain links (levels 4-7) or
    four 2-byte link arrays (8-9), 4-byte descriptors, an anchor bit, 4-byte tokens -- and two words of counts"""
    s = 65536
    assert P.lz_chunk_bytes(6) == 2 * s + 4 * s + s // 8 + 4 * s + 8 == 648 * 1024 + 8
    assert P.lz_chunk_bytes(9) == 8 * s + 4 * s + s // 8 + 4 * s + 8
    assert P.lz_chunk_bytes(4) == P.lz_chunk_bytes(7) and P.lz_chunk_bytes(8) == P.lz_chunk_bytes(9)
    assert P.block_bytes() > 320 * 4 + 8
