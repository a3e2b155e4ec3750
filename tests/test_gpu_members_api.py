"""decompress_members on the three facade modules (flate_amd.flate / gzip / zlib) and `tools/gunzip.py --members`: the
concatenated members' bytes, or the facade's error for the first member that fails."""
import io
import os
import subprocess
import sys

import pytest

import _oracle as O
from conftest import ROOT
from flate_amd import api, flate, gzip, synth, zlib
from gpu_util import engine

pytestmark = pytest.mark.gpu

PARTS = [synth.text(synth.SEED_TEXT + k, n).tobytes() for k, n in enumerate((1000, 0, 70000))]


@pytest.mark.parametrize("mod,container", [(flate, O.RAW), (gzip, O.GZIP), (zlib, O.ZLIB)])
def test_facade_decompress_members(mod, container):
    engine()
    data = b"".join(O.compress(p, container, m) for p, m in zip(PARTS, (6, 1, 0)))
    assert mod.decompress_members(data) == b"".join(PARTS)
    assert mod.decompress_members(io.BytesIO(data)) == b"".join(PARTS)
    with pytest.raises(api.EndOfStream):
        mod.decompress_members(b"")
    with pytest.raises(api.EndOfStream):
        mod.decompress_members(data[:-1] if container != O.RAW else data[:-3])


def test_facade_raises_the_failing_members_error():
    engine()
    good = O.compress(PARTS[0], O.GZIP, 6)
    with pytest.raises(api.WrongGzipChecksum):
        gzip.decompress_members(good + good[:-8] + bytes([good[-8] ^ 1]) + good[-7:] + good)
    with pytest.raises(api.BadGzipHeader):
        gzip.decompress_members(good + bytes(10))


def test_gunzip_members(tmp_path):
    engine()
    gz = tmp_path / "two.txt.gz"
    gz.write_bytes(O.compress(PARTS[0], O.GZIP, 6) + O.compress(PARTS[2], O.GZIP, 1))
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gunzip.py"), "--members", str(gz)], check=True)
    assert (tmp_path / "two.txt").read_bytes() == PARTS[0] + PARTS[2]
