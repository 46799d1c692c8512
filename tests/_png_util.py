"""Shared by tests/test_png_host.py and tests/test_gpu_png.py: the PNG fixtures (tests/golden/png/fixtures.npz, tools/gen_png_golden.py),
chunk surgery with the CRC recomputed, and the seeded corruption matrix of one fixture's zlib stream."""
import io
import os
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "png", "fixtures.npz")
SIG = b"\x89PNG\r\n\x1a\n"
_CACHE = {}


def fixtures():
    """-> [(name, PNG bytes, PIL's convert("RGB") uint8 [H, W, 3], supported on the GPU)], loaded once"""
    if "fx" not in _CACHE:
        z = np.load(FIXTURES)
        _CACHE["fx"] = [(str(n), z["png_%d" % i].tobytes(), (np.cumsum(z["rgbd_%d" % i].astype(np.int64), axis=1) % 256).astype(np.uint8), bool(s))
                        for i, (n, s) in enumerate(zip(z["names"], z["supported"]))]
    return _CACHE["fx"]


def fixture(name):
    return [f for f in fixtures() if f[0] == name][0]


def chunks(data):
    """a PNG file -> [[type, payload]]"""
    out, pos = [], 8
    while pos < len(data):
        n = struct.unpack(">I", data[pos:pos + 4])[0]
        out.append([data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]])
        pos += 12 + n
    return out


def join(ch, bad_crc=None):
    """chunks -> file, every CRC recomputed (bad_crc: the index of a chunk whose CRC is written wrong)"""
    b = bytearray(SIG)
    for i, (t, d) in enumerate(ch):
        crc = zlib.crc32(t + d) & 0xFFFFFFFF
        b += struct.pack(">I", len(d)) + t + d + struct.pack(">I", crc ^ (0x10 if i == bad_crc else 0))
    return bytes(b)


def with_stream(data, stream):
    """the file with its (single) IDAT payload replaced"""
    ch = chunks(data)
    k = [i for i, c in enumerate(ch) if c[0] == b"IDAT"]
    assert len(k) == 1
    ch[k[0]][1] = bytes(stream)
    return join(ch)


def stream_of(data):
    return b"".join(d for t, d in chunks(data) if t == b"IDAT")


def corruption_matrix(name, flips=200, seed=0, cuts=5):
    """-> [(label, file)]: one byte of the zlib stream of fixture `name` altered at each of `flips` seeded positions (a seeded non-zero
    XOR mask), and the stream cut at `cuts` seeded lengths; CRCs recomputed"""
    data = fixture(name)[1]
    z = stream_of(data)
    g = np.random.default_rng(seed)
    out = []
    for pos in sorted(int(p) for p in g.choice(len(z), size=min(flips, len(z)), replace=False)):
        b = bytearray(z)
        b[pos] ^= int(g.integers(1, 256))
        out.append(("%s flip@%d" % (name, pos), with_stream(data, b)))
    for n in sorted(int(p) for p in g.choice(np.arange(3, len(z) - 1), size=cuts, replace=False)):
        out.append(("%s cut@%d" % (name, n), with_stream(data, z[:n])))
    return out


def pil_rgb(data):
    """PIL's convert("RGB") of the file, or None where PIL refuses it"""
    from PIL import Image
    try:
        with Image.open(io.BytesIO(data)) as im:
            return np.array(im.convert("RGB"))
    except Exception:
        return None
