"""Shared by tests/test_jpeg_host.py and tests/test_gpu_jpeg.py: the JPEG fixtures (tests/golden/jpeg/fixtures.npz,
tools/gen_jpeg_golden.py), segment surgery, the seeded corruption matrix of one fixture's scan, and PIL's decode with libjpeg's C IDCT.

    python tests/_jpeg_util.py DIR      writes every damaged stream of MATRIX (+ the renumbered-RST and the planted-EOI case) as
                                        DIR/<n>.jpg: the input of tools/jpeg_host_check.cpp --asis"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "jpeg", "fixtures.npz")
_CACHE = {}

# the host corruption matrix: (fixture, flips, seed), 5 cuts each
MATRIX = (("53x37_ss2_q75", 300, 0), ("53x37_ss0_q95", 200, 1), ("53x37_ss1_restart_marker_blocks", 200, 2),
          ("53x37_ss2_restart_marker_rows", 200, 3), ("17x9_ss1_q75_opt", 150, 4), ("320x240_ss2_q75", 300, 5),
          ("321x239_ss1_q90_rows", 300, 6))
CUTS = 5


def fixtures():
    """-> [(name, JPEG bytes, PIL's uint8 [H, W, 3] decode)], loaded once"""
    if "fx" not in _CACHE:
        z = np.load(FIXTURES)
        _CACHE["fx"] = [(str(n), z["jpg_%d" % i].tobytes(), (np.cumsum(z["rgbd_%d" % i].astype(np.int64), axis=1) % 256).astype(np.uint8))
                        for i, n in enumerate(z["names"])]
    return _CACHE["fx"]


def fixture(name):
    return [f for f in fixtures() if f[0] == name][0]


def segments(data):
    """a JPEG file -> [(marker, payload)] up to and including SOS, then ("scan", rest of the file)"""
    out, pos = [], 2
    while True:
        m = data[pos + 1]
        L = (data[pos + 2] << 8) | data[pos + 3]
        out.append((m, bytearray(data[pos + 4:pos + 2 + L])))
        pos += 2 + L
        if m == 0xDA:
            out.append(("scan", bytearray(data[pos:])))
            return out


def join(segs):
    b = bytearray(b"\xff\xd8")
    for m, p in segs:
        if m == "scan":
            b += p
        else:
            b += bytes([0xFF, m, (len(p) + 2) >> 8, (len(p) + 2) & 255]) + p
    return bytes(b)


def scan_range(data):
    """-> (scan_begin, eoi): the entropy-coded bytes of a single-scan file are data[scan_begin:eoi], data[eoi:] is FF D9"""
    begin = len(data) - len(segments(data)[-1][1])
    assert data[-2:] == b"\xff\xd9"
    return begin, len(data) - 2


def corruption_matrix(name, flips=200, seed=0, cuts=CUTS):
    """-> [(label, file)]: one byte of the scan of fixture `name` altered at each of `flips` seeded positions of [scan_begin, EOI) (a
    seeded non-zero XOR mask), and the scan cut at `cuts` seeded lengths with FF D9 appended.  Labels: '<name> flip@<offset into the
    scan>', '<name> cut@<bytes of the scan kept>'"""
    data = fixture(name)[1]
    begin, eoi = scan_range(data)
    n = eoi - begin
    g = np.random.default_rng(seed)
    out = []
    for pos in sorted(int(p) for p in g.choice(n, size=min(flips, n), replace=False)):
        b = bytearray(data)
        b[begin + pos] ^= int(g.integers(1, 256))
        out.append(("%s flip@%d" % (name, pos), bytes(b)))
    for k in sorted(int(p) for p in g.choice(np.arange(1, n - 1), size=cuts, replace=False)):
        out.append(("%s cut@%d" % (name, k), data[:begin + k] + b"\xff\xd9"))
    return out


def offset_of(label):
    return int(label.rsplit("@", 1)[1])


def full_matrix():
    """every case of MATRIX, in order -> [(label, file)]; built once"""
    if "matrix" not in _CACHE:
        _CACHE["matrix"] = [c for name, flips, seed in MATRIX for c in corruption_matrix(name, flips, seed)]
    return _CACHE["matrix"]


def renumbered_rst(name="53x37_ss0_restart_marker_rows"):
    """the fixture with its first RST0 renumbered to RST1: a restart marker out of sequence"""
    data = fixture(name)[1]
    begin, eoi = scan_range(data)
    at = data.index(b"\xff\xd0", begin, eoi)
    return ("%s rst@%d" % (name, at - begin), data[:at + 1] + b"\xd1" + data[at + 2:])


def planted_eoi(name="53x37_ss2_q75"):
    """the fixture with an EOI written over two bytes half way through its scan: the decoder runs out of data"""
    data = fixture(name)[1]
    mid = (data.index(b"\xff\xda") + len(data)) // 2
    return ("%s eoi@%d" % (name, mid), data[:mid] + b"\xff\xd9" + data[mid + 2:])


_CHILD = r"""
import io, sys
import numpy as np
from PIL import Image
z = np.load(sys.argv[1])
out = {}
for i in range(int(z["n"])):
    try:
        with Image.open(io.BytesIO(z["b%d" % i].tobytes())) as im:
            im.load()
            out["a%d" % i] = np.array(im)
    except Exception as e:
        out["e%d" % i] = np.array(repr(e))
np.savez(sys.argv[2], **out)
"""


def pil_rgb_c_idct(blobs):
    """PIL's decode of every file with libjpeg-turbo's C IDCT (jidctint.c, which the decoder under test follows): one fresh child
    process with JSIMD_FORCENONE=1 in its environment, which imports PIL and numpy only -> [uint8 [H, W, 3] or None where PIL refuses]"""
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "pil_in.npz"), os.path.join(tmp, "pil_out.npz")
        np.savez(src, n=np.array(len(blobs)), **{"b%d" % i: np.frombuffer(b, dtype=np.uint8) for i, b in enumerate(blobs)})
        env = dict(os.environ, JSIMD_FORCENONE="1")
        subprocess.run([sys.executable, "-c", _CHILD, src, dst], env=env, check=True, timeout=300)
        with np.load(dst) as z:
            return [z["a%d" % i] if "a%d" % i in z.files else None for i in range(len(blobs))]


if __name__ == "__main__":
    os.makedirs(sys.argv[1], exist_ok=True)
    for k, (_, data) in enumerate(full_matrix() + [renumbered_rst(), planted_eoi()]):
        with open(os.path.join(sys.argv[1], "%05d.jpg" % k), "wb") as f:
            f.write(data)
