"""Writes tests/golden/jpeg/fixtures.npz: JPEG files of synthetic images written with PIL, and PIL's decode of each
(PIL.Image.open(f).load(), the reference's read_single_image, video_reader.py:334-343) - the expected output of decode.jpeg_decode.

    python tools/gen_jpeg_golden.py
    python tools/gen_jpeg_golden.py --dump DIR      (writes the committed fixtures out as DIR/<name>.jpg)

The matrix: 4:4:4 / 4:2:2 / 4:2:0, qualities 50 / 75 / 95 and optimize=True, restart_marker_blocks=3 and restart_marker_rows=1, sizes
320x240, 321x239, 53x37, 17x9 and 1..4 pixels wide or high, and one progressive file (the host fallback).  Keys: "names" (one string
per fixture), "jpg_<i>" (the file's bytes as uint8), "rgbd_<i>" (PIL's uint8 [H, W, 3] decode, stored as differences along each
row mod 256 so that it compresses: rgb = cumsum(rgbd, axis=1) mod 256, load_fixtures())."""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic(h, w, seed, noise=12.0):
    """smooth colour ramps + a few hard edges (+ mild noise on the small images): every DCT band and the chroma upsampling get
    exercised; the large images stay noise-free so the fixtures compress"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.stack([128 + 100 * np.sin(x / (3 + seed % 5) + y / 11.0), 128 + 100 * np.cos(y / (4 + seed % 3) - x / 13.0),
                  255 * ((x // 7 + y // 5) % 2) if noise else 128 + 90 * np.sin((x + 2 * y) / 17.0)], -1)
    a += g.normal(0, noise, a.shape) if noise else 0
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(img, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


def decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        return np.array(im)


def matrix():
    out = []
    seed = 0
    for (w, h) in ((53, 37), (17, 9)):
        for ss in (0, 1, 2):
            for q, extra in ((50, {}), (75, {}), (95, {}), (75, {"optimize": True})):
                seed += 1
                out.append(("%dx%d_ss%d_q%d%s" % (w, h, ss, q, "_opt" if extra else ""), synthetic(h, w, seed), dict(quality=q, subsampling=ss, **extra)))
    for ss in (0, 1, 2):
        for extra in ({"restart_marker_blocks": 3}, {"restart_marker_rows": 1}):
            seed += 1
            out.append(("53x37_ss%d_%s" % (ss, list(extra)[0]), synthetic(37, 53, seed), dict(quality=75, subsampling=ss, **extra)))
    for (w, h) in ((1, 1), (2, 3), (4, 1), (3, 4), (1, 4), (4, 4)):
        for ss in (0, 1, 2):
            seed += 1
            out.append(("%dx%d_ss%d" % (w, h, ss), synthetic(h, w, seed), dict(quality=75, subsampling=ss)))
    out.append(("320x240_ss2_q75", synthetic(240, 320, 101, noise=0), dict(quality=75, subsampling=2)))
    out.append(("321x239_ss1_q90_rows", synthetic(239, 321, 102, noise=0), dict(quality=90, subsampling=1, restart_marker_rows=1)))
    out.append(("53x37_progressive", synthetic(37, 53, 105), dict(quality=75, progressive=True)))
    return out


def load_fixtures(path=os.path.join(ROOT, "tests", "golden", "jpeg", "fixtures.npz")):
    """-> [(name, JPEG bytes, expected uint8 [H, W, 3])]"""
    z = np.load(path)
    return [(str(n), z["jpg_%d" % i].tobytes(), (np.cumsum(z["rgbd_%d" % i].astype(np.int64), axis=1) % 256).astype(np.uint8))
            for i, n in enumerate(z["names"])]


def main(path=os.path.join(ROOT, "tests", "golden", "jpeg", "fixtures.npz")):
    arrays, names = {}, []
    for i, (name, img, kw) in enumerate(matrix()):
        data = encode(img, **kw)
        names.append(name)
        arrays["jpg_%d" % i] = np.frombuffer(data, dtype=np.uint8)
        rgb = decode(data).astype(np.int64)
        arrays["rgbd_%d" % i] = (np.diff(rgb, axis=1, prepend=0) % 256).astype(np.uint8)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, names=np.array(names), **arrays)
    print("%s: %d fixtures, %d bytes" % (path, len(names), os.path.getsize(path)))


def dump(directory):
    """the files of the committed fixtures as <directory>/<name>.jpg (the input of tools/jpeg_host_check.cpp)"""
    os.makedirs(directory, exist_ok=True)
    for name, data, _ in load_fixtures():
        with open(os.path.join(directory, name + ".jpg"), "wb") as f:
            f.write(data)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--dump"]:
        dump(sys.argv[2])
    else:
        main(*sys.argv[1:])
