"""Writes tests/golden/png/fixtures.npz: PNG files and PIL's decode of each (PIL.Image.open(f).convert("RGB"), the teacher-side readers'
read_single_image, AuxDataset.py:129-136) - the expected output of decode.png_decode.

    python tools/gen_png_golden.py
    python tools/gen_png_golden.py --dump DIR      (writes the committed fixtures out as DIR/<name>.png)

Most files come from the small PNG writer below, which chooses what an encoder library chooses for itself: the filter of every row, the
deflate level / strategy / memLevel, flush points in mid-stream, and where the stream is cut into IDAT chunks.  PIL's own encoder adds
one file per mode.  The expected pixels are always PIL's decode of the bytes written, never the array the writer was given.

Keys: "names", "supported" (1 = the GPU decodes it, 0 = the PIL fallback set), "png_<i>" (the file's bytes as uint8), "rgbd_<i>" (PIL's
uint8 [H, W, 3], stored as differences along each row mod 256 so that it compresses: load_fixtures())."""
import heapq
import io
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def ihdr(w, h, depth, ctype, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))


def paeth_predict(a, b, c):
    p = a.astype(np.int64) + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(rows, bpp, filters):
    """rows: uint8 [H, stride]; filters: one type per row -> the filtered scanlines with their filter bytes"""
    h, stride = rows.shape
    out = np.zeros((h, stride + 1), dtype=np.uint8)
    z = np.zeros(stride, dtype=np.int64)
    for y in range(h):
        x = rows[y].astype(np.int64)
        b = rows[y - 1].astype(np.int64) if y else z
        a = np.concatenate([z[:bpp], x[:-bpp]]) if stride > bpp else z[:stride].copy()
        c = np.concatenate([z[:bpp], b[:-bpp]]) if stride > bpp else z[:stride].copy()
        f = filters[y]
        pred = (z, a, b, (a + b) // 2, paeth_predict(a, b, c))[f]
        out[y, 0] = f
        out[y, 1:] = (x - pred) % 256
    return out


def paeth_ties(rows, bpp):
    """(pa == pb < pc or pa == pb with all equal, pb == pc < pa) counts over an image: the tie cases the Paeth rows must hold"""
    x = rows.astype(np.int64)
    z = np.zeros_like(x)
    b = np.vstack([z[:1], x[:-1]])
    a = np.hstack([z[:, :bpp], x[:, :-bpp]])
    c = np.hstack([z[:, :bpp], b[:, :-bpp]])
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return int(((pa == pb) & (a != b)).sum()), int(((pb == pc) & (pb < pa) & (b != c)).sum())


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8, flushes=()):
    """flushes: ((byte position, zlib flush mode), ...)"""
    co = zlib.compressobj(level, zlib.DEFLATED, 15, mem, strategy)
    out, last = b"", 0
    for pos, mode in flushes:
        out += co.compress(raw[last:pos]) + co.flush(mode)
        last = pos
    return out + co.compress(raw[last:]) + co.flush()


def split_idat(stream, every=None, empty_in_middle=False):
    if every:
        return b"".join(chunk(b"IDAT", stream[i:i + every]) for i in range(0, len(stream), every))
    if empty_in_middle:
        m = len(stream) // 2
        return chunk(b"IDAT", stream[:m]) + chunk(b"IDAT", b"") + chunk(b"IDAT", stream[m:])
    return chunk(b"IDAT", stream)


def write_png(img, ctype, filters, palette=None, trns=None, extra=b"", every=None, empty_in_middle=False, stream=None, **dk):
    """img: uint8 [H, W] (types 0, 3) or [H, W, C]; filters: a type for all rows or a list"""
    h, w = img.shape[:2]
    bpp = CHANNELS[ctype]
    rows = img.reshape(h, w * bpp)
    if isinstance(filters, int):
        filters = [filters] * h
    raw = filter_rows(rows, bpp, filters).tobytes()
    body = ihdr(w, h, 8, ctype) + extra
    if palette is not None:
        body += chunk(b"PLTE", palette.astype(np.uint8).tobytes())
    if trns is not None:
        body += chunk(b"tRNS", bytes(trns))
    z = stream(raw) if stream else deflate(raw, **dk)
    return SIG + body + split_idat(z, every, empty_in_middle) + chunk(b"IEND", b"")


ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def write_interlaced(img):
    """8-bit RGB, Adam7, filter 0 on every row of every pass"""
    h, w = img.shape[:2]
    raw = b""
    for xs, ys, dx, dy in ADAM7:
        sub = img[ys::dy, xs::dx]
        if sub.size:
            raw += filter_rows(sub.reshape(sub.shape[0], -1), 3, [0] * sub.shape[0]).tobytes()
    return SIG + ihdr(w, h, 8, 2, 1) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")


# ---- a deflate stream whose distance code set is ONE code of length 1 (zlib's own encoder always sends two) ----
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):                 # LSB first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):                 # Huffman codes go MSB first
        self.bits(int(bin(c)[2:].zfill(n)[::-1], 2), n)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def huffman_lengths(freq):
    """{symbol: count} -> {symbol: code length} (plain Huffman; at least two symbols)"""
    heap = [(f, i, (s,)) for i, (s, f) in enumerate(sorted(freq.items()))]
    heapq.heapify(heap)
    depth = {s: 0 for s in freq}
    k = len(heap)
    while len(heap) > 1:
        f1, _, s1 = heapq.heappop(heap)
        f2, _, s2 = heapq.heappop(heap)
        for s in s1 + s2:
            depth[s] += 1
        heapq.heappush(heap, (f1 + f2, k, s1 + s2))
        k += 1
    return depth


def canonical(lengths, n):
    """code lengths [n] -> codes [n]"""
    codes, code = [0] * n, 0
    for l in range(1, 16):
        for s in range(n):
            if lengths[s] == l:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


def lone_distance_stream(raw):
    """zlib stream of `raw`: one dynamic block, run-length matches at distance 1 only, distance code set = {symbol 0: length 1}"""
    tokens, i = [], 0
    while i < len(raw):
        run = 1
        while i + run < len(raw) and raw[i + run] == raw[i] and run < 11:      # lengths 3..10 need no extra bits
            run += 1
        tokens.append(("lit", raw[i]))
        if run - 1 >= 3:
            tokens.append(("len", run - 1))
            i += run
        else:
            i += 1
    freq = {256: 1}
    for kind, v in tokens:
        s = v if kind == "lit" else 257 + v - 3
        freq[s] = freq.get(s, 0) + 1
    assert any(k == "len" for k, _ in tokens), "the image needs runs"
    ll = huffman_lengths(freq)
    assert max(ll.values()) <= 15
    nlen = max(ll) + 1
    lit_len = [ll.get(s, 0) for s in range(nlen)]
    all_len = lit_len + [1]                # ndist = 1: distance symbol 0, length 1 - an incomplete set that inflate accepts
    cl = huffman_lengths({v: all_len.count(v) for v in set(all_len)} if len(set(all_len)) > 1 else {all_len[0]: 1, (all_len[0] + 1) % 16: 1})
    assert max(cl.values()) <= 7
    cl_len = [cl.get(s, 0) for s in range(19)]
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    ncode = max(i for i, s in enumerate(order) if cl_len[s]) + 1
    ncode = max(ncode, 4)
    w = BitWriter()
    w.bits(1, 1)
    w.bits(2, 2)
    w.bits(nlen - 257, 5)
    w.bits(0, 5)
    w.bits(ncode - 4, 4)
    for s in order[:ncode]:
        w.bits(cl_len[s], 3)
    cl_codes = canonical(cl_len, 19)
    for v in all_len:
        w.code(cl_codes[v], cl_len[v])
    codes = canonical(lit_len, nlen)
    for kind, v in tokens:
        s = v if kind == "lit" else 257 + v - 3
        w.code(codes[s], lit_len[s])
        if kind == "len":
            w.code(0, 1)
    w.code(codes[256], lit_len[256])
    z = b"\x78\x9c" + w.done() + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)
    assert zlib.decompress(z) == raw
    return z


# ---- images ----
def noisy(h, w, c, seed, span=24):
    """values in a narrow band around ramps: neighbours differ by little, so every Paeth branch and its ties occur"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = (96 + 4 * ((x // 3 + y // 2) % 9))[..., None] + 7 * np.arange(c)
    a = base + g.integers(0, span, (h, w, c))
    a[h // 2:, : max(1, w // 3)] = 200      # a flat area
    return np.clip(a, 0, 255).astype(np.uint8)


def smooth(h, w, c, seed):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.stack([128 + 100 * np.sin(x / (29 + 3 * k + seed % 5) + y / 43.0) for k in range(c)], -1)
    return (np.round(a / 32) * 32).clip(0, 255).astype(np.uint8)


def image_of(ctype, h, w, seed, big=False):
    """-> (array for write_png, palette or None)"""
    c = CHANNELS[ctype]
    if ctype == 3:
        g = np.random.default_rng(seed)
        pal = g.integers(0, 256, (40, 3)).astype(np.uint8)
        idx = (smooth(h, w, 1, seed)[..., 0] // 32 * 3 + (0 if big else g.integers(0, 3, (h, w)))) % 40
        return idx.astype(np.uint8), pal
    a = smooth(h, w, c, seed) if big else noisy(h, w, c, seed)
    return (a[..., 0] if c == 1 else a), None


def periodic_320x240():
    """rows repeat with a period of 34 rows (34 x 961 = 32 674 bytes with filter 0: matches reach back nearly the whole 32 768 window),
    with flat runs (length-258 matches at distance 1)"""
    g = np.random.default_rng(7)
    tile = (g.integers(0, 8, (34, 320, 3)) * 32 + 5).astype(np.uint8)
    tile[5:9, 20:300] = 77
    tile[20, :] = 9
    return np.concatenate([tile] * 8)[:240]


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def far_match_stream(raw, period=34 * 961):
    """zlib stream of `raw` in one fixed-Huffman block: the first period as literals and distance-1 runs of up to 258, the rest as
    length-258 matches at distance `period` (zlib's own encoder stops 262 bytes short of the window and would not find them)"""
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)

    def lit(v):
        if v < 144:
            w.code(0x30 + v, 8)
        elif v < 256:
            w.code(0x190 + v - 144, 9)
        elif v < 280:
            w.code(v - 256, 7)
        else:
            w.code(0xC0 + v - 280, 8)

    def match(n, d):
        ls = max(i for i, b in enumerate(LEN_BASE) if b <= n)
        lit(257 + ls)
        w.bits(n - LEN_BASE[ls], LEN_EXTRA[ls])
        ds = max(i for i, b in enumerate(DIST_BASE) if b <= d)
        w.code(ds, 5)
        w.bits(d - DIST_BASE[ds], DIST_EXTRA[ds])
    i = 0
    while i < len(raw):
        if i >= period:
            n = min(258, len(raw) - i)
            if n >= 3:
                match(n, period)
                i += n
                continue
        run = 1
        while i + run < min(len(raw), period) and raw[i + run] == raw[i] and run < 259:
            run += 1
        lit(raw[i])
        if run - 1 >= 3:
            match(run - 1, 1)
            i += run
        else:
            i += 1
    lit(256)
    z = b"\x78\x9c" + w.done() + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)
    assert zlib.decompress(z) == raw
    return z


def pil_bytes(img, mode, **kw):
    from PIL import Image
    b = io.BytesIO()
    (Image.fromarray(img) if mode in ("L", "RGB", "RGBA") else Image.fromarray(img, mode)).save(b, "PNG", **kw)
    return b.getvalue()


def pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"))


def matrix():
    """-> [(name, bytes, supported)]"""
    out = []
    seed = 0
    mix = lambda h, s: [int(v) for v in np.random.default_rng(s).integers(0, 5, h)]      # noqa: E731
    for (w, h) in ((1, 1), (1, 2), (3, 1), (17, 9), (53, 37)):
        for ct in (0, 2, 3, 6):
            seed += 1
            img, pal = image_of(ct, h, w, seed)
            out.append(("%dx%d_t%d_mix" % (w, h, ct), write_png(img, ct, mix(h, seed), palette=pal), 1))
    for ct in (0, 2, 6):
        for f in range(5):
            seed += 1
            img, _ = image_of(ct, 37, 53, seed)
            if f == 4:
                t = paeth_ties(img.reshape(37, -1), CHANNELS[ct])
                assert t[0] > 0 and t[1] > 0, ("the Paeth rows need both tie cases", t)
            out.append(("53x37_t%d_f%d" % (ct, f), write_png(img, ct, f), 1))
    img, _ = image_of(2, 37, 53, 900)
    fl = mix(37, 900)
    Z = zlib
    for name, dk in (("level0", dict(level=0)), ("fixed", dict(strategy=Z.Z_FIXED)), ("level1", dict(level=1)), ("level9", dict(level=9)),
                     ("huffman_only", dict(strategy=Z.Z_HUFFMAN_ONLY)), ("rle", dict(strategy=Z.Z_RLE)), ("mem1", dict(mem=1)),
                     ("sync_flush", dict(flushes=((1000, Z.Z_SYNC_FLUSH), (1001, Z.Z_SYNC_FLUSH), (3777, Z.Z_SYNC_FLUSH)))),
                     ("full_flush", dict(flushes=((2222, Z.Z_FULL_FLUSH), (4000, Z.Z_FULL_FLUSH))))):
        out.append(("53x37_t2_" + name, write_png(img, 2, fl, **dk), 1))
    out.append(("53x37_t2_split7", write_png(img, 2, fl, every=7), 1))
    out.append(("53x37_t2_level0_split7", write_png(img, 2, fl, every=7, level=0), 1))
    out.append(("53x37_t2_empty_idat", write_png(img, 2, fl, empty_in_middle=True), 1))
    out.append(("53x37_t2_ancillary", write_png(img, 2, fl, extra=chunk(b"gAMA", struct.pack(">I", 45455)) + chunk(b"tEXt", b"Comment\0frames")), 1))
    img, pal = image_of(3, 37, 53, 901)
    out.append(("53x37_t3_trns", write_png(img, 3, fl, palette=pal, trns=[0, 128, 255, 7]), 1))
    g = np.repeat(np.random.default_rng(5).integers(0, 256, (9, 4)).astype(np.uint8), 5, axis=1)[:, :17]
    out.append(("17x9_t0_lone_distance", write_png(g, 0, 0, stream=lone_distance_stream), 1))
    for ct in (0, 2, 3, 6):
        seed += 1
        img, pal = image_of(ct, 239, 321, seed, big=True)
        out.append(("321x239_t%d_mix" % ct, write_png(img, ct, mix(239, seed), palette=pal, level=9), 1))
    img, _ = image_of(2, 239, 321, 950, big=True)
    out.append(("321x239_t2_level0", write_png(img, 2, mix(239, 950), level=0), 1))
    out.append(("320x240_t2_period34", write_png(periodic_320x240(), 2, 0, stream=far_match_stream), 1))
    # PIL's own encoder, one file per mode (its adaptive filter choice)
    out.append(("17x9_pil_L", pil_bytes(noisy(9, 17, 1, 70)[..., 0], "L"), 1))
    out.append(("53x37_pil_RGB", pil_bytes(noisy(37, 53, 3, 71), "RGB"), 1))
    out.append(("53x37_pil_RGBA", pil_bytes(noisy(37, 53, 4, 72), "RGBA"), 1))
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(noisy(37, 53, 3, 73), "RGB").quantize(40).save(b, "PNG")
    out.append(("53x37_pil_P", b.getvalue(), 1))
    # the fallback set
    out.append(("17x9_interlaced", write_interlaced(noisy(9, 17, 3, 80)), 0))
    out.append(("17x9_gray16", pil_bytes((noisy(9, 17, 1, 81)[..., 0].astype(np.uint16) * 257), "I;16"), 0))
    b = io.BytesIO()
    Image.fromarray(noisy(9, 17, 3, 82), "RGB").quantize(12).save(b, "PNG")
    out.append(("17x9_palette4", b.getvalue(), 0))
    out.append(("17x9_gray_alpha", pil_bytes(noisy(9, 17, 2, 83), "LA"), 0))
    return out


def load_fixtures(path=os.path.join(ROOT, "tests", "golden", "png", "fixtures.npz")):
    """-> [(name, PNG bytes, expected uint8 [H, W, 3], supported)]"""
    z = np.load(path)
    return [(str(n), z["png_%d" % i].tobytes(), (np.cumsum(z["rgbd_%d" % i].astype(np.int64), axis=1) % 256).astype(np.uint8), bool(s))
            for i, (n, s) in enumerate(zip(z["names"], z["supported"]))]


def main(path=os.path.join(ROOT, "tests", "golden", "png", "fixtures.npz")):
    arrays, names, sup = {}, [], []
    for i, (name, data, supported) in enumerate(matrix()):
        names.append(name)
        sup.append(supported)
        arrays["png_%d" % i] = np.frombuffer(data, dtype=np.uint8)
        rgb = pil_rgb(data).astype(np.int64)
        arrays["rgbd_%d" % i] = (np.diff(rgb, axis=1, prepend=0) % 256).astype(np.uint8)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, names=np.array(names), supported=np.array(sup, dtype=np.uint8), **arrays)
    print("%s: %d fixtures, %d bytes" % (path, len(names), os.path.getsize(path)))


def dump(directory):
    """the files of the committed fixtures as <directory>/<name>.png (the input of tools/png_host_check.cpp)"""
    os.makedirs(directory, exist_ok=True)
    for name, data, _, _ in load_fixtures():
        with open(os.path.join(directory, name + ".png"), "wb") as f:
            f.write(data)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--dump"]:
        dump(sys.argv[2])
    else:
        main(*sys.argv[1:])
