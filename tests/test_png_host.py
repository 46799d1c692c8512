"""CPU: the PNG plan's verdicts (csrc/png.hip lmkd_png_plan), the device routines run on the host (lmkd_png_decode_host, csrc/png_core.h)
against PIL's convert("RGB") (tests/golden/png/fixtures.npz, tools/gen_png_golden.py; a seeded matrix of PIL-written files; a corruption
matrix), decode.ImagePlan over both formats, and the loaders' frame lists (train.jpeg_frame_index, pretrain.video_frames)."""
import io
import os
import random
import struct
import sys
import zipfile
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _png_util as U  # noqa: E402


def _verdict(data):
    from litemkd_amd import decode
    return decode.PngPlan([data], pin=False, fallback=False).verdicts()[0]


def _patch_ihdr(data, **kw):
    ch = U.chunks(data)
    f = dict(zip(("w", "h", "depth", "ctype", "comp", "filt", "lace"), struct.unpack(">IIBBBBB", ch[0][1])))
    f.update(kw)
    ch[0][1] = struct.pack(">IIBBBBB", f["w"], f["h"], f["depth"], f["ctype"], f["comp"], f["filt"], f["lace"])
    return U.join(ch)


def _patch_zlib_header(data, cmf, flg):
    z = U.stream_of(data)
    return U.with_stream(data, bytes([cmf, flg]) + z[2:])


def test_plan_verdicts():
    from litemkd_amd import decode
    base = U.fixture("53x37_t2_mix")[1]
    pal = U.fixture("53x37_t3_trns")[1]
    anc = U.fixture("53x37_t2_ancillary")[1]
    assert _verdict(base) == (decode.SUPPORTED, "supported")
    assert _verdict(pal) == (decode.SUPPORTED, "supported") and _verdict(anc) == (decode.SUPPORTED, "supported")
    # unsupported: the fallback fixtures, APNG, a size above 4096
    un = decode.UNSUPPORTED
    assert _verdict(U.fixture("17x9_interlaced")[1]) == (un, "Adam7 interlace")
    assert _verdict(U.fixture("17x9_gray16")[1]) == (un, "bit depth other than 8")
    assert _verdict(U.fixture("17x9_palette4")[1]) == (un, "bit depth other than 8")
    assert _verdict(U.fixture("17x9_gray_alpha")[1]) == (un, "gray + alpha")
    ch = U.chunks(base)
    assert _verdict(U.join(ch[:1] + [[b"acTL", struct.pack(">II", 1, 0)]] + ch[1:])) == (un, "APNG")
    assert _verdict(_patch_ihdr(base, w=5000)) == (un, "size above 4096")
    assert _verdict(_patch_ihdr(base, w=65535, h=2048)) == (un, "size above 4096")
    # malformed
    bad = decode.MALFORMED
    assert _verdict(b"\x89PNG\r\n\x1a\x0b" + base[8:]) == (bad, "bad signature")
    assert _verdict(base[:5]) == (bad, "bad signature")
    ch = U.chunks(anc)
    assert ch[1][0] == b"gAMA"
    assert _verdict(U.join([ch[1], ch[0]] + ch[2:])) == (bad, "IHDR is not the first chunk")
    assert _verdict(_patch_ihdr(base, w=0)) == (bad, "bad IHDR")
    assert _verdict(_patch_ihdr(base, h=0)) == (bad, "bad IHDR")
    assert _verdict(_patch_ihdr(base, comp=1)) == (bad, "bad IHDR")
    assert _verdict(_patch_ihdr(base, filt=1)) == (bad, "bad IHDR")
    assert _verdict(_patch_ihdr(base, depth=3)) == (bad, "bad IHDR")
    # a size no frame has is damage, not a job for the fallback: it never reaches shapes() or the output size
    huge = "size above 65535 or more than 2^27 pixels"
    assert _verdict(_patch_ihdr(base, w=65536)) == (bad, huge) and _verdict(_patch_ihdr(base, h=0x7FFFFFFF)) == (bad, huge)
    assert _verdict(_patch_ihdr(base, w=65535, h=2049)) == (bad, huge)
    plan = decode.PngPlan([_patch_ihdr(base, w=0x7FFFFFFF, h=0x7FFFFFFF), base], pin=False, fallback=False)
    assert plan.shapes() == [(0, 0), (37, 53)] and int(plan.totals[2]) == 37 * 53 * 3
    idat = base.index(b"IDAT")
    assert _verdict(base[:idat + 40]) == (bad, "truncated chunk")            # cut inside the IDAT payload
    assert _verdict(base[:-12]) == (bad, "truncated chunk")                  # no IEND
    assert _verdict(base[:idat - 2]) == (bad, "truncated chunk")             # cut inside a chunk's length field
    for data in (base, pal):
        for i, (t, _) in enumerate(U.chunks(data)):
            v = _verdict(U.join(U.chunks(data), bad_crc=i))
            assert v == ((bad, "CRC mismatch") if t in (b"IHDR", b"PLTE", b"IDAT", b"IEND") else (decode.SUPPORTED, "supported")), t
    assert _verdict(U.join([c for c in U.chunks(pal) if c[0] != b"PLTE"])) == (bad, "palette image without PLTE")
    assert _verdict(U.join([c for c in U.chunks(base) if c[0] != b"IDAT"])) == (bad, "no IDAT")
    z = U.stream_of(base)
    assert (z[0], z[1]) == (0x78, 0x9C)
    assert _verdict(_patch_zlib_header(base, 0x77, 0x9C + (31 - (0x779C % 31)) % 31)) == (bad, "bad zlib header")      # CM = 7
    assert _verdict(_patch_zlib_header(base, 0x88, 0x1C)) == (bad, "bad zlib header") and 0x881C % 31 == 0           # CINFO = 8
    assert _verdict(_patch_zlib_header(base, 0x78, 0xBB)) == (bad, "bad zlib header") and 0x78BB % 31 == 0           # FDICT
    assert _verdict(_patch_zlib_header(base, 0x78, 0x9D)) == (bad, "bad zlib header")                                 # FCHECK
    assert _verdict(_patch_zlib_header(base, 0x78, 0x01)) == (decode.SUPPORTED, "supported")                        # another valid FLG
    assert _verdict(U.with_stream(base, z[:1])) == (bad, "bad zlib header")
    # one batch: the others are unaffected, check() names the malformed one
    plan = decode.PngPlan([base, base[:idat + 40], U.fixture("17x9_gray16")[1], pal], names=["a.png", "b.png", "c.png", "d.png"], pin=False,
                          fallback=False)
    assert [v for v, _ in plan.verdicts()] == [0, 2, 1, 0]
    with pytest.raises(ValueError, match=r"image 1 \(b\.png\) is malformed: truncated chunk"):
        plan.check()
    assert plan.shapes() == [(37, 53), (0, 0), (9, 17), (37, 53)]


def test_host_decode_equals_fixtures():
    from litemkd_amd import decode
    fx = U.fixtures()
    assert len(fx) >= 60 and sum(not f[3] for f in fx) == 4
    imgs, plan, status = decode.png_decode_host([f[1] for f in fx])
    assert not status.any(), [(f[0], int(s)) for f, s in zip(fx, status) if s]
    for (name, _, ref, supported), img, (v, _) in zip(fx, imgs, plan.verdicts()):
        if supported:
            assert img is not None and v == decode.SUPPORTED, name       # decoded by the routines under test, not by PIL
            assert img.shape == ref.shape and np.array_equal(img, ref), (name, int((img != ref).sum()))
        else:
            assert img is None and v == decode.UNSUPPORTED, name
    # the caller's bytes are untouched by the plan's compaction
    assert all(U.pil_rgb(f[1]) is not None for f in fx if "split7" in f[0])


def _pil_file(g, k):
    from PIL import Image
    w, h = int(g.integers(1, 65)), int(g.integers(1, 65))
    mode = ("L", "RGB", "P", "RGBA")[k % 4]
    c = {"L": 1, "RGB": 3, "P": 1, "RGBA": 4}[mode]
    kind = int(g.integers(0, 3))
    if kind == 0:
        a = g.integers(0, 256, (h, w, c))
    elif kind == 1:
        a = (np.add.outer(np.arange(h) * 3, np.arange(w) * 2)[..., None] + 40 * np.arange(c) + g.integers(0, 4, (h, w, c))) % 256
    else:
        a = np.full((h, w, c), int(g.integers(0, 256))) + (g.integers(0, 50, (h, w, c)) == 0) * 99
    a = (a % 256).astype(np.uint8)
    im = Image.fromarray(a[..., 0] if c == 1 else a)
    if mode == "P":
        im = Image.fromarray(a[..., 0])
        im.putpalette(bytes(g.integers(0, 256, 768).astype(np.uint8)))      # 256 entries: written with 8-bit indices
    b = io.BytesIO()
    im.save(b, "PNG", compress_level=int(g.integers(0, 10)), optimize=bool(g.integers(0, 2)))
    return b.getvalue()


def test_host_decode_equals_pil_random():
    """40 files from PIL's encoder: random sizes 1..64, the four modes, its adaptive filter choice, random compression settings"""
    from litemkd_amd import decode
    g = np.random.default_rng(2024)
    files = [_pil_file(g, k) for k in range(40)]
    imgs, plan, status = decode.png_decode_host(files)
    assert not status.any() and all(v == decode.SUPPORTED for v, _ in plan.verdicts()), (status, plan.verdicts())
    for k, (data, img) in enumerate(zip(files, imgs)):
        ref = U.pil_rgb(data)
        assert img is not None and img.shape == ref.shape and np.array_equal(img, ref), k


def test_corruption_matrix():
    """one altered byte at seeded positions of the zlib stream, and cut streams: every case is either flagged (the plan's verdict or a
    status word) or decodes to exactly PIL's pixels; the good image that shares the batch is untouched"""
    from litemkd_amd import decode
    cases = (U.corruption_matrix("53x37_t2_mix", flips=200, seed=0) + U.corruption_matrix("53x37_t2_fixed", flips=60, seed=1)
             + U.corruption_matrix("53x37_t2_level0", flips=60, seed=2) + U.corruption_matrix("53x37_t2_mem1", flips=60, seed=3))
    good = U.fixture("53x37_t6_mix")
    imgs, plan, status = decode.png_decode_host([c[1] for c in cases] + [good[1]])
    assert status[-1] == 0 and np.array_equal(imgs[-1], good[2])
    seen = {}
    unflagged = 0
    for (label, data), img, (v, _), s in zip(cases, imgs, plan.verdicts(), status):
        assert v in (decode.SUPPORTED, decode.MALFORMED), label
        if v == decode.MALFORMED or s:
            seen[int(s) if v == decode.SUPPORTED else "plan"] = seen.get(int(s) if v == decode.SUPPORTED else "plan", 0) + 1
            assert 0 <= s <= 9, (label, s)          # 10 would be the decoder leaving its own window
            continue
        unflagged += 1
        ref = U.pil_rgb(data)
        assert ref is not None and np.array_equal(img, ref), label
    assert all("cut@" not in label or s == 7 for (label, _), s in zip(cases, status)), "a cut stream ends early"
    assert {5, 7, 9} <= set(seen), seen              # bad distance, data ends early, Adler-32 mismatch (the GPU test picks among them)
    assert unflagged < len(cases) // 10, (unflagged, seen)


def _gray_jpeg():
    from PIL import Image
    a = (np.add.outer(np.arange(24) * 5, np.arange(40) * 3) % 256).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=80)
    return b.getvalue()


def _jpeg_fixture(name="53x37_ss2_q75"):
    z = np.load(os.path.join(U.ROOT, "tests", "golden", "jpeg", "fixtures.npz"))
    i = [str(n) for n in z["names"]].index(name)
    return z["jpg_%d" % i].tobytes()


def test_image_plan():
    from litemkd_amd import decode
    jpg, png = _jpeg_fixture(), U.fixture("53x37_t2_mix")[1]
    prog = _jpeg_fixture("53x37_progressive")
    g16 = U.fixture("17x9_gray16")
    names = ["a.jpg", "b.png", "c.jpg", "d.png", "e.png"]
    plan = decode.ImagePlan([jpg, png, prog, U.fixture("53x37_t0_f4")[1], g16[1]], names=names, pin=False, convert_rgb=True)
    assert plan.n == 5 and plan.shapes() == [(37, 53)] * 4 + [(9, 17)]
    assert [v for v, _ in plan.verdicts()] == [0, 0, 1, 0, 1]
    assert plan.verdicts()[2][1] == "progressive" and plan.verdicts()[4][1] == "bit depth other than 8"
    plan.check()
    fb = plan.fallback_images()
    assert sorted(fb) == [2, 4] and np.array_equal(fb[4].numpy(), g16[2]) and np.array_equal(fb[2].numpy(), U.pil_rgb(prog))
    # a status word is reported under the image's position in the batch and its own format
    with pytest.raises(ValueError, match=r"PNG image 3 \(d\.png\) is malformed: Adler-32 mismatch"):
        plan.raise_on_status([0, 0, 0, 9, 0])
    with pytest.raises(ValueError, match=r"JPEG image 0 \(a\.jpg\) is malformed: bad Huffman code"):
        plan.raise_on_status([1, 0, 0, 9, 0])
    # malformed members, named in batch order
    bad = decode.ImagePlan([jpg, png[:60], jpg[:30]], names=names[:3], pin=False)
    assert [v for v, _ in bad.verdicts()] == [0, 2, 2]
    with pytest.raises(ValueError, match=r"PNG image 1 \(b\.png\) is malformed"):
        bad.check()
    with pytest.raises(ValueError, match=r"image 1 \(x\.gif\): neither a JPEG nor a PNG"):
        decode.ImagePlan([jpg, b"GIF89a" + bytes(20)], names=["a.jpg", "x.gif"], pin=False)
    # convert_rgb: non-RGB frames through the fallback, for both formats
    gj = _gray_jpeg()
    conv = decode.ImagePlan([gj, g16[1]], pin=False, convert_rgb=True)
    assert [v for v, _ in conv.verdicts()] == [1, 1] and conv.verdicts()[0][1] == "component count other than 3"
    fb = conv.fallback_images()
    assert np.array_equal(fb[0].numpy(), U.pil_rgb(gj)) and fb[0].shape == (24, 40, 3) and np.array_equal(fb[1].numpy(), g16[2])
    with pytest.raises(ValueError, match="PIL decodes it as mode L, the frame transform takes RGB"):
        decode.ImagePlan([gj], pin=False)
    with pytest.raises(ValueError, match="PNG image 0.*PIL decodes it as mode I;16.*the frame transform takes RGB"):
        decode.ImagePlan([g16[1]], pin=False)
    with pytest.raises(ValueError, match="PIL decodes it as mode L, the frame transform takes RGB"):
        decode.JpegPlan([gj], pin=False)                                        # the default of the JPEG plan is what it was


def _cfg(**kw):
    from litemkd_amd.options import default_args
    d = dict(way=2, shot=1, query_per_class=1, query_per_class_test=1, seq_len=4, img_size=84, device="cpu")
    d.update(kw)
    return default_args(**d)


def _tree(root, ext_of, classes=3, videos=3, frames=6):
    """<root>/Class_<c>/Vid_<v>/<frame><ext> + a file that is no frame; ext_of(c, v, f) -> extension"""
    jpg, png = _jpeg_fixture(), U.fixture("53x37_t2_mix")[1]
    for c in range(classes):
        for v in range(videos):
            d = os.path.join(root, "Class_%d" % c, "Vid_%d" % v)
            os.makedirs(d)
            for f in range(frames):
                e = ext_of(c, v, f)
                with open(os.path.join(d, "%05d%s" % (frames - f, e)), "wb") as fh:
                    fh.write(png if e == ".png" else jpg)
            with open(os.path.join(d, "notes.txt"), "w") as fh:
                fh.write("not a frame")
            with open(os.path.join(d, "thumb.gif"), "wb") as fh:
                fh.write(b"GIF89a")


def _zip(root, path):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as z:
        for dp, _, files in sorted(os.walk(root)):
            for f in sorted(files):
                full = os.path.join(dp, f)
                z.write(full, os.path.join("frames", os.path.relpath(full, root)))


def _jpg_only_index(root):
    """jpeg_frame_index as it was when it kept only *.jpg"""
    index, paths = {}, {}
    for c in sorted(os.listdir(root)):
        index[c] = {}
        for v in sorted(os.listdir(os.path.join(root, c))):
            fr = sorted(f for f in os.listdir(os.path.join(root, c, v)) if f.endswith(".jpg"))
            index[c][v] = fr
            paths[(c, v)] = [os.path.join(root, c, v, f) for f in fr]
    return index, paths


def test_loaders(tmp_path):
    from litemkd_amd import pretrain as PT
    from litemkd_amd.train import JpegFrameEpisodes, jpeg_frame_index
    # a .jpg-only tree: the index and a seeded draw are what they were
    root = str(tmp_path / "jpg")
    _tree(root, lambda c, v, f: ".jpg")
    index, paths = jpeg_frame_index(root)
    assert (index, paths) == _jpg_only_index(root)
    ds = JpegFrameEpisodes(_cfg(), root, device="cpu")
    random.seed(11)
    sup, tgt = ds._draw(True)
    from litemkd_amd import train as T
    keep = T.jpeg_frame_index
    T.jpeg_frame_index = _jpg_only_index
    try:
        old = JpegFrameEpisodes(_cfg(), root, device="cpu")
    finally:
        T.jpeg_frame_index = keep
    random.seed(11)
    sup_old, tgt_old = old._draw(True)
    assert old.splits == ds.splits and (sup, tgt) == (sup_old, tgt_old)
    assert all(v[2][i].endswith(".jpg") for v in sup + tgt for i in v[3])
    random.seed(11)
    sup2, tgt2, plan = ds._plan(True)
    assert [(v[0], v[1], v[3]) for v in sup2 + tgt2] == [(v[0], v[1], v[3]) for v in sup + tgt]
    assert plan.n == 4 * 4 and [v for v, _ in plan.verdicts()] == [0] * 16 and plan.shapes() == [(37, 53)] * 16
    # .png and .jpeg frames beside .jpg, from a directory and from its zip
    root = str(tmp_path / "mixed")
    _tree(root, lambda c, v, f: (".png", ".jpeg", ".jpg")[(c + v + f) % 3] if c else ".png")
    _zip(root, str(tmp_path / "mixed.zip"))
    a, pa = jpeg_frame_index(root)
    b, pb = jpeg_frame_index(str(tmp_path / "mixed.zip"))
    assert a == b and list(a) == ["Class_0", "Class_1", "Class_2"]
    assert a["Class_0"]["Vid_1"] == ["%05d.png" % i for i in range(1, 7)]
    assert a["Class_1"]["Vid_0"] == ["00001.png", "00002.jpg", "00003.jpeg", "00004.png", "00005.jpg", "00006.jpeg"]
    assert pb[("Class_0", "Vid_0")][0] == "frames/Class_0/Vid_0/00001.png"
    for src in (root, str(tmp_path / "mixed.zip")):
        ds = JpegFrameEpisodes(_cfg(), src, device="cpu")
        random.seed(3)
        sup, tgt, plan = ds._plan(True)
        assert plan.n == 16 and [v for v, _ in plan.verdicts()] == [0] * 16
        assert {type(p).__name__ for p, _ in plan.plans} <= {"JpegPlan", "PngPlan"}
    # the teacher side: mixed extensions, sorted by name
    got = PT.video_frames(root, "Class_1/Vid_0")
    assert [os.path.basename(p) for p in got] == a["Class_1"]["Vid_0"]
    os.makedirs(os.path.join(root, "Class_9", "Empty"))
    with pytest.raises(ValueError, match="No frames found"):
        PT.video_frames(root, "Class_9/Empty")
    # a depth-like video of grayscale PNGs is planned with the conversion the reference's reader applies
    d = os.path.join(root, "Depth", "Vid_0")
    os.makedirs(d)
    g8 = U.fixture("53x37_t0_f4")
    g16 = U.fixture("17x9_gray16")
    for f in range(4):
        with open(os.path.join(d, "%05d.png" % f), "wb") as fh:
            fh.write(g16[1] if f == 2 else g8[1])
    names = PT.video_frames(root, "Depth/Vid_0")
    plan = PT.decode.ImagePlan([open(p, "rb").read() for p in names], names=names, pin=False, convert_rgb=True)
    assert [v for v, _ in plan.verdicts()] == [0, 0, 1, 0] and np.array_equal(plan.fallback_images()[2].numpy(), g16[2])


class _Passed:
    """stands for the event decode() records after the upload"""

    def __init__(self, log, tag):
        self.log, self.tag = log, tag

    def synchronize(self):
        self.log.append(self.tag)


def test_ring_keeps_plans_that_are_not_uploaded():
    """A loader's prefetch thread builds plans ahead of the consumer, each in a slot of a PinnedRing.  A slot whose plan has not been
    uploaded has no event to wait for: wrapping the ring must leave that plan's bytes alone.  Mixed episodes take a slot per format."""
    from litemkd_amd import decode
    jpg = _jpeg_fixture()
    pngs = [f[1] for f in U.fixtures() if f[3] and f[0].startswith("53x37")]
    assert len(pngs) >= 8
    ring = decode.PinnedRing(3, pin=False)                        # (pageable buffers: no GPU here; the slots' states are the same)

    def episode(k, ring=ring):                                 # mixed, each with PNG bytes of its own
        return decode.ImagePlan([jpg, pngs[k % len(pngs)], jpg, pngs[(k + 1) % len(pngs)]], ring=ring, pin=ring is not None, fallback=False)

    def content(plan):
        # the images' bytes (compacted, for PNG) and the table / palette pool; between the parts lies padding nobody writes
        return [torch.cat([p.buf[p.data_off:p.data_off + int(p.offsets[-1])], p.buf[p.pool_off:p.nbytes]]) for p, _ in plan.plans]

    plans = [episode(k) for k in range(8)]                     # the ring wraps twice and nothing has been decoded
    for k, plan in enumerate(plans):
        assert all(torch.equal(a, b) for a, b in zip(content(plan), content(episode(k, ring=None)))), k
    bufs = [p.buf.data_ptr() for plan in plans for p, _ in plan.plans]
    assert len(set(bufs)) == len(bufs) == 16                   # no two of them share a buffer
    assert all(p.slot["event"] is decode._NOT_UPLOADED for plan in plans for p, _ in plan.plans)
    # an episode takes one slot of its format's lane: 3 slots serve 3 mixed episodes, as they serve 3 of one format
    assert ring.lane("jpeg").i == ring.lane("png").i == 8 and ring.i == 0
    # once uploaded (decode() puts its event there) or released, a slot is reused: after the event has passed, and in place
    log = []
    for k, plan in enumerate(plans[5:]):
        for p, _ in plan.plans:
            p.slot["event"] = _Passed(log, (k, p._C))
    a = episode(8)
    assert sorted(log) == [(0, "jpeg"), (0, "png")]
    assert [p.buf.data_ptr() for p, _ in a.plans] == [p.buf.data_ptr() for p, _ in plans[5].plans]
    plans[6].release()                                         # not pending, so release() leaves the event alone
    b = episode(9)
    assert sorted(log)[2:] == [(1, "jpeg"), (1, "png")]
    b.release()
    assert all(p.slot["event"] is None for p, _ in b.plans)
    # a single-format batch through the same ring uses its lane alone
    decode.ImagePlan([pngs[0]], ring=ring, pin=True, fallback=False)
    assert ring.lane("png").i == 11 and ring.lane("jpeg").i == 10


def test_scratch_buffers_grow_together():
    """decode._scratch, the one grow-on-demand policy of both formats' device buffers (here on the CPU): when any buffer is too small all
    are reallocated, "in" to max(need, previous) * 5 // 4 rounded up to 1 MiB, every other one to max(need, previous, 64) * 5 // 4 rounded
    up to 256 elements; a request that fits gets the same tensors back."""
    from litemkd_amd import decode
    align = lambda n, a=256: (n + a - 1) // a * a      # noqa: E731
    dtypes = {"in": torch.uint8, "coef": torch.int16, "planes": torch.uint8}
    needs = [{"in": 1000, "coef": 640, "planes": 640},                   # the first request allocates
             {"in": 1000, "coef": 640, "planes": 640},                   # fits
             {"in": 1000, "coef": 2000, "planes": 640},                  # one buffer grows: all are reallocated, "in" a quarter above itself
             {"in": 10, "coef": 10, "planes": 10},                       # shrinks: fits
             {"in": 0, "coef": 0, "planes": 0},                          # nothing asked for: fits
             {"in": (2 << 20) + 1, "coef": 2000, "planes": 640},         # "in" crosses a 1 MiB boundary
             {"in": 3 << 20, "coef": 3328, "planes": 1792}]              # exactly what is there: fits
    keys = [("test", 0, 0), ("test", 0, 1)]
    try:
        have, last, grown = {}, None, []
        for need in needs:
            grow = not have or any(have[k] < n for k, n in need.items())
            if grow:
                have = {k: align(max(n, have.get(k, 0)) * 5 // 4, 1 << 20) if k == "in" else align(max(n, have.get(k, 0), 64) * 5 // 4)
                        for k, n in need.items()}
            sc = decode._scratch(keys[0], {k: (n, dtypes[k]) for k, n in need.items()}, torch.device("cpu"))
            assert {k: t.numel() for k, t in sc.items()} == have, need
            assert all(sc[k].dtype == dtypes[k] and sc[k].device.type == "cpu" for k in need)
            if not grow:
                assert all(sc[k] is last[k] for k in need), need
            last = sc
            grown.append(grow)
        assert grown == [True, False, True, False, False, True, False]
        assert have == {"in": 3 << 20, "coef": 3328, "planes": 1792}          # (the figures the formulas give, by hand)
        # a first request for nothing: no bytes of "in", the floor of 64 elements for the others; another key's buffers are its own
        sc0 = decode._scratch(keys[1], {"in": (0, torch.uint8), "scr": (0, torch.uint8)}, torch.device("cpu"))
        assert {k: t.numel() for k, t in sc0.items()} == {"in": 0, "scr": 256}
        assert decode._scratch(keys[0], {k: (1, dt) for k, dt in dtypes.items()}, torch.device("cpu")) is last
    finally:
        for k in keys:
            decode._SCRATCH.pop(k, None)


def test_split_videos():
    """decode.split_videos cuts decode()'s frames into videos as the loaders did: views of a tensor, stacked frames of a list"""
    from litemkd_amd import decode
    g = torch.Generator().manual_seed(0)
    L = 3
    frames = torch.randint(0, 256, (6, 4, 5, 3), dtype=torch.uint8, generator=g)
    videos = decode.split_videos(frames, L)
    assert len(videos) == 2
    for i, v in enumerate(videos):
        assert torch.equal(v, frames[i * L:(i + 1) * L]) and tuple(v.shape) == (3, 4, 5, 3)
        assert v.data_ptr() == frames[i * L].data_ptr()                      # a view: no copy
    mixed = [torch.randint(0, 256, (4, 5, 3) if i < 3 else (7, 2, 3), dtype=torch.uint8, generator=g) for i in range(6)]
    videos = decode.split_videos(mixed, L)
    assert len(videos) == 2
    for i, v in enumerate(videos):
        assert torch.equal(v, torch.stack(mixed[i * L:(i + 1) * L]))
    assert tuple(videos[0].shape) == (3, 4, 5, 3) and tuple(videos[1].shape) == (3, 7, 2, 3)


def test_chunk_surgery_round_trips():
    """the test utility itself: taking a file's chunks and its zlib stream apart and putting them back gives the same bytes (the
    verdict and corruption tests patch files this way)"""
    f = U.fixture("53x37_t2_mix")
    assert U.join(U.chunks(f[1])) == f[1]
    assert U.with_stream(f[1], U.stream_of(f[1])) == f[1]
    raw = zlib.decompress(U.stream_of(f[1]))
    assert len(raw) == 37 * (53 * 3 + 1)
