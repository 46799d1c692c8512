"""CPU: the JPEG plan's verdicts (csrc/jpeg.hip lmkd_jpeg_plan), the device routines run on the host (lmkd_jpeg_decode_host) against
PIL's decode (tests/golden/jpeg/fixtures.npz, tools/gen_jpeg_golden.py), and the dataset side of train.JpegFrameEpisodes: the index of
a frame directory and of its .zip, split-list filtering (video_reader.py:305-319 _select_fold), teacher features matched by name."""
import io
import os
import random
import zipfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "jpeg", "fixtures.npz")


def _fixtures():
    z = np.load(FIXTURES)
    return [(str(n), z["jpg_%d" % i].tobytes(), (np.cumsum(z["rgbd_%d" % i].astype(np.int64), axis=1) % 256).astype(np.uint8))
            for i, n in enumerate(z["names"])]


def _segments(data):
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


def _join(segs):
    b = bytearray(b"\xff\xd8")
    for m, p in segs:
        if m == "scan":
            b += p
        else:
            b += bytes([0xFF, m, (len(p) + 2) >> 8, (len(p) + 2) & 255]) + p
    return bytes(b)


def _baseline():
    return [f for f in _fixtures() if f[0] == "53x37_ss2_q75"][0][1]


def _verdict(data):
    from litemkd_amd import ops
    return ops.JpegPlan([data], pin=False, fallback=False).verdicts()[0]


def test_plan_verdicts():
    from litemkd_amd import ops
    base = _baseline()
    assert _verdict(base) == (ops.JPEG_SUPPORTED, "supported")
    segs = _segments(base)
    sof = [i for i, s in enumerate(segs) if s[0] == 0xC0][0]
    dqt = [i for i, s in enumerate(segs) if s[0] == 0xDB][0]
    dht = [i for i, s in enumerate(segs) if s[0] == 0xC4][0]
    sos = [i for i, s in enumerate(segs) if s[0] == 0xDA][0]

    def patched(fn):
        s = [(m, bytearray(p)) for m, p in segs]
        fn(s)
        return _join(s)
    U, M = ops.JPEG_UNSUPPORTED, ops.JPEG_MALFORMED
    # unsupported: decoded on the host with PIL
    prog = [f for f in _fixtures() if f[0] == "53x37_progressive"][0][1]
    assert _verdict(prog) == (U, "progressive")
    assert _verdict(patched(lambda s: s.__setitem__(sof, (0xC1, s[sof][1])))) == (U, "frame type other than baseline (SOF0)")
    assert _verdict(patched(lambda s: s.__setitem__(sof, (0xC9, s[sof][1])))) == (U, "arithmetic coding")

    def qt16(s):
        s[dqt][1][0] |= 0x10
    assert _verdict(patched(qt16)) == (U, "16-bit quantisation table")

    def sampling(s):
        s[sof][1][10] = 0x21                      # Cb 2x1
    assert _verdict(patched(sampling)) == (U, "sampling other than 4:4:4 / 4:2:2 / 4:2:0")
    assert _verdict(patched(lambda s: s.insert(1, (0xEE, bytearray(b"Adobe\x00\x64\x00\x00\x00\x00\x00"))))) == (U, "colour space other than YCbCr")

    def gray(s):
        s[sof] = (0xC0, bytearray(s[sof][1][:6] + s[sof][1][6:9]))
        s[sof][1][5] = 1
    assert _verdict(patched(gray)) == (U, "component count other than 3")
    # malformed: raise
    assert _verdict(base[:20]) == (M, "truncated header")
    assert _verdict(b"\x00\x01" + base[2:]) == (M, "no SOI marker")

    def bad_id(s):
        s[dht][1][0] = (s[dht][1][0] & 0xF0) | 5
    assert _verdict(patched(bad_id)) == (M, "bad table id")

    def oversubscribed(s):                         # three 1-bit codes, consistent with the segment length
        tc = s[dht][1][0]
        s[dht] = (0xC4, bytearray([tc] + [3] + [0] * 15 + [0, 1, 2]))
    assert _verdict(patched(oversubscribed)) == (M, "bad Huffman table")

    def too_many(s):
        tc = s[dht][1][0]
        s[dht] = (0xC4, bytearray([tc] + [0] * 15 + [255] + list(range(255))))
    assert _verdict(patched(too_many)) == (M, "bad Huffman table")

    def undefined(s):                              # the scan's Y component names DC table 2, never defined
        s[sos][1][2] = 0x20 | (s[sos][1][2] & 15)
    assert _verdict(patched(undefined)) == (M, "table referenced but never defined")

    def scan_params(s):
        s[sos][1][-2] = 62                         # Se
    assert _verdict(patched(scan_params)) == (M, "bad scan parameters")
    cut = base[:len(base) // 2]
    assert _verdict(cut) == (M, "scan does not end in a marker inside the buffer")
    # one batch: every verdict on its own image, the supported ones packed
    plan = ops.JpegPlan([base, cut, prog, base], pin=False, fallback=False)
    assert [v for v, _ in plan.verdicts()] == [0, 2, 1, 0]
    with pytest.raises(ValueError, match="image 1"):
        plan.check()


def test_host_decode_equals_fixtures():
    from litemkd_amd import ops
    fx = _fixtures()
    imgs, plan, status = ops.jpeg_decode_host([f[1] for f in fx])
    assert not status.any()
    for (name, _, ref), img, (v, why) in zip(fx, imgs, plan.verdicts()):
        if name.endswith("progressive"):
            assert img is None and v == ops.JPEG_UNSUPPORTED, name
            continue
        assert v == ops.JPEG_SUPPORTED, (name, why)
        assert np.array_equal(img, ref), (name, int((img != ref).sum()))


def test_host_decode_equals_pil_random():
    Image = pytest.importorskip("PIL.Image")
    from litemkd_amd import ops
    g = np.random.default_rng(1234)
    blobs = []
    for _ in range(40):
        h, w = int(g.integers(1, 90)), int(g.integers(1, 90))
        a = np.clip(g.normal(128, 60, (h, w, 3)).cumsum(1) / np.arange(1, w + 1)[None, :, None] + g.normal(0, 20, (h, w, 3)), 0, 255)
        kw = {"quality": int(g.integers(5, 100)), "subsampling": int(g.integers(0, 3))}
        if g.random() < 0.3:
            kw["optimize"] = True
        if g.random() < 0.3:
            kw["restart_marker_blocks"] = int(g.integers(1, 6))
        b = io.BytesIO()
        Image.fromarray(a.astype(np.uint8)).save(b, "JPEG", **kw)
        blobs.append(b.getvalue())
    imgs, plan, status = ops.jpeg_decode_host(blobs)
    assert not status.any()
    for b, img in zip(blobs, imgs):
        assert np.array_equal(img, np.array(Image.open(io.BytesIO(b))))


def test_host_decode_flags_altered_scan():
    from litemkd_amd import ops
    base = _baseline()
    sos = base.index(b"\xff\xda")
    mid = (sos + len(base)) // 2
    bad = base[:mid] + b"\xff\xd9" + base[mid + 2:]            # the scan now ends half way: the decoder runs out of data
    imgs, plan, status = ops.jpeg_decode_host([base, bad, base])
    assert list(plan.verdicts()[1]) == [ops.JPEG_SUPPORTED, "supported"]
    assert status[0] == 0 and status[1] != 0 and status[2] == 0
    with pytest.raises(ValueError, match="image 1"):
        plan.raise_on_status(status)


def _tree(root, classes=3, videos=3, frames=9, short=None):
    """<root>/<class>/<video>/<frame>.jpg from the fixtures' bytes (video names with mixed case); `short` videos get 3 frames"""
    jpg = _baseline()
    for c in range(classes):
        for v in range(videos):
            d = os.path.join(root, "Class_%d" % c, "Vid_%d_Of_C%d" % (v, c))
            os.makedirs(d)
            for f in range(3 if (c, v) == short else frames):
                with open(os.path.join(d, "%05d.jpg" % (frames - f)), "wb") as fh:
                    fh.write(jpg)
            with open(os.path.join(d, "notes.txt"), "w") as fh:
                fh.write("not a frame")


def _zip(root, path):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as z:
        for dp, _, files in sorted(os.walk(root)):
            for f in sorted(files):
                full = os.path.join(dp, f)
                z.write(full, os.path.join("frames", os.path.relpath(full, root)))


def _cfg(**kw):
    from litemkd_amd.options import default_args
    d = dict(way=2, shot=1, query_per_class=1, query_per_class_test=1, seq_len=4, img_size=84, device="cpu")
    d.update(kw)
    return default_args(**d)


def test_index_of_directory_and_zip(tmp_path):
    from litemkd_amd.train import JpegFrameEpisodes, jpeg_frame_index
    root = str(tmp_path / "rgb")
    _tree(root, short=(1, 2))
    _zip(root, str(tmp_path / "rgb.zip"))
    a, pa = jpeg_frame_index(root)
    b, pb = jpeg_frame_index(str(tmp_path / "rgb.zip"))
    assert a == b and list(a) == ["Class_0", "Class_1", "Class_2"]
    assert a["Class_0"]["Vid_0_Of_C0"] == ["%05d.jpg" % i for i in range(1, 10)]
    assert pb[("Class_0", "Vid_0_Of_C0")][0] == "frames/Class_0/Vid_0_Of_C0/00001.jpg"
    ds = JpegFrameEpisodes(_cfg(), root, device="cpu")
    dz = JpegFrameEpisodes(_cfg(), str(tmp_path / "rgb.zip"), device="cpu")
    assert ds.splits == dz.splits
    assert "Vid_2_Of_C1" not in ds.splits[True]["Class_1"]                   # fewer than seq_len frames: dropped
    assert ds.splits[True] == ds.splits[False]                               # no split lists: every video in both modes
    p, n = dz._open("Class_2", "Vid_1_Of_C2")
    assert n == 9 and dz._read(p[0]) == ds._read(ds._open("Class_2", "Vid_1_Of_C2")[0][0]) == _baseline()


def test_split_lists(tmp_path):
    from litemkd_amd.train import JpegFrameEpisodes, read_split_lists
    root = str(tmp_path / "rgb")
    _tree(root)
    lists = tmp_path / "lists"
    lists.mkdir()
    # the reference's normalisation: spaces -> '_', lower case, first token, basename without extension
    (lists / "trainlist02.txt").write_text("Class_0/VID_0_of_c0.avi 1\nClass_1/Vid_0_Of_C1.AVI\nclass_2/vid_0_of_c2\n"
                                           "Class_0/Vid_1 Of C0.avi\n")
    (lists / "testlist02.txt").write_text("Class_0/vid_2_of_c0.avi\nClass_1/Vid_2_Of_C1.avi\nClass_2/VID_2_OF_C2.mp4\n")
    got = read_split_lists(str(lists), 2)
    assert got["train"] == {"vid_0_of_c0", "vid_0_of_c1", "vid_0_of_c2", "vid_1_of_c0"}
    assert got["test"] == {"vid_2_of_c0", "vid_2_of_c1", "vid_2_of_c2"}
    ds = JpegFrameEpisodes(_cfg(query_per_class_test=0), root, traintestlist=str(lists), split=2, device="cpu")
    # 'Class_0/VID_0_of_c0.avi 1' keeps the label: the reference's name is 'vid_0_of_c0.avi_1' -> 'vid_0_of_c0' after splitext
    # 'Class_0/Vid_1 Of C0.avi' becomes 'vid_1_of_c0': the folder Vid_1_Of_C0 matches it
    assert ds.splits[True] == {"Class_0": ["Vid_0_Of_C0", "Vid_1_Of_C0"], "Class_1": ["Vid_0_Of_C1"], "Class_2": ["Vid_0_Of_C2"]}
    assert ds.splits[False] == {"Class_0": ["Vid_2_Of_C0"], "Class_1": ["Vid_2_Of_C1"], "Class_2": ["Vid_2_Of_C2"]}
    assert "Vid_1_Of_C1" not in sum(ds.splits[True].values(), []) + sum(ds.splits[False].values(), [])     # in neither list: dropped
    ds.train = False
    random.seed(0)
    sup, tgt = ds._draw(False)
    assert all(v[1].startswith("Vid_2") for v in sup + tgt)


def test_teacher_features_by_name(tmp_path):
    from litemkd_amd.train import JpegFrameEpisodes
    root = str(tmp_path / "rgb")
    _tree(root)
    feat = tmp_path / "feat"
    for c in range(3):
        for v in range(3):
            d = feat / ("Class_%d" % c) / ("Vid_%d_Of_C%d" % (v, c))
            d.mkdir(parents=True)
            np.save(d / "b_feature.npy", np.full((4, 2048), 10 * c + v, dtype=np.float32))
            np.save(d / "z_other.npy", np.zeros((4, 2048), dtype=np.float32))
    ds = JpegFrameEpisodes(_cfg(), root, teacher_path=str(feat), device="cpu")
    for c in range(3):
        for v in range(3):
            f = ds._feature("Class_%d" % c, "Vid_%d_Of_C%d" % (v, c))
            assert f.shape == (4, 2048) and float(f[0, 0]) == 10 * c + v     # the first file in sorted order, by name
    os.remove(feat / "Class_1" / "Vid_1_Of_C1" / "b_feature.npy")
    os.remove(feat / "Class_1" / "Vid_1_Of_C1" / "z_other.npy")
    with pytest.raises(ValueError, match="Class_1/Vid_1_Of_C1"):
        JpegFrameEpisodes(_cfg(), root, teacher_path=str(feat), device="cpu")
