"""CPU: the JPEG plan's verdicts (csrc/jpeg.hip lmkd_jpeg_plan), the device routines run on the host (lmkd_jpeg_decode_host, and
lmkd_jpeg_decode_host_windowed: the entropy kernel's own windowed program, csrc/jpeg_core.h) against PIL's decode
(tests/golden/jpeg/fixtures.npz, tools/gen_jpeg_golden.py; a corruption matrix, tests/_jpeg_util.py), and the dataset side of
train.JpegFrameEpisodes: the index of a frame directory and of its .zip, split-list filtering (video_reader.py:305-319 _select_fold),
teacher features matched by name."""
import io
import os
import random
import sys
import zipfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _jpeg_util as U  # noqa: E402

_fixtures, _segments, _join = U.fixtures, U.segments, U.join


def _baseline():
    return [f for f in _fixtures() if f[0] == "53x37_ss2_q75"][0][1]


def _verdict(data):
    from litemkd_amd import decode
    return decode.JpegPlan([data], pin=False, fallback=False).verdicts()[0]


def test_plan_verdicts():
    from litemkd_amd import decode
    base = _baseline()
    assert _verdict(base) == (decode.SUPPORTED, "supported")
    segs = _segments(base)
    sof = [i for i, s in enumerate(segs) if s[0] == 0xC0][0]
    dqt = [i for i, s in enumerate(segs) if s[0] == 0xDB][0]
    dht = [i for i, s in enumerate(segs) if s[0] == 0xC4][0]
    sos = [i for i, s in enumerate(segs) if s[0] == 0xDA][0]

    def patched(fn):
        s = [(m, bytearray(p)) for m, p in segs]
        fn(s)
        return _join(s)
    U, M = decode.UNSUPPORTED, decode.MALFORMED
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
    plan = decode.JpegPlan([base, cut, prog, base], pin=False, fallback=False)
    assert [v for v, _ in plan.verdicts()] == [0, 2, 1, 0]
    with pytest.raises(ValueError, match="image 1"):
        plan.check()


def test_host_decode_equals_fixtures():
    from litemkd_amd import decode
    fx = _fixtures()
    imgs, plan, status = decode.jpeg_decode_host([f[1] for f in fx])
    assert not status.any()
    for (name, _, ref), img, (v, why) in zip(fx, imgs, plan.verdicts()):
        if name.endswith("progressive"):
            assert img is None and v == decode.UNSUPPORTED, name
            continue
        assert v == decode.SUPPORTED, (name, why)
        assert np.array_equal(img, ref), (name, int((img != ref).sum()))


def test_host_decode_equals_pil_random():
    Image = pytest.importorskip("PIL.Image")
    from litemkd_amd import decode
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
    imgs, plan, status = decode.jpeg_decode_host(blobs)
    assert not status.any()
    for b, img in zip(blobs, imgs):
        assert np.array_equal(img, np.array(Image.open(io.BytesIO(b))))


def test_host_decode_flags_altered_scan():
    from litemkd_amd import decode
    base = _baseline()
    sos = base.index(b"\xff\xda")
    mid = (sos + len(base)) // 2
    bad = base[:mid] + b"\xff\xd9" + base[mid + 2:]            # the scan now ends half way: the decoder runs out of data
    imgs, plan, status = decode.jpeg_decode_host([base, bad, base])
    assert list(plan.verdicts()[1]) == [decode.SUPPORTED, "supported"]
    assert status[0] == 0 and status[1] != 0 and status[2] == 0
    with pytest.raises(ValueError, match="image 1"):
        plan.raise_on_status(status)


def test_corruption_matrix():
    """One altered byte at seeded positions of the scan, and scans cut short with an EOI appended (U.MATRIX: 1 615 flips, 35 cuts),
    through the flat host twin and through the entropy launch's own windowed program run lane by lane.  JPEG has no checksum: a flip
    that leaves the Huffman stream decodable to the right number of blocks is not flagged (13 % to 79 % of the flips of a fixture,
    55 % over the matrix), so an unflagged case has to decode to exactly what libjpeg decodes with its C IDCT (jidctint.c)."""
    from litemkd_amd import decode
    cases = U.full_matrix()
    rst = U.renumbered_rst()
    good = U.fixture("53x37_ss1_q95")
    blobs = [c[1] for c in cases] + [rst[1], good[1]]
    imgs, plan, status = decode.jpeg_decode_host(blobs, fallback=False)
    wimgs, wplan, wstatus = decode.jpeg_decode_host(blobs, windowed=True, fallback=False)
    verdicts = plan.verdicts()
    assert wplan.verdicts() == verdicts
    # the windowed twin: the flat twin's status on every case, its pixels wherever the status is 0
    assert wstatus.tolist() == status.tolist(), [(c[0], int(a), int(b)) for c, a, b in zip(cases, status, wstatus) if a != b][:10]
    for k, (a, b, s) in enumerate(zip(imgs, wimgs, status)):
        if a is not None and s == 0:
            assert np.array_equal(a, b), k
    # the good image is untouched
    assert verdicts[-1] == (decode.SUPPORTED, "supported") and status[-1] == 0
    assert np.array_equal(imgs[-1], good[2]) and np.array_equal(wimgs[-1], good[2])
    # the renumbered RST
    assert verdicts[-2][0] == decode.SUPPORTED and status[-2] == 4, (verdicts[-2], status[-2])
    seen, unflagged, deep = {}, [], 0
    for k, ((label, data), (v, why), s) in enumerate(zip(cases, verdicts, status.tolist())):
        assert v in (decode.SUPPORTED, decode.MALFORMED) or (v, why) == (decode.UNSUPPORTED, "more than one scan"), (label, v, why)
        if label.startswith("321x239") and "flip@" in label and U.offset_of(label) > 8192:
            deep += 1
        if v != decode.SUPPORTED:
            assert s == 0, label
            seen["plan"] = seen.get("plan", 0) + 1
        elif s:
            assert 1 <= s <= 5, (label, s)          # 6 would be the decoder leaving its own window
            seen[s] = seen.get(s, 0) + 1
        else:
            unflagged.append(k)
        if "cut@" in label:
            assert v == decode.SUPPORTED and s == 3, (label, v, s)      # a cut scan ends early
    print("corruption matrix: %d cases, flagged %s, unflagged %d, beyond the first window %d" % (len(cases), seen, len(unflagged), deep))
    assert {1, 2, 3, 5} <= set(seen), seen
    flagged = len(cases) - len(unflagged)
    assert 4 * flagged >= len(cases), (flagged, len(cases))          # not vacuous: at least 25 % flagged ...
    assert len(unflagged) >= 500, len(unflagged)                     # ... and at least 500 compared with libjpeg
    assert deep >= 50, deep                                          # the refill path under damage
    refs = U.pil_rgb_c_idct([cases[k][1] for k in unflagged])
    refused = [cases[k][0] for k, r in zip(unflagged, refs) if r is None]
    assert not refused, refused[:10]
    for k, ref in zip(unflagged, refs):
        assert imgs[k].shape == ref.shape and np.array_equal(imgs[k], ref), (cases[k][0], int((imgs[k] != ref).sum()))


def test_unsupported_image_that_pil_refuses_is_named():
    """a flip that plants a marker inside the scan makes the plan's verdict 'unsupported: more than one scan'; the image goes to PIL,
    and where PIL refuses it too the error is the ValueError every other damaged image raises, naming the image"""
    from PIL import Image
    from litemkd_amd import decode
    import _png_util as PU
    cases = U.corruption_matrix("53x37_ss2_q75", flips=300, seed=0)
    plan = decode.JpegPlan([c[1] for c in cases], pin=False, fallback=False)
    un = [k for k, (v, why) in enumerate(plan.verdicts()) if v == decode.UNSUPPORTED]
    assert len(un) == 3 and all(plan.verdicts()[k][1] == "more than one scan" for k in un)

    def pil_error(data):
        try:
            with Image.open(io.BytesIO(data)) as im:
                im.load()
        except OSError as e:
            return e
        return None
    errors = {k: pil_error(cases[k][1]) for k in un}
    refused = [k for k in un if errors[k] is not None]
    assert refused, "PIL decodes all three"
    good = _baseline()
    for k in un:
        blobs, names = [good, cases[k][1], good], ["a.jpg", "b.jpg", "c.jpg"]
        if errors[k] is None:
            p = decode.JpegPlan(blobs, names=names, pin=False)
            assert sorted(p.fallback) == [1] and p.fallback[1].shape == (37, 53, 3)
            continue
        with pytest.raises(ValueError) as ei:
            decode.JpegPlan(blobs, names=names, pin=False)
        assert "JPEG image 1 (b.jpg) is malformed" in str(ei.value) and str(errors[k]) in str(ei.value), str(ei.value)
        assert isinstance(ei.value.__cause__, OSError) and str(ei.value.__cause__) == str(errors[k])
        with pytest.raises(ValueError, match=r"JPEG image 1 is malformed: PIL refuses it"):
            decode.jpeg_decode_host(blobs)
    # PngPlan shares the fallback: an interlaced file (unsupported) whose stream is cut short
    lace = PU.fixture("17x9_interlaced")[1]
    z = PU.stream_of(lace)
    cut = PU.with_stream(lace, z[:len(z) // 2])
    assert decode.PngPlan([cut], pin=False, fallback=False).verdicts()[0] == (decode.UNSUPPORTED, "Adam7 interlace")
    err = pil_error(cut)
    assert err is not None
    with pytest.raises(ValueError) as ei:
        decode.PngPlan([PU.fixture("53x37_t2_mix")[1], cut], names=["a.png", "b.png"], pin=False)
    assert "PNG image 1 (b.png) is malformed" in str(ei.value) and str(err) in str(ei.value), str(ei.value)
    assert isinstance(ei.value.__cause__, OSError)


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
