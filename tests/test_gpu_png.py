"""GPU: PNG frames decoded on the MI355X (csrc/png.hip through decode.png_decode) bit-identical to PIL's convert("RGB"); streams the host
twin has already shown to stop cleanly stop their own image only; decode.ImagePlan over PNG and JPEG frames into one preallocated tensor;
a depth-like tree of grayscale PNGs through extract --stage modality, and a PNG tree through train.JpegFrameEpisodes and
trainloop.StreamedEpisodes, against the same pipeline fed with PIL's decodes."""
import io
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _png_util as U  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    return torch.device("cuda", 0)


def test_fixtures_one_mixed_batch_bit_exact(dev):
    from litemkd_amd import decode
    fx = [f for f in U.fixtures() if f[3]]
    assert len(fx) >= 56
    before = decode.png_stats()
    frames, status = decode.png_decode([f[1] for f in fx])
    assert isinstance(frames, list) and len(frames) == len(fx)               # mixed sizes: one view per image
    st = status.cpu().tolist()
    assert not any(st), [(f[0], s) for f, s in zip(fx, st) if s]
    first = [f.cpu() for f in frames]
    for (name, _, ref, _), got in zip(fx, first):
        assert tuple(got.shape) == ref.shape and np.array_equal(got.numpy(), ref), (name, int((got.numpy() != ref).sum()))
    after = decode.png_stats()
    assert after["fallback"] - before["fallback"] == 0 and after["gpu"] - before["gpu"] == len(fx) == after["images"] - before["images"]
    frames2, _ = decode.png_decode([f[1] for f in fx])                          # the scratch buffers are reused
    assert all(torch.equal(a, b.cpu()) for a, b in zip(first, frames2))
    # the fallback set goes through PIL (convert_rgb: these are not RGB files) and is counted
    fb = [f for f in U.fixtures() if not f[3]]
    after = decode.png_stats()
    plan = decode.PngPlan([f[1] for f in fb], convert_rgb=True)
    frames, status = plan.decode()
    assert not status.cpu().any()
    for (name, _, ref, _), got in zip(fb, frames):
        assert np.array_equal(got.cpu().numpy(), ref), name
    last = decode.png_stats()
    assert last["fallback"] - after["fallback"] == len(fb) == 4 and last["gpu"] == after["gpu"]
    with pytest.raises(ValueError, match="the frame transform takes RGB"):
        decode.png_decode([fb[1][1]])


def test_altered_streams_stop_their_own_image(dev):
    """three streams of the host corruption matrix that the host twin stopped with 'distance too far back', 'data ends early' and
    'Adler-32 mismatch', between good images"""
    from litemkd_amd import decode
    cases = U.corruption_matrix("53x37_t2_mix", flips=200, seed=0)
    _, _, hs = decode.png_decode_host([c[1] for c in cases])
    pick = {}
    for (label, data), s in zip(cases, hs.tolist()):
        if s not in pick and (s == 7 if "cut@" in label else s in (5, 9)):
            pick[s] = (label, data)
    assert sorted(pick) == [5, 7, 9], sorted(pick)
    good = [U.fixture(n) for n in ("53x37_t6_mix", "53x37_t3_trns", "321x239_t2_mix")]
    blobs = [good[0][1], pick[5][1], good[1][1], pick[7][1], pick[9][1], good[2][1]]
    names = ["g0.png", "far.png", "g1.png", "cut.png", "adler.png", "g2.png"]
    frames, status = decode.png_decode(blobs, check=False)
    assert status.cpu().tolist() == [0, 5, 0, 7, 9, 0]
    for k, g in zip((0, 2, 5), good):
        assert np.array_equal(frames[k].cpu().numpy(), g[2]), g[0]
    with pytest.raises(ValueError, match=r"PNG image 1 \(far\.png\) is malformed: distance too far back"):
        decode.png_decode(blobs, names=names)
    with pytest.raises(ValueError, match=r"image 0 .*malformed: truncated chunk"):
        decode.png_decode([good[0][1][:90]])


def _jpeg_fixtures():
    z = np.load(os.path.join(U.ROOT, "tests", "golden", "jpeg", "fixtures.npz"))
    return [(str(n), z["jpg_%d" % i].tobytes(), (np.cumsum(z["rgbd_%d" % i].astype(np.int64), axis=1) % 256).astype(np.uint8))
            for i, n in enumerate(z["names"])]


def test_image_plan_into_one_tensor(dev):
    from litemkd_amd import decode
    png = [f for f in U.fixtures() if f[0].startswith("53x37") and f[3]]
    jpg = [f for f in _jpeg_fixtures() if f[0].startswith("53x37") and "progressive" not in f[0]]
    assert len(png) >= 30 and len(jpg) >= 12
    # all PNG: straight into the caller's tensor
    out = torch.empty((len(png), 37, 53, 3), dtype=torch.uint8, device=dev)
    plan = decode.ImagePlan([f[1] for f in png], names=[f[0] for f in png])
    assert plan.shapes() == [(37, 53)] * len(png)
    got, status = plan.decode(out=out, check=False)
    assert got is out and not status.cpu().any()
    alone, _ = decode.png_decode([f[1] for f in png])
    assert torch.equal(out, alone) and all(np.array_equal(out[i].cpu().numpy(), f[2]) for i, f in enumerate(png))
    # JPEG and PNG interleaved
    mixed, ref = [], []
    for i in range(2 * len(jpg)):
        f = (jpg if i % 2 == 0 else png)[i // 2]
        mixed.append(f[1])
        ref.append(f[2])
    out = torch.full((len(mixed), 37, 53, 3), 7, dtype=torch.uint8, device=dev)
    plan = decode.ImagePlan(mixed)
    got, status = plan.decode(out=out, check=True)
    assert got is out and status.shape == (len(mixed),) and not status.cpu().any()
    ja, _ = decode.jpeg_decode(mixed[0::2])
    pa, _ = decode.png_decode(mixed[1::2])
    assert torch.equal(out[0::2], ja) and torch.equal(out[1::2], pa)
    assert all(np.array_equal(out[i].cpu().numpy(), r) for i, r in enumerate(ref))
    # mixed sizes and formats without `out`: a list of views in batch order
    big = U.fixture("321x239_t0_mix")
    frames, _ = decode.image_decode([jpg[0][1], big[1], png[0][1]])
    assert [tuple(f.shape) for f in frames] == [(37, 53, 3), (239, 321, 3), (37, 53, 3)]
    assert np.array_equal(frames[1].cpu().numpy(), big[2]) and np.array_equal(frames[0].cpu().numpy(), jpg[0][2])
    # a bad stream inside a mixed batch is reported under its position in the batch
    bad = U.with_stream(png[0][1], U.stream_of(png[0][1])[:200])
    with pytest.raises(ValueError, match=r"PNG image 1 \(b\) is malformed: data ends early"):
        decode.image_decode([jpg[0][1], bad, png[1][1]], names=["a", "b", "c"])


def test_mixed_episodes_staged_past_the_ring(dev):
    """a loader's prefetch thread stages episodes ahead of the consumer in a PinnedRing: more mixed episodes than the ring has slots,
    none decoded before all are built, each then decodes to its own frames; afterwards the slots are reused in place"""
    from litemkd_amd import decode
    png = [f for f in U.fixtures() if f[0].startswith("53x37") and f[3]]
    jpg = [f for f in _jpeg_fixtures() if f[0].startswith("53x37") and "progressive" not in f[0]]
    ring = decode.PinnedRing(2)

    def files(k):
        return [jpg[k % len(jpg)], png[k % len(png)], png[(k + 7) % len(png)], jpg[(k + 3) % len(jpg)]]

    staged = [decode.ImagePlan([f[1] for f in files(k)], ring=ring) for k in range(5)]
    assert all(p.buf.is_pinned() for plan in staged for p, _ in plan.plans)
    for k, plan in enumerate(staged):
        out = torch.empty((4, 37, 53, 3), dtype=torch.uint8, device=dev)
        _, status = plan.decode(out=out, check=True)
        assert all(np.array_equal(out[i].cpu().numpy(), f[2]) for i, f in enumerate(files(k))), k
    held = {p.buf.data_ptr() for plan in staged[3:] for p, _ in plan.plans}              # the ring's four buffers now
    again = [decode.ImagePlan([f[1] for f in files(k)], ring=ring) for k in (5, 6)]         # waits for the uploads, allocates nothing
    assert {p.buf.data_ptr() for plan in again for p, _ in plan.plans} == held
    for k, plan in zip((5, 6), again):
        frames, _ = plan.decode()
        assert all(np.array_equal(frames[i].cpu().numpy(), f[2]) for i, f in enumerate(files(k))), k


def _depth_frame(c, v, f, h=48, w=64):
    y, x = np.mgrid[0:h, 0:w]
    return ((x * 3 + y * 2 + 37 * c + 11 * v + 5 * f) % 256).astype(np.uint8)


def test_depth_tree_through_extract(dev, tmp_path):
    """2 classes x 2 videos x 8 single-channel PNG frames of 64 x 48 (one of them 16-bit: the PIL fallback with the conversion) through
    extract --stage modality, against the same model fed with PIL's convert("RGB") of the same files"""
    from PIL import Image
    from litemkd_amd import extract as E
    from litemkd_amd import decode
    from litemkd_amd import pretrain as PT
    depth, lists = tmp_path / "depth", tmp_path / "lists"
    lists.mkdir()
    entries = []
    for c in range(2):
        for v in range(2):
            d = depth / ("Cls%d" % c) / ("vid%d" % v)
            d.mkdir(parents=True)
            entries.append("Cls%d/vid%d" % (c, v))
            for f in range(8):
                a = _depth_frame(c, v, f)
                im = Image.fromarray(a.astype(np.uint16) * 257) if (c, v, f) == (1, 0, 3) else Image.fromarray(a)
                im.save(str(d / ("depth_%05d.png" % f)), "PNG")
    (lists / "testlist03.txt").write_text("".join(e + "\n" for e in entries))
    ck = str(tmp_path / "ck.pt")
    flags = ["--stage", "modality", "--path", str(depth), "--traintestlist", str(lists), "--mode", "test", "--modality", "depth",
             "--checkpoint_dir", ck, "--seq_len", "8", "--img_size", "64", "--videos_per_call", "4", "--num_classes", "5"]
    parser = E.build_parser()
    args = E.args_check(parser, parser.parse_args(flags + ["--out", str(tmp_path / "ref")]))
    torch.manual_seed(7)
    torch.save({"model_state_dict": {k: v.detach().cpu() for k, v in PT.build_model(args, dev).state_dict().items()}}, ck)
    before = decode.png_stats()
    rec = E.main(flags + ["--out", str(tmp_path / "feats")])
    after = decode.png_stats()
    assert (rec["written"], rec["skipped"], rec["model_calls"]) == (4, 0, 1)
    assert after["images"] - before["images"] == 32 and after["fallback"] - before["fallback"] == 1
    model = E.build_modality_model(args, dev)
    tf = PT.frame_transform(64, dev)

    def load_batch(batch):
        videos = []
        for e in batch:
            paths = PT.video_frames(str(depth), e)
            videos.append(torch.from_numpy(np.stack([np.array(Image.open(paths[i]).convert("RGB")) for i in PT.frame_indices(len(paths), 8)])).to(dev))
        return tf(videos, train=False)
    E.extract_modality(model, args, dev, load_batch=load_batch)
    for e in entries:
        a = np.load(str(tmp_path / "feats" / "depth" / e / "feature.npy"))
        b = np.load(str(tmp_path / "ref" / "depth" / e / "feature.npy"))
        assert a.shape == (8, 2048) and np.isfinite(a).all() and a.std() > 0 and np.array_equal(a, b), e


def _rgb_frame(c, v, f, h=48, w=64):
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * 2 + 40 * c + 3 * f) % 256, (y * 3 + 25 * v) % 256, (x + y + 60 * c + f) % 256], -1)
    return (a + np.random.default_rng(100 * c + 10 * v + f).integers(0, 6, a.shape)).clip(0, 255).astype(np.uint8)


def _equal_dicts(a, b):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k].cpu(), b[k].cpu()), k


def test_png_tree_gives_the_episodes_of_its_decoded_frames(dev, tmp_path):
    """a tree of PNG frames (one class holds .jpg frames too) through JpegFrameEpisodes, directly and through StreamedEpisodes, against
    ClipDirectoryEpisodes over the .npy tree of PIL's decodes"""
    from PIL import Image
    from litemkd_amd import trainloop as TL
    from litemkd_amd.options import default_args
    from litemkd_amd.train import ClipDirectoryEpisodes, JpegFrameEpisodes
    rgb, npy, feat = tmp_path / "rgb", tmp_path / "npy", tmp_path / "feat"
    for c in range(5):
        for v in range(2):
            name = "V%d_c%d" % (v, c)
            d = rgb / ("Cls%d" % c) / name
            d.mkdir(parents=True)
            dec = []
            for f in range(9 + v):
                b = io.BytesIO()
                jpeg = c == 0 and f % 2 == 1
                Image.fromarray(_rgb_frame(c, v, f)).save(b, "JPEG" if jpeg else "PNG", **({"quality": 80} if jpeg else {}))
                (d / ("img_%05d.%s" % (f + 1, "jpg" if jpeg else "png"))).write_bytes(b.getvalue())
                dec.append(np.array(Image.open(io.BytesIO(b.getvalue()))))
            (npy / ("Cls%d" % c)).mkdir(parents=True, exist_ok=True)
            np.save(npy / ("Cls%d" % c) / (name + ".npy"), np.stack(dec))
            fe = np.random.default_rng(100 * c + v).standard_normal((8, 2048)).astype(np.float32)
            np.save(npy / ("Cls%d" % c) / (name + ".feature.npy"), fe)
            (feat / ("Cls%d" % c) / name).mkdir(parents=True)
            np.save(feat / ("Cls%d" % c) / name / "feature.npy", fe)
    cfg = default_args(shot=1, query_per_class=1, query_per_class_test=1, img_size=84, trans_dropout=0.1, device=dev)
    for train in (True, False):
        a = ClipDirectoryEpisodes(cfg, str(npy), device=dev, train=train)
        b = JpegFrameEpisodes(cfg, str(rgb), teacher_path=str(feat), device=dev, train=train)
        for seed in (1, 2):
            random.seed(seed)
            ea = a.episode()
            random.seed(seed)
            eb = b.episode()
            _equal_dicts(ea, eb)

    def first(src):
        random.seed(5)
        loader = TL.StreamedEpisodes(src, cfg, dev)
        try:
            for td in loader:
                torch.cuda.synchronize()
                return {k: v.clone() for k, v in td.items() if torch.is_tensor(v)}
        finally:
            loader.close()
    fa = first(ClipDirectoryEpisodes(cfg, str(npy), device=dev, length=2))
    fb = first(JpegFrameEpisodes(cfg, str(rgb), teacher_path=str(feat), device=dev, length=2))
    _equal_dicts(fa, fb)
