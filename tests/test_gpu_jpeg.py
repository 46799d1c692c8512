"""GPU: JPEG frames decoded on the MI355X (csrc/jpeg.hip through decode.jpeg_decode) bit-identical to PIL, malformed scans isolated to their
image, train.JpegFrameEpisodes giving the same episodes as ClipDirectoryEpisodes over the same decoded frames (directly and through
trainloop.StreamedEpisodes), the --rgb_path command lines, and no train / test mixing when test() runs in mid-training."""
import io
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _jpeg_util as U  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "jpeg", "fixtures.npz")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    return torch.device("cuda", 0)


def _fixtures():
    z = np.load(FIXTURES)
    return [(str(n), z["jpg_%d" % i].tobytes(), (np.cumsum(z["rgbd_%d" % i].astype(np.int64), axis=1) % 256).astype(np.uint8))
            for i, n in enumerate(z["names"])]


def test_fixtures_one_mixed_batch_bit_exact(dev):
    from litemkd_amd import decode
    fx = _fixtures()
    before = decode.jpeg_stats()
    frames, status = decode.jpeg_decode([f[1] for f in fx])
    assert isinstance(frames, list) and len(frames) == len(fx)          # mixed sizes: one view per image
    assert not status.cpu().any()
    first = [f.cpu() for f in frames]
    for (name, _, ref), got in zip(fx, first):
        assert np.array_equal(got.numpy(), ref), (name, int((got.numpy() != ref).sum()))
    after = decode.jpeg_stats()
    assert after["fallback"] - before["fallback"] == 1 and after["gpu"] - before["gpu"] == len(fx) - 1      # the progressive fixture
    frames2, _ = decode.jpeg_decode([f[1] for f in fx])
    assert all(torch.equal(a, b.cpu()) for a, b in zip(first, frames2))
    # one size: one [F, H, W, 3] tensor, into a caller's buffer too
    same = [f for f in fx if f[0].startswith("53x37_ss2")]
    out = torch.empty((len(same), 37, 53, 3), dtype=torch.uint8, device=dev)
    got, _ = decode.jpeg_decode([f[1] for f in same], out=out)
    assert got is out and all(np.array_equal(out[i].cpu().numpy(), f[2]) for i, f in enumerate(same))


def test_altered_scan_is_malformed_and_isolated(dev):
    """Damaged streams of the host corruption matrix (tests/_jpeg_util.py; every one of them has been through
    tools/jpeg_host_check.cpp) between good images, in one batch: an EOI planted half way, one case per status word 1..5, and four
    321x239 cases damaged beyond the first 8 KiB window (two the host twin flags, two it does not).  The GPU gives the host twin's
    status list, the good images bit for bit, the host twin's pixels for the unflagged damaged ones, and the same bits twice."""
    from litemkd_amd import decode
    good = [U.fixture(n) for n in ("53x37_ss1_q95", "53x37_ss0_restart_marker_rows", "320x240_ss2_q75")]
    cases = U.full_matrix() + [U.renumbered_rst()]
    _, hplan, hs = decode.jpeg_decode_host([c[1] for c in cases], fallback=False)
    pick, deep = {}, {True: [], False: []}
    for (label, data), (v, _), s in zip(cases, hplan.verdicts(), hs.tolist()):
        if v != decode.SUPPORTED:
            continue
        if s not in pick and (s == 3 if "cut@" in label else s == 4 if "rst@" in label else s in (1, 2, 5)):
            pick[s] = (label, data)
        if label.startswith("321x239") and "flip@" in label and U.offset_of(label) > 8192 and len(deep[s != 0]) < 2:
            deep[s != 0].append((label, data))
    assert sorted(pick) == [1, 2, 3, 4, 5] and len(deep[True]) == 2 and len(deep[False]) == 2, (sorted(pick), deep)
    blobs = ([good[0][1], U.planted_eoi()[1]] + [pick[s][1] for s in (1, 2, 3, 4, 5)] + [good[1][1]]
             + [c[1] for c in deep[True] + deep[False]] + [good[2][1]])
    names = ["g0.jpg", "eoi.jpg", "s1.jpg", "s2.jpg", "s3.jpg", "s4.jpg", "s5.jpg", "g1.jpg", "deep_f0.jpg", "deep_f1.jpg", "deep_u0.jpg",
             "deep_u1.jpg", "g2.jpg"]
    himgs, _, hstatus = decode.jpeg_decode_host(blobs, fallback=False)
    assert hstatus.tolist()[2:7] == [1, 2, 3, 4, 5] and hstatus.tolist()[10:] == [0, 0, 0] and all(hstatus.tolist()[8:10])
    frames, status = decode.jpeg_decode(blobs, check=False)
    st = status.cpu().tolist()
    assert st == hstatus.tolist(), (st, hstatus.tolist())
    assert st[0] == 0 and st[1] != 0 and st[7] == 0 and st[12] == 0
    first = [f.cpu().numpy() for f in frames]
    for k, g in zip((0, 7, 12), good):
        assert np.array_equal(first[k], g[2]), g[0]
    for k in (10, 11):                                   # damaged, not flagged: whatever libjpeg makes of them, the host twin's pixels
        assert np.array_equal(first[k], himgs[k]), names[k]
        assert not np.array_equal(first[k], U.fixture("321x239_ss1_q90_rows")[2]), names[k]
    frames2, status2 = decode.jpeg_decode(blobs, check=False)
    # the same bits twice, the stopped images included: the blocks a stopped image never wrote keep what the scratch held, and the two
    # decodes share the scratch of this (device, stream) with nothing in between
    assert status2.cpu().tolist() == st
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(first, frames2)), [n for n, a, b in zip(names, first, frames2)
                                                                                    if not np.array_equal(a, b.cpu().numpy())]
    with pytest.raises(ValueError, match=r"JPEG image 1 \(eoi\.jpg\) is malformed"):
        decode.jpeg_decode(blobs, names=names)
    with pytest.raises(ValueError, match="image 1"):
        decode.jpeg_decode(blobs)
    with pytest.raises(ValueError, match="image 0 .*malformed"):
        decode.jpeg_decode([good[0][1][:40]])


def _frame(value, g, h=100, w=132):
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([value + 30 * np.sin(x / 9.0 + g), value + 30 * np.cos(y / 7.0 - g), value + 20 * np.sin((x + y) / 5.0)], -1)
    return np.clip(a + np.random.default_rng(int(g * 1000)).normal(0, 6, a.shape), 0, 255).astype(np.uint8)


def _datasets(tmp, classes=6, videos=4, frames=10, split_value=True, n_train=2):
    """a JPEG tree (4:2:0, quality 75), the .npy tree of its PIL decodes, teacher features, split lists (the first n_train videos of a
    class train, the others test).
    Train videos are bright (~190), test videos dark (~60): a transformed frame tells its split."""
    from PIL import Image
    rgb, npy, feat, lists = tmp / "rgb", tmp / "npy", tmp / "feat", tmp / "lists"
    lists.mkdir()
    train_l, test_l = [], []
    for c in range(classes):
        for v in range(videos):
            name = "V%d_c%d" % (v, c)
            (train_l if v < n_train else test_l).append("Cls%d/%s.avi 1" % (c, name))
            d = rgb / ("Cls%d" % c) / name
            d.mkdir(parents=True)
            dec = []
            for f in range(frames + (v % 3)):
                b = io.BytesIO()
                Image.fromarray(_frame(190 if (v < n_train or not split_value) else 60, c + v / 10 + f / 100)).save(b, "JPEG", quality=75)
                (d / ("img_%05d.jpg" % (f + 1))).write_bytes(b.getvalue())
                dec.append(np.array(Image.open(io.BytesIO(b.getvalue()))))
            (npy / ("Cls%d" % c)).mkdir(parents=True, exist_ok=True)
            np.save(npy / ("Cls%d" % c) / (name + ".npy"), np.stack(dec))
            fe = np.random.default_rng(100 * c + v).standard_normal((8, 2048)).astype(np.float32)
            np.save(npy / ("Cls%d" % c) / (name + ".feature.npy"), fe)
            (feat / ("Cls%d" % c) / name).mkdir(parents=True)
            np.save(feat / ("Cls%d" % c) / name / "feature.npy", fe)
    (lists / "trainlist03.txt").write_text("\n".join(train_l) + "\n")
    (lists / "testlist03.txt").write_text("\n".join(test_l) + "\n")
    return rgb, npy, feat, lists


def _cfg(dev, **kw):
    from litemkd_amd.options import default_args
    d = dict(shot=1, query_per_class=1, query_per_class_test=1, img_size=84, trans_dropout=0.1, device=dev, learning_rate=1e-2,
             training_iterations=4, tasks_per_batch=2, print_freq=10 ** 9, save_freq=10 ** 9)
    d.update(kw)
    return default_args(**d)


def _equal_dicts(a, b):
    assert set(a) == set(k for k in b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k].cpu(), b[k].cpu()), k


def test_same_episodes_as_npy_loader(dev, tmp_path):
    from litemkd_amd import trainloop as TL
    from litemkd_amd.schedule import Schedule
    from litemkd_amd.train import ClipDirectoryEpisodes, JpegFrameEpisodes
    rgb, npy, feat, _ = _datasets(tmp_path, split_value=False)
    cfg = _cfg(dev)
    for train in (True, False):
        a = ClipDirectoryEpisodes(cfg, str(npy), device=dev, train=train)
        b = JpegFrameEpisodes(cfg, str(rgb), teacher_path=str(feat), device=dev, train=train)
        for seed in (1, 2):
            random.seed(seed)
            ea = a.episode()
            random.seed(seed)
            eb = b.episode()
            _equal_dicts(ea, eb)
    # through StreamedEpisodes, and four training iterations with identical losses
    def run(jpeg):
        sched = Schedule.bench(conv_dtype="fp32h2")
        torch.manual_seed(17)
        with sched.applied():
            student, teacher, _, distiller, acc_fn, _, opt, sch = TL.make(cfg)
            src = (JpegFrameEpisodes(cfg, str(rgb), teacher_path=str(feat), device=dev, length=cfg.training_iterations) if jpeg
                   else ClipDirectoryEpisodes(cfg, str(npy), device=dev, length=cfg.training_iterations))
            random.seed(5)
            loader = TL.StreamedEpisodes(src, cfg, dev)
            first = None
            for td in loader:
                torch.cuda.synchronize()
                first = {k: v.clone() for k, v in td.items() if torch.is_tensor(v)}
                break
            loader.close()
            random.seed(5)
            loader = TL.StreamedEpisodes(src, cfg, dev)
            torch.manual_seed(3)
            losses, _ = TL.train(student, teacher, loader, distiller, opt, sch, acc_fn, cfg, schedule=sched)
            torch.cuda.synchronize()
            loader.close()
        return first, losses
    fa, la = run(False)
    fb, lb = run(True)
    _equal_dicts(fa, fb)
    assert len(la) == 4 and la == lb, (la, lb)


@pytest.fixture
def restore_schedule():
    """train.main installs its schedule process-wide (trainloop.make): put back the one the later tests of the session expect"""
    from litemkd_amd import ops
    from litemkd_amd.schedule import Schedule
    prev = Schedule.current()
    yield
    ops.join_all_streams()
    prev.apply()


def test_train_and_evaluate_command_lines(dev, tmp_path, restore_schedule):
    import glob
    import zipfile
    from litemkd_amd import evaluate as E
    from litemkd_amd import train as T
    rgb, _, feat, lists = _datasets(tmp_path)
    common = ["--shot", "1", "--query_per_class", "1", "--img_size", "84", "--tasks_per_batch", "2", "--training_iterations", "4",
              "--traintestlist", str(lists), "--teacher_path", str(feat), "--test_iters", "100", "--seed", "3"]
    ck = tmp_path / "ckpt"
    losses, _ = T.main(common + ["--rgb_path", str(rgb), "--checkpoint_dir", str(ck)])
    assert len(losses) == 4 and all(np.isfinite(losses))
    zp = tmp_path / "rgb.zip"
    with zipfile.ZipFile(zp, "w", compression=zipfile.ZIP_STORED) as z:
        for f in sorted(rgb.rglob("*.jpg")):
            z.write(f, os.path.join("rgb", os.path.relpath(f, rgb)))
    losses_z, _ = T.main(common + ["--rgb_path", str(zp), "--no_save"])
    assert len(losses_z) == 4 and all(np.isfinite(losses_z))
    path = glob.glob(str(ck / "*.pt"))[0]
    res = E.main(["--test_model", "student", "--test_model_path", path, "--num_test_tasks", "3", "--shot", "1", "--img_size", "84",
                  "--rgb_path", str(rgb), "--traintestlist", str(lists), "--split", "3"])
    r = res[list(res)[0]]
    assert 0 <= r["accuracy"] <= 100 and np.isfinite(r["confidence"])


def test_mid_training_test_uses_only_test_split(dev, tmp_path):
    """test_iters in the middle of a streamed run: every test episode is made of test-split videos (dark frames) with
    query_per_class_test queries, every training episode of train-split videos (bright frames) with query_per_class queries"""
    from litemkd_amd import trainloop as TL
    from litemkd_amd.schedule import Schedule
    from litemkd_amd.train import JpegFrameEpisodes
    rgb, _, feat, lists = _datasets(tmp_path, classes=3, videos=5, n_train=3)
    cfg = _cfg(dev, query_per_class=2, query_per_class_test=1, training_iterations=8, test_iters=[4], num_test_tasks=3, way=3, split=3)
    seen = []
    orig = TL.prepare_task

    def spy(task_dict, device, images_to_device=True):
        x = task_dict["target_set"][0]
        seen.append((torch.is_grad_enabled(), x.shape[0], float(x[..., :3].mean())))
        return orig(task_dict, device, images_to_device)
    sched = Schedule.bench(conv_dtype="fp32h2")
    TL.prepare_task = spy
    try:
        with sched.applied():
            torch.manual_seed(0)
            random.seed(0)
            student, teacher, _, distiller, acc_fn, _, opt, sch = TL.make(cfg)
            src = JpegFrameEpisodes(cfg, str(rgb), str(lists), str(feat), device=dev, length=10 ** 6)
            loader = TL.StreamedEpisodes(src, cfg, dev)
            losses, _ = TL.train(student, teacher, loader, distiller, opt, sch, acc_fn, cfg, schedule=sched)
            torch.cuda.synchronize()
            loader.close()
    finally:
        TL.prepare_task = orig
    L = cfg.seq_len
    train_eps = [s for s in seen if s[0]]
    test_eps = [s for s in seen if not s[0]]
    assert len(losses) == 8 and len(train_eps) == 8 and len(test_eps) == 3
    assert all(n == 3 * 2 * L and m > 0.5 for _, n, m in train_eps), train_eps
    assert all(n == 3 * 1 * L and m < 0.5 for _, n, m in test_eps), test_eps
