"""CPU: the host side of the teacher's pretraining and feature extraction (litemkd_amd.pretrain, litemkd_amd.extract,
teacher.action_recognition, trainloop.MomentumSGD / StepLR, csrc/clipcls.hip's argument checks) against the restatements of
tests/_pretrain_ref.py.  No GPU is touched: the C entry points are called with arguments their checks refuse before any launch."""
import argparse
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pretrain_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"lmkd_global_avgpool_fwd": 8, "lmkd_global_avgpool_bwd": 8, "lmkd_softmax_ce": 10, "lmkd_sgd_momentum_step": 9}
EINVAL = -1


# ---- ABI ----
def test_header_declares_the_entry_points_and_the_library_exports_them():
    import litemkd_amd
    L = litemkd_amd.lib()
    assert L.value("lmkd_abi_version") == 3
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "lmkd.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", litemkd_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name, nargs in ENTRY_POINTS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert len(L.protos[name][1]) == nargs, name
        assert name in exported, name


def test_argument_errors_return_the_code_before_any_launch():
    import litemkd_amd
    lib = litemkd_amd.lib()
    c = lib.cdll
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    null = None
    f32 = ctypes.c_float

    def refused(rc, text):
        assert rc == EINVAL and text in lib.last_error(), (rc, text, lib.last_error())
    for fn in (c.lmkd_global_avgpool_fwd, c.lmkd_global_avgpool_bwd):
        refused(fn(null, p, 8, 7, 7, 64, 1, null), "null pointer")
        refused(fn(p, null, 8, 7, 7, 64, 1, null), "null pointer")
        refused(fn(p, p, 8, 7, 7, 64, 3, null), "8 frames are no multiple of the group of 3")
        refused(fn(p, p, 8, 7, 7, 66, 1, null), "C=66 must be a multiple of 4")
        refused(fn(odd, p, 8, 7, 7, 64, 1, null), "16-byte aligned")
        refused(fn(p, odd, 8, 7, 7, 64, 1, null), "16-byte aligned")
        refused(fn(p, p, 0, 7, 7, 64, 1, null), "empty tensor")
        refused(fn(p, p, 8, 7, 7, 64, 0, null), "empty tensor")
    labels = (ctypes.c_longlong * 3)(0, 5, 2)
    lp = ctypes.cast(labels, ctypes.c_void_p)
    refused(c.lmkd_softmax_ce(p, p, lp, p, null, null, p, 3, 5, null), "label 5 of row 1 outside [0, 5)")
    labels[1] = -1
    refused(c.lmkd_softmax_ce(p, p, lp, p, null, null, p, 3, 5, null), "label -1 of row 1 outside [0, 5)")
    labels[1] = 4
    refused(c.lmkd_softmax_ce(null, p, lp, p, null, null, p, 3, 5, null), "null pointer")      # the labels pass, the null logits do not
    refused(c.lmkd_softmax_ce(p, p, null, p, null, null, null, 3, 5, null), "null pointer")      # the scratch rows are not optional
    refused(c.lmkd_softmax_ce(p, p, null, p, null, null, p, 3, 0, null), "3 rows of 0 classes")
    refused(c.lmkd_softmax_ce(p, p, null, p, null, null, p, 0, 5, null), "0 rows of 5 classes")
    sgd = c.lmkd_sgd_momentum_step
    for args in ((null, p, p, 8), (p, null, p, 8), (p, p, null, 8), (p, p, p, 6), (p, p, p, 0), (odd, p, p, 8), (p, odd, p, 8), (p, p, odd, 8)):
        refused(sgd(args[0], args[1], args[2], f32(0.1), f32(0.9), args[3], 1, 0, null), "lmkd_sgd_momentum_step")
    with pytest.raises(RuntimeError, match="lmkd_sgd_momentum_step"):
        lib.call("lmkd_sgd_momentum_step", null, null, null, f32(0.1), f32(0.9), 8, 1, 0, null)


def test_ops_refuse_host_tensors():
    from litemkd_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.GlobalAvgPoolFn.apply(torch.zeros(2, 2, 2, 8), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.softmax_ce(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="int64"):
        ops.softmax_ce(torch.zeros(2, 5), torch.zeros(2))


# ---- data rules ----
@pytest.mark.parametrize("seq_len", [8, 1])
@pytest.mark.parametrize("n", [1, 5, 8, 9, 17, 300])
def test_frame_indices_follow_the_dataset_in_every_mode(n, seq_len):
    import random
    from litemkd_amd import pretrain as PT
    got = PT.frame_indices(n, seq_len)
    assert len(got) == seq_len and all(0 <= i < n for i in got) and got == sorted(got)
    for train in (True, False):
        random.seed(n)
        assert got == R.get_seq_indices(n, seq_len, train), (n, seq_len, train)
    if n < seq_len:
        assert len(set(got)) == n      # a short video repeats frames and skips none
    with pytest.raises(ValueError):
        PT.frame_indices(0, seq_len)


def test_lists_and_labels_on_a_tree_with_a_space_in_a_class_name(tmp_path):
    from litemkd_amd import pretrain as PT
    rgb, lists = str(tmp_path / "rgb"), str(tmp_path / "lists")
    entries = R.write_jpeg_tree(rgb, lists, classes=("Bowl", "Apply Eye", "Climb"), videos=2, frames=(3, 9), hw=(16, 24))
    train_text = open(os.path.join(lists, "trainlist03.txt")).read()
    assert "Apply Eye/" in train_text
    assert PT.read_video_list(lists, "train", 3) == entries == R.parse_list(train_text)
    labels = PT.class_index(lists)
    assert labels == {"Bowl": 0, "Apply_Eye": 1, "Climb": 2} == R.labels_by_first_appearance(train_text)      # first appearance, not sorted
    frames = PT.video_frames(rgb, entries[2])
    assert [os.path.basename(f) for f in frames] == ["img_%05d.jpg" % i for i in (1, 2, 3)]
    args = PT.build_parser().parse_args(["--path", rgb, "--traintestlist", lists, "--checkpoint_dir", str(tmp_path), "--img_size", "64",
                                         "--batch_size", "4", "--mode", "test"])
    loader = PT.ClipBatches(args, "cpu", shuffle=False)
    assert len(loader) == 2 and loader.train is False and loader.tf.resize == 73
    # a list that names a class trainlist03 does not know is refused when the loader is built, not in the middle of an epoch
    with open(os.path.join(lists, "testlist03.txt"), "a") as f:
        f.write("Unknown/v_x\n")
    with pytest.raises(ValueError, match="Unknown"):
        PT.ClipBatches(args, "cpu")


# ---- command lines ----
PRETRAIN_LINE = ("--path imp_datasets/video_datasets/data/kinetics/rgb_l8 --checkpoint_dir work/kinetics/single/rgb "
                 "--model Action_Recognition_Resnet50 --num_gpus 2 --getitem_name get_video_with_label --modality rgb").split()
EXTRACT_LINE = ("--num_gpus=2 --modality=depth --checkpoint_dir=work/kinetics/single/depth/best_checkpoint.pt "
                "--path imp_datasets/video_datasets/data/kinetics/depth_l8 --mode=train --dataset=kinetics --model Action_Recognition_Resnet50 "
                "--traintestlist=imp_datasets/video_datasets/splits/kineticsTrainTestlist --getitem_name get_video --num_classes 64").split()
FUSION_LINE = ("--checkpoint_dir work/kinetics/trx_fusion/checkpoint15000.pt --model ThreeTRXShiftLoopTime --trans_num 4 --shirt_num 1 "
               "--dataset kinetics --mode test --getitem_name get_multi_fea --base_model TRM "
               "--traintestlist imp_datasets/video_datasets/splits/kineticsTrainTestlist").split()


def test_both_tools_parse_the_reference_command_lines():
    from litemkd_amd import extract as E
    from litemkd_amd import pretrain as PT
    p = PT.build_parser()
    a = PT.args_check(p, p.parse_args(PRETRAIN_LINE))
    assert (a.modality, a.lr_1, a.lr_2, a.num_classes, a.seq_len, a.img_size, a.split, a.mode) == ("rgb", 1e-6, 1e-2, 64, 8, 224, 3, "train")
    assert (a.epochs, a.batch_size, a.resume, a.init_weights, a.num_workers) == (50, 8, False, None, 1)
    assert p.parse_args(PRETRAIN_LINE + ["--resume", "True"]).resume is True and p.parse_args(PRETRAIN_LINE + ["-r"]).resume is True
    assert p.parse_args(PRETRAIN_LINE + ["--resume", "False"]).resume is False
    with pytest.raises(SystemExit):
        PT.args_check(p, p.parse_args(["--path", "x"]))
    q = E.build_parser()
    m = E.args_check(q, q.parse_args(EXTRACT_LINE + ["--out", "feats"]))
    assert (m.stage, m.modality, m.mode, m.videos_per_call, m.augment, m.resume) == ("modality", "depth", "train", 8, False, False)
    f = E.args_check(q, q.parse_args(FUSION_LINE + ["--stage", "fusion", "--feature_save_path", "feats", "--out", "fused"]))
    assert (f.stage, f.shirt_num, f.seq_len) == ("fusion", 1, 8)
    for bad in (EXTRACT_LINE, FUSION_LINE + ["--stage", "fusion", "--out", "fused"], ["--stage", "modality", "--out", "o", "--path", "p"]):
        with pytest.raises(SystemExit):
            E.args_check(q, q.parse_args(bad))


# ---- optimizer groups and their schedule ----
class _TwoPart(nn.Module):
    def __init__(self):
        super().__init__()
        self.convnet = nn.Sequential(nn.Linear(6, 5), nn.Linear(5, 3))
        self.fc = nn.Linear(3, 7)


def test_learning_rates_of_both_groups_follow_steplr_stepped_first():
    from litemkd_amd import pretrain as PT
    model = _TwoPart()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt, s1, s2 = PT.build_optimizer(model, argparse.Namespace(lr_1=1e-6, lr_2=1e-2))
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())      # moving into the flat buffer changes no value
    assert set(opt.groups) == {"convnet", "fc"} and [g["momentum"] for g in opt.groups.values()] == [0.9, 0.9]
    # each group is ONE run of the flat buffer (one launch), every parameter starts on a 16-byte boundary, the runs tile the buffer
    assert opt.groups["convnet"]["runs"] == [(0, 32 + 8 + 16 + 4)] and opt.groups["fc"]["runs"] == [(60, 60 + 24 + 8)] and opt.bucket.numel == 92
    want1, want2 = R.step_lr_sequence(1e-6, 25), R.step_lr_sequence(1e-2, 25)
    for e in range(25):
        s1.step()
        s2.step()
        assert math.isclose(opt.groups["convnet"]["lr"], want1[e], rel_tol=1e-12), (e, opt.groups["convnet"]["lr"], want1[e])
        assert math.isclose(opt.groups["fc"]["lr"], want2[e], rel_tol=1e-12), (e, opt.groups["fc"]["lr"], want2[e])
    assert math.isclose(want1[8], 1e-6) and math.isclose(want1[9], 1e-7, rel_tol=1e-9)      # stepped first: the 10th epoch already trains at a tenth
    st = s1.state()
    s3 = type(s1)(opt, "convnet")
    s3.load_state(json.loads(json.dumps(st)))
    assert s3.n == 25 and math.isclose(opt.groups["convnet"]["lr"], want1[24], rel_tol=1e-12)


def test_optimizer_groups_must_cover_every_parameter_once():
    from litemkd_amd import trainloop as TL
    with pytest.raises(ValueError, match="belongs to 0 groups"):
        TL.MomentumSGD(_TwoPart(), {"convnet": ("convnet.", 1e-3, 0.9)})
    with pytest.raises(ValueError, match="belongs to 2 groups"):
        TL.MomentumSGD(_TwoPart(), {"a": ("convnet.", 1e-3, 0.9), "b": ("convnet.0", 1e-3, 0.9), "fc": ("fc.", 1e-3, 0.9)})
    with pytest.raises(ValueError, match="holds no trainable parameter"):
        TL.MomentumSGD(_TwoPart(), {"convnet": ("convnet.", 1e-3, 0.9), "fc": ("fc.", 1e-3, 0.9), "none": ("head.", 1e-3, 0.9)})
    opt = TL.MomentumSGD(_TwoPart(), {"convnet": ("convnet.", 1e-3, 0.9), "fc": ("fc.", 1e-2, 0.5)})
    opt.buf.copy_(torch.arange(92.0))
    opt.groups["fc"]["steps"] = 3
    s = opt.state("fc")
    assert (s["lr"], s["momentum"], s["steps"]) == (1e-2, 0.5, 3) and torch.equal(s["momentum_buffer"], torch.arange(60.0, 92.0))
    other = TL.MomentumSGD(_TwoPart(), {"convnet": ("convnet.", 1e-3, 0.9), "fc": ("fc.", 1.0, 0.0)})
    other.load_state("fc", s)
    assert other.groups["fc"]["steps"] == 3 and other.groups["fc"]["lr"] == 1e-2 and torch.equal(other.buf[60:], torch.arange(60.0, 92.0))
    assert float(other.buf[:60].abs().max()) == 0.0
    with pytest.raises(ValueError, match="momentum buffer"):
        other.load_state("convnet", s)


# ---- the model's keys ----
def test_torchvision_weights_map_onto_the_sequential_keys(tmp_path):
    from litemkd_amd.teacher.action_recognition import Action_Recognition_Resnet50, map_torchvision_keys
    tv = R.torchvision_resnet50_state()
    assert len(tv) == 320      # torchvision resnet50: 318 trunk entries + fc.weight, fc.bias
    model = Action_Recognition_Resnet50(argparse.Namespace(num_classes=70))
    own = model.state_dict()
    want_keys = {"convnet." + R.sequential_key(k) for k in tv if not k.startswith("fc.")} | {"fc.weight", "fc.bias"}
    assert set(own) == want_keys      # what nn.Sequential(*children[:-1]) + fc hold: strict=True in both directions
    assert tuple(own["fc.weight"].shape) == (70, 2048)
    fc_before = own["fc.weight"].clone()
    path = str(tmp_path / "resnet50.pth")
    torch.save(tv, path)
    model.load_torchvision_resnet50(path)
    now = model.state_dict()
    for k, v in tv.items():
        if k.startswith("fc."):
            continue
        got = now["convnet." + R.sequential_key(k)]
        assert got.shape == v.shape and torch.equal(got.to(v.dtype), v), k
    assert torch.equal(now["fc.weight"], fc_before)      # the ImageNet classifier is dropped
    mapped = map_torchvision_keys(tv)
    model.convnet.load_state_dict(mapped, strict=True)
    with pytest.raises(KeyError, match="stem"):
        map_torchvision_keys({"stem.weight": torch.zeros(1)})
    # and back: a reference-shaped checkpoint of this model loads strictly
    Action_Recognition_Resnet50(argparse.Namespace(num_classes=70)).load_state_dict({k: v.clone() for k, v in now.items()}, strict=True)


# ---- the extract drivers with stand-in models ----
class _FrameModel:
    def __init__(self):
        self.calls = []

    def extract_feature(self, x):
        self.calls.append(int(x.shape[0]))
        return x.reshape(x.shape[0], 1).float().expand(-1, 2048)


def _extract_args(tmp_path, lists, **kw):
    from litemkd_amd import extract as E
    q = E.build_parser()
    flags = ["--stage", "modality", "--path", "unused", "--traintestlist", lists, "--out", str(tmp_path / "feats"), "--init_weights", "unused",
             "--mode", "test", "--seq_len", "4", "--videos_per_call", "4"]
    a = E.args_check(q, q.parse_args(flags))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_modality_stage_layout_batches_and_resume(tmp_path, capsys):
    from litemkd_amd import extract as E
    lists = str(tmp_path / "lists")
    entries = R.write_jpeg_tree(str(tmp_path / "rgb"), lists, videos=2, frames=(1,), hw=(8, 8))      # 6 videos
    order = {e: i for i, e in enumerate(entries)}

    def load_batch(batch):      # frame t of video i carries 10 i + t
        return torch.tensor([10 * order[e] + t for e in batch for t in range(4)])
    model = _FrameModel()
    rec = E.extract_modality(model, _extract_args(tmp_path, lists, modality="flow"), "cpu", load_batch)
    assert model.calls == [16, 8] and (rec["written"], rec["skipped"], rec["model_calls"]) == (6, 0, 2)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["stage"] == "modality" and line["written"] == 6 and line["videos_per_s"] > 0
    for e, i in order.items():
        f = np.load(os.path.join(str(tmp_path / "feats"), "flow", e, "feature.npy"))
        assert f.dtype == np.float32 and f.shape == (4, 2048) and np.array_equal(f[:, 0], 10 * i + np.arange(4)), e
    assert not [n for _, _, files in os.walk(str(tmp_path / "feats")) for n in files if n != "feature.npy"]
    # --resume: only the missing file is computed again
    os.remove(os.path.join(str(tmp_path / "feats"), "flow", entries[4], "feature.npy"))
    model = _FrameModel()
    rec = E.extract_modality(model, _extract_args(tmp_path, lists, modality="flow", resume=True), "cpu", load_batch)
    assert model.calls == [4] and (rec["written"], rec["skipped"]) == (1, 5)
    assert np.load(os.path.join(str(tmp_path / "feats"), "flow", entries[4], "feature.npy"))[0, 0] == 40
    # without --resume everything is written again
    model = _FrameModel()
    assert E.extract_modality(model, _extract_args(tmp_path, lists, modality="flow"), "cpu", load_batch)["written"] == 6


class _SumFusion:
    def extract_feature(self, feature):
        assert set(feature) == {"rgb", "depth", "flow"} and all(v.shape == (1, 4, 2048) for v in feature.values())
        return feature["rgb"] + 2 * feature["depth"] + 4 * feature["flow"]


def test_fusion_stage_layout_resume_and_both_checkpoint_shapes(tmp_path):
    from litemkd_amd import extract as E
    feats, out = tmp_path / "feats", tmp_path / "fused"
    vids = [("A", "v0"), ("A", "v1"), ("B_b", "v0")]
    for mi, m in enumerate(("rgb", "depth", "flow")):
        for vi, (c, v) in enumerate(vids):
            (feats / m / c / v).mkdir(parents=True)
            np.save(feats / m / c / v / "feature.npy", np.full((4, 2048), 10 * mi + vi, dtype=np.float32))
    q = E.build_parser()
    flags = ["--stage", "fusion", "--feature_save_path", str(feats), "--out", str(out), "--checkpoint_dir", "unused", "--seq_len", "4"]
    a = E.args_check(q, q.parse_args(flags))
    rec = E.extract_fusion(_SumFusion(), a, "cpu")
    assert (rec["written"], rec["skipped"]) == (3, 0)
    for vi, (c, v) in enumerate(vids):
        f = np.load(out / c / v / "feature.npy")
        assert f.dtype == np.float32 and f.shape == (4, 2048) and float(f[0, 0]) == vi + 2 * (10 + vi) + 4 * (20 + vi)
    os.remove(out / "A" / "v1" / "feature.npy")
    rec = E.extract_fusion(_SumFusion(), E.args_check(q, q.parse_args(flags + ["--resume"])), "cpu")
    assert (rec["written"], rec["skipped"]) == (1, 2)
    os.remove(feats / "flow" / "B_b" / "v0" / "feature.npy")      # all three modalities are read: a missing one raises
    with pytest.raises(FileNotFoundError):
        E.extract_fusion(_SumFusion(), a, "cpu")
    # checkpoint<N>.pt holds {"model_state_dict": ...}, checkpoint_final.pt the state dict alone; the head's keys are left out
    sd = {"fusion.f1.weight": torch.ones(2), "three_fusion.f1.weight": torch.zeros(2), "bracnch.transformers.0.k_linear.weight": torch.ones(1),
          "fusion.transformer_encoder.layers.0.norm1.weight": torch.ones(1)}
    torch.save({"iteration": 7, "model_state_dict": sd, "optimizer_state_dict": {}, "scheduler": {}}, tmp_path / "checkpoint7.pt")
    torch.save(sd, tmp_path / "checkpoint_final.pt")
    a7, af = E.fusion_checkpoint_state(str(tmp_path / "checkpoint7.pt")), E.fusion_checkpoint_state(str(tmp_path / "checkpoint_final.pt"))
    assert set(a7) == set(af) == {k for k in sd if not k.startswith("bracnch.")}
    torch.save({"fc.weight": torch.ones(1)}, tmp_path / "other.pt")
    with pytest.raises(KeyError, match="not a checkpoint of the MFM teacher"):
        E.fusion_checkpoint_state(str(tmp_path / "other.pt"))
