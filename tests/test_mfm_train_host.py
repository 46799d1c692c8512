"""Training the MFM teacher, host side (no GPU): the library exports the four new entry points under the unchanged ABI
version and checks its shapes before any HIP call, the module keeps its state-dict keys and gains the reference's `bracnch.*` ones with
head=True, the trainer's command line, optimizer-step cadence and feature-tree reader, and the plain-torch restatement
tests/_mfm_train_ref.py against torch's own containers and against the reference's numbers (tests/golden/mfm_train.npz)."""
import argparse
import functools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mfm_train_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ENTRY_POINTS = {"lmkd_layernorm_train_fwd": 14, "lmkd_layernorm_train_bwd": 11, "lmkd_mha_small_train_fwd": 9, "lmkd_mha_small_bwd": 10}
EINVAL = -1


def _args(**kw):
    a = dict(seq_len=8, trans_num=2, shirt_num=1, temp_set=[2], way=5, trans_linear_out_dim=1152, trans_linear_in_dim=2048,
             trans_dropout=0.1, m1="rgb", m2="depth", m3="flow")
    a.update(kw)
    return argparse.Namespace(**a)


# ---- ABI ----
def test_library_exports_the_entry_points_under_abi_3():
    import litemkd_amd
    L = litemkd_amd.lib()
    assert L.value("lmkd_abi_version") == 3
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "lmkd.h")).read(), flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        assert hasattr(L.cdll, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert len(L.protos[name][1]) == nargs, name
    assert len(L.protos["lmkd_layernorm_fwd"][1]) == 11 and len(L.protos["lmkd_mha_small"][1]) == 7      # the inference entry points stay


def test_shapes_are_checked_before_any_hip_call():
    """null buffers and no GPU: the checks come first, so these return the invalid-argument code instead of touching the device"""
    import litemkd_amd
    lib = litemkd_amd.lib()
    c = lib.cdll

    def attn(B, L, D, H, expect):
        rf = c.lmkd_mha_small_train_fwd(None, None, None, None, B, L, D, H, None)
        mf = lib.last_error()
        rb = c.lmkd_mha_small_bwd(None, None, None, None, None, B, L, D, H, None)
        mb = lib.last_error()
        assert rf == EINVAL and rb == EINVAL, (B, L, D, H)
        assert expect in mf and expect in mb, (expect, mf, mb)
    attn(0, 8, 128, 2, "0 sequences")
    attn(2, 8, 128, 0, "0 heads")
    attn(2, 0, 128, 2, "0 tokens")
    attn(2, 9, 128, 2, "9 tokens")
    attn(2, 8, 0, 2, "width 0")
    attn(2, 8, 130, 4, "width 130 is no multiple of 4 heads")
    attn(2, 8, 128, 2, "null pointer")      # the shapes pass and the null buffers are what is refused

    def ln_fwd(ldy, rows, D, expect, res_rows=0):
        assert c.lmkd_layernorm_train_fwd(None, None, res_rows, None, None, None, None, ldy, None, None, rows, D, 1e-5, None) == EINVAL
        assert expect in lib.last_error(), (expect, lib.last_error())

    def ln_bwd(lddy, rows, D, expect):
        assert c.lmkd_layernorm_train_bwd(None, lddy, None, None, None, None, None, None, rows, D, None) == EINVAL
        assert expect in lib.last_error(), (expect, lib.last_error())
    for f in (ln_fwd, ln_bwd):
        f(64, 0, 64, "0 rows")
        f(64, 4, 0, "4 rows of 0")
        f(63, 4, 64, "row stride 63 below the row length 64")
        f(24576, 4, 24576, "null pointer")      # 96 KB, the limit
        f(64, 4, 64, "null pointer")
    ln_fwd(24577, 1, 24577, "does not fit in LDS")
    ln_bwd(24577, 1, 24577, "past the forward's limit")


# ---- module ----
def test_default_construction_keeps_its_state_dict_keys():
    from litemkd_amd.teacher.mfm import ThreeTRXShiftLoopTime
    from oracle import ref_cpu as O
    m = ThreeTRXShiftLoopTime(_args(), in_channels=64)
    shapes = O.mfm_param_shapes(d=64)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == shapes
    assert not hasattr(m, "bracnch")
    with pytest.raises(RuntimeError, match="head=True"):
        m({}, None, {})


def test_head_adds_the_reference_keys():
    from litemkd_amd.teacher.mfm import ThreeTRXShiftLoopTime
    from oracle import ref_cpu as O
    with torch.device("meta"):
        m = ThreeTRXShiftLoopTime(_args(temp_set=[2, 3], trans_num=1), head=True)
        plain = ThreeTRXShiftLoopTime(_args(trans_num=1))
    keys = list(m.state_dict())
    head = [k for k in keys if k.startswith("bracnch.")]
    assert [k for k in keys if not k.startswith("bracnch.")] == list(plain.state_dict())
    assert keys[:len(head)] == head      # `bracnch` first, as the reference constructs it (model.py:1592-1594)
    per = ["pe.pe", "k_linear.weight", "k_linear.bias", "v_linear.weight", "v_linear.bias", "norm_k.weight", "norm_k.bias", "norm_v.weight", "norm_v.bias"]
    assert head == ["bracnch.transformers.%d.%s" % (i, k) for i in (0, 1) for k in per]
    sd = m.state_dict()
    assert tuple(sd["bracnch.transformers.0.k_linear.weight"].shape) == (1152, 4096)
    assert tuple(sd["bracnch.transformers.1.k_linear.weight"].shape) == (1152, 6144)
    assert sorted(O.mfm_param_shapes(num_layers=1)) == sorted(plain.state_dict())


def test_head_at_another_width_is_refused():
    from litemkd_amd.teacher.mfm import ThreeTRXShiftLoopTime
    with pytest.raises(ValueError, match="width 2048, not in_channels = 64"):
        ThreeTRXShiftLoopTime(_args(), in_channels=64, head=True)


def test_dropout_sites_and_shapes():
    from litemkd_amd.teacher.mfm import ThreeTransforTemproal
    m = ThreeTransforTemproal(_args(seq_len=5), in_channels=64)
    s = m.dropout_shapes(3, 5)
    assert list(s) == ["pe1", "pe2", "pe3", "l0.attn", "l0.dropout1", "l0.dropout", "l0.dropout2", "l1.attn", "l1.dropout1", "l1.dropout",
                       "l1.dropout2", "f1"]
    assert all(p == 0.1 for _, p in s.values())
    assert s["pe2"][0] == (15, 64) and s["l1.attn"][0] == (9, 5, 5) and s["l0.dropout"][0] == (15, 2048) and s["l0.dropout2"][0] == (15, 192)
    assert s["f1"][0] == (15, 64)


# ---- the restatement ----
def test_restatement_equals_the_nn_containers():
    for n_mod, L in ((3, 5), (2, 8)):
        errs = R.check_against_containers(n_mod=n_mod, L=L)
        assert len(errs) > 20 and max(errs.values()) < 1e-12, max(errs.items(), key=lambda kv: kv[1])


def test_masks_change_the_restatement_and_scale_by_keep():
    mod = R.make_fusion(2, 64, 5, 1, 3)
    xs = R.fusion_inputs(4, 2, 2, 5, 64)
    p = {"m." + k: v for k, v in mod.named_parameters()}
    base = R.fusion(xs, p, "m", 1)
    ones = {k: torch.ones(shape) for k, (shape, _) in mod.dropout_shapes(2, 5).items()}
    assert torch.equal(R.fusion(xs, p, "m", 1, ones), base)
    ones["f1"] = torch.full_like(ones["f1"], 1 / 0.9)
    assert torch.allclose(R.fusion(xs, p, "m", 1, ones), base / 0.9, rtol=1e-6, atol=0)
    masks = R.make_masks(mod, 2, 5, 9)
    assert all(set(m.unique().tolist()) <= {0.0, float(torch.tensor(1.0) / torch.tensor(0.9))} for m in masks.values())
    assert float((R.fusion(xs, p, "m", 1, masks) - base).abs().max()) > 1e-2


@functools.lru_cache(maxsize=None)
def _restated(dtype):
    return R.restated_teacher(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_restatement_reproduces_the_reference(dtype):
    G = np.load(os.path.join(GOLD, "mfm_train.npz"))
    errs, bounds = R.digest_errors(_restated(dtype), G), R.fixture_bounds(G)
    assert set(errs) == set(bounds) and len(errs) == 1 + 2 * sum(R.trainable(k) for k in R.teacher_params())
    for k in sorted(errs):
        print("%-72s err %.3e bound %.3e" % (k, errs[k], bounds[k]))
    bad = {k: (errs[k], bounds[k]) for k in errs if not errs[k] <= bounds[k]}
    assert not bad, bad


def test_fixture_is_small_holds_numbers_only_and_its_gradients_are_not_zero():
    path = os.path.join(GOLD, "mfm_train.npz")
    assert os.path.getsize(path) < 400 * 1024
    G = np.load(path)
    assert all(G[k].dtype == np.float64 and G[k].size <= R.SAMPLE for k in G.files)
    assert tuple(G["logits"].shape) == (R.WT["n_query"], R.WT["way"])
    missing = sorted(set(range(R.WT["way"])) - set(R.WT["labels"]))
    assert missing == [1] and float(np.abs(G["logits"][:, missing]).max()) == 0.0 and float(np.abs(G["logits"][:, [0, 2, 3]]).min()) > 0.1
    norms = {k[2:]: float(G[k][0]) for k in G.files if k.startswith("n:")}
    top = max(norms.values())
    zero = [k for k, v in norms.items() if v < 1e-8 * top]      # the reference holds the rounding of its column sums there
    assert zero == ["bracnch.transformers.0.v_linear.bias"]
    assert all(v > 0 for v in norms.values())


# ---- trainer ----
_write_tree = R.write_feature_tree


def test_trainer_flags():
    from litemkd_amd import train_teacher as TT
    p = TT.build_parser()
    a = TT.args_check(p, p.parse_args(
        "--way 3 --shot 1 --query_per_class 1 --seq_len 8 --trans_linear_out_dim 1152 --trans_dropout 0.0 --temp_set 2 3 --tasks_per_batch 2 "
        "--training_iterations 4 --save_freq 2 --print_freq 1 --split 1 --traintestlist lists --checkpoint_dir ck --resume_from_checkpoint "
        "--feature_save_path feats --seed 7 --m1 rgb --m2 flow --m3 depth --shirt_num 2 --trans_num 1 --opt adam -lr 0.001 --sch 10 20 "
        "--log_jsonl log.jsonl".split()))
    assert (a.way, a.shot, a.query_per_class, a.temp_set, a.tasks_per_batch, a.training_iterations, a.save_freq) == (3, 1, 1, [2, 3], 2, 4, 2)
    assert (a.m1, a.m2, a.m3, a.shirt_num, a.trans_num, a.opt, a.learning_rate, a.sch) == ("rgb", "flow", "depth", 2, 1, "adam", 0.001, [10, 20])
    assert a.resume_from_checkpoint and a.trans_linear_in_dim == 2048 and not a.no_save and a.log_jsonl == "log.jsonl"
    d = p.parse_args([])
    assert (d.m1, d.m2, d.m3, d.shirt_num, d.trans_num, d.temp_set, d.opt) == ("rgb", "depth", "flow", 1, 2, [2], "sgd")
    for bad in ([], ["--feature_save_path", "x"], ["--synthetic", "--resume_from_checkpoint", "--no_save"]):
        with pytest.raises(SystemExit):
            TT.args_check(p, p.parse_args(bad))
    TT.args_check(p, p.parse_args(["--synthetic", "--no_save"]))


def test_optimizer_step_cadence_with_stand_ins():
    """the reference's counting (multi_run.py:380-396): `iteration` runs from 1, the optimizer steps when (iteration + 1) % tasks_per_batch
    == 0 or iteration == training_iterations - 1, the scheduler every episode, a checkpoint when (iteration + 1) % save_freq == 0"""
    from litemkd_amd import train_teacher as TT
    events = []

    class Opt:
        lr, steps = 0.1, 0

        def step(self):
            self.steps += 1
            events.append(("step", it[0]))

        def zero_grad(self):
            events.append(("zero", it[0]))

    class Sch:
        n = 0

        def step(self):
            self.n += 1
    it = [0]

    def task(model, t, args):
        it[0] += 1
        return torch.tensor(float(it[0])), torch.tensor(0.5)
    saved = []
    real = TT.train_task, TT.save_checkpoint
    TT.train_task, TT.save_checkpoint = task, lambda m, o, s, i, d: saved.append(i)
    try:
        for tpb, total, want in ((2, 4, [1, 3]), (3, 7, [2, 5, 6]), (16, 5, [4]), (1, 3, [1, 2, 3])):
            events.clear()
            saved.clear()
            it[0] = 0
            args = argparse.Namespace(tasks_per_batch=tpb, training_iterations=total, print_freq=2, save_freq=2, no_save=False, checkpoint_dir="x")
            opt, sch = Opt(), Sch()
            logged = []
            losses, accs = TT.train(None, iter(range(100)), opt, sch, args, log=lambda i, a, b: logged.append((i, a, b)))
            assert losses == [float(i) for i in range(1, total + 1)] and accs == [0.5] * total
            assert [i for e, i in events if e == "step"] == want, (tpb, total, events)
            assert events[0] == ("zero", 0) and [i for e, i in events[1:] if e == "zero"] == want
            assert sch.n == total and it[0] == total
            assert saved == [i + 1 for i in range(1, total + 1) if (i + 1) % 2 == 0 and i + 1 != total]      # labelled iteration + 1 (:423-426)
            assert [i for i, _, _ in logged] == [i for i in range(2, total + 2, 2) if i - 1 <= total]
        it[0] = 2      # resumed at iteration 2 of 4
        events.clear()
        args = argparse.Namespace(tasks_per_batch=2, training_iterations=4, print_freq=100, save_freq=100, no_save=True, checkpoint_dir=None)
        losses, _ = TT.train(None, iter(range(100)), Opt(), Sch(), args, start_iteration=2)
        assert losses == [3.0, 4.0] and [i for e, i in events if e == "step"] == [3]
    finally:
        TT.train_task, TT.save_checkpoint = real


def test_feature_tree_reader(tmp_path):
    import random
    from litemkd_amd import train_teacher as TT
    root = str(tmp_path / "feats")
    _write_tree(root, missing={("depth", "c1", "v1_0"), ("flow", "c1", "v1_0"), ("flow", "c2", "v2_2")})
    os.makedirs(os.path.join(root, "rgb", "c0", "empty_video"))      # no feature.npy: not a video
    cfg = argparse.Namespace(way=3, shot=1, query_per_class=1, query_per_class_test=1, seq_len=8, m1="rgb", m2="depth", m3="flow", split=1)
    E = TT.FeatureTreeEpisodes(cfg, root, device="cpu")
    assert sorted(E.splits[True]) == ["c0", "c1", "c2", "c3"] and E.splits[True]["c0"] == ["v0_0", "v0_1", "v0_2"]
    r, d, f = E.read("c1", "v1_0")
    assert r.shape == (8, 2048) and r.dtype == torch.float32 and float(r.abs().sum()) > 0 and float(d.abs().sum()) == 0.0 and float(f.abs().sum()) == 0.0
    r, d, f = E.read("c2", "v2_2")
    assert float(d.abs().sum()) > 0 and float(f.abs().sum()) == 0.0
    assert torch.equal(E.read("c0", "v0_1")[2], torch.from_numpy(np.load(os.path.join(root, "flow", "c0", "v0_1", "feature.npy"))))
    random.seed(5)
    a = E.episode()
    random.seed(5)
    b = E.episode()
    assert sorted(a["context_features"]) == ["depth", "flow", "rgb"]
    assert a["context_features"]["rgb"].shape == (3, 8, 2048) and a["target_features"]["flow"].shape == (3, 8, 2048)
    assert sorted(a["context_labels"].tolist()) == [0.0, 1.0, 2.0] and sorted(a["target_labels"].tolist()) == [0.0, 1.0, 2.0]
    assert all(torch.equal(a["context_features"][m], b["context_features"][m]) for m in a["context_features"])
    # the draws are ClipDirectoryEpisodes' own: classes, then per class shot + queries videos, then the two shuffles
    random.seed(5)
    classes = random.sample(["c0", "c1", "c2", "c3"], 3)
    picks = [random.sample(range(3), 2) for _ in classes]
    sup = [(c, E.splits[True][c][p[0]], i) for i, (c, p) in enumerate(zip(classes, picks))]
    random.shuffle(sup)
    assert a["context_labels"].tolist() == [float(s[2]) for s in sup]
    assert torch.equal(a["context_features"]["rgb"][0], E.read(sup[0][0], sup[0][1])[0])
    # split lists: only the listed videos, matched in lower case
    lists = tmp_path / "lists"
    lists.mkdir()
    names = ["c%d/V%d_%d.avi" % (c, c, v) for c in range(3) for v in range(2)]
    (lists / "trainlist01.txt").write_text("\n".join(names) + "\n")
    (lists / "testlist01.txt").write_text("c3/v3_0.avi\n")
    S = TT.FeatureTreeEpisodes(cfg, root, str(lists), 1, device="cpu")
    assert sorted(S.splits[True]) == ["c0", "c1", "c2"] and S.splits[True]["c2"] == ["v2_0", "v2_1"] and S.splits[False] == {"c3": ["v3_0"]}
    with pytest.raises(ValueError, match="the episodes need 3"):
        TT.FeatureTreeEpisodes(cfg, root, str(lists), 1, device="cpu", train=False)
    bad = os.path.join(root, "rgb", "c0", "v0_0", "feature.npy")
    np.save(bad, np.zeros((4, 2048), np.float32))
    with pytest.raises(ValueError, match="expected \\(8, 2048\\)"):
        E.read("c0", "v0_0")
    # only a file that is not there reads as zeros: a wrongly shaped or unreadable second / third modality is an error, not silence
    np.save(os.path.join(root, "depth", "c0", "v0_1", "feature.npy"), np.zeros((8, 1024), np.float32))
    with pytest.raises(ValueError, match="depth/c0/v0_1"):
        E.read("c0", "v0_1")
    with open(os.path.join(root, "flow", "c0", "v0_2", "feature.npy"), "wb") as f:
        f.write(b"not a numpy file")
    with pytest.raises(Exception) as err:
        E.read("c0", "v0_2")
    assert not isinstance(err.value, FileNotFoundError)


def test_synthetic_source_is_seeded():
    from litemkd_amd import train_teacher as TT
    cfg = argparse.Namespace(way=3, shot=2, query_per_class=1, seq_len=8, m1="rgb", m2="depth", m3="flow")
    a, b = TT.SyntheticFeatureEpisodes(cfg, 4, "cpu").episode(), TT.SyntheticFeatureEpisodes(cfg, 4, "cpu").episode()
    assert a["context_features"]["depth"].shape == (6, 8, 2048) and a["target_features"]["rgb"].shape == (3, 8, 2048)
    assert torch.equal(a["context_features"]["flow"], b["context_features"]["flow"]) and torch.equal(a["target_labels"], b["target_labels"])
    assert sorted(a["context_labels"].tolist()) == [0.0, 0.0, 1.0, 1.0, 2.0, 2.0] and float(a["context_features"]["rgb"].min()) >= 0.0
