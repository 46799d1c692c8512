"""STRM students on clips of 9-16 frames, host side (no GPU): the C ABI's refusals (checked before any HIP call), the A/B setter of
the patch-distance dispatch, and both students built at seq_len 12 with exactly the reference's keys and shapes
(tests/golden/strm_long.npz, written by tools/gen_strm_long_golden.py)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CPU = torch.device("cpu")


def _lib():
    import litemkd_amd
    return litemkd_amd.lib()


def _buf(n=1024):
    b = (ctypes.c_float * n)()
    return b, ctypes.cast(b, ctypes.c_void_p)


@pytest.mark.parametrize("L", [1, 17, 0, -3])
def test_token_mlp_refuses_lengths_outside_2_to_16(L):
    lib = _lib()
    keep, p = _buf()
    rc = lib.cdll.lmkd_strm_tokmlp_fwd(p, p, None, p, p, p, p, p, p, None, 1, L, 4, None)
    assert rc != 0
    msg = lib.last_error()
    assert "lmkd_strm_tokmlp_fwd" in msg and "2 <= L <= 16" in msg and "got %d" % L in msg, msg
    rc = lib.cdll.lmkd_strm_tokmlp_bwd(p, p, None, p, p, p, p, p, p, 1, L, 4, None)
    assert rc != 0
    msg = lib.last_error()
    assert "lmkd_strm_tokmlp_bwd" in msg and "2 <= L <= 16" in msg and "got %d" % L in msg, msg


def test_null_pointers_are_refused_before_the_length():
    lib = _lib()
    keep, p = _buf()
    assert lib.cdll.lmkd_strm_tokmlp_fwd(None, p, None, p, p, p, p, p, p, None, 1, 17, 4, None) != 0
    assert "bad arguments" in lib.last_error() and "17" not in lib.last_error()
    assert lib.cdll.lmkd_strm_tokmlp_bwd(p, p, None, p, p, p, None, p, p, 1, 17, 4, None) != 0
    assert "bad arguments" in lib.last_error() and "17" not in lib.last_error()


def test_patch_distance_names_its_limit_at_17_frames():
    lib = _lib()
    keep, p = _buf()
    assert lib.cdll.lmkd_strm_patchdist_fwd(p, p, p, p, p, 2, 2, 2, 1, 17, 1024, None) != 0
    assert "2 <= L <= 16" in lib.last_error() and "L 17" in lib.last_error()


def test_part_rows_do_not_depend_on_the_clip_length():
    """256 lanes per workgroup at every L: the row count of `part` is what it was"""
    lib = _lib()
    for V, D, want in ((50, 2048, 400), (1, 2048, 8), (3, 136, 2), (1, 1, 1), (0, 5, 0), (5, 0, 0), (1, 257, 2)):
        assert lib.value("lmkd_strm_tokmlp_parts", V, D) == want, (V, D)


def test_set_tiled_is_declared_exported_and_checks_its_mode():
    from litemkd_amd import ops
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "lmkd.h")).read()
    assert re.search(r"\bint\s+lmkd_patchdist_set_tiled\s*\(\s*int\s+mode\s*\)\s*;", header)
    assert "lmkd_patchdist_set_tiled" in lib.protos and hasattr(lib.cdll, "lmkd_patchdist_set_tiled")
    try:
        for mode in (-1, 0, 1):
            assert lib.cdll.lmkd_patchdist_set_tiled(mode) == 0
            ops.set_patchdist_tiled(mode)
        for mode in (-2, 2, 7):
            assert lib.cdll.lmkd_patchdist_set_tiled(mode) != 0
            assert "lmkd_patchdist_set_tiled" in lib.last_error() and "got %d" % mode in lib.last_error()
            with pytest.raises(RuntimeError, match="lmkd_patchdist_set_tiled"):
                ops.set_patchdist_tiled(mode)
    finally:
        lib.cdll.lmkd_patchdist_set_tiled(-1)


@pytest.mark.parametrize("backbone,classifier,cls_name", [
    ("strm18_student", "strm_res18_sup", "strmclassifiers_resnet18_sup"),
    ("strmbackbone", "strmclassifiers", "strmclassifiers"),
    ("strmbackbone", "strm_res18", "strmclassifiers_resnet18"),
])
def test_students_at_12_frames_have_the_reference_keys(backbone, classifier, cls_name):
    from litemkd_amd.model.model_select import Student
    from litemkd_amd.options import default_args
    G = np.load(os.path.join(GOLD, "strm_long.npz"))
    assert int(G["seq_len"]) == 12
    ref = json.loads(str(G["keys_json"]))
    s = Student(default_args(device=CPU, model_backbone=backbone, model_classifier=classifier, seq_len=12))
    for part, name in ((s.backbone, backbone), (s.classifier, cls_name)):
        own = {k: list(v.shape) for k, v in part.state_dict().items() if not k.startswith("resnet.")}
        assert own == ref[name]["state_dict"], sorted(set(own) ^ set(ref[name]["state_dict"]))
        n = sum(p.numel() for k, p in part.named_parameters() if not k.startswith("resnet."))
        assert n == ref[name]["parameters"]
    assert ref[backbone]["state_dict"]["fr_enrich.Tok_MLP.inp_fc.weight"] == [12, 12]
    assert ref[backbone]["state_dict"]["fr_enrich.Tok_MLP.out_fc.weight"] == [12, 12]
    assert ref[backbone]["state_dict"]["fr_enrich.pe.pe"] == [1, 18, 2048]
    assert ref[cls_name]["state_dict"]["transformers.pe.pe"] == [1, 18, 2048]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_restatement_reproduces_the_reference_at_12_frames(case):
    """fp64 restatement at seq_len 12 against the reference's fp32 CPU evaluation of the same graph: logits and input-gradient digests
    to 1e-5 relative (relative L2 per tensor), as tests/test_strm_host.py holds it at 8 frames"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _strm_ref as R
    G = np.load(os.path.join(GOLD, "strm_long.npz"))
    pre, L = "c%d_" % case, int(G["seq_len"])
    seed, way, shot, query = (int(G[pre + k]) for k in ("seed", "way", "shot", "query"))
    backbone = str(G[pre + "backbone"])
    ns, nq = way * shot, way * query
    fm = R.make_fmaps(seed, (ns + nq) * L)
    np.testing.assert_allclose(R.gsum(fm).numpy()[::64], G[pre + "in_digest"], rtol=1e-6, atol=1e-6)
    labels = torch.arange(way).repeat_interleave(shot)
    bp = R.cast(R.make_backbone_params(seed, backbone, seq_len=L), torch.float64)
    cp = R.cast(R.make_classifier_params(seed, seq_len=L), torch.float64)
    fm = fm.double().requires_grad_()
    logits, _, _ = R.head(fm, ns, labels, bp, cp, way, shot, seq_len=L, backbone=backbone)
    ref = {k[len(pre) + 7:]: torch.from_numpy(G[k]) for k in G.files if k.startswith(pre + "logits_")}
    assert sorted(logits) == sorted(ref)
    for k, v in ref.items():
        err = float((logits[k].detach() - v.double()).norm() / v.double().norm())
        assert err <= 1e-5, (k, err)
    R.fixture_loss(logits).backward()
    for name, g in (("g_support", fm.grad[:ns * L]), ("g_query", fm.grad[ns * L:])):
        want = torch.from_numpy(G[pre + name]).double()
        err = float((R.gsum(g) - want).norm() / want.norm())
        assert err <= 1e-5, (name, err)
