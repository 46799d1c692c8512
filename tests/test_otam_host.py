"""OTAM matcher head, host side (no GPU): the registry builds it under its three names, the built library exports the four entry points
under the unchanged ABI version and checks its shapes before any HIP call, the plain-torch restatement tests/_otam_ref.py reproduces the
reference's own outputs (tests/golden/otam.npz, written by tools/gen_otam_golden.py), and stays finite where the reference is not."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _anchor  # noqa: E402
import _otam_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CPU = torch.device("cpu")
ENTRY_POINTS = {"lmkd_otam_frame_dist_fwd": 11, "lmkd_otam_align_fwd": 10, "lmkd_otam_align_bwd": 11, "lmkd_otam_frame_dist_bwd": 14}


def _args(**kw):
    from litemkd_amd.options import default_args
    return default_args(device=CPU, **kw)


# ---- registry ----
def test_student_builds_an_otam_head():
    from litemkd_amd.model import classifiers as C
    from litemkd_amd.model.model_select import select_model_student
    backbone, clf = select_model_student(_args(model_backbone="resnet18_student", model_classifier="otam"))
    assert type(clf) is C.OTAM and type(backbone).__name__ == "resnet18_student"
    assert len(clf.state_dict()) == 0 and not list(clf.parameters())


def test_teacher_keys_resolve_without_a_checkpoint():
    from litemkd_amd.model import classifiers as C
    from litemkd_amd.model.model_select import Teacher, select_model_teacher
    assert type(select_model_teacher(_args(model_teacher="train_teacher_otam", teacher_checkpoint=None))) is C.OTAM
    fixed = select_model_teacher(_args(model_teacher="test_teacher_otam", teacher_checkpoint=None))
    assert type(fixed) is C.OTAM_fixed and isinstance(fixed, C.OTAM) and len(fixed.state_dict()) == 0
    assert len(Teacher(_args(model_teacher="test_teacher_otam")).state_dict()) == 0


@pytest.mark.parametrize("backbone", ["resnet18_2fc", "resnet50_2fc", "moblienetv3_fc2", "strmbackbone", "strm18_student"])
def test_backbones_that_return_dicts_are_refused_by_name(backbone):
    from litemkd_amd.model.model_select import select_model_student
    with pytest.raises(NotImplementedError) as e:
        select_model_student(_args(model_backbone=backbone, model_classifier="otam"))
    assert backbone in str(e.value) and "otam" in str(e.value)


def test_head_refuses_a_feature_dict():
    from litemkd_amd.model import classifiers as C
    with pytest.raises(NotImplementedError, match="OTAM"):
        C.OTAM(_args())({"context_features_1": None}, torch.zeros(5), {"target_features_1": None})


def test_train_parser_accepts_the_command_line():
    from litemkd_amd import train
    a = train.args_check(train.build_parser().parse_args(
        "--debug True --model_backbone resnet18_student --model_classifier otam --model_teacher test_teacher_otam --distill_name KD".split()))
    assert (a.model_backbone, a.model_classifier, a.model_teacher, a.distill_name) == ("resnet18_student", "otam", "test_teacher_otam", "KD")
    from litemkd_amd.model.model_select import name2classifier, name2teacher
    assert name2classifier[a.model_classifier] == "OTAM" and name2teacher[a.model_teacher] == "OTAM_fixed"
    assert name2teacher["train_teacher_otam"] == "OTAM"


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


def test_shapes_are_checked_before_any_hip_call():
    """null buffers and no GPU: the checks come first, so these return the invalid-argument code instead of touching the device"""
    import litemkd_amd
    L = litemkd_amd.lib()
    EINVAL = -1
    ok_cls = (ctypes.c_int * 513)(*([0] * 513))
    fwd, bwd = L.cdll.lmkd_otam_align_fwd, L.cdll.lmkd_otam_align_bwd
    for Nq, Ns, way, seq in ((1, 2, 2, 17), (1, 513, 2, 8), (1, 2, 2, 0), (1, 0, 1, 8), (0, 2, 2, 8), (1, 2, 3, 8)):
        assert fwd(None, None, ok_cls, None, None, Nq, Ns, way, seq, None) == EINVAL, (Nq, Ns, way, seq)
        assert bwd(None, None, None, None, ok_cls, None, Nq, Ns, way, seq, None) == EINVAL, (Nq, Ns, way, seq)
    assert "seq_len 17" in L.last_error() or "way" in L.last_error()
    assert fwd(None, None, None, None, None, 1, 2, 2, 17, None) == EINVAL and "seq_len 17" in L.last_error()
    assert fwd(None, None, None, None, None, 1, 513, 2, 8, None) == EINVAL and "513" in L.last_error()
    bad_cls = (ctypes.c_int * 2)(0, 2)
    assert fwd(None, None, bad_cls, None, None, 1, 2, 2, 8, None) == EINVAL and "class 2" in L.last_error()
    neg_cls = (ctypes.c_int * 2)(-1, 0)
    assert bwd(None, None, None, None, neg_cls, None, 1, 2, 2, 8, None) == EINVAL and "class -1" in L.last_error()
    assert fwd(None, None, ok_cls, None, None, 1, 2, 1, 8, None) == EINVAL and "null" in L.last_error()      # valid shapes, null buffers
    for D in (0, 6, -4):
        assert L.cdll.lmkd_otam_frame_dist_fwd(None, None, None, None, None, None, 1, 2, 8, D, None) == EINVAL
        assert L.cdll.lmkd_otam_frame_dist_bwd(None, None, None, None, None, None, None, None, None, 1, 2, 8, D, None) == EINVAL
    assert L.cdll.lmkd_otam_frame_dist_fwd(None, None, None, None, None, None, 1, 2, 17, 64, None) == EINVAL
    assert L.cdll.lmkd_otam_frame_dist_bwd(None, None, None, None, None, None, None, None, None, 1, 513, 8, 64, None) == EINVAL


def test_missing_class_is_named_from_the_host_plan():
    from litemkd_amd import ops

    class Plan:
        way, classes, labels = 3, [0, 2], [0, 0, 2]
    with pytest.raises(ValueError, match="class 1 has none"):
        ops.otam_plan_check(Plan())


# ---- the restatement against the reference's own numbers ----
@pytest.mark.parametrize("case", list(R.FIXTURE_CASES))
def test_restatement_reproduces_the_reference(case):
    """cum within 2e-5 absolute (ten times the 1.9e-6 the reference's fp32 recursion is away from fp64 at L = 8, D = 2048, cum about 14),
    logits within 3e-6 (the same factor over 3e-7), gradient chunk sums within 2e-3 of the reference's maximum"""
    G = np.load(os.path.join(GOLD, "otam.npz"))
    pre = "c%d_" % case
    way, L, sup, lab, qry = R.case_data(case)
    assert L <= 8
    digest = R.gsum(torch.cat([sup.reshape(-1), qry.reshape(-1)])).numpy()[::64]
    assert np.array_equal(digest, G[pre + "in_digest"])
    ref = {k: torch.from_numpy(G[pre + k]).double() for k in ("logits", "cum", "g_support", "g_query")}
    assert tuple(ref["logits"].shape) == (qry.shape[0], way) and tuple(ref["cum"].shape) == (qry.shape[0], sup.shape[0])
    assert float(ref["cum"].max()) - float(ref["cum"].min()) > 4 and float(ref["logits"].max()) > 1.5 / way      # not a flat softmax
    for dt in (torch.float32, torch.float64):
        out = R.run(case, dt)
        e_cum = float((out["cum"].double() - ref["cum"]).abs().max())
        e_log = float((out["logits"].double() - ref["logits"]).abs().max())
        print("case %d %s: cum err %.2e logits err %.2e" % (case, dt, e_cum, e_log))
        assert e_cum <= 2e-5 and e_log <= 3e-6
        assert torch.allclose(out["logits"].sum(1).double(), torch.ones(qry.shape[0], dtype=torch.float64), atol=1e-6)
        for name in ("g_support", "g_query"):
            err = float((R.gsum(out[name]).double() - ref[name]).abs().max())
            assert err <= 2e-3 * float(ref[name].abs().max()), name


def test_fixture_is_small_and_holds_numbers_only():
    path = os.path.join(GOLD, "otam.npz")
    assert os.path.getsize(path) < 100 * 1024
    G = np.load(path)
    assert sorted(G.files) == sorted("c%d_%s" % (c, k) for c in R.FIXTURE_CASES for k in ("logits", "cum", "g_support", "g_query", "in_digest"))
    assert all(G[k].dtype == np.float32 for k in G.files)


# ---- where the reference is inf ----
def _reference_form(sup, qry):
    """the soft minimum without the subtraction, -0.1 log sum exp(-a / 0.1), on the same table: inf once a cumulative distance passes ~10.4"""
    keep = R.softmin
    R.softmin = lambda *a: -R.LBDA * torch.log(sum(torch.exp(-x / R.LBDA) for x in a))
    try:
        Ns, L, _ = sup.shape
        B = R.frame_dist(sup, qry).reshape(qry.shape[0], L, Ns, L).permute(0, 2, 1, 3)
        return R.align(B) + R.align(B.transpose(-1, -2))
    finally:
        R.softmin = keep


@pytest.mark.parametrize("case", [5, 6])
def test_restatement_is_finite_where_the_plain_form_is_not(case):
    """seq_len 12 and 16 with randn features.  fp32 against fp64 by _anchor.anchored with the fp64 result rounded to fp32 as the
    yardstick: 3 x its rounding plus 2e-5 relative.  The floor: the table is (L + 1) L <= 272 cells, each a handful of fp32 operations on
    values no larger than the result (the soft minimum's weights sum to 1, so errors add and are not amplified); 272 cells x 2^-24 is
    1.6e-5 if every rounding pointed the same way, a non-finite or unstable evaluation is orders of magnitude beyond it."""
    way, L, sup, lab, qry = R.case_data(case)
    assert L in (12, 16)
    assert not bool(torch.isfinite(_reference_form(sup, qry)).all())
    r32, r64 = R.run(case, torch.float32), R.run(case, torch.float64)
    for k in ("cum", "logits", "g_support", "g_query"):
        assert bool(torch.isfinite(r32[k]).all()), k
        e, _ = _anchor.anchored(k, r32[k], r64[k].float(), r64[k], floor=2e-5)
        print("case %d %s: fp32 vs fp64 rel-L2 %.2e" % (case, k, e))
