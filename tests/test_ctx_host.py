"""CTX matcher head, host side (no GPU): the registry builds it under its three names with the reference's state-dict keys, the pairing
errors name both plugins, the teacher loader copies a `bracnch.transformers.*` checkpoint, the built library exports the three entry
points under the unchanged ABI version and checks its shapes before any HIP call, and the plain-torch restatement tests/_ctx_ref.py
reproduces the reference's own outputs (tests/golden/ctx.npz, written by tools/gen_ctx_golden.py) within _ctx_ref.FIXTURE_BOUNDS."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ctx_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CPU = torch.device("cpu")
ENTRY_POINTS = {"lmkd_ctx_ln_fwd": 10, "lmkd_ctx_attend_fwd": 15, "lmkd_ctx_attend_bwd": 19}
MAX_FRAMES = 256
# the reference's CrossTransformer(seq_len 8, trans_linear_out_dim 1152).state_dict() under CTXBranch's `transformers.`
REFERENCE_KEYS = {
    "transformers.pe.pe": (1, 12, 2048),
    "transformers.k_linear.weight": (1152, 2048), "transformers.k_linear.bias": (1152,),
    "transformers.v_linear.weight": (1152, 2048), "transformers.v_linear.bias": (1152,),
    "transformers.norm_k.weight": (1152,), "transformers.norm_k.bias": (1152,),
    "transformers.norm_v.weight": (1152,), "transformers.norm_v.bias": (1152,),
}


def _args(**kw):
    from litemkd_amd.options import default_args
    return default_args(device=CPU, **kw)


# ---- registry ----
def test_student_builds_a_ctx_head():
    from litemkd_amd.model import classifiers as C
    from litemkd_amd.model.model_select import name2classifier, select_model_student
    assert name2classifier["CTX"] == "CTX"
    backbone, clf = select_model_student(_args(model_backbone="resnet18_student", model_classifier="CTX"))
    assert type(clf) is C.CTX and type(clf.transformers) is C.CrossTransformer and type(backbone).__name__ == "resnet18_student"
    assert {k: tuple(v.shape) for k, v in clf.state_dict().items()} == REFERENCE_KEYS
    assert list(clf.state_dict()) == list(REFERENCE_KEYS)


def test_teacher_names_resolve():
    from litemkd_amd.model import classifiers as C
    from litemkd_amd.model.model_select import name2teacher, select_model_teacher
    assert name2teacher["train_teacher_ctx"] == "CTX" and name2teacher["test_teacher_ctx"] == "CTX_fixed"
    t = select_model_teacher(_args(model_teacher="train_teacher_ctx", teacher_checkpoint=None))
    assert type(t) is C.CTX and {k: tuple(v.shape) for k, v in t.state_dict().items()} == REFERENCE_KEYS
    assert issubclass(C.CTX_fixed, C.CTX)


def test_default_initialisation_is_the_containers():
    """nn.Linear / nn.LayerNorm defaults and the sinusoid table: the same draws as a module built from the same containers in order"""
    from litemkd_amd.model import classifiers as C
    torch.manual_seed(5)
    a = C.CrossTransformer(_args())
    torch.manual_seed(5)
    k, v = torch.nn.Linear(2048, 1152), torch.nn.Linear(2048, 1152)
    assert torch.equal(a.k_linear.weight, k.weight) and torch.equal(a.v_linear.bias, v.bias)
    assert torch.equal(a.pe.pe[0], R.positional_encoding(12, 2048))
    assert float(a.norm_k.weight.detach().min()) == 1.0 and float(a.norm_v.bias.detach().abs().max()) == 0.0


def test_train_parser_accepts_the_command_line():
    from litemkd_amd import train
    a = train.args_check(train.build_parser().parse_args(
        "--debug True --model_backbone resnet18_student --model_classifier CTX --model_teacher test_teacher_ctx --distill_name KD".split()))
    assert (a.model_backbone, a.model_classifier, a.model_teacher, a.distill_name) == ("resnet18_student", "CTX", "test_teacher_ctx", "KD")
    a = train.build_parser().parse_args("--model_teacher train_teacher_ctx".split())
    assert a.model_teacher == "train_teacher_ctx"


@pytest.mark.parametrize("backbone", ["resnet18_2fc", "resnet50_2fc", "moblienetv3_fc2", "strmbackbone", "strm18_student"])
def test_backbones_that_return_dicts_are_refused_by_name(backbone):
    from litemkd_amd.model.model_select import select_model_student
    with pytest.raises(NotImplementedError) as e:
        select_model_student(_args(model_backbone=backbone, model_classifier="CTX"))
    assert backbone in str(e.value) and "'CTX'" in str(e.value)


def test_head_refuses_a_feature_dict():
    from litemkd_amd.model import classifiers as C
    with pytest.raises(NotImplementedError, match="classifier 'CTX' reads plain"):
        C.CTX(_args())({"context_features_1": None}, torch.zeros(5), {"target_features_1": None})
    with pytest.raises(NotImplementedError, match="classifier 'CTX_fixed' reads plain"):
        C.CTX_fixed(_args())(torch.zeros(5, 8, 2048), torch.zeros(5), {"target_features_1": None})


# ---- teacher checkpoint ----
def _checkpoint(tmp_path, drop=None):
    g = torch.Generator().manual_seed(31)
    sd = {"bracnch." + k: torch.randn(shape, generator=g) for k, shape in REFERENCE_KEYS.items()}
    sd["fusion.some.weight"] = torch.randn(3, generator=g)
    if drop:
        del sd[drop]
    path = str(tmp_path / "two_ctx.pt")
    torch.save({"model_state_dict": sd}, path)
    return path, sd


def test_teacher_loader_copies_a_two_ctx_checkpoint(tmp_path):
    from litemkd_amd.evaluate import select_test
    from litemkd_amd.model import classifiers as C
    from litemkd_amd.model.model_select import Teacher
    path, sd = _checkpoint(tmp_path)
    t = Teacher(_args(model_teacher="test_teacher_ctx", teacher_checkpoint=path))
    assert type(t.classifier) is C.CTX_fixed
    got = t.classifier.state_dict()
    assert list(got) == list(REFERENCE_KEYS)
    for k, v in got.items():
        assert torch.equal(v, sd["bracnch." + k]), k
    e = select_test(_args(model_teacher="test_teacher_ctx", teacher_checkpoint=path, test_model="teacher"))
    assert type(e) is C.CTX_fixed and all(torch.equal(v, sd["bracnch." + k]) for k, v in e.state_dict().items())


@pytest.mark.parametrize("key", ["bracnch.transformers.pe.pe", "bracnch.transformers.norm_v.bias", "bracnch.transformers.k_linear.weight"])
def test_teacher_loader_names_a_missing_key(tmp_path, key):
    from litemkd_amd.model.model_select import select_model_teacher
    path, _ = _checkpoint(tmp_path, drop=key)
    with pytest.raises(KeyError, match=re.escape(key)):
        select_model_teacher(_args(model_teacher="test_teacher_ctx", teacher_checkpoint=path))


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
    from litemkd_amd import ops
    assert ops.CTX_MAX_FRAMES == MAX_FRAMES and "at most 256 support FRAMES per class" in open(os.path.join(ROOT, "include", "lmkd.h")).read()


def test_shapes_are_checked_before_any_hip_call():
    """null buffers and no GPU: the checks come first, so these return the invalid-argument code instead of touching the device"""
    import litemkd_amd
    lib = litemkd_amd.lib()
    EINVAL = -1
    ints = lambda *v: (ctypes.c_int * len(v))(*v)      # noqa: E731

    def both(Ns, Nq, way, L, D, nseg, off, cnt, col, expect):
        rf = lib.cdll.lmkd_ctx_attend_fwd(None, None, None, None, None, Ns, Nq, way, L, D, nseg, off, cnt, col, None)
        mf = lib.last_error()
        rb = lib.cdll.lmkd_ctx_attend_bwd(None, None, None, None, None, None, None, None, None, Ns, Nq, way, L, D, nseg, off, cnt, col, None)
        mb = lib.last_error()
        assert rf == EINVAL and rb == EINVAL, (Ns, Nq, way, L, D, nseg)
        assert expect in mf and expect in mb, (expect, mf, mb)
    one = (1, ints(0), ints(2), ints(0))
    both(2, 1, 2, 0, 8, *one, "seq_len 0")
    both(2, 1, 2, 17, 8, *one, "seq_len 17")
    both(2, 1, 2, 8, 6, *one, "D = 6")
    both(2, 1, 2, 8, 0, *one, "D = 0")
    both(2, 1, 2, 8, 8, 1, ints(0), ints(2), ints(2), "class column 2 outside [0, 2)")
    both(2, 1, 2, 8, 8, 1, ints(0), ints(2), ints(-1), "class column -1")
    both(2, 1, 2, 8, 8, 17, ints(*range(17)), ints(*([1] * 17)), ints(*([0] * 17)), "17 classes")
    both(2, 1, 2, 8, 8, 0, ints(0), ints(2), ints(0), "0 classes")
    both(3, 1, 2, 8, 8, 2, ints(0, 2), ints(1, 1), ints(0, 1), "does not follow")      # a gap between the segments
    both(3, 1, 2, 8, 8, 1, ints(0), ints(2), ints(0), "hold 2 support videos, not 3")
    # frames per class: 32 videos of 8 frames and 16 of 16 are the limit, one more video is refused
    for L, n in ((8, 33), (16, 17), (1, 257)):
        both(n, 1, 1, L, 8, 1, ints(0), ints(n), ints(0), "%d support frames in class 0, at most %d" % (n * L, MAX_FRAMES))
    for L, n in ((8, 32), (16, 16), (1, 256)):      # at the limit the shapes pass and the null buffers are what is refused
        both(n, 1, 1, L, 8, 1, ints(0), ints(n), ints(0), "null pointer")
    assert lib.cdll.lmkd_ctx_ln_fwd(None, None, None, None, None, None, 0, 8, ctypes.c_float(1e-5), None) == EINVAL
    assert lib.cdll.lmkd_ctx_ln_fwd(None, None, None, None, None, None, 4, 8, ctypes.c_float(1e-5), None) == EINVAL and "null" in lib.last_error()


def test_the_python_layer_refuses_a_class_past_the_limit_before_the_library():
    from litemkd_amd import ops

    class Plan:
        ns, counts, classes = 33, [33], [0]
    with pytest.raises(RuntimeError, match="256 frames per class"):
        ops._ctx_layout(Plan(), 33, 8)


# ---- the restatement against the reference's own numbers ----
@functools.lru_cache(maxsize=None)
def _restated(case, dtype):
    return R.run(case, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", list(R.FIXTURE_CASES))
def test_restatement_reproduces_the_reference(case, dtype):
    G = np.load(os.path.join(GOLD, "ctx.npz"))
    pre = "c%d_" % case
    d = R.case_data(case)
    digest = R.gsum(torch.cat([d["sup"].reshape(-1), d["qry"].reshape(-1)])).numpy()[::64]
    assert np.array_equal(digest, G[pre + "in_digest"])
    assert tuple(G[pre + "logits"].shape) == (d["qry"].shape[0], d["way"])
    out = _restated(case, dtype)
    for k in R.KEYS:
        err = R.fixture_error(k, out[k], G[pre + k])
        print("case %d %s %-9s err %.2e bound %.2e" % (case, dtype, k, err, R.FIXTURE_BOUNDS[case][k]))
        assert err <= R.FIXTURE_BOUNDS[case][k], (k, err, R.FIXTURE_BOUNDS[case][k])


def test_missing_class_column_is_zero_and_the_overflow_case_overflows():
    G = np.load(os.path.join(GOLD, "ctx.npz"))
    assert float(np.abs(G["c2_logits"][:, 1]).max()) == 0.0 and float(np.abs(G["c2_logits"][:, [0, 2, 3]]).min()) > 0.1
    d = R.case_data(7)
    sc = []
    R.ctx_head(d["sup"], d["lab"], d["qry"], d["way"], *(d[k] for k in R.PARAMS), d["pe"], scores=sc)
    top = max(float(s.max()) for s in sc)
    assert top > 89 and not bool(torch.isfinite(torch.exp(torch.tensor(top, dtype=torch.float32))))


def test_case_table_reaches_the_edges():
    """the cases the kernels' paths need: the frames-per-class limit, a D beyond one 1024-column tile that is no multiple of it or of the 64-column
    workgroups, seq_len 1 and 16, a missing class, unsorted ragged labels"""
    shapes = [(len(c[2]), c[4], c[6], max(c[2].count(v) for v in set(c[2])) * c[4]) for c in R.CASES]
    assert max(s[3] for s in shapes) == MAX_FRAMES
    assert any(s[2] > 1024 and s[2] % 64 and s[2] % 4 == 0 for s in shapes)
    assert {1, 16} <= {s[1] for s in shapes}
    assert any(set(range(c[1])) - set(c[2]) for c in R.CASES)
    assert any(c[2] != sorted(c[2]) and len({c[2].count(v) for v in set(c[2])}) > 1 for c in R.CASES)


def test_fixture_is_small_and_holds_numbers_only():
    path = os.path.join(GOLD, "ctx.npz")
    assert os.path.getsize(path) < 512 * 1024
    G = np.load(path)
    assert sorted(G.files) == sorted("c%d_%s" % (c, k) for c in R.FIXTURE_CASES for k in R.KEYS + ("in_digest",))
    assert all(G[k].dtype == np.float32 for k in G.files)
