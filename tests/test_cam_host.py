"""Attention maps, host side (no GPU): the two entry points are declared and exported under the unchanged ABI version and check their
arguments before any launch, ops.jet_lut is the integer table, the numpy restatement tests/_cam_ref.py gives the closed forms, and
cam.grad_cam refuses an STRM student by name."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cam_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"lmkd_gradcam_fwd": 10, "lmkd_cam_overlay_u8": 17}
EINVAL = -1


def test_prototypes_are_declared_and_exported_under_abi_3():
    import litemkd_amd
    from litemkd_amd._lib import parse_header
    protos = parse_header()
    L = litemkd_amd.lib()
    assert L.value("lmkd_abi_version") == 3
    for name, nargs in ENTRY_POINTS.items():
        assert name in protos and len(protos[name][1]) == nargs, name
        assert hasattr(L.cdll, name), name
    text = open(os.path.join(ROOT, "include", "lmkd.h")).read()
    assert "heatmap_vis.py:20-48" in text and "teacher/code/heatmap_vis.py:16-27" in text


def test_gradcam_arguments_are_checked_before_any_launch():
    import litemkd_amd
    from litemkd_amd import ops
    lib = litemkd_amd.lib()

    def refused(F, HW, C, mode, expect):
        assert lib.cdll.lmkd_gradcam_fwd(None, None, None, None, None, F, HW, C, mode, None) == EINVAL, (F, HW, C, mode)
        assert re.search(expect, lib.last_error()), (expect, lib.last_error())
    refused(2, 49, 512, 2, r"mode 2")
    refused(2, 49, 512, -1, r"mode -1")
    refused(2, 49, 12, 0, r"\bC 12\b")
    refused(2, 49, 0, 0, r"\bC 0\b")
    refused(2, 49, ops.CAM_MAX_C + 8, 0, r"\bC %d\b" % (ops.CAM_MAX_C + 8))
    refused(2, ops.CAM_MAX_HW + 1, 512, 1, r"\bHW %d\b" % (ops.CAM_MAX_HW + 1))
    refused(2, 0, 512, 0, r"\bHW 0\b")
    refused(0, 49, 512, 0, r"\bF 0\b")
    for C, HW in ((ops.CAM_MAX_C, ops.CAM_MAX_HW), (512, 49), (960, 1), (8, 1024)):      # inside the limits: the null buffers are what is refused
        refused(2, HW, C, 0, r"null")
    assert ops.CAM_MAX_C >= 4096 and ops.CAM_MAX_HW >= 1024


def test_overlay_arguments_are_checked_before_any_launch():
    import litemkd_amd
    lib = litemkd_amd.lib()

    def refused(F, h, w, Ho, Wo, alpha, expect, ks=3):
        rc = lib.cdll.lmkd_cam_overlay_u8(None, None, None, None, None, ks, None, None, ks, None, F, h, w, Ho, Wo, alpha, None)
        assert rc == EINVAL and re.search(expect, lib.last_error()), (expect, rc, lib.last_error())
    refused(2, 7, 7, 224, 224, 257, r"alpha256 257")
    refused(2, 7, 7, 224, 224, -1, r"alpha256 -1")
    refused(65536, 7, 7, 224, 224, 128, r"\bF 65536\b")
    refused(2, 0, 7, 224, 224, 128, r"\bh 0\b")
    refused(2, 7, 7, 224, 0, 128, r"\bWo 0\b")
    refused(2, 7, 7, 224, 224, 128, r"ksize_h 0", ks=0)
    refused(2, 7, 7, 224, 224, 128, r"null")


def test_jet_lut_is_the_integer_table():
    from litemkd_amd import ops
    lut = ops.jet_lut()
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3) and not lut.is_cuda
    assert np.array_equal(lut.numpy(), R.jet_lut())
    assert tuple(lut[0].tolist()) == (0, 0, 128) and tuple(lut[128].tolist()) == (130, 255, 126) and tuple(lut[255].tolist()) == (128, 0, 0)
    # written out per entry, without numpy
    for i in range(256):
        for k, centre in enumerate((1530, 1020, 510)):
            assert int(lut[i, k]) == (min(510, max(0, 765 - abs(8 * i - centre))) + 1) >> 1, (i, k)


@pytest.mark.parametrize("mode", [0, 1])
def test_reference_closed_forms(mode):
    g = np.random.default_rng(3)
    F, HW, C = 2, 12, 16
    A = g.standard_normal((F, HW, C))
    # constant dA = k: w = k, the Grad-CAM sum is k * sum_c A - and so is HiResCAM's
    w, raw, cam = R.gradcam(A, np.full((F, HW, C), 0.25), mode)
    assert np.allclose(w, 0.25, rtol=0, atol=1e-15)
    want = np.maximum(0.25 * A.sum(-1), 0)
    assert np.allclose(raw, want, rtol=1e-13, atol=1e-15)
    assert np.allclose(cam, (want - want.min(1, keepdims=True)) / (1e-7 + want.max(1, keepdims=True) - want.min(1, keepdims=True)), rtol=1e-12)
    assert float(cam.min()) == 0.0 and 1.0 - 1e-6 < float(cam.max()) < 1.0
    # one-hot dA at (p0, c0): w = e_c0 / HW; Grad-CAM shows channel c0 everywhere, HiResCAM only position p0
    dA = np.zeros((F, HW, C))
    dA[:, 5, 3] = 2.0
    w, raw, _ = R.gradcam(A, dA, mode)
    assert np.array_equal(np.nonzero(w[0])[0], [3]) and np.allclose(w[:, 3], 2.0 / HW, rtol=1e-15)
    if mode == 0:
        assert np.allclose(raw, np.maximum(A[:, :, 3] * 2.0 / HW, 0), rtol=1e-13)
    else:
        only = np.zeros((F, HW))
        only[:, 5] = np.maximum(2.0 * A[:, 5, 3], 0)
        assert np.array_equal(raw, only)


@pytest.mark.parametrize("mode", [0, 1])
def test_reference_single_position_and_constant_maps_are_zero(mode):
    g = np.random.default_rng(4)
    for dt in (np.float64, np.float32):
        A, dA = g.standard_normal((3, 1, 8)).astype(dt), g.standard_normal((3, 1, 8)).astype(dt)
        _, raw, cam = R.gradcam(A, dA, mode)
        assert raw.dtype == dt and float(np.abs(cam).max()) == 0.0          # HW = 1: raw - min = 0
        A = np.abs(g.standard_normal((2, 6, 8))).astype(dt)
        _, raw, cam = R.gradcam(A, -np.abs(g.standard_normal((2, 6, 8))).astype(dt), mode)
        assert float(np.abs(raw).max()) == 0.0 and float(np.abs(cam).max()) == 0.0      # A >= 0, dA <= 0: nothing survives the ReLU


def test_reference_blend_and_quantisation():
    col = np.array([[0, 255, 128]], dtype=np.uint8)
    frm = np.array([[255, 0, 128]], dtype=np.uint8)
    assert np.array_equal(R.blend(col, frm, 0), col) and np.array_equal(R.blend(col, frm, 256), frm)
    assert np.array_equal(R.blend(col, frm, 128), [[128, 128, 128]]) and R.blend(col, None, 128) is col
    assert R.quantise(np.array([0.0, 1.0, 0.5, 1.0 / 1024, 2.0 / 1024, 1023.0 / 1024])).tolist() == [0, 255, 128, 0, 0, 255]


def test_module_imports_without_a_gpu_and_refuses_strm():
    from litemkd_amd import cam, heatmap  # noqa: F401
    from litemkd_amd.model.model_select import Student
    from litemkd_amd.options import default_args
    args = default_args(device=torch.device("cpu"), model_backbone="strm18_student", model_classifier="strm_res18_sup", seq_len=4,
                        trans_linear_out_dim=64)
    student = Student(args)
    x = torch.zeros(4, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="strm18_student"):
        cam.grad_cam(student, x, torch.zeros(1), x)
    with pytest.raises(ValueError, match="logits_fn"):
        cam.accuracy_logits({"support_set": None, "query": None})
    assert cam.accuracy_logits({"query": 5}, logits_fn=lambda d: d["query"]) == 5


def test_ops_refuse_cpu_tensors():
    from litemkd_amd import ops
    a = torch.zeros(1, 2, 2, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gradcam(a, a, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cam_overlay(torch.zeros(1, 2, 2), None, (8, 8))
    assert ops._CAM_TAP[0] is None
    with pytest.raises(ZeroDivisionError):
        with ops.cam_tap(3) as tap:
            assert ops._CAM_TAP[0] is tap
            1 / 0
    assert ops._CAM_TAP[0] is None


def test_tap_split_names_what_went_wrong():
    from litemkd_amd import ops
    tap = ops.CamTap(6)
    tap.leaves.append(torch.zeros(9, 2, 2, 8))
    s, q = tap.split()
    assert s.shape[0] == 6 and q.shape[0] == 3
    tap = ops.CamTap(6)
    tap.leaves.append(torch.zeros(6, 2, 2, 8))          # the support frames alone: not a backbone that pools elsewhere
    with pytest.raises(RuntimeError, match="no query frames"):
        tap.split()
    with pytest.raises(RuntimeError, match="0 maps reached the pooled head"):
        ops.CamTap(6).split()
    tap = ops.CamTap(6)
    tap.leaves += [torch.zeros(5, 2, 2, 8), torch.zeros(3, 2, 2, 8)]
    with pytest.raises(RuntimeError, match="holds 5 frames, the support set 6"):
        tap.split()


def test_module_k_block_touches_these_modules_alone_and_restores():
    from litemkd_amd import ops
    net = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Sequential(torch.nn.Linear(4, 4)))
    other = torch.nn.Linear(4, 4)
    net[0].gemm_k_block = 64          # a module that carries its own, as the MFM teacher's head does
    with pytest.raises(RuntimeError, match="boom"):
        with ops.module_k_block(net, 128):
            assert all(m.gemm_k_block == 128 for m in net.modules()) and "gemm_k_block" not in other.__dict__
            raise RuntimeError("boom")
    assert net[0].gemm_k_block == 64
    assert ["gemm_k_block" in m.__dict__ for m in net.modules()] == [False, True, False, False]
    assert not hasattr(ops, "GEMM_K_BLOCK")          # no process-wide default: gemm() sums in blocks only where the call says so
