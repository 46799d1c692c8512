"""MobileNetV3-Large students (moblienetv3_fc2 / moblienetv3, model/backbone/moblienetv3.py) on the host: registry, parameter counts,
state_dict keys against torchvision's features, the torchvision-weights loader, and the exported C ABI.  No GPU needed."""
import re

import pytest
import torch

import litemkd_amd  # noqa: F401
from litemkd_amd.model import model_select as ms
from litemkd_amd.options import default_args

from _mnv3_ref import feature_shapes

FEATURES = 2971952          # torchvision mobilenet_v3_large: 5,483,032 total - classifier 2,511,080
HEAD = 960 * 2048 + 2048     # one Linear(960, 2048)
TRX_2FCSUP = 9444096


def _cpu_args(**kw):
    return default_args(device=torch.device("cpu"), **kw)


def _count(m, prefix=""):
    return sum(p.numel() for n, p in m.named_parameters() if n.startswith(prefix))


def test_registry_has_both_mobilenet_students():
    assert ms.name2backbone["moblienetv3_fc2"] is not None
    assert ms.name2backbone["moblienetv3"] is not None
    for name in ("strm18_student", "strmbackbone", "meta_baseline", "meta_baseline_fc2"):
        assert ms.name2backbone[name] is None


def test_restated_features_parameter_count():
    n = 0
    for k, shp in feature_shapes().items():
        if "running" in k or "num_batches" in k:
            continue
        c = 1
        for d in shp:
            c *= d
        n += c
    assert n == FEATURES


def test_student_moblienetv3_fc2_builds_with_derived_counts():
    a = _cpu_args(model_backbone="moblienetv3_fc2", model_classifier="TRX_2fcsup")
    s = ms.Student(a)
    assert a.trans_linear_in_dim == 2048
    assert _count(s, "backbone.mobile.") == FEATURES
    assert _count(s, "backbone.fc1.") == HEAD and _count(s, "backbone.fc2.") == HEAD
    assert _count(s, "classifier.") == TRX_2FCSUP
    assert _count(s) == 16352304


def test_state_dict_keys_and_shapes_match_torchvision_features():
    s = ms.Student(_cpu_args(model_backbone="moblienetv3_fc2"))
    sd = s.state_dict()
    ref = feature_shapes()
    own = {k[len("backbone.mobile.0."):]: tuple(v.shape) for k, v in sd.items() if k.startswith("backbone.mobile.0.")}
    assert own == ref
    spot = {"0.0.weight": (16, 3, 3, 3), "1.block.0.0.weight": (16, 1, 3, 3), "4.block.2.fc1.weight": (24, 72, 1, 1),
            "16.1.running_var": (960,), "13.block.1.0.weight": (672, 1, 5, 5), "15.block.2.fc2.bias": (960,)}
    for k, shp in spot.items():
        assert tuple(sd["backbone.mobile.0." + k].shape) == shp, k
    assert not any(k.startswith("backbone.mobile.1") for k in sd)


def test_squeeze_widths():
    widths = [v[0] for k, v in feature_shapes().items() if k.endswith("fc1.weight")]
    assert widths == [24, 32, 32, 120, 168, 168, 240, 240]


def test_student_moblienetv3_single_head():
    s = ms.Student(_cpu_args(model_backbone="moblienetv3", model_classifier="TRX"))
    sd = s.state_dict()
    assert tuple(sd["backbone.fc.weight"].shape) == (2048, 960)
    assert "backbone.fc1.weight" not in sd
    assert _count(s, "backbone.") == FEATURES + HEAD


def test_initialisation_as_torchvision():
    torch.manual_seed(0)
    s = ms.Student(_cpu_args(model_backbone="moblienetv3_fc2"))
    sd = s.state_dict()
    assert torch.equal(sd["backbone.mobile.0.5.block.1.1.weight"], torch.ones(120))
    assert torch.equal(sd["backbone.mobile.0.5.block.1.1.bias"], torch.zeros(120))
    assert torch.equal(sd["backbone.mobile.0.4.block.2.fc1.bias"], torch.zeros(24))
    assert int(sd["backbone.mobile.0.16.1.num_batches_tracked"]) == 0
    w = sd["backbone.mobile.0.16.0.weight"]           # kaiming normal, fan_out = 960: std sqrt(2 / 960)
    assert abs(float(w.std()) - (2.0 / 960) ** 0.5) < 0.1 * (2.0 / 960) ** 0.5


def test_torchvision_state_dict_loads():
    from litemkd_amd.model.backbone.mobilenetv3 import load_torchvision_features
    g = torch.Generator().manual_seed(3)
    tv = {"features." + k: (torch.randn(shp, generator=g) if shp else torch.tensor(7)) for k, shp in feature_shapes().items()}
    tv["classifier.0.weight"] = torch.randn(1280, 960, generator=g)
    tv["classifier.3.bias"] = torch.randn(1000, generator=g)
    s = ms.Student(_cpu_args(model_backbone="moblienetv3_fc2"))
    fc1 = s.backbone.fc1.weight.detach().clone()
    load_torchvision_features(s.backbone, tv)
    sd = s.state_dict()
    for k in feature_shapes():
        assert torch.equal(sd["backbone.mobile.0." + k], tv["features." + k]), k
    assert torch.equal(s.backbone.fc1.weight, fc1)
    s.backbone.load_torchvision({"state_dict": tv})      # the wrapped form and the method
    with pytest.raises(KeyError):
        load_torchvision_features(s.backbone, {k: v for k, v in tv.items() if "16.1" not in k})
    bad = dict(tv)
    bad["features.1.block.0.0.weight"] = torch.zeros(16, 1, 5, 5)
    with pytest.raises(ValueError):
        load_torchvision_features(s.backbone, bad)


def test_mobilenet_prototypes_exported():
    from litemkd_amd._lib import lib, parse_header
    names = ["lmkd_mnv3_stat_tiles", "lmkd_dw_conv_fwd", "lmkd_dw_conv_bwd_data", "lmkd_dw_conv_bwd_weight_workspace", "lmkd_dw_conv_bwd_weight",
             "lmkd_col_stats", "lmkd_bn_act_fwd", "lmkd_bn_act_bwd_workspace", "lmkd_bn_act_bwd", "lmkd_se_mean", "lmkd_se_scale_fwd",
             "lmkd_se_scale_bwd", "lmkd_hardsigmoid_fwd", "lmkd_hardsigmoid_bwd", "lmkd_stem3x3_fwd", "lmkd_stem3x3_bwd_weight_workspace",
             "lmkd_stem3x3_bwd_weight"]
    protos = parse_header()
    L = lib()
    for n in names:
        assert n in protos, n
        assert getattr(L.cdll, n) is not None
    assert L.value("lmkd_abi_version") == 3
    assert L.value("lmkd_mnv3_stat_tiles", 1024) == 1 and L.value("lmkd_mnv3_stat_tiles", 1025) == 2
    # workspaces are sized without a device: 400 frames of block 2's 56 x 56 depthwise output, 4096 pixels per partial row
    assert L.value("lmkd_dw_conv_bwd_weight_workspace", 400, 112, 112, 64, 3, 2) == -(-400 * 56 * 56 // 4096) * 64 * 9 * 4
    assert L.value("lmkd_stem3x3_bwd_weight_workspace", 16, 224, 224) == -(-16 * 112 * 112 // 4096) * 432 * 4
    # argument checks run before any launch: C % 8 and the kernel size
    assert L.value("lmkd_dw_conv_fwd", None, None, None, None, 1, 8, 8, 12, 3, 1, None) != 0
    assert "C % 8" in L.last_error()
    assert L.value("lmkd_dw_conv_fwd", None, None, None, None, 1, 8, 8, 16, 7, 1, None) != 0
    hdr = open(litemkd_amd._lib.HEADER).read()
    assert re.search(r"moblienetv3\.py:\d+", hdr)


def test_bf16_activations_refused():
    from litemkd_amd import ops
    prev = ops._ACT_DTYPE[0]
    ops._ACT_DTYPE[0] = torch.bfloat16
    try:
        with pytest.raises(RuntimeError, match="fp32 activations only"):
            ops._mnv3_chk(torch.zeros(1))
    finally:
        ops._ACT_DTYPE[0] = prev
