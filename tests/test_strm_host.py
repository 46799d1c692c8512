"""STRM student family, host side (no GPU): the registry builds the students with the reference's parameters and state_dict keys,
the plain-torch restatement tests/_strm_ref.py reproduces the reference's own outputs (tests/golden/strm.npz, written by
tools/gen_strm_golden.py), and the built library exports the new entry points."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _strm_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CPU = torch.device("cpu")


def _args(**kw):
    from litemkd_amd.options import default_args
    return default_args(device=CPU, **kw)


def _keys():
    with open(os.path.join(GOLD, "strm_keys.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("backbone,classifier,cls_name", [
    ("strm18_student", "strm_res18_sup", "strmclassifiers_resnet18_sup"),
    ("strmbackbone", "strmclassifiers", "strmclassifiers"),
    ("strmbackbone", "strm_res18", "strmclassifiers_resnet18"),
])
def test_student_builds_with_reference_keys(backbone, classifier, cls_name):
    from litemkd_amd.model.model_select import Student
    ref = _keys()
    s = Student(_args(model_backbone=backbone, model_classifier=classifier))
    assert type(s.backbone).__name__ == backbone and type(s.classifier).__name__ == cls_name
    for part, name in ((s.backbone, backbone), (s.classifier, cls_name)):
        own = {k: list(v.shape) for k, v in part.state_dict().items() if not k.startswith("resnet.")}
        assert own == ref[name]["state_dict"], sorted(set(own) ^ set(ref[name]["state_dict"]))
        assert list(own) == [k for k in part.state_dict() if not k.startswith("resnet.")]
        n = sum(p.numel() for k, p in part.named_parameters() if not k.startswith("resnet."))
        assert n == ref[name]["parameters"]
    assert float(s.backbone.attn_pat.gamma.detach()) == 0.0      # reference initialisation
    assert s.backbone.distribute_model() is None


def test_reference_counts_of_the_issue():
    ref = _keys()
    assert ref["strm18_student"]["parameters"] == 18952849 and len(ref["strm18_student"]["state_dict"]) == 29
    assert ref["strmclassifiers_resnet18_sup"]["parameters"] == 13639424
    assert sorted(ref["strmclassifiers_resnet18_sup"]["state_dict"]) == sorted(
        ["transformers." + k for k in ("pe.pe", "k_linear.weight", "k_linear.bias", "v_linear.weight", "v_linear.bias", "norm_k.weight",
                                       "norm_k.bias", "norm_v.weight", "norm_v.bias")] + ["DistanceLoss.clsW.weight", "DistanceLoss.clsW.bias"])
    assert ref["strm18_student"]["state_dict"]["attn_pat.pe.pe"] == [1, 24, 512]
    assert ref["strm18_student"]["state_dict"]["fr_enrich.pe.pe"] == [1, 12, 2048]
    assert ref["strmbackbone"]["state_dict"]["fc1.weight"] == [2048, 512]


@pytest.mark.parametrize("backbone,classifier", [
    ("strmbackbone", "TRX_2fcsup"), ("strm18_student", "TRX_2fcsup"), ("strm18_student", "strmclassifiers"), ("strmbackbone", "strm_res18_sup"),
    ("resnet18_2fc", "strm_res18_sup"), ("resnet18_2fc", "strmclassifiers"), ("moblienetv3_fc2", "strm_res18"),
    ("meta_baseline", "TRX_2fcsup"), ("meta_baseline_fc2", "strm_res18_sup"), ("strm18_student", "strm_1fc_sup"), ("resnet18_2fc", "strm_1fc_sup"),
])
def test_other_pairings_still_raise(backbone, classifier):
    from litemkd_amd.model.model_select import Student
    with pytest.raises(NotImplementedError) as e:
        Student(_args(model_backbone=backbone, model_classifier=classifier))
    assert backbone in str(e.value) or classifier in str(e.value)


def test_mismatched_pairing_names_both_plugins():
    from litemkd_amd.model.model_select import select_model_student
    with pytest.raises(NotImplementedError) as e:
        select_model_student(_args(model_backbone="strmbackbone", model_classifier="TRX_2fcsup"))
    assert "strmbackbone" in str(e.value) and "TRX_2fcsup" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        select_model_student(_args(model_backbone="resnet18_2fc", model_classifier="strm_res18"))
    assert "resnet18_2fc" in str(e.value) and "strm_res18" in str(e.value)


def _case(G, c):
    pre = "c%d_" % c
    seed, way, shot, query = (int(G[pre + k]) for k in ("seed", "way", "shot", "query"))
    backbone = str(G[pre + "backbone"])
    ns, nq = way * shot, way * query
    fm = R.make_fmaps(seed, (ns + nq) * 8)
    np.testing.assert_allclose(R.gsum(fm).numpy()[::64], G[pre + "in_digest"], rtol=1e-6, atol=1e-6,
                               err_msg="the seeded inputs differ from the generator's: regenerate the fixture")
    labels = torch.arange(way).repeat_interleave(shot)
    logits = {k[len(pre) + 7:]: torch.from_numpy(G[k]) for k in G.files if k.startswith(pre + "logits_")}
    return pre, seed, way, shot, backbone, ns, fm, labels, logits


@pytest.mark.parametrize("case", [0, 1, 2])
def test_restatement_reproduces_the_reference(case):
    """fp64 restatement against the reference's fp32 CPU evaluation of the same graph: logits and input-gradient digests to 1e-5
    relative (relative L2 per tensor)"""
    G = np.load(os.path.join(GOLD, "strm.npz"))
    pre, seed, way, shot, backbone, ns, fm, labels, ref = _case(G, case)
    bp, cp = R.cast(R.make_backbone_params(seed, backbone), torch.float64), R.cast(R.make_classifier_params(seed), torch.float64)
    fm = fm.double().requires_grad_()
    logits, _, _ = R.head(fm, ns, labels, bp, cp, way, shot, backbone=backbone)
    assert sorted(logits) == sorted(ref)
    for k, v in ref.items():
        err = float((logits[k].detach() - v.double()).norm() / v.double().norm())
        assert err <= 1e-5, (k, err)
    R.fixture_loss(logits).backward()
    for name, g in (("g_support", fm.grad[:ns * 8]), ("g_query", fm.grad[ns * 8:])):
        want = torch.from_numpy(G[pre + name]).double()
        err = float((R.gsum(g) - want).norm() / want.norm())
        assert err <= 1e-5, (name, err)


def test_restatement_pooling_matches_torch_on_zero_windows():
    x = R.make_fmaps(3, 8)
    x[:, :2, :2] = 0      # whole windows of zeros: the first position wins
    vals, idx = R.patch_pool(x)
    want, widx = torch.nn.functional.adaptive_max_pool2d(x.permute(0, 3, 1, 2), (4, 4), return_indices=True)
    assert torch.equal(vals, want.permute(0, 2, 3, 1).reshape(8, 16, 512))
    assert torch.equal(idx, widx.permute(0, 2, 3, 1).reshape(8, 16, 512))
    again, _ = R.patch_pool(x, idx)
    assert torch.equal(again, vals)


def test_accuracy_combination_of_the_strm_distillers():
    """trainwandb.py:259-273: 0.2 * pat + fr1 + fr2 and 0.1 * pat + fr; logits built so that `pat` decides the argmax"""
    from litemkd_amd import trainloop as TL
    fr = torch.tensor([[1.0, 1.05], [0.0, 3.0]])
    pat = torch.tensor([[1.0, 0.0], [0.0, 0.0]])
    got = TL.strm_accuracy_logits("strm_fc_2_sup_dist", {"pat": pat, "fr1": fr, "fr2": torch.zeros(2, 2), "sup": torch.zeros(2, 1)})
    assert torch.allclose(got, 0.2 * pat + fr) and got.argmax(-1).tolist() == [0, 1] and fr.argmax(-1).tolist() == [1, 1]
    for name in ("strm", "strm_KD"):
        got = TL.strm_accuracy_logits(name, {"pat": pat, "fr": fr})
        assert torch.allclose(got, 0.1 * pat + fr) and got.argmax(-1).tolist() == [0, 1]
    assert TL.strm_accuracy_logits("fc_2_sup_dist", {"kl": fr, "ce": fr}) is None


def test_new_symbols_are_declared_and_exported():
    import litemkd_amd
    header = open(os.path.join(ROOT, "include", "lmkd.h")).read()
    names = sorted(set(re.findall(r"\b(lmkd_strm_\w+)\s*\(", header)))
    assert names == ["lmkd_strm_attn_bwd", "lmkd_strm_attn_fwd", "lmkd_strm_pair_embed", "lmkd_strm_patchdist_bwd", "lmkd_strm_patchdist_fwd",
                     "lmkd_strm_patchpool_bwd", "lmkd_strm_patchpool_fwd", "lmkd_strm_tokmlp_bwd", "lmkd_strm_tokmlp_fwd", "lmkd_strm_tokmlp_parts"]
    cdll = litemkd_amd.lib().cdll
    for n in names:
        assert hasattr(cdll, n), n


def test_bf16_activations_are_refused():
    from litemkd_amd import ops
    try:
        ops._ACT_DTYPE[0] = torch.bfloat16
        with pytest.raises(RuntimeError, match="fp32 activations only"):
            ops._strm_chk()
    finally:
        ops._ACT_DTYPE[0] = torch.float32
