"""Writes tests/golden/strm.npz and tests/golden/strm_keys.json from the reference's own STRM modules (runs only where the reference
tree exists; nothing of it is stored but numbers and names).

    python tools/gen_strm_golden.py [--reference /path/to/Lite-MKD]

The reference's model/backbone/strm18_student.py, strmbackbone.py and model/classifiers/strm_res18_sup.py, strmclassifiers.py,
strmclassifiers_res18.py are imported as they are, with the two test-only shims oracle/gen_golden.py describes: a stub
`torchvision.models` whose resnet18().children()[:-2] is an identity (so the 'frames' handed to the backbone ARE trunk output maps
[F,512,7,7]) and `Tensor.cuda = identity` for the tuple-index tensors.  Parameters and inputs are NOT stored: tests/_strm_ref.py
generates them from a seed (make_backbone_params / make_classifier_params / make_fmaps), here they are loaded into the reference
modules with load_state_dict.  attn_pat.gamma is 0.3 (its initial 0 would hide the attention path).  Eval mode: dropout off.

strm.npz, per case c (`c<c>_`): seed, way, shot, query, the reference's logit tensors, 64-wide chunk sums of the gradient of
_strm_ref.fixture_loss(logits) with respect to the support / query maps (NHWC order), and chunk sums of the inputs themselves (so a test
can tell a changed random stream from a wrong result).  strm_keys.json: the reference's state_dict keys and shapes beyond the trunk, and
parameter counts, of the two backbones and the three classifiers."""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _strm_ref as R  # noqa: E402
from oracle.gen_golden import REF  # noqa: E402  (where the oracle's own generator looks for the reference tree)

CASES = [      # the reference's SupportDK is written for 5 classes (strm_res18_sup.py:277-283)
    # (seed, backbone module / class, classifier module, class name, way, shot, query per class)
    (11, "strm18_student", "strm_res18_sup", "strmclassifiers_resnet18_sup", 5, 2, 1),
    (12, "strmbackbone", "strmclassifiers_res18", "strmclassifiers_resnet18", 3, 2, 1),
    (13, "strmbackbone", "strmclassifiers", "strmclassifiers", 2, 1, 2),
]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def shims(ref):
    import torch.nn as nn
    sys.path.insert(0, ref)
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.models"] = tv.models

    class _StubResNet(nn.Module):
        def __init__(self):
            super().__init__()
            self.trunk = nn.Identity()
            self.avgpool = nn.Identity()
            self.fc = nn.Identity()
    tv.models.resnet18 = lambda pretrained=True: _StubResNet()
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.modules["utils"] = _load("utils", os.path.join(ref, "utils.py"))


def ref_args(way, shot, query):
    return argparse.Namespace(way=way, shot=shot, query_per_class=query, seq_len=8, trans_linear_out_dim=1152, trans_linear_in_dim=2048,
                              trans_dropout=0.1, num_gpus=1, device=torch.device("cpu"), temp_set=[2])


def keys_of(module, skip=("resnet.",)):
    sd = module.state_dict()
    keys = {k: list(v.shape) for k, v in sd.items() if not k.startswith(skip)}
    n = sum(p.numel() for k, p in module.named_parameters() if not k.startswith(skip))
    return {"state_dict": keys, "parameters": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("LMKD_REFERENCE", REF))
    a = ap.parse_args()
    ref = a.reference
    if not os.path.isdir(ref):
        raise SystemExit("reference tree not found at %s" % ref)
    shims(ref)
    out, keys = {}, {}
    for c, (seed, bb, cm, cc, way, shot, query) in enumerate(CASES):
        args = ref_args(way, shot, query)
        bmod = _load("ref_" + bb, os.path.join(ref, "model/backbone/%s.py" % bb))
        cmod = _load("ref_" + cm, os.path.join(ref, "model/classifiers/%s.py" % cm))
        backbone, clf = getattr(bmod, bb)(args), getattr(cmod, cc)(args)
        keys[bb] = keys_of(backbone)
        keys[cc] = keys_of(clf)
        bp, cp = R.make_backbone_params(seed, bb), R.make_classifier_params(seed)
        missing = backbone.load_state_dict(bp, strict=True)
        clf.load_state_dict(cp, strict=True)
        assert not missing.missing_keys
        backbone.eval()
        clf.eval()
        ns, nq = way * shot, way * query
        fm = R.make_fmaps(seed, (ns + nq) * 8)
        labels = torch.arange(way).repeat_interleave(shot).float()
        fs = fm[:ns * 8].permute(0, 3, 1, 2).contiguous().requires_grad_()      # the reference reads NCHW
        fq = fm[ns * 8:].permute(0, 3, 1, 2).contiguous().requires_grad_()
        cf, tf = backbone(fs, labels, fq)
        logits = clf(cf, labels, tf)["logits"]
        R.fixture_loss(logits).backward()
        pre = "c%d_" % c
        out[pre + "seed"], out[pre + "way"], out[pre + "shot"], out[pre + "query"] = seed, way, shot, query
        out[pre + "backbone"] = np.array(bb)
        for k, v in logits.items():
            out[pre + "logits_" + k] = v.detach().numpy()
        out[pre + "g_support"] = R.gsum(fs.grad.permute(0, 2, 3, 1).contiguous()).numpy()
        out[pre + "g_query"] = R.gsum(fq.grad.permute(0, 2, 3, 1).contiguous()).numpy()
        out[pre + "in_digest"] = R.gsum(fm).numpy()[::64].copy()
        print("case %d %s / %s: %s" % (c, bb, cc, {k: tuple(v.shape) for k, v in logits.items()}))
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "strm.npz"), **out)
    with open(os.path.join(gold, "strm_keys.json"), "w") as f:
        json.dump(keys, f, indent=1, sort_keys=True)
        f.write("\n")
    for n in ("strm.npz", "strm_keys.json"):
        print(n, os.path.getsize(os.path.join(gold, n)), "bytes")


if __name__ == "__main__":
    main()
