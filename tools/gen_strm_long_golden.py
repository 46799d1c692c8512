"""Writes tests/golden/strm_long.npz from the reference's own, unmodified STRM modules at seq_len = 12 (runs only where the reference
tree exists; nothing of it is stored but numbers and names).

    python tools/gen_strm_long_golden.py [--reference /path/to/Lite-MKD]

The shims, the three cases and the stored quantities are those of tools/gen_strm_golden.py (imported from it): per case c (`c<c>_`) the
seed, way, shot, query, the reference's logit tensors, 64-wide chunk sums of the gradient of _strm_ref.fixture_loss(logits) with respect
to the support / query maps, and chunk sums of the inputs.  Added here: `seq_len`, and `keys_json` - the state_dict keys and shapes beyond
the trunk, and the parameter counts, of the two backbones and three classifiers built at 12 frames (a JSON string, the layout of
tests/golden/strm_keys.json).  Parameters and inputs come from tests/_strm_ref.py's seeded generators at seq_len = 12."""
import argparse
import json
import os

import numpy as np
import torch

import gen_strm_golden as G8
from gen_strm_golden import R, REF, ROOT

SEQ_LEN = 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("LMKD_REFERENCE", REF))
    ref = ap.parse_args().reference
    if not os.path.isdir(ref):
        raise SystemExit("reference tree not found at %s" % ref)
    G8.shims(ref)
    out, keys = {"seq_len": SEQ_LEN}, {}
    for c, (seed, bb, cm, cc, way, shot, query) in enumerate(G8.CASES):
        args = G8.ref_args(way, shot, query)
        args.seq_len = SEQ_LEN
        bmod = G8._load("ref_" + bb, os.path.join(ref, "model/backbone/%s.py" % bb))
        cmod = G8._load("ref_" + cm, os.path.join(ref, "model/classifiers/%s.py" % cm))
        backbone, clf = getattr(bmod, bb)(args), getattr(cmod, cc)(args)
        keys[bb] = G8.keys_of(backbone)
        keys[cc] = G8.keys_of(clf)
        backbone.load_state_dict(R.make_backbone_params(seed, bb, seq_len=SEQ_LEN), strict=True)
        clf.load_state_dict(R.make_classifier_params(seed, seq_len=SEQ_LEN), strict=True)
        backbone.eval()
        clf.eval()
        ns, nq = way * shot, way * query
        fm = R.make_fmaps(seed, (ns + nq) * SEQ_LEN)
        labels = torch.arange(way).repeat_interleave(shot).float()
        fs = fm[:ns * SEQ_LEN].permute(0, 3, 1, 2).contiguous().requires_grad_()      # the reference reads NCHW
        fq = fm[ns * SEQ_LEN:].permute(0, 3, 1, 2).contiguous().requires_grad_()
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
    out["keys_json"] = np.array(json.dumps(keys, sort_keys=True))
    path = os.path.join(ROOT, "tests", "golden", "strm_long.npz")
    np.savez_compressed(path, **out)
    print("strm_long.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
