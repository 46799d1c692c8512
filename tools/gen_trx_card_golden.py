"""Writes tests/golden/trx_card.npz from the reference's own modules (runs only where the reference tree exists; nothing of it is stored
but numbers).

    python tools/gen_trx_card_golden.py

Cases (tests/_trx_card_ref.CASES): a head of several cardinalities is the reference's teacher head TrxBranch (teacher/code/model.py:
1094-1128, one TemporalCrossTransformer per entry of args.temp_set, logits averaged); a single cardinality 3 is
model/classifiers/TRX.py's TemporalCrossTransformer(args, 3).  Both are imported as they are through oracle.gen_golden's
load_reference() / load_reference_teacher().  Parameters and inputs are NOT stored: tests/_trx_card_ref.py generates them from a seed,
here they are loaded with load_state_dict.  Eval mode: dropout off.

trx_card.npz, per case c (`c<c>_`): the logits, 64-wide chunk sums of the gradients of _trx_card_ref.fixture_loss(logits) with respect
to the support and query features, per cardinality i the parameter gradients (`g<i>_kb`, `g<i>_vb`, `g<i>_nkw`, `g<i>_nkb`, row sums
of the two weight gradients), and chunk sums of the inputs (so a test can tell a changed random stream from a wrong result)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _trx_card_ref as R  # noqa: E402
from oracle.gen_golden import REF, _load, load_reference, load_reference_teacher  # noqa: E402


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not found at %s" % REF)
    load_reference()
    teacher = load_reference_teacher()
    trx = _load("ref_TRX", os.path.join(REF, "model/classifiers/TRX.py"))
    out = {}
    for c in range(len(R.CASES)):
        way, L, ts, params, sup, lab, qry = R.case_data(c)
        args = argparse.Namespace(way=way, shot=1, query_per_class=1, seq_len=L, trans_linear_out_dim=R.OUT_DIM, trans_linear_in_dim=R.IN_DIM,
                                  trans_dropout=0.1, num_gpus=1, temp_set=ts)
        sup.requires_grad_()
        qry.requires_grad_()
        if len(ts) > 1:
            head = teacher.TrxBranch(args).eval()
            mods = list(head.transformers)
            for m, p in zip(mods, params):
                m.load_state_dict(p, strict=True)
            logits = head(sup, qry, lab)["logits"].reshape(qry.shape[0], way)
        else:
            m = trx.TemporalCrossTransformer(args, ts[0]).eval()
            m.load_state_dict(params[0], strict=True)
            mods = [m]
            logits = m(sup, lab, qry)["logits"]
        R.fixture_loss(logits).backward()
        pre = "c%d_" % c
        out[pre + "logits"] = logits.detach().numpy()
        out[pre + "g_support"] = R.gsum(sup.grad).numpy()
        out[pre + "g_query"] = R.gsum(qry.grad).numpy()
        out[pre + "in_digest"] = R.gsum(torch.cat([sup.detach().reshape(-1), qry.detach().reshape(-1)])).numpy()[::64].copy()
        for i, m in enumerate(mods):
            g = pre + "g%d_" % i
            out[g + "kb"], out[g + "vb"] = m.k_linear.bias.grad.numpy(), m.v_linear.bias.grad.numpy()
            out[g + "nkw"], out[g + "nkb"] = m.norm_k.weight.grad.numpy(), m.norm_k.bias.grad.numpy()
            out[g + "kw_sum"], out[g + "vw_sum"] = m.k_linear.weight.grad.sum(1).numpy(), m.v_linear.weight.grad.sum(1).numpy()
            assert tuple(m.k_linear.weight.shape) == (R.OUT_DIM, R.IN_DIM * ts[i]) and m.tuples_len == len(R.frame_tuples(L, ts[i]))
        # the restatement against the module it restates, fp32 and fp64
        with torch.no_grad():
            r32 = R.head_logits(sup.detach(), lab, qry.detach(), params, way, L, ts)
            r64 = R.head_logits(sup.detach().double(), lab, qry.detach().double(), [R.cast(p, torch.float64) for p in params], way, L, ts)
        print("case %d temp_set %s: logits %s max |logit| %.1f | restatement fp32 - reference %.2e | fp64 - reference %.2e"
              % (c, ts, tuple(logits.shape), float(logits.abs().max()), float((r32 - logits).abs().max()), float((r64 - logits.double()).abs().max())))
    path = os.path.join(ROOT, "tests", "golden", "trx_card.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
