"""Writes tests/golden/otam.npz from the reference's own CNN_OTAM (teacher/code/model.py:3260-3343), imported as it is through
oracle.gen_golden's load_reference() / load_reference_teacher().  Runs only where the reference tree exists; nothing of it is stored
but numbers.

    python tools/gen_otam_golden.py

Inputs are NOT stored: tests/_otam_ref.py generates them from a seed.  Only the cases in _otam_ref.FIXTURE_CASES are written: those
for which the reference itself is finite (seq_len <= 8; it evaluates the soft minimum as -0.1 log sum exp(-a / 0.1) and underflows to
inf once a cumulative distance passes about 10.4).  For the other cases the tool prints what the reference returns.

otam.npz, per case c (`c<c>_`): the logits (probabilities), cum [Nq, Ns] (recomputed from the reference's cos_sim / OTAM_cum_dist,
CNN_OTAM does not return it), 64-wide chunk sums of the gradients of _otam_ref.fixture_loss(logits) with respect to the support and
query features, and a digest of the inputs (so a test can tell a changed random stream from a wrong result)."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _otam_ref as R  # noqa: E402
from oracle.gen_golden import REF, load_reference, load_reference_teacher  # noqa: E402


def reference_cum(T, sup, qry):
    Nq, Ns = qry.shape[0], sup.shape[0]
    L = sup.shape[1]
    d = 1 - T.cos_sim(qry.reshape(Nq * L, -1), sup.reshape(Ns * L, -1))
    d = d.reshape(Nq, L, Ns, L).permute(0, 2, 1, 3)
    return T.OTAM_cum_dist(d) + T.OTAM_cum_dist(d.transpose(-1, -2))


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not found at %s" % REF)
    load_reference()
    T = load_reference_teacher()
    warnings.simplefilter("ignore")      # F.softmax without dim, as the reference calls it
    head = T.CNN_OTAM()
    out = {}
    for c in range(len(R.CASES)):
        way, L, sup, lab, qry = R.case_data(c)
        s, q = sup.clone().requires_grad_(), qry.clone().requires_grad_()
        logits = head(s, lab, q)["logits"]
        with torch.no_grad():
            cum = reference_cum(T, sup, qry)
        if c not in R.FIXTURE_CASES:
            r32 = R.run(c, torch.float32, loss=False)
            print("case %d L %d: reference cum finite: %s, logits finite: %s | restatement fp32 finite: %s" % (
                c, L, bool(torch.isfinite(cum).all()), bool(torch.isfinite(logits).all()), bool(torch.isfinite(r32["cum"]).all())))
            continue
        R.fixture_loss(logits).backward()
        assert all(bool(torch.isfinite(t).all()) for t in (logits, cum, s.grad, q.grad)), "case %d: the reference is not finite" % c
        assert tuple(logits.shape) == (qry.shape[0], way)
        pre = "c%d_" % c
        out[pre + "logits"] = logits.detach().numpy()
        out[pre + "cum"] = cum.numpy()
        out[pre + "g_support"] = R.gsum(s.grad).numpy()
        out[pre + "g_query"] = R.gsum(q.grad).numpy()
        out[pre + "in_digest"] = R.gsum(torch.cat([sup.reshape(-1), qry.reshape(-1)])).numpy()[::64].copy()
        r32, r64 = R.run(c, torch.float32), R.run(c, torch.float64)
        dev = lambda a, b: float((a.double() - b.double()).abs().max())      # noqa: E731
        print("case %d L %d D %d: cum %.2f .. %.2f | reference - fp64 restatement: cum %.2e logits %.2e | fp32 restatement - fp64: cum %.2e "
              "logits %.2e | gradient chunk sums, reference - fp64: %.2e of %.2e" % (
                  c, L, sup.shape[2], float(cum.min()), float(cum.max()), dev(cum, r64["cum"]), dev(logits.detach(), r64["logits"]),
                  dev(r32["cum"], r64["cum"]), dev(r32["logits"], r64["logits"]),
                  max(dev(R.gsum(s.grad), R.gsum(r64["g_support"])), dev(R.gsum(q.grad), R.gsum(r64["g_query"]))),
                  max(float(R.gsum(r64["g_support"]).abs().max()), float(R.gsum(r64["g_query"]).abs().max()))))
    path = os.path.join(ROOT, "tests", "golden", "otam.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
