"""Writes tests/golden/ctx.npz from the reference's own CrossTransformer (teacher/code/model.py:2840-2936), imported as it is through
oracle.gen_golden's load_reference() / load_reference_teacher().  Runs only where the reference tree exists; nothing of it is stored
but numbers.

    python tools/gen_ctx_golden.py

Inputs and parameters are NOT stored: tests/_ctx_ref.py generates them from a seed and this tool copies the parameters into the
reference module (trans_dropout 0).  Only the cases in _ctx_ref.FIXTURE_CASES are written (the reference's Linear is 2048 wide).

ctx.npz, per case c (`c<c>_`): the logits, 64-wide chunk sums of the gradients of _ctx_ref.fixture_loss(logits) with respect to the
support and query features and the six parameters the head applies, and a digest of the inputs.  The tool asserts that the reference is
finite on every fixture case, prints how far the fp32 and fp64 restatements are from it, and prints the FIXTURE_BOUNDS literal that
tests/_ctx_ref.py carries: 3 x the fp32 restatement's deviation, not below 3e-6 of the largest |value| of the reference's tensor
(of the gradient itself, not of its chunk sums, which cancel where a gradient sums to zero along D; g_bv, which is 0 in exact
arithmetic, takes the rounding of its own column sums as the floor - see main())."""
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _ctx_ref as R  # noqa: E402
from oracle.gen_golden import REF, load_reference, load_reference_teacher  # noqa: E402


def reference_run(T, case):
    d = R.case_data(case)
    Dk, Din = d["wk"].shape
    assert Din == 2048, "the reference's CrossTransformer is 2048 wide"
    args = types.SimpleNamespace(seq_len=d["L"], trans_dropout=0.0, trans_linear_out_dim=Dk, way=d["way"])
    head = T.CrossTransformer(args)
    assert float((head.pe.pe[0] - d["pe"]).abs().max()) == 0.0
    with torch.no_grad():
        for mod, w, b in ((head.k_linear, "wk", "bk"), (head.v_linear, "wv", "bv"), (head.norm_k, "gamma", "beta")):
            mod.weight.copy_(d[w])
            mod.bias.copy_(d[b])
    s, q = d["sup"].clone().requires_grad_(), d["qry"].clone().requires_grad_()
    dv_max = []
    head.v_linear.register_full_backward_hook(lambda m, gi, go: dv_max.append(float(go[0].abs().max())))
    logits = head(s, d["lab"], q)["logits"]
    R.fixture_loss(logits).backward()
    assert head.norm_v.weight.grad is None and head.norm_v.bias.grad is None
    out = {"logits": logits.detach(), "g_support": s.grad, "g_query": q.grad, "g_wk": head.k_linear.weight.grad, "g_bk": head.k_linear.bias.grad,
           "g_wv": head.v_linear.weight.grad, "g_bv": head.v_linear.bias.grad, "g_gamma": head.norm_k.weight.grad,
           "g_beta": head.norm_k.bias.grad}
    assert all(bool(torch.isfinite(v).all()) for v in out.values()), "case %d: the reference is not finite" % case
    assert tuple(out["logits"].shape) == (d["qry"].shape[0], d["way"])
    return d, out, max(dv_max)


def round_up(x):
    """x to three significant digits, never below x (a bound printed with %.2e may land under the 3 x deviation it stands for)"""
    b = float("%.2e" % x)
    if b < x:
        b = float("%.2e" % (b + 10.0 ** (math.floor(math.log10(x)) - 2)))
    assert b >= x
    return "%.2e" % b


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not found at %s" % REF)
    load_reference()
    T = load_reference_teacher()
    out, bounds = {}, []
    for c in R.FIXTURE_CASES:
        d, ref, dv_max = reference_run(T, c)
        pre = "c%d_" % c
        stored = {k: (ref[k] if k == "logits" else R.gsum(ref[k])).float() for k in R.KEYS}
        for k in R.KEYS:
            out[pre + k] = stored[k].numpy()
        out[pre + "in_digest"] = R.gsum(torch.cat([d["sup"].reshape(-1), d["qry"].reshape(-1)])).numpy()[::64].copy()
        sc = []
        R.ctx_head(d["sup"], d["lab"], d["qry"], d["way"], *(d[k] for k in ("wk", "bk", "wv", "bv", "gamma", "beta", "pe")), scores=sc)
        print("case %d L %d Dk %d: largest score %.1f, logits %.3f .. %.3f" % (c, d["L"], d["wk"].shape[0], max(float(s.max()) for s in sc),
                                                                             float(ref["logits"].min()), float(ref["logits"].max())))
        r32, r64 = R.run(c, torch.float32), R.run(c, torch.float64)
        lines = []
        for k in R.KEYS:
            e32, e64 = R.fixture_error(k, r32[k], stored[k]), R.fixture_error(k, r64[k], stored[k])
            vmax = float(ref[k].abs().max())      # of the tensor itself: chunk sums may cancel (a bias gradient sums to 0 over D)
            print("   %-9s fp32 restatement - reference %.2e | fp64 restatement - reference %.2e | largest |value| %.3e" % (k, e32, e64, vmax))
            floor = 3e-6 * vmax
            if k == "g_bv":
                # exactly 0 in exact arithmetic (every attention row sums to 1, so the value gradients of a (query, class) block cancel
                # column by column): what the reference holds is the rounding of its column sums, and 3e-6 of THAT bounds nothing - the
                # fp64 restatement, which returns 1e-16, would miss it.  The floor is the rounding of the sum itself: a 64-wide chunk sum
                # adds 64 x rows values of dV, a random walk of sqrt(64 rows) roundings of 2^-24 max |dV|, times the project's factor 3.
                rows = (d["sup"].shape[0] + d["qry"].shape[0]) * d["L"]
                vmax = dv_max
                floor = 3 * (64 * rows) ** 0.5 * 2.0 ** -24 * dv_max
            lines.append('"%s": %s,      # (%.2e, %.3e)' % (k, round_up(max(3 * e32, floor)), e32, vmax))
        bounds.append("    %d: {\n        %s\n    }," % (c, "\n        ".join(lines)))
    path = os.path.join(ROOT, "tests", "golden", "ctx.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print("FIXTURE_BOUNDS = {\n%s\n}" % "\n".join(bounds))


if __name__ == "__main__":
    main()
