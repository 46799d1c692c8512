"""Writes tests/golden/mfm_train.npz from the reference's own ThreeTRXShiftLoopTime.forward (teacher/code/model.py:1597-1636; eval mode,
autograd on) at width 2048, trans_num 1, on the seeded case of tests/_mfm_train_ref.py (WT: 7 support videos with ragged, unsorted labels
and a class without support, 4 queries; weights oracle.make_mfm_params(77, num_layers=1) and _trx_card_ref.make_params for the head).
Needs the reference tree; the tests read only the fixture.

The fixture holds numbers only: the logits and, per parameter gradient of sum(w o logits), its norm ("n:"), its largest magnitude ("m:")
and a fixed strided sample of at most 256 entries ("s:"); beside each compared figure the deviation of the fp32 restatement from the
reference ("e:"), from which _mfm_train_ref.fixture_bounds takes the bound - 3 x that deviation, never below 3e-6 of the tensor's largest
magnitude (of its norm, for the norm); and "dv_max", the largest |dV| of the head, for the absolute floor of the value bias whose
gradient is 0 in exact arithmetic.  Asserts that the reference's gradients are non-zero and prints every bound."""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mfm_train_ref as R  # noqa: E402
from oracle.gen_golden import REF, load_reference, load_reference_teacher  # noqa: E402


def reference_run(T):
    W = R.WT
    args = argparse.Namespace(seq_len=W["seq_len"], trans_num=W["num_layers"], shirt_num=W["shirt_num"], num_gpus=1, temp_set=W["temp_set"],
                              trans_linear_in_dim=2048, trans_linear_out_dim=W["out_dim"], trans_dropout=0.1, way=W["way"], m1="rgb",
                              m2="depth", m3="flow")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = T.ThreeTRXShiftLoopTime(args).eval()
    p = R.teacher_params()
    assert sorted(model.state_dict()) == sorted(p), "the reference's state-dict keys differ from _mfm_train_ref.teacher_params()"
    model.load_state_dict(p, strict=True)
    ctx, labels, tgt = R.teacher_inputs()
    names = ("rgb", "depth", "flow")
    dv_max = []
    model.bracnch.transformers[0].v_linear.register_full_backward_hook(lambda m, gi, go: dv_max.append(float(go[0].abs().max())))
    logits = model(dict(zip(names, ctx)), labels, dict(zip(names, tgt)))["logits"]
    logits = logits.reshape(W["n_query"], W["way"])
    (logits * R.teacher_weights()).sum().backward()
    grads = {}
    for k, v in model.named_parameters():
        if R.trainable(k):
            assert v.grad is not None and bool(torch.isfinite(v.grad).all()), k
            grads[k] = v.grad
        else:
            assert v.grad is None, k
    return logits.detach(), grads, max(dv_max)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not found at %s" % REF)
    load_reference()
    T = load_reference_teacher()
    logits, grads, dv_max = reference_run(T)
    ref = R.digest(logits, grads)
    r32, r64 = R.restated_teacher(torch.float32), R.restated_teacher(torch.float64)
    # which gradients are 0 in exact arithmetic: the fp64 restatement tells (the reference's fp32 holds the rounding of its sums there)
    top = max(float(r64["n:" + k]) for k in grads)
    zero = [k for k in grads if float(r64["n:" + k]) < 1e-9 * top]
    print("logits %.3f .. %.3f; gradients that are 0 in exact arithmetic: %s (the reference holds %s)"
          % (float(logits.min()), float(logits.max()), zero, ["%.2e" % float(grads[k].norm()) for k in zero]))
    assert zero == [k for k in grads if k.endswith("v_linear.bias")], zero
    assert all(float(g.norm()) > 1e-6 * top for k, g in grads.items() if k not in zero), "a reference gradient is zero"
    out = {k: v.numpy().astype(np.float64) for k, v in ref.items()}
    out["dv_max"] = np.array([dv_max])
    e32, e64 = R.digest_errors(r32, ref), R.digest_errors(r64, ref)
    for k, e in e32.items():
        out["e:" + k] = np.array([e])
    path = os.path.join(ROOT, "tests", "golden", "mfm_train.npz")
    np.savez_compressed(path, **out)
    G = np.load(path)
    bounds = R.fixture_bounds(G)
    for k in sorted(bounds):
        scale = float(np.abs(G["logits"]).max()) if k == "logits" else float(G[("n:" if k[:2] == "n:" else "m:") + k[2:]][0])
        print("%-74s fp32 restatement - reference %.2e | fp64 restatement - reference %.2e | scale %.3e | bound %.2e"
              % (k, e32[k], e64[k], scale, bounds[k]))
    print(path, os.path.getsize(path), "bytes,", len(G.files), "arrays")
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
