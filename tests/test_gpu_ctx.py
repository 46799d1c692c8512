"""GPU: the CTX matcher head (csrc/ctx.hip) against its fp64 restatement tests/_ctx_ref.py by the project's anchored
criterion - HIP vs fp64 at most 3 x (the fp32 restatement on the CPU vs fp64) + 2e-6, for the logits, both feature gradients and the six
parameter gradients - in the library's default GEMM mode and in the native fp32 mode, at the smallest shapes that reach each path; against
the reference's own numbers (tests/golden/ctx.npz) within _ctx_ref.FIXTURE_BOUNDS; determinism, unwritten outputs, dropout, CTX_fixed,
norm_v."""
import functools
import os

import numpy as np
import pytest
import torch

import _anchor
import _ctx_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GEMM_MODES = {"default": -1, "native_fp32": 0}
ARGS = ("wk", "bk", "wv", "bv", "gamma", "beta")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _cpu(case):
    """the restatement in fp32 and fp64, computed once per case and left unchanged"""
    return R.run(case, torch.float32), R.run(case, torch.float64)


def _plan(dev, d):
    from litemkd_amd import ops
    return ops.ClassPlan(d["lab"].to(dev), d["way"], cpu_copy=d["lab"])


def _hip(dev, case, gemm_mode=-1, mask=None):
    """CtxLogitsFn forward + backward of _ctx_ref.fixture_loss -> dict like _ctx_ref.run, on the CPU"""
    import litemkd_amd
    from litemkd_amd import ops
    d = R.case_data(case)
    s, q = d["sup"].to(dev).requires_grad_(), d["qry"].to(dev).requires_grad_()
    P = {k: d[k].to(dev).requires_grad_() for k in ARGS}
    pe = d["pe"][:d["L"]].contiguous().to(dev)
    lib = litemkd_amd.lib()
    lib.call("lmkd_gemm_set_mode", gemm_mode)
    try:
        logits = ops.CtxLogitsFn.apply(s, q, *(P[k] for k in ARGS), pe, mask, _plan(dev, d))
        R.fixture_loss(logits).backward()
        torch.cuda.synchronize()
    finally:
        lib.call("lmkd_gemm_set_mode", -1)
    out = {"logits": logits.detach().cpu(), "g_support": s.grad.cpu(), "g_query": q.grad.cpu()}
    out.update({"g_" + k: P[k].grad.cpu() for k in ARGS})
    return out


def _check_anchored(tag, out, r32, r64):
    pairs = {}
    for k in R.KEYS:
        assert bool(torch.isfinite(out[k]).all()), k
        assert out[k].shape == r64[k].shape, k
        pairs[k] = (_anchor.rel_l2(out[k], r64[k]), _anchor.rel_l2(r32[k], r64[k]))
        print("%s %-9s HIP vs fp64 %.3e | CPU fp32 vs fp64 %.3e" % (tag, k, pairs[k][0], pairs[k][1]))
    _anchor.record(tag, pairs)
    _anchor.anchored("logits", out["logits"], r32["logits"], r64["logits"])
    _anchor.anchored_dict({k: out[k] for k in R.GRAD_KEYS}, {k: r32[k] for k in R.GRAD_KEYS}, {k: r64[k] for k in R.GRAD_KEYS})


@pytest.mark.parametrize("mode", list(GEMM_MODES))
@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_head_is_anchored_to_fp64(dev, case, mode):
    r32, r64 = _cpu(case)
    out = _hip(dev, case, GEMM_MODES[mode])
    c = R.CASES[case]
    _check_anchored("ctx case %d L %d Din %d Dk %d gemm %s" % (case, c[4], c[5], c[6], mode), out, r32, r64)
    missing = sorted(set(range(c[1])) - set(c[2]))
    for m in missing:
        assert float(out["logits"][:, m].abs().max()) == 0.0


@pytest.mark.parametrize("mode", list(GEMM_MODES))
@pytest.mark.parametrize("case", list(R.FIXTURE_CASES))
def test_head_reproduces_the_reference(dev, case, mode):
    """the reference's own CrossTransformer, within the bounds its fp32 restatement sets on the CPU (_ctx_ref.FIXTURE_BOUNDS): those
    bounds as they stand in the library's default GEMM mode, whose three-plane products are below fp32 rounding.  In the native fp32
    MFMA mode the projections, and every tensor downstream of them, also carry what lmkd_gemm_f32 is held to in every mode, 2e-6 relative
    (test_gpu_ops.py::test_gemm_on_the_bf16_pipe): 2e-6 of the tensor's largest |value| on a logit, and sqrt(64) times that on a 64-wide
    chunk sum of mixed-sign gradient elements.  (Against the CPU-derived bounds alone the first GPU run of that mode missed two of its 27
    figures: case 2 g_wk 1.49e-4 against 1.26e-4, case 7 g_beta 1.70e-6 against 1.27e-6; the default mode met all 27.)"""
    G = np.load(os.path.join(GOLD, "ctx.npz"))
    out = _hip(dev, case, GEMM_MODES[mode])
    errs = {k: R.fixture_error(k, out[k], G["c%d_%s" % (case, k)]) for k in R.KEYS}
    bounds = dict(R.FIXTURE_BOUNDS[case])
    if mode == "native_fp32":
        for k in R.KEYS:
            bounds[k] += (1.0 if k == "logits" else 8.0) * 2e-6 * float(out[k].abs().max())
    for k in R.KEYS:
        print("case %d %s %-9s err %.2e bound %.2e" % (case, mode, k, errs[k], bounds[k]))
    for k in R.KEYS:
        assert errs[k] <= bounds[k], (k, errs[k], bounds[k])


@pytest.mark.parametrize("case", [1, 8])
def test_two_calls_are_bit_identical(dev, case):
    a, b = _hip(dev, case), _hip(dev, case)
    for k in R.KEYS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("case", [1, 2, 5, 6])      # ragged unsorted; a class without support; partial D tiles; the frames-per-class limit
def test_every_output_element_is_written(dev, case):
    """the entry points on NaN-filled outputs: an element a kernel leaves out shows; the results equal CtxLogitsFn's bit for bit"""
    import litemkd_amd
    from litemkd_amd import ops
    lib = litemkd_amd.lib()
    d = R.case_data(case)
    Ns, L, Din = d["sup"].shape
    Nq, way, D = d["qry"].shape[0], d["way"], d["wk"].shape[0]
    rows = (Ns + Nq) * L
    plan = _plan(dev, d)
    nseg, off, cnt, col = ops._ctx_layout(plan, Ns, L)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)      # noqa: E731
    P = {k: d[k].to(dev) for k in ARGS}
    p, st = ops._p, ops._stream()
    X = torch.cat([d["sup"].reshape(Ns * L, Din), d["qry"].reshape(Nq * L, Din)]).to(dev)
    Xp, pe = nan(rows, Din), d["pe"][:L].contiguous().to(dev)
    lib.call("lmkd_add_pe", p(X), p(pe), None, p(Xp), rows, Din, L, st)
    Kraw, V = nan(rows, D), nan(rows, D)
    ops.gemm("K", "K", rows, D, Din, Xp, Din, P["wk"], Din, Kraw, D, bias=P["bk"])
    ops.gemm("K", "K", rows, D, Din, Xp, Din, P["wv"], Din, V, D, bias=P["bv"])
    Kn, Khat, rstd = nan(rows, D), nan(rows, D), nan(rows)
    lib.call("lmkd_ctx_ln_fwd", p(Kraw), p(P["gamma"]), p(P["beta"]), p(Kn), p(Khat), p(rstd), rows, D, ops._f32(1e-5), st)
    A, logits = nan(Nq * L, Ns * L), nan(Nq, way)
    lib.call("lmkd_ctx_attend_fwd", p(Kn), p(V), p(plan.order), p(A), p(logits), Ns, Nq, way, L, D, nseg, off, cnt, col, st)
    g = R.fixture_weights((Nq, way)).to(dev)
    dS, E, dK, dV = nan(Nq * L, Ns * L), nan(nseg * Nq * L, D), nan(rows, D), nan(rows, D)
    lib.call("lmkd_ctx_attend_bwd", p(g), p(Kn), p(V), p(plan.order), p(A), p(dS), p(E), p(dK), p(dV), Ns, Nq, way, L, D, nseg, off, cnt, col, st)
    torch.cuda.synchronize()
    for name, t in (("Kn", Kn), ("Khat", Khat), ("rstd", rstd), ("A", A), ("logits", logits), ("dS", dS), ("E", E), ("dK", dK), ("dV", dV)):
        assert bool(torch.isfinite(t).all()), name
    # every attention row sums to 1 over each class's frames
    assert torch.allclose(A.sum(1), torch.full((Nq * L,), float(nseg), device=dev), atol=1e-5)
    for m in sorted(set(range(way)) - set(plan.classes)):
        assert float(logits[:, m].abs().max()) == 0.0
    out = _hip(dev, case)
    assert torch.equal(out["logits"], logits.cpu())
    # the rest of the backward as CtxLogitsFn runs it
    lib.call("lmkd_layernorm_bwd_rows", p(dK), p(Khat), p(rstd), p(P["gamma"]), rows, D, st)
    dX = nan(rows, Din)
    ops.gemm("K", "N", rows, Din, D, dK, D, P["wk"], Din, dX, Din)
    ops.gemm("K", "N", rows, Din, D, dV, D, P["wv"], Din, dX, Din, beta=1.0)
    torch.cuda.synchronize()
    assert torch.equal(out["g_support"].reshape(Ns * L, Din), dX[:Ns * L].cpu()) and torch.equal(out["g_query"].reshape(Nq * L, Din), dX[Ns * L:].cpu())


# (rows, D): most lanes idle; D no multiple of the 256 lanes; 24 elements per lane; the head's own width
@pytest.mark.parametrize("shape", [(5, 64), (6, 300), (4, 6144), (7, 1152)], ids=lambda s: "r%dD%d" % s)
def test_key_layernorm_equals_the_training_layernorm_bit_for_bit(dev, shape):
    """lmkd_ctx_ln_fwd against lmkd_layernorm_train_fwd without residual and mask; in place against out of place; without Khat and rstd"""
    import litemkd_amd
    from litemkd_amd import ops
    lib, p, st = litemkd_amd.lib(), ops._p, ops._stream()
    rows, D = shape
    g = torch.Generator().manual_seed(4000 + rows + D)
    Kraw, gamma, beta = torch.randn(rows, D, generator=g).to(dev), (1 + 0.1 * torch.randn(D, generator=g)).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)      # noqa: E731
    eps = ops._f32(1e-5)
    Kn, Khat, rstd = nan(rows, D), nan(rows, D), nan(rows)
    lib.call("lmkd_ctx_ln_fwd", p(Kraw), p(gamma), p(beta), p(Kn), p(Khat), p(rstd), rows, D, eps, st)
    y, xhat, rs = nan(rows, D), nan(rows, D), nan(rows)
    lib.call("lmkd_layernorm_train_fwd", p(Kraw), None, 0, p(gamma), p(beta), None, p(y), D, p(xhat), p(rs), rows, D, eps, st)
    Kin, Khat_in, rstd_in = Kraw.clone(), nan(rows, D), nan(rows)
    lib.call("lmkd_ctx_ln_fwd", p(Kin), p(gamma), p(beta), p(Kin), p(Khat_in), p(rstd_in), rows, D, eps, st)
    Kbare = nan(rows, D)
    lib.call("lmkd_ctx_ln_fwd", p(Kraw), p(gamma), p(beta), p(Kbare), None, None, rows, D, eps, st)
    torch.cuda.synchronize()
    for t in (Kn, Khat, rstd):
        assert bool(torch.isfinite(t).all())
    assert torch.equal(Kn, y) and torch.equal(Khat, xhat) and torch.equal(rstd, rs)
    assert torch.equal(Kin, Kn) and torch.equal(Khat_in, Khat) and torch.equal(rstd_in, rstd)
    assert torch.equal(Kbare, Kn)


def test_dropout_mask_is_applied_forward_and_backward(dev):
    from litemkd_amd import ops
    case = 1
    d = R.case_data(case)
    Ns, L, Din = d["sup"].shape
    rows = (Ns + d["qry"].shape[0]) * L
    mask = ops.dropout_mask((rows, Din), 0.1, 1234, dev)
    m = mask.cpu()
    kept = float((m != 0).float().mean())
    assert 0.8 < kept < 0.97 and bool(((m == 0) | ((m - 1 / 0.9).abs() < 1e-6)).all())
    out = _hip(dev, case, mask=mask)
    r32, r64 = R.run(case, torch.float32, mask=m), R.run(case, torch.float64, mask=m)
    _check_anchored("ctx case %d dropout 0.1" % case, out, r32, r64)
    assert not torch.equal(out["logits"], _hip(dev, case)["logits"])
    gx = torch.cat([out["g_support"].reshape(Ns * L, Din), out["g_query"].reshape(-1, Din)])
    assert float(gx[m == 0].abs().max()) == 0.0 and float(gx[m != 0].abs().max()) > 0


def _module_args(dev, d, **kw):
    from litemkd_amd.options import default_args
    return default_args(device=dev, way=d["way"], seq_len=d["L"], trans_linear_out_dim=d["wk"].shape[0], trans_dropout=0.0, **kw)


def _load(head, d, dev):
    t = head.transformers
    with torch.no_grad():
        for mod, w, b in ((t.k_linear, "wk", "bk"), (t.v_linear, "wv", "bv"), (t.norm_k, "gamma", "beta")):
            mod.weight.copy_(d[w])
            mod.bias.copy_(d[b])
    return head.to(dev)


def test_modules_match_the_function_and_norm_v_gets_no_gradient(dev):
    from litemkd_amd.model import classifiers as C
    case = 2
    d = R.case_data(case)
    a = _load(C.CTX(_module_args(dev, d)), d, dev)
    b = _load(C.CTX_fixed(_module_args(dev, d)), d, dev)
    s, q, lb = d["sup"].to(dev).requires_grad_(), d["qry"].to(dev).requires_grad_(), d["lab"].to(dev)
    la = a(s, lb, q)["logits"]
    lf = b(s, lb, q)["logits"]
    assert la.grad_fn is not None and lf.grad_fn is None and not lf.requires_grad
    assert torch.equal(la.detach(), lf) and torch.equal(lf.cpu(), _hip(dev, case)["logits"])
    # the flattened [N * L, D] layout the backbones may hand over reshapes the same way
    assert torch.equal(lf, b(s.detach().reshape(-1, 2048), lb, q.detach().reshape(-1, 2048))["logits"])
    R.fixture_loss(la).backward()
    t = a.transformers
    assert t.norm_v.weight.grad is None and t.norm_v.bias.grad is None
    for p_ in (t.k_linear.weight, t.k_linear.bias, t.v_linear.weight, t.v_linear.bias, t.norm_k.weight, t.norm_k.bias):
        assert p_.grad is not None and bool(torch.isfinite(p_.grad).all())
        assert p_ is t.v_linear.bias or float(p_.grad.abs().max()) > 0      # (v_linear.bias: 0 in exact arithmetic, the attention rows sum to 1)
    assert torch.equal(t.k_linear.weight.grad.cpu(), _hip(dev, case)["g_wk"])


def test_training_mode_draws_a_dropout_mask_per_call(dev):
    from litemkd_amd.model import classifiers as C
    from litemkd_amd.options import default_args
    d = R.case_data(2)
    args = default_args(device=dev, way=d["way"], seq_len=d["L"], trans_linear_out_dim=d["wk"].shape[0], trans_dropout=0.1)
    head = _load(C.CTX(args), d, dev)
    s, q, lb = d["sup"].to(dev), d["qry"].to(dev), d["lab"].to(dev)
    torch.manual_seed(4)
    l1, l2 = head(s, lb, q)["logits"], head(s, lb, q)["logits"]
    torch.manual_seed(4)
    l3 = head(s, lb, q)["logits"]
    assert not torch.equal(l1, l2) and torch.equal(l1, l3)
    head.eval()
    assert torch.equal(head(s, lb, q)["logits"].detach().cpu(), _hip(dev, 2)["logits"])
