"""GPU: the OTAM matcher head (csrc/otam.hip) against its fp64 restatement tests/_otam_ref.py by the project's anchored
criterion - HIP vs fp64 at most 3 x (the fp32 restatement on the CPU vs fp64) + 2e-6, for cum, the logits and both feature gradients - in
the library's default GEMM mode and in the native fp32 mode, at the smallest shapes that reach each path; against the reference's own
numbers (tests/golden/otam.npz) where the reference is finite; determinism, unwritten outputs, the missing-class error, OTAM_fixed."""
import functools
import os

import numpy as np
import pytest
import torch

import _anchor
import _otam_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("cum", "logits", "g_support", "g_query")
GEMM_MODES = {"default": -1, "native_fp32": 0}


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


def _hip(dev, case, gemm_mode=-1):
    """OtamFn forward + backward of _otam_ref.fixture_loss -> dict like _otam_ref.run, on the CPU"""
    import litemkd_amd
    from litemkd_amd import ops
    way, L, sup, lab, qry = R.case_data(case)
    s, q = sup.to(dev).requires_grad_(), qry.to(dev).requires_grad_()
    plan = ops.ClassPlan(lab.to(dev), way, cpu_copy=lab)
    lib = litemkd_amd.lib()
    lib.call("lmkd_gemm_set_mode", gemm_mode)
    try:
        logits, cum = ops.OtamFn.apply(s, q, plan)
        R.fixture_loss(logits).backward()
        torch.cuda.synchronize()
    finally:
        lib.call("lmkd_gemm_set_mode", -1)
    return {"logits": logits.detach().cpu(), "cum": cum.detach().cpu(), "g_support": s.grad.cpu(), "g_query": q.grad.cpu()}


@pytest.mark.parametrize("mode", list(GEMM_MODES))
@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_head_is_anchored_to_fp64(dev, case, mode):
    r32, r64 = _cpu(case)
    out = _hip(dev, case, GEMM_MODES[mode])
    way, L, sup, lab, qry = R.case_data(case)
    assert tuple(out["logits"].shape) == (qry.shape[0], way) and tuple(out["cum"].shape) == (qry.shape[0], sup.shape[0])
    pairs = {}
    for k in KEYS:
        assert bool(torch.isfinite(out[k]).all()), k
        pairs[k] = (_anchor.rel_l2(out[k], r64[k]), _anchor.rel_l2(r32[k], r64[k]))
        print("case %d %s %-9s HIP vs fp64 %.3e | CPU fp32 vs fp64 %.3e" % (case, mode, k, pairs[k][0], pairs[k][1]))
    _anchor.record("otam case %d L %d D %d gemm %s" % (case, L, sup.shape[2], mode), pairs)
    for k in ("cum", "logits"):
        _anchor.anchored(k, out[k], r32[k], r64[k])
    _anchor.anchored_dict({k: out[k] for k in ("g_support", "g_query")}, {k: r32[k] for k in ("g_support", "g_query")},
                          {k: r64[k] for k in ("g_support", "g_query")})
    assert torch.allclose(out["logits"].sum(1), torch.ones(qry.shape[0]), atol=1e-5)


@pytest.mark.parametrize("mode", list(GEMM_MODES))
@pytest.mark.parametrize("case", list(R.FIXTURE_CASES))
def test_head_reproduces_the_reference(dev, case, mode):
    """the reference's own CNN_OTAM.  Logits within 3e-6 and gradient chunk sums within 2e-3 of the reference's maximum, the bounds its
    restatement meets on the CPU (test_otam_host.py).  cum: those 2e-5 for the reference's own fp32 recursion, plus what the frame
    products may add: lmkd_gemm_f32 is held to 2e-6 relative in every mode (test_gpu_ops.py::test_gemm_on_the_bf16_pipe), |sim| <= 1, so
    each frame distance carries up to 2e-6, and the two alignment paths of a pair cross at most 2 (2 L - 1) cells, where same-sign
    products (a query that resembles its support video) can make the MFMA's truncation add up coherently: 2e-5 + 2 (2 L - 1) 2e-6,
    8e-5 at L = 8.  (The first GPU run measured 3.5e-5 / 3.8e-5 in the three-plane GEMM mode at L = 8, D = 2048 against a bound of
    2e-5 that had left the product's error out; 4.8e-7 at L = 4, D = 64.)"""
    G = np.load(os.path.join(GOLD, "otam.npz"))
    pre = "c%d_" % case
    L = R.CASES[case][4]
    out = _hip(dev, case, GEMM_MODES[mode])
    e_cum = float((out["cum"].double() - torch.from_numpy(G[pre + "cum"]).double()).abs().max())
    e_log = float((out["logits"].double() - torch.from_numpy(G[pre + "logits"]).double()).abs().max())
    print("case %d %s: cum err %.2e logits err %.2e" % (case, mode, e_cum, e_log))
    assert e_cum <= 2e-5 + 2 * (2 * L - 1) * 2e-6 and e_log <= 3e-6
    for name in ("g_support", "g_query"):
        r = torch.from_numpy(G[pre + name]).double()
        err = float((R.gsum(out[name]).double() - r).abs().max())
        print("case %d %s: %s chunk sums err %.2e of %.2e" % (case, mode, name, err, float(r.abs().max())))
        assert err <= 2e-3 * float(r.abs().max()), name


def test_two_calls_are_bit_identical(dev):
    a, b = _hip(dev, 4), _hip(dev, 4)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("case", [1, 5, 9])      # register path with ragged classes; LDS path; a row pitch with pad columns
def test_every_output_element_is_written(dev, case):
    """the four entry points on NaN-filled outputs: an element a kernel leaves out shows; the results equal OtamFn's bit for bit"""
    import litemkd_amd
    from litemkd_amd import ops
    lib = litemkd_amd.lib()
    way, L, sup, lab, qry = R.case_data(case)
    Ns, _, D = sup.shape
    Nq = qry.shape[0]
    Ms, ldd = Ns * L, ops.otam_pitch(Ns, L)
    assert (ldd != Ms) == (case == 9)
    plan = ops.ClassPlan(lab.to(dev), way, cpu_copy=lab)
    host = ops.otam_plan_check(plan)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)      # noqa: E731
    X = qry.reshape(Nq * L, D).to(dev)
    Y = torch.cat([sup.reshape(Ms, D), torch.zeros(ldd - Ms, D)]).to(dev)
    n, dist, rq, rs, cum, logits = nan(Nq * L, ldd), nan(Nq * L, ldd), nan(Nq * L), nan(Ms), nan(Nq, Ns), nan(Nq, way)
    dD, Gd, dQ, dS = nan(Nq * L, ldd), nan(Nq * L, ldd), nan(Nq * L, D), nan(ldd, D)
    p, st = ops._p, ops._stream()
    lib.call("lmkd_otam_frame_dist_fwd", p(X), p(Y), p(n), p(rq), p(rs), p(dist), Nq, Ns, L, D, st)
    lib.call("lmkd_otam_align_fwd", p(dist), p(plan.cls), host, p(cum), p(logits), Nq, Ns, way, L, st)
    g = R.fixture_weights((Nq, way)).to(dev)
    lib.call("lmkd_otam_align_bwd", p(g), p(logits), p(dist), p(plan.cls), host, p(dD), Nq, Ns, way, L, st)
    lib.call("lmkd_otam_frame_dist_bwd", p(dD), p(X), p(Y), p(n), p(rq), p(rs), p(Gd), p(dQ), p(dS), Nq, Ns, L, D, st)
    torch.cuda.synchronize()
    for name, t in (("n", n[:, :Ms]), ("dist", dist), ("rq", rq), ("rs", rs), ("cum", cum), ("logits", logits), ("dD", dD[:, :Ms]), ("Gd", Gd),
                    ("dQ", dQ), ("dS", dS)):
        assert bool(torch.isfinite(t).all()), name
    assert float(dist[:, Ms:].abs().sum()) == 0 and float(Gd[:, Ms:].abs().sum()) == 0 and float(dS[Ms:].abs().sum()) == 0
    out = _hip(dev, case)
    assert torch.equal(out["cum"], cum.cpu()) and torch.equal(out["logits"], logits.cpu())
    assert torch.equal(out["g_query"].reshape(Nq * L, D), dQ.cpu()) and torch.equal(out["g_support"].reshape(Ms, D), dS[:Ms].cpu())


def _args(dev, way, L):
    from litemkd_amd.options import default_args
    return default_args(device=dev, way=way, shot=1, query_per_class=1, seq_len=L)


def test_missing_class_raises_before_any_launch(dev):
    from litemkd_amd.model import classifiers as C
    head = C.OTAM(_args(dev, 3, 8))
    sup, qry = torch.randn(3, 8, 64, device=dev), torch.randn(2, 8, 64, device=dev)
    with pytest.raises(ValueError, match="class 1 has none"):
        head(sup, torch.tensor([0., 0., 2.], device=dev), qry)


def test_fixed_head_equals_the_trainable_one_without_a_graph(dev):
    from litemkd_amd.model import classifiers as C
    way, L, sup, lab, qry = R.case_data(1)
    s, q, lb = sup.to(dev).requires_grad_(), qry.to(dev).requires_grad_(), lab.to(dev)
    a = C.OTAM(_args(dev, way, L))(s, lb, q)["logits"]
    b = C.OTAM_fixed(_args(dev, way, L))(s, lb, q)["logits"]
    assert a.grad_fn is not None and b.grad_fn is None and not b.requires_grad
    assert torch.equal(a.detach(), b)
    # the head takes D from the tensor and seq_len from args: the flattened [N * L, D] layout the backbones may hand over reshapes the same way
    c = C.OTAM_fixed(_args(dev, way, L))(s.detach().reshape(-1, sup.shape[2]), lb, q.detach().reshape(-1, sup.shape[2]))["logits"]
    assert torch.equal(b, c)
