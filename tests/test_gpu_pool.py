"""The stem and head pooling kernels of csrc/norm_pool.hip against tests/_pool_ref.py, the numpy statement of the same operations, by
EQUALITY: lmkd_bn_relu_maxpool_fwd[_seg], lmkd_maxpool_bwd, lmkd_bn_backward_stats[_seg], lmkd_stem_unpool_bn_bwd[_seg],
lmkd_adaptive_maxpool_mean_fwd / _bwd.

The inputs lie on a small dyadic grid (tests/test_pool_ref_host.py: fp32 and fp64 evaluation of the reference agree in every bit, every
tensor is bf16-representable, at least a tenth of the windows have a tied maximum), so the result does not depend on summation order or
FMA contraction and one wrong arg-max byte, tap number, table or dropped window fails `torch.equal`.  The reference itself is anchored
to torch's CPU kernels there.  The entry points are called the way ops.StemFn / ops.PoolHeadFn call them; every output buffer is
pre-filled with a sentinel, so an element that was never written shows."""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pool_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -1024.0      # bf16-representable, outside the range of every result (y <= 9, |dc| <= 44, sums of the small cases)
IDX_SENTINEL = 0xEE
KINDS = ["fp32", "bf16"]
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    return torch.device("cuda", 0)


@contextlib.contextmanager
def tensors(kind):
    """the storage type of the activation tensors, set the way the bf16_act fixture of test_gpu_ops.py sets it -> the torch dtype"""
    from litemkd_amd import ops
    if kind == "bf16":
        ops.set_conv_compute_dtype("bf16")
        ops.set_activation_dtype("bf16")
    try:
        yield torch.bfloat16 if kind == "bf16" else torch.float32
    finally:
        ops.set_activation_dtype("fp32")
        ops.reset_compute_dtypes()


def dv(a, dev, dtype=torch.float32):
    """numpy -> device; the conversions are exact (the grid is fp32- and bf16-representable)"""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return torch.from_numpy(a.copy()).to(dev)
    return torch.from_numpy(a.astype(np.float32)).to(dev).to(dtype)


def filled(shape, dev, dtype=torch.float32, value=SENTINEL):
    return torch.full(tuple(shape), value, dtype=dtype, device=dev)


def rounded(a, dt):
    """the reference as the kernel instance stores it: fp32, or fp32 rounded once to bf16 (ties to even)"""
    a = np.asarray(a).astype(np.float32)
    return torch.from_numpy(R.round_bf16(a) if dt is torch.bfloat16 else a)


def same(got, ref, what):
    got, ref = got.detach().cpu(), (ref if torch.is_tensor(ref) else torch.from_numpy(np.asarray(ref)))
    if got.dtype is torch.bfloat16:
        got = got.float()
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = (got != ref) | (got != got)
        first = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError("%s: %d of %d elements differ, first at %s: %r instead of %r"
                             % (what, int(bad.sum()), bad.numel(), first, got[tuple(first)].item(), ref[tuple(first)].item()))


@functools.lru_cache(maxsize=None)
def stem_ref(case):
    """the reference of a case, computed once (float64) and shared by every test; nobody writes to it"""
    N, H, W, C, N0 = case
    c, dy, stats, coef = R.grid_inputs(R.STEM_SEED, N, H, W, C, N0)
    gamma = R.grid_gamma(R.STEM_SEED, C)
    y, idx, cmax = R.bn_relu_maxpool(c, stats, N0)
    OH, OW = y.shape[1:3]
    two = 0 < N0 < N
    seg = (N0 * OH * OW, N0 * H * W) if two else (0, 0)
    sg, sgx, own = R.pooled_bn_stats(dy, cmax, stats, gamma, N * H * W, *seg)
    return dict(N=N, H=H, W=W, C=C, N0=N0, OH=OH, OW=OW, two=two, seg=seg, c=c, dy=dy, stats=stats, coef=coef, gamma=gamma, y=y, idx=idx,
                cmax=cmax, sg=sg, sgx=sgx, own_coef=own)


def _ops():
    import litemkd_amd
    from litemkd_amd import ops
    return litemkd_amd.lib(), ops


def _workspace(r, dev):
    lib, ops = _ops()
    ws = torch.empty((2 if r["two"] else 1) * lib.value("lmkd_bn_bwd_workspace", r["C"]), dtype=torch.uint8, device=dev)
    return ws, ops._tickets(ws)


# ---- 1. forward ----
def check_forward(dev, case, kind):
    lib, ops = _ops()
    r = stem_ref(case)
    N, H, W, C, N0, OH, OW = (r[k] for k in ("N", "H", "W", "C", "N0", "OH", "OW"))
    p, st = ops._p, ops._stream
    with tensors(kind) as dt:
        c, stats = dv(r["c"], dev, dt), dv(r["stats"], dev)
        runs = [("seg", True), ("seg", False)] + ([("plain", True), ("plain", False)] if N0 == N else [])
        for entry, with_cmax in runs:
            y, cmax = filled((N, OH, OW, C), dev, dt), filled((N, OH, OW, C), dev, dt)
            idx = filled((N, OH, OW, C), dev, torch.uint8, IDX_SENTINEL)
            if entry == "seg":
                lib.call("lmkd_bn_relu_maxpool_fwd_seg", p(c), p(stats), p(y), p(idx), p(cmax) if with_cmax else None, N, N0, H, W, C, st(), None)
            else:
                lib.call("lmkd_bn_relu_maxpool_fwd", p(c), p(stats), p(y), p(idx), p(cmax) if with_cmax else None, N, H, W, C, st())
            tag = "%s %s cmax=%s %s" % (case, kind, with_cmax, entry)
            same(idx, r["idx"], "idx " + tag)
            same(y, rounded(r["y"], None), "y " + tag)
            same(cmax, rounded(r["cmax"], None) if with_cmax else filled(cmax.shape, "cpu"), "cmax " + tag)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.STEM_CASES, ids=str)
def test_forward_writes_the_first_maximum_its_tap_and_its_conv_output(dev, case, kind):
    """y, the arg-max bytes and cmax of lmkd_bn_relu_maxpool_fwd_seg, with and without the cmax pointer (a null pointer leaves no trace);
    with one segment the plain entry point gives the same"""
    check_forward(dev, case, kind)


# ---- 2. max-pool backward ----
def check_maxpool_bwd(dev, case, kind):
    lib, ops = _ops()
    r = stem_ref(case)
    N, H, W, C = r["N"], r["H"], r["W"], r["C"]
    with tensors(kind) as dt:
        dy, idx, g = dv(r["dy"], dev, dt), dv(r["idx"], dev), filled((N, H, W, C), dev, dt)
        lib.call("lmkd_maxpool_bwd", ops._p(dy), ops._p(idx), ops._p(g), N, H, W, C, ops._stream())
        same(g, rounded(R.maxpool_bwd(r["dy"], r["idx"], H, W), dt), "g %s %s" % (case, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.STEM_CASES, ids=str)
def test_maxpool_bwd_routes_every_window_to_its_tap(dev, case, kind):
    check_maxpool_bwd(dev, case, kind)


# ---- 3. fused un-pool + BatchNorm backward apply, dyadic coefficients ----
def check_unpool(dev, case, kind):
    lib, ops = _ops()
    r = stem_ref(case)
    N, H, W, C, N0 = r["N"], r["H"], r["W"], r["C"], r["N0"]
    p, st = ops._p, ops._stream
    ref = R.stem_unpool_bn_bwd(r["dy"], r["idx"], r["c"], r["stats"], r["coef"], N0)
    with tensors(kind) as dt:
        dy, idx, c = dv(r["dy"], dev, dt), dv(r["idx"], dev), dv(r["c"], dev, dt)
        stats, coef = dv(r["stats"], dev), dv(r["coef"], dev)
        want = rounded(ref, dt)
        prior = R._steps(np.random.default_rng(C), -1.0, 1.0, 0.125, (2, C)).astype(np.float32)
        for acc in (0, 1):
            dc = filled((N, H, W, C), dev, dt)
            dgamma, dbeta = dv(prior[0], dev), dv(prior[1], dev)
            lib.call("lmkd_stem_unpool_bn_bwd_seg", p(dy), p(idx), p(c), p(stats), p(coef), p(dc), p(dgamma), p(dbeta), acc, N, N0, H, W, C, st(), None)
            same(dc, want, "dc %s %s" % (case, kind))
            if r["two"]:
                cf = np.asarray(r["coef"]).astype(np.float32)
                same(dgamma, (prior[0] if acc else 0) + (cf[0, 3] + cf[1, 3]), "dgamma %s acc=%d" % (case, acc))
                same(dbeta, (prior[1] if acc else 0) + (cf[0, 4] + cf[1, 4]), "dbeta %s acc=%d" % (case, acc))
            else:      # one segment: the parameter gradients belong to the coefficient kernel and are not touched here
                same(dgamma, prior[0], "dgamma untouched %s" % (case,))
                same(dbeta, prior[1], "dbeta untouched %s" % (case,))
        if not r["two"]:
            dc = filled((N, H, W, C), dev, dt)
            lib.call("lmkd_stem_unpool_bn_bwd", p(dy), p(idx), p(c), p(stats), p(coef), p(dc), N, H, W, C, st(), None)
            same(dc, want, "dc (plain entry) %s %s" % (case, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.STEM_CASES, ids=str)
def test_stem_unpool_bn_bwd_equals_the_reference(dev, case, kind):
    """dc of lmkd_stem_unpool_bn_bwd[_seg] with the dyadic coefficient table of grid_inputs: exact in fp32, the once-rounded reference
    with bf16 tensors; two segments: dgamma / dbeta (+)= rows 3 / 4 of both segments' tables"""
    check_unpool(dev, case, kind)


# ---- 4. the BatchNorm backward sums from the pooled side ----
def run_stats(dev, r, dt, acc=0, prior=None):
    """-> coef, dgamma, dbeta (None with two segments), the ticket words"""
    lib, ops = _ops()
    p, st = ops._p, ops._stream
    N, H, W, C, OH, OW = (r[k] for k in ("N", "H", "W", "C", "OH", "OW"))
    dy, cmax, stats, gamma = dv(r["dy"], dev, dt), dv(r["cmax"], dev, dt), dv(r["stats"], dev), dv(r["gamma"], dev)
    ws, tickets = _workspace(r, dev)
    assert int(tickets.abs().max()) == 0
    if r["two"]:
        coef = filled((2, 5, C), dev)
        lib.call("lmkd_bn_backward_stats_seg", p(dy), p(cmax), p(stats), p(gamma), p(coef), p(ws), p(tickets), N * OH * OW, r["seg"][0],
                 N * H * W, r["seg"][1], C, st())
        return coef, None, None, tickets
    coef = filled((3, C), dev)
    dgamma, dbeta = (dv(prior[0], dev), dv(prior[1], dev)) if prior is not None else (filled((C,), dev), filled((C,), dev))
    lib.call("lmkd_bn_backward_stats", p(dy), p(cmax), p(stats), p(gamma), p(dgamma), p(dbeta), p(coef), p(ws), p(tickets), N * OH * OW,
             N * H * W, C, acc, st())
    return coef, dgamma, dbeta, tickets


def check_stats(dev, case):
    r = stem_ref(case)
    C = r["C"]
    prior = R._steps(np.random.default_rng(C + 1), -1.0, 1.0, 0.125, (2, C)).astype(np.float32)
    tables = {}
    for kind in KINDS:
        with tensors(kind) as dt:
            for acc in ((0,) if r["two"] else (0, 1)):
                coef, dgamma, dbeta, tickets = run_stats(dev, r, dt, acc, prior if acc else None)
                tag = "%s %s acc=%d" % (case, kind, acc)
                same(coef, r["own_coef"], "coef " + tag)      # sums exact, every quotient rounded once
                if not r["two"]:
                    same(dgamma, (prior[0] if acc else 0) + r["sgx"].astype(np.float32), "dgamma " + tag)
                    same(dbeta, (prior[1] if acc else 0) + r["sg"].astype(np.float32), "dbeta " + tag)
                assert int(tickets.abs().max()) == 0, "ticket words not zero after " + tag
                if not acc:
                    tables[kind] = [coef.cpu()] + ([dgamma.cpu(), dbeta.cpu()] if dgamma is not None else [])
    for a, b in zip(tables["fp32"], tables["bf16"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", R.STEM_CASES, ids=str)
def test_bn_backward_stats_tables_are_bit_equal_to_the_reference(dev, case):
    """dgamma, dbeta and every row of coef of lmkd_bn_backward_stats[_seg] on the reference's cmax: the sums are exact and each quotient is
    one fp64 division rounded once; the accumulate flag adds to a prior value; the ticket words are zero again; the fp32 and the bf16
    tensor instance give identical tables"""
    check_stats(dev, case)


# ---- 5. stats -> un-pool with the kernel's own coefficients ----
@pytest.mark.parametrize("case", R.STEM_CASES, ids=str)
def test_stats_then_unpool_within_the_rounding_bound(dev, case):
    """lmkd_bn_backward_stats[_seg] -> lmkd_stem_unpool_bn_bwd[_seg] on the same inputs, fp32 tensors, against the float64 reference per
    element.  mean(g) and mean(g * xhat) are quotients now, so dc is not exact.  With u = 2^-24 the kernel evaluates

        dc = A * ((g - mg') - ((c - mean) * invstd * mgx'))

    where c, mean, invstd, g and A are exact (grid values; g a sum of at most four multiples of 1/8) and mg' = mg (1 + d1), mgx' = mgx
    (1 + d2), |d| <= u, are the coefficients rounded once from their fp64 quotients (the sums behind them are exact).  Six operations
    round: c - mean, * invstd, * mgx', g - mg', the outer difference, * A (an FMA contraction only removes one).  The term g passes
    through 3 of them, mg through 3 plus d1, xhat * mgx through 5 plus d2: to first order
        |dc - ref| <= u |A| (3 |g| + 4 |mg| + 6 |xhat mgx|) <= 6 u |A| (|g| + |mg| + |xhat mgx|),
    and 8 u leaves room for the second-order terms and the 2^-53 of the reference's own fp64 arithmetic.  The bound is derived, not
    measured: if it fails, this derivation or the kernel is wrong.  Two segments: dgamma / dbeta are the exact sums of both."""
    lib, ops = _ops()
    r = stem_ref(case)
    N, H, W, C, N0 = r["N"], r["H"], r["W"], r["C"], r["N0"]
    p, st = ops._p, ops._stream
    _, _, coef64 = R.pooled_bn_stats(r["dy"], r["cmax"], r["stats"], r["gamma"], N * H * W, *r["seg"], round_coef=False)
    A, g, mg, xm = R.stem_unpool_terms(r["dy"], r["idx"], r["c"], r["stats"], coef64, N0)
    ref = A * (g - mg - xm)
    bound = 8 * U * np.abs(A) * (np.abs(g) + np.abs(mg) + np.abs(xm))
    with tensors("fp32") as dt:
        coef, _, _, _ = run_stats(dev, r, dt)
        dy, idx, c, stats = dv(r["dy"], dev), dv(r["idx"], dev), dv(r["c"], dev), dv(r["stats"], dev)
        dc, dgamma, dbeta = filled((N, H, W, C), dev), filled((C,), dev), filled((C,), dev)
        lib.call("lmkd_stem_unpool_bn_bwd_seg", p(dy), p(idx), p(c), p(stats), p(coef), p(dc), p(dgamma), p(dbeta), 0, N, N0, H, W, C, st(), None)
    err = np.abs(dc.cpu().numpy().astype(np.float64) - ref)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print("stats -> unpool %s: max err %.3e, max err / bound %.3f" % (case, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (case, worst, err[worst], np.broadcast_to(bound, err.shape)[worst])
    if r["two"]:
        same(dgamma, r["sgx"].sum(0).astype(np.float32), "dgamma %s" % (case,))
        same(dbeta, r["sg"].sum(0).astype(np.float32), "dbeta %s" % (case,))


# ---- the large case once more with a quarter of the workgroups: every grid-stride loop takes further trips ----
def test_large_case_with_one_workgroup_per_cu(dev):
    lib, _ = _ops()
    lib.call("lmkd_set_elementwise_wg_per_cu", 1)
    try:
        for kind in KINDS:
            check_forward(dev, R.STEM_BIG, kind)
            check_maxpool_bwd(dev, R.STEM_BIG, kind)
            check_unpool(dev, R.STEM_BIG, kind)
        check_stats(dev, R.STEM_BIG)
    finally:
        lib.call("lmkd_set_elementwise_wg_per_cu", 4)      # include/lmkd.h: the default


# ---- 6. head pooling ----
HEAD_F = 3


@functools.lru_cache(maxsize=None)
def head_ref(H, W, C):
    x, dy = R.head_grid_inputs(R.HEAD_SEED, HEAD_F, H, W, C)
    return x, dy, R.head_pool(x), (R.head_pool_bwd(x, dy) if H >= 2 and W >= 2 else None)


def check_head(dev, H, W, C, kind, backward=True):
    lib, ops = _ops()
    x64, dy64, y64, dx64 = head_ref(H, W, C)
    with tensors(kind) as dt:
        x, y = dv(x64, dev, dt), filled((HEAD_F, C), dev)
        lib.call("lmkd_adaptive_maxpool_mean_fwd", ops._p(x), ops._p(y), HEAD_F, H, W, C, ops._stream())
        same(y, y64.astype(np.float32), "head y %dx%d C=%d %s" % (H, W, C, kind))
        if backward:
            dy, dx = dv(dy64, dev), filled((HEAD_F, H, W, C), dev, dt)
            lib.call("lmkd_adaptive_maxpool_mean_bwd", ops._p(x), ops._p(dy), ops._p(dx), HEAD_F, H, W, C, ops._stream())
            same(dx, rounded(dx64, None), "head dx %dx%d C=%d %s" % (H, W, C, kind))      # k * dy / 16, k <= 4: exact in bf16 too


@pytest.mark.parametrize("H,W", [(h, w) for h in range(2, 9) for w in range(2, 9)])
def test_head_pool_forward_and_backward_at_every_geometry(dev, H, W):
    """lmkd_adaptive_maxpool_mean_fwd / _bwd on post-ReLU grid input with ties (a third zeros), 3 frames, every (H, W) the backward
    accepts: y and dx equal the reference for fp32 tensors (C = 4, 64) and bf16 tensors (C = 8, 64)"""
    for kind, Cs in (("fp32", (4, 64)), ("bf16", (8, 64))):
        for C in Cs:
            check_head(dev, H, W, C, kind)


@pytest.mark.parametrize("H,W", [(1, w) for w in range(1, 9)] + [(h, 1) for h in range(2, 9)])
def test_head_pool_forward_on_single_rows_and_columns(dev, H, W):
    for kind, Cs in (("fp32", (4, 64)), ("bf16", (8, 64))):
        for C in Cs:
            check_head(dev, H, W, C, kind, backward=False)


@pytest.mark.parametrize("H,W", [(1, 4), (4, 9), (9, 8)])
def test_head_pool_backward_refuses_what_its_counter_cannot_hold(dev, H, W):
    """H = 1, W = 9, H * W > 64: a RuntimeError before any launch, dx untouched"""
    lib, ops = _ops()
    C = 8
    x, dy, dx = filled((HEAD_F, H, W, C), dev, value=1.0), filled((HEAD_F, C), dev, value=1.0), filled((HEAD_F, H, W, C), dev)
    with pytest.raises(RuntimeError):
        lib.call("lmkd_adaptive_maxpool_mean_bwd", ops._p(x), ops._p(dy), ops._p(dx), HEAD_F, H, W, C, ops._stream())
    same(dx, filled(dx.shape, "cpu"), "dx after a refused call")


@pytest.mark.parametrize("H,W", [(3, 3), (7, 5)])
def test_pool_head_fn_with_ties(dev, H, W):
    """the autograd wrapper ops.PoolHeadFn on the same tie-heavy input"""
    _, ops = _ops()
    x64, dy64, y64, dx64 = head_ref(H, W, 64)
    x = dv(x64, dev).requires_grad_()
    y = ops.PoolHeadFn.apply(x)
    y.backward(dv(dy64, dev))
    same(y, y64.astype(np.float32), "PoolHeadFn y")
    same(x.grad, dx64.astype(np.float32), "PoolHeadFn dx")
