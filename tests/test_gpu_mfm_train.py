"""GPU: training the MFM teacher.  Kernel level: the training LayerNorm and 8-token attention of csrc/mfm.hip, forward and
backward, against fp64 torch by the project's anchored criterion (HIP vs fp64 at most 3 x torch-CPU-fp32 vs fp64 + 2e-6), on NaN-filled
outputs and twice for bit-identity.  Fusion level: `_Fusion.forward` and every parameter gradient of a seeded sum(w o fused) against the
module's own nn containers on the CPU (dropout off) and against the restatement tests/_mfm_train_ref.py (explicit masks).  The whole
teacher at width 2048 against the reference's own numbers (tests/golden/mfm_train.npz), and the trainer against a hand-written loop."""
import argparse
import copy
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _anchor
import _mfm_train_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CPU_FP32_LIMIT = 1e-5      # the regime in which the anchored criterion discriminates: torch-CPU fp32's own deviation from fp64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    return torch.device("cuda", 0)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _record(tag, pairs):
    for k, (eh, ec) in pairs.items():
        print("%s %-40s HIP vs fp64 %.3e | CPU fp32 vs fp64 %.3e" % (tag, k, eh, ec))
    _anchor.record(tag, pairs)


# ---------------------------------------------------------------------------------------------------------------------------------
# attention kernels
# ---------------------------------------------------------------------------------------------------------------------------------
ATTN_SHAPES = [(3, 8, 128, 2), (2, 5, 960, 3), (2, 1, 128, 2), (2, 8, 6144, 3)]      # (B, L, D, H)


@functools.lru_cache(maxsize=None)
def _attn_case(B, L, D, H, masked):
    g = torch.Generator().manual_seed(1000 + B + 10 * L + D + 7 * H)
    qkv, dO = torch.randn(B * L, 3 * D, generator=g), torch.randn(B * L, D, generator=g)
    mask = (torch.rand(B * H, L, L, generator=g) >= R.P_DROP).float() / (1 - R.P_DROP) if masked else None
    refs = []
    for dt in (torch.float32, torch.float64):
        x = qkv.detach().to(dt).clone().requires_grad_()
        hd = D // H
        q, k, v = (t.reshape(B, L, H, hd).transpose(1, 2) for t in x.chunk(3, dim=-1))
        P = torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(hd), dim=-1)
        PM = P if mask is None else P * mask.reshape(B, H, L, L).to(dt)
        out = (PM @ v).transpose(1, 2).reshape(B * L, D)
        out.backward(dO.to(dt))
        P8 = torch.zeros(B * H, 8, 8, dtype=dt)
        P8[:, :L, :L] = P.detach().reshape(B * H, L, L)
        refs.append({"out": out.detach(), "P": P8, "dqkv": x.grad})
    return qkv, dO, mask, refs[0], refs[1]


def _attn_hip(dev, qkv, dO, mask, B, L, D, H):
    import litemkd_amd
    from litemkd_amd import ops
    lib, p, st = litemkd_amd.lib(), ops._p, ops._stream()
    q, g = qkv.to(dev), dO.to(dev)
    m = None if mask is None else mask.to(dev)
    out, P, dqkv = _nan(dev, B * L, D), _nan(dev, B * H, 8, 8), _nan(dev, B * L, 3 * D)
    lib.call("lmkd_mha_small_train_fwd", p(q), p(m), p(out), p(P), B, L, D, H, st)
    lib.call("lmkd_mha_small_bwd", p(q), p(P), p(m), p(g), p(dqkv), B, L, D, H, st)
    torch.cuda.synchronize()
    return {"out": out.cpu(), "P": P.cpu(), "dqkv": dqkv.cpu()}


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "B%dL%dD%dH%d" % s)
def test_attention_kernels_are_anchored_to_fp64(dev, shape, masked):
    B, L, D, H = shape
    qkv, dO, mask, r32, r64 = _attn_case(B, L, D, H, masked)
    a = _attn_hip(dev, qkv, dO, mask, B, L, D, H)
    b = _attn_hip(dev, qkv, dO, mask, B, L, D, H)
    for k in a:
        assert bool(torch.isfinite(a[k]).all()), "%s: an element was not written" % k
        assert torch.equal(a[k], b[k]), "%s differs between two calls" % k
    assert float(a["P"][:, L:, :].abs().max() if L < 8 else 0.0) == 0.0 and float(a["P"][:, :, L:].abs().max() if L < 8 else 0.0) == 0.0
    pairs = {}
    split = lambda t: dict(zip(("dq", "dk", "dv"), t.chunk(3, dim=-1)))      # noqa: E731
    got, c32, c64 = ({"out": r["out"], "P": r["P"], **split(r["dqkv"])} for r in (a, r32, r64))
    for k in got:
        if L == 1 and k in ("dq", "dk"):      # a one-token softmax is the constant 1: dS = 0 exactly
            assert float(c64[k].abs().max()) == 0.0 and float(got[k].abs().max()) == 0.0, k
            continue
        assert float(c64[k].norm()) > 0.0, k
        pairs[k] = (_anchor.rel_l2(got[k], c64[k]), _anchor.rel_l2(c32[k], c64[k]))
    _record("mfm attn B%d L%d D%d H%d %s" % (B, L, D, H, "mask" if masked else "nomask"), pairs)
    for k in pairs:
        _anchor.anchored(k, got[k], c32[k], c64[k])
    if not masked:      # the inference kernel computes the same forward
        import litemkd_amd
        from litemkd_amd import ops
        o = _nan(dev, B * L, D)
        litemkd_amd.lib().call("lmkd_mha_small", ops._p(qkv.to(dev)), ops._p(o), B, L, D, H, ops._stream())
        assert torch.equal(o.cpu(), a["out"])


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm kernels
# ---------------------------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(5, 64, 5), (24, 960, 8), (16, 6144, 8)]      # (rows, D, res_rows = L)


@functools.lru_cache(maxsize=None)
def _ln_case(rows, D, L, masked):
    g = torch.Generator().manual_seed(2000 + rows + D)
    x, emb, dy = torch.randn(rows, D, generator=g), torch.randn(L, D, generator=g), torch.randn(rows, D, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    mask = (torch.rand(rows, D, generator=g) >= R.P_DROP).float() / (1 - R.P_DROP) if masked else None
    refs = []
    for dt in (torch.float32, torch.float64):
        xx, ee, ga, be = (t.detach().to(dt).clone().requires_grad_() for t in (x, emb, gamma, beta))
        pre = xx + ee.repeat(rows // L, 1)
        pre.retain_grad()
        y = F.layer_norm(pre, (D,), ga, be, R.EPS)
        if mask is not None:
            y = y * mask.to(dt)
        y.backward(dy.to(dt))
        mean, var = pre.detach().mean(1, keepdim=True), pre.detach().var(1, unbiased=False, keepdim=True)
        rstd = 1 / torch.sqrt(var + R.EPS)
        refs.append({"y": y.detach(), "xhat": (pre.detach() - mean) * rstd, "rstd": rstd.reshape(-1), "dpre": pre.grad, "demb": ee.grad,
                     "dgamma": ga.grad, "dbeta": be.grad})
    return x, emb, dy, gamma, beta, mask, refs[0], refs[1]


def _ln_hip(dev, x, emb, dy, gamma, beta, mask, L):
    """forward into a column slice of a wider buffer, backward from a column slice of a wider gradient"""
    import ctypes
    import litemkd_amd
    from litemkd_amd import ops
    lib, p, st = litemkd_amd.lib(), ops._p, ops._stream()
    rows, D = x.shape
    ld, off = 2 * D + 4, D + 4
    xd, ed, ga, be = (t.to(dev) for t in (x, emb, gamma, beta))
    m = None if mask is None else mask.to(dev)
    wide, xhat, rstd = _nan(dev, rows, ld), _nan(dev, rows, D), _nan(dev, rows)
    lib.call("lmkd_layernorm_train_fwd", p(xd), p(ed), L, p(ga), p(be), p(m), ctypes.c_void_p(wide.data_ptr() + 4 * off), ld, p(xhat), p(rstd),
             rows, D, ops._f32(R.EPS), st)
    gwide = _nan(dev, rows, ld)
    gwide[:, off:off + D] = dy.to(dev)
    dpre, dyc = _nan(dev, rows, D), _nan(dev, rows, D)
    lib.call("lmkd_layernorm_train_bwd", ctypes.c_void_p(gwide.data_ptr() + 4 * off), ld, p(m), p(xhat), p(rstd), p(ga), p(dpre), p(dyc), rows, D, st)
    out = {"y": wide[:, off:off + D], "xhat": xhat, "rstd": rstd, "dpre": dpre, "demb": ops.colsum(dpre.view(rows // L, L * D)).view(L, D),
           "dgamma": ops.colsum(dyc, xhat), "dbeta": ops.colsum(dyc)}
    torch.cuda.synchronize()
    untouched = torch.cat([wide[:, :off].reshape(-1), wide[:, off + D:].reshape(-1)])
    assert bool(torch.isnan(untouched).all()), "the forward wrote outside its column slice"
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: "r%dD%dL%d" % s)
def test_layernorm_kernels_are_anchored_to_fp64(dev, shape, masked):
    rows, D, L = shape
    x, emb, dy, gamma, beta, mask, r32, r64 = _ln_case(rows, D, L, masked)
    a = _ln_hip(dev, x, emb, dy, gamma, beta, mask, L)
    b = _ln_hip(dev, x, emb, dy, gamma, beta, mask, L)
    pairs = {}
    for k in a:
        assert bool(torch.isfinite(a[k]).all()), "%s: an element was not written" % k
        assert torch.equal(a[k], b[k]), "%s differs between two calls" % k
        pairs[k] = (_anchor.rel_l2(a[k], r64[k]), _anchor.rel_l2(r32[k], r64[k]))
    _record("mfm layernorm rows %d D %d L %d %s" % (rows, D, L, "mask" if masked else "nomask"), pairs)
    for k in a:
        _anchor.anchored(k, a[k], r32[k], r64[k])
    if not masked:      # the inference kernel computes the same forward
        from litemkd_amd.teacher import mfm
        y = mfm.layernorm(x.to(dev), gamma.to(dev), beta.to(dev), emb.to(dev), L)
        assert torch.equal(y.cpu(), a["y"])


# entry points that state the same arithmetic must agree to the bit.  (rows, D, res_rows): most lanes idle; D no multiple of the 256
# lanes and 6 % 3 wrapping the residual rows; 24 elements per lane; no residual
LN_EQ_CASES = [(5, 64, 5), (6, 300, 3), (4, 6144, 4), (6, 300, None)]


@pytest.mark.parametrize("case", LN_EQ_CASES, ids=lambda c: "r%dD%dres%s" % c)
def test_inference_and_training_layernorm_forward_are_bit_equal(dev, case):
    import ctypes
    import litemkd_amd
    from litemkd_amd import ops
    lib, p, st = litemkd_amd.lib(), ops._p, ops._stream()
    rows, D, rr = case
    g = torch.Generator().manual_seed(3000 + rows + D)
    x, gamma, beta = torch.randn(rows, D, generator=g).to(dev), (1 + 0.1 * torch.randn(D, generator=g)).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev)
    res = torch.randn(rr, D, generator=g).to(dev) if rr else None
    ld, off = 2 * D + 4, D + 4
    wi, wt, xhat, rstd = _nan(dev, rows, ld), _nan(dev, rows, ld), _nan(dev, rows, D), _nan(dev, rows)
    lib.call("lmkd_layernorm_fwd", p(x), p(res), rr or 0, p(gamma), p(beta), ctypes.c_void_p(wi.data_ptr() + 4 * off), ld, rows, D,
             ops._f32(R.EPS), st)
    lib.call("lmkd_layernorm_train_fwd", p(x), p(res), rr or 0, p(gamma), p(beta), None, ctypes.c_void_p(wt.data_ptr() + 4 * off), ld, p(xhat),
             p(rstd), rows, D, ops._f32(R.EPS), st)
    torch.cuda.synchronize()
    for w in (wi, wt):
        assert bool(torch.isnan(torch.cat([w[:, :off].reshape(-1), w[:, off + D:].reshape(-1)])).all()), "wrote outside its column slice"
        assert bool(torch.isfinite(w[:, off:off + D]).all())
    assert torch.equal(wi[:, off:off + D], wt[:, off:off + D])


@pytest.mark.parametrize("shape", [c[:2] for c in LN_EQ_CASES[:3]], ids=lambda s: "r%dD%d" % s)
def test_in_place_and_training_layernorm_backward_are_bit_equal(dev, shape):
    import litemkd_amd
    from litemkd_amd import ops
    lib, p, st = litemkd_amd.lib(), ops._p, ops._stream()
    rows, D = shape
    g = torch.Generator().manual_seed(3100 + rows + D)
    dy, xhat, gamma = torch.randn(rows, D, generator=g).to(dev), torch.randn(rows, D, generator=g).to(dev), (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    rstd = (0.5 + torch.rand(rows, generator=g)).to(dev)
    dK, dpre = dy.clone(), _nan(dev, rows, D)
    lib.call("lmkd_layernorm_bwd_rows", p(dK), p(xhat), p(rstd), p(gamma), rows, D, st)
    lib.call("lmkd_layernorm_train_bwd", p(dy), D, None, p(xhat), p(rstd), p(gamma), p(dpre), None, rows, D, st)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dpre).all()) and not torch.equal(dK, dy)
    assert torch.equal(dK, dpre)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fusions
# ---------------------------------------------------------------------------------------------------------------------------------
FUSION_CONFIGS = [(n, d, L) for d in (64, 320) for L in (8, 5) for n in (2, 3)]      # (modalities, in_channels, seq_len); trans_num 2, 3 videos
N_VID, N_LAYERS = 3, 2


@functools.lru_cache(maxsize=None)
def _fusion_case(n_mod, d, L):
    seed = 300 + 10 * n_mod + d + L
    return R.make_fusion(n_mod, d, L, N_LAYERS, seed), tuple(R.fusion_inputs(seed + 1, n_mod, N_VID, L, d)), R.weights(seed + 2, (N_VID, L, d))


@functools.lru_cache(maxsize=None)
def _fusion_ref(n_mod, d, L, mask_seed=None):
    """(fp32, fp64) on the CPU, computed once: torch's nn containers with dropout off, the restatement with explicit masks"""
    mod, xs, w = _fusion_case(n_mod, d, L)
    fn = R.nn_fusion if mask_seed is None else R.restated(R.make_masks(mod, N_VID, L, mask_seed))
    return R.fusion_grads(fn, mod, xs, w, torch.float32), R.fusion_grads(fn, mod, xs, w, torch.float64)


def _fusion_hip(dev, mod, xs, w, masks=None, train=False):
    m = copy.deepcopy(mod).to(dev).train(train)
    xd = [x.to(dev).requires_grad_() for x in xs]
    y = m(*xd, masks=None if masks is None else {k: v.to(dev) for k, v in masks.items()})
    (y * w.to(dev)).sum().backward()
    torch.cuda.synchronize()
    out = {"out": y.detach().cpu()}
    out.update({"g_in%d" % i: x.grad.cpu() for i, x in enumerate(xd)})
    out.update({"g_" + k: v.grad.cpu() for k, v in m.named_parameters()})
    return out


def _check_fusion(tag, got, r32, r64):
    assert set(got) == set(r64)
    pairs = {k: (_anchor.rel_l2(got[k], r64[k]), _anchor.rel_l2(r32[k], r64[k])) for k in r64}
    _record(tag, pairs)
    grads = [k for k in r64 if k != "out"]
    for k in r64:
        assert bool(torch.isfinite(got[k]).all()) and got[k].shape == r64[k].shape, k
        assert float(r64[k].norm()) > 0.0, "%s: the fp64 reference is zero" % k
        assert pairs[k][1] < CPU_FP32_LIMIT, "%s: torch-CPU fp32 is %.2e off fp64 on this input: choose another input" % (k, pairs[k][1])
    _anchor.anchored("out", got["out"], r32["out"], r64["out"])
    worst = _anchor.anchored_dict({k: got[k] for k in grads}, {k: r32[k] for k in grads}, {k: r64[k] for k in grads})
    print("%s worst ratio %.2f at %s (hip %.3e cpu %.3e)" % ((tag,) + worst))


@pytest.mark.parametrize("cfg", FUSION_CONFIGS, ids=lambda c: "mod%d_d%d_L%d" % c)
def test_fusion_without_dropout_matches_the_nn_containers(dev, cfg):
    mod, xs, w = _fusion_case(*cfg)
    r32, r64 = _fusion_ref(*cfg)
    _check_fusion("mfm fusion mod %d d %d L %d eval" % cfg, _fusion_hip(dev, mod, xs, w), r32, r64)


@pytest.mark.parametrize("cfg", [(3, 64, 5), (2, 320, 8)], ids=lambda c: "mod%d_d%d_L%d" % c)
def test_fusion_with_explicit_masks_matches_the_restatement(dev, cfg):
    mod, xs, w = _fusion_case(*cfg)
    masks = R.make_masks(mod, N_VID, cfg[2], 17)
    r32, r64 = _fusion_ref(*cfg, mask_seed=17)
    assert float((r64["out"] - _fusion_ref(*cfg)[1]["out"]).abs().max()) > 1e-2      # the masks do something
    _check_fusion("mfm fusion mod %d d %d L %d masks" % cfg, _fusion_hip(dev, mod, xs, w, masks, train=True), r32, r64)


def test_training_mode_draws_its_masks_and_eval_mode_has_none(dev):
    mod, xs, w = _fusion_case(3, 64, 5)
    torch.manual_seed(5)
    a = _fusion_hip(dev, mod, xs, w, train=True)
    b = _fusion_hip(dev, mod, xs, w, train=True)
    torch.manual_seed(5)
    c = _fusion_hip(dev, mod, xs, w, train=True)
    ev = _fusion_hip(dev, mod, xs, w)
    p0 = _fusion_hip(dev, mod, xs, w, masks={}, train=True)
    assert not torch.equal(a["out"], b["out"]) and not torch.equal(a["out"], ev["out"])
    for k in a:
        assert bool(torch.isfinite(a[k]).all()), k
        assert torch.equal(a[k], c[k]), "%s: the same generator state must draw the same masks" % k
        assert torch.equal(ev[k], p0[k]), "%s: eval mode with gradients is the training path with p = 0" % k
    # eval mode stays the frozen extractor's arithmetic up to the inference Linear's rounding, and training mode still refuses it
    m = copy.deepcopy(mod).to(dev)
    ref = m.extract_feature(*[x.to(dev) for x in xs]).cpu()
    assert _anchor.rel_l2(ev["out"], ref.double()) < 1e-5
    with pytest.raises(NotImplementedError):
        m.train().extract_feature(*[x.to(dev) for x in xs])


def test_second_use_of_the_shared_fusion_accumulates(dev):
    mod, xs, w = _fusion_case(2, 64, 8)
    ys = [xs[0], torch.roll(xs[1], -1, 1)]

    def both(fn, m, dt, to):
        a = [x.detach().to(dt).to(to).clone().requires_grad_() for x in xs]
        b = [a[0], ys[1].detach().to(dt).to(to).clone().requires_grad_()]
        y = fn(m, a) + fn(m, b)
        (y * w.to(dt).to(to)).sum().backward()
        out = {"out": y.detach().cpu(), "g_in0": a[0].grad.cpu()}
        out.update({"g_" + k: v.grad.cpu() for k, v in m.named_parameters()})
        return out
    r32 = both(R.nn_fusion, copy.deepcopy(mod), torch.float32, "cpu")
    r64 = both(R.nn_fusion, copy.deepcopy(mod).double(), torch.float64, "cpu")
    got = both(lambda m, a: m(*a), copy.deepcopy(mod).to(dev), torch.float32, dev)
    one = _fusion_ref(2, 64, 8)[1]
    assert float((r64["g_f1.weight"] - one["g_f1.weight"]).norm()) > 0.1 * float(one["g_f1.weight"].norm())      # the second use adds
    _check_fusion("mfm fusion shared, two uses", got, r32, r64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the GEMM summed in blocks of K
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", ["KK", "KN", "MN"])
def test_gemm_in_k_blocks_matches_fp64(dev, lay):
    """ops.gemm(k_block=128) at K = 300 (blocks of 128, 128 and 44), two batches, C given (beta = 1), bias and ReLU with the last
    block: against fp64 by the anchored criterion; equal to the one-launch GEMM to rounding, bit-identical on a second call."""
    from litemkd_amd import ops
    M, N, K, nb = 20, 36, 300, 2
    g = torch.Generator().manual_seed(23)
    A = torch.randn((nb, M, K) if lay[0] == "K" else (nb, K, M), generator=g)
    B = torch.randn((nb, N, K) if lay[1] == "K" else (nb, K, N), generator=g)
    C0, bias = torch.randn(nb, M, N, generator=g), torch.randn(N, generator=g)

    def ref(dt):
        a = A.to(dt) if lay[0] == "K" else A.to(dt).transpose(1, 2)
        b = B.to(dt).transpose(1, 2) if lay[1] == "K" else B.to(dt)
        return torch.relu(0.5 * (a @ b) + C0.to(dt) + bias.to(dt))

    def run(**kw):
        c = C0.to(dev).clone()
        a, b = A.to(dev), B.to(dev)
        ops.gemm(lay[0], lay[1], M, N, K, a, A.shape[2], b, B.shape[2], c, N, alpha=0.5, beta=1.0, bias=bias.to(dev), relu=True,
                 batch=nb, sA=A[0].numel(), sB=B[0].numel(), sC=M * N, **kw)
        torch.cuda.synchronize()
        return c.cpu()
    one, blk = run(), run(k_block=128)
    assert torch.equal(blk, run(k_block=128))
    assert not torch.equal(one, blk) and float((one - blk).abs().max()) < 1e-4
    _record("gemm k_block 128 " + lay, {"C": _anchor.anchored("C", blk, ref(torch.float32), ref(torch.float64))})


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole teacher at width 2048 against the reference's numbers
# ---------------------------------------------------------------------------------------------------------------------------------
def _teacher_args(**kw):
    a = dict(seq_len=R.WT["seq_len"], trans_num=R.WT["num_layers"], shirt_num=R.WT["shirt_num"], temp_set=R.WT["temp_set"], way=R.WT["way"],
             trans_linear_out_dim=R.WT["out_dim"], trans_linear_in_dim=2048, trans_dropout=0.0, m1="rgb", m2="depth", m3="flow")
    a.update(kw)
    return argparse.Namespace(**a)


def test_whole_teacher_reproduces_the_reference(dev):
    """ThreeTRXShiftLoopTime.forward (eval mode, autograd on) on 7 support videos with ragged, unsorted labels and a class without support
    plus 4 queries: logits and the gradients of sum(w o logits) against the reference's own module, within the bounds the fixture carries
    (3 x the fp32 restatement's deviation, not below 3e-6 of the tensor's largest magnitude; _mfm_train_ref.fixture_bounds).

    The Linear layers and the head's GEMMs sum K in blocks of ops.MFM_K_BLOCK = 128 terms (gemm's k_block).  One accumulator per output over
    all of K (2048 - 18432 terms here) missed 41 of the 99 bounds by up to 2.28 x, its sampled gradients a median 3.3 x as far from fp64
    as torch's CPU fp32; blocks of 1024 / 512 / 256 missed 20 / 5 / 6; blocks of 128 meet all 99, the worst at 0.95 of its bound, a
    median 0.8 x torch's CPU fp32 error against fp64.  The bounds are narrow because the fp32 restatement they come
    from repeats the reference's operations on the same CPU kernels: the fp64 restatement itself uses up to 0.80 of one."""
    from litemkd_amd.teacher.mfm import ThreeTRXShiftLoopTime
    G = np.load(os.path.join(GOLD, "mfm_train.npz"))
    with torch.device("meta"):
        model = ThreeTRXShiftLoopTime(_teacher_args(), head=True)
    model = model.to_empty(device=dev).eval()
    model.load_state_dict({k: v.to(dev) for k, v in R.teacher_params().items()}, strict=True)
    ctx, labels, tgt = R.teacher_inputs()
    names = ("rgb", "depth", "flow")
    logits = model({n: c.to(dev) for n, c in zip(names, ctx)}, labels.to(dev), {n: t.to(dev) for n, t in zip(names, tgt)})["logits"]
    (logits * R.teacher_weights().to(dev)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad.cpu() for k, v in model.named_parameters() if R.trainable(k)}
    assert all(g is not None for g in grads.values())
    got = R.digest(logits.cpu(), grads)
    errs, bounds = R.digest_errors(got, G), R.fixture_bounds(G)
    missing = sorted(set(range(R.WT["way"])) - set(R.WT["labels"]))
    assert float(logits[:, missing].abs().max()) == 0.0
    for k in sorted(errs):
        print("%-72s err %.3e bound %.3e" % (k, errs[k], bounds[k]))
    bad = {k: (errs[k], bounds[k]) for k in errs if not errs[k] <= bounds[k]}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
TRAIN_FLAGS = ("--way 3 --shot 1 --query_per_class 1 --trans_num 1 --training_iterations 4 --tasks_per_batch 2 --trans_dropout 0.0 --opt adam "
               "-lr 0.0001 --print_freq 1 --save_freq 2 --seed 11").split()
LR = 1e-4


@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
    """python -m litemkd_amd.train_teacher's main() on a tree of seeded features for 4 classes: 4 iterations, optimizer steps after
    iterations 1 and 3, checkpoint 2 after iteration 1.  (On separable classes this loop's losses and gradients are exactly 0.0, so the
    features carry no class.)"""
    from litemkd_amd import train_teacher as TT
    root = tmp_path_factory.mktemp("mfm_trainer")
    feats, ck, log = str(root / "feats"), str(root / "ck"), str(root / "log.jsonl")
    R.write_feature_tree(feats, classes=4, videos=2, proto_scale=0.0)      # classes that cannot be told apart: the loss does not saturate
    flags = TRAIN_FLAGS + ["--feature_save_path", feats, "--checkpoint_dir", ck, "--log_jsonl", log]
    losses, accs, model, opt = TT.main(flags)
    torch.cuda.synchronize()
    out = dict(flags=flags, feats=feats, ck=ck, log=log, losses=losses, accs=accs, steps=opt.steps,
               params={k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    del model, opt
    torch.cuda.empty_cache()
    return out


def test_trainer_matches_a_hand_written_loop(dev, trained):
    """the same module, seeds and reader under torch.optim.Adam and torch's cross-entropy, with the reference's counting written out.  Both
    loops run the same deterministic kernels on the same masks, so the losses agree as the first two of test_episode_loop_matches_oracle_loop do
    (1e-4 relative) and the parameters by its Adam criterion: per tensor, the fraction of elements whose update is off by more than
    0.2 lr stays below 0.05."""
    import random
    from litemkd_amd import train_teacher as TT
    p = TT.build_parser()
    args = TT.args_check(p, p.parse_args(trained["flags"]))
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    model = TT.build_model(args, dev)
    first = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    loader = iter(TT.FeatureTreeEpisodes(args, args.feature_save_path, None, args.split, dev))
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    losses, steps = [], []
    for iteration in (1, 2, 3, 4):
        task = next(loader)
        logits = model(task["context_features"], task["context_labels"], task["target_features"])["logits"]
        loss = F.cross_entropy(logits, task["target_labels"].long(), reduction="sum") / 2
        loss.backward()
        losses.append(float(loss))
        if (iteration + 1) % 2 == 0 or iteration == 4 - 1:
            opt.step()
            opt.zero_grad()
            steps.append(iteration)
    assert steps == [1, 3] and trained["steps"] == 2 and len(trained["losses"]) == 4
    print("losses", trained["losses"], losses, "accuracies", trained["accs"])
    assert all(0.0 <= a <= 1.0 for a in trained["accs"]) and all(math.isfinite(v) and v > 0 for v in losses)
    for a, b in zip(trained["losses"], losses):
        assert abs(a - b) < 1e-4 * max(1.0, abs(b)), (trained["losses"], losses)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    moved, worst, failed = 0, (0.0, ""), {}
    for k, v in sd.items():
        if not R.trainable(k):
            assert torch.equal(trained["params"][k], first[k]) and torch.equal(v, first[k]), k
            continue
        want, got = v.double() - first[k].double(), trained["params"][k].double() - first[k].double()
        if k.endswith("v_linear.bias"):
            # its gradient is 0 in exact arithmetic (every attention row sums to 1), so what Adam sees is rounding noise and
            # each element moves by lr x the noise's sign - in either loop (measured: 46 % of the elements differ).  As in
            # test_episode_loop_matches_oracle_loop such a tensor is held to its gradient-free invariant: two steps of at most lr each.
            assert float(want.abs().max()) <= 2.001 * LR and float(got.abs().max()) <= 2.001 * LR, k
            moved += 1
            continue
        assert float(want.abs().max()) > 0.5 * LR, "%s did not move" % k
        if k.endswith("self_attn.in_proj_bias"):
            # the key third: a bias on every key shifts each score row by a constant, which the softmax removes - gradient 0 in exact
            # arithmetic, rounding noise in fp32 (measured: 18 % of the tensor's elements, half of that third, differ).  Same invariant.
            third = want.numel() // 3
            assert float(want[third:2 * third].abs().max()) <= 2.001 * LR and float(got[third:2 * third].abs().max()) <= 2.001 * LR, k
            want, got = torch.cat((want[:third], want[2 * third:])), torch.cat((got[:third], got[2 * third:]))
        bad = float(((got - want).abs() > 0.2 * LR).double().mean())
        worst = max(worst, (bad, k))
        if bad > 0.05:
            failed[k] = bad
        moved += 1
    assert not failed, failed
    assert moved == sum(R.trainable(k) for k in sd)
    print("worst fraction of elements off by more than 0.2 lr: %.4f at %s" % worst)
    log = [json.loads(line) for line in open(trained["log"])]
    assert [r["iteration"] for r in log] == [2, 3, 4, 5] and abs(log[0]["loss"] - trained["losses"][0]) < 1e-6


def test_trainer_checkpoints_load_where_the_project_reads_them(dev, trained):
    from litemkd_amd.model import classifiers as C
    from litemkd_amd.model.model_select import load_teacher
    from litemkd_amd.teacher.mfm import ThreeTRXShiftLoopTime
    assert sorted(os.listdir(trained["ck"])) == ["checkpoint.pt", "checkpoint2.pt", "checkpoint_final.pt"]
    ck = torch.load(os.path.join(trained["ck"], "checkpoint.pt"), map_location="cpu")
    assert sorted(ck) == ["iteration", "model_state_dict", "optimizer_state_dict", "scheduler"] and ck["iteration"] == 2
    assert ck["optimizer_state_dict"]["steps"] == 1 and float(ck["optimizer_state_dict"]["exp_avg"].abs().max()) > 0
    final = torch.load(os.path.join(trained["ck"], "checkpoint_final.pt"), map_location="cpu")
    assert list(final) == list(trained["params"]) and all(torch.equal(final[k], v) for k, v in trained["params"].items())
    assert sorted(final) == sorted(R.teacher_params())      # the reference's keys: fusion.*, three_fusion.*, bracnch.transformers.0.*
    assert any(not torch.equal(final[k], ck["model_state_dict"][k]) for k in final)      # the second step came after checkpoint 2
    # the head through model_select.load_teacher
    args = _teacher_args(way=3, teacher_checkpoint=os.path.join(trained["ck"], "checkpoint2.pt"))
    teacher = load_teacher(C.TRX_fixed(args), args)
    for k, v in teacher.transformers.state_dict().items():
        assert torch.equal(v, ck["model_state_dict"]["bracnch.transformers.0." + k]), k
    # the fusions into a default-constructed module
    with torch.device(dev):
        plain = ThreeTRXShiftLoopTime(_teacher_args())
    plain.load_state_dict({k: v for k, v in final.items() if not k.startswith("bracnch.")}, strict=True)


def test_trainer_resumes_at_the_saved_iteration(dev, trained, tmp_path):
    import shutil
    from litemkd_amd import train_teacher as TT
    ck = str(tmp_path / "ck")
    shutil.copytree(trained["ck"], ck)
    os.remove(os.path.join(ck, "checkpoint_final.pt"))
    flags = [f if f != trained["ck"] else ck for f in trained["flags"] if f != trained["log"] and f != "--log_jsonl"]
    # what load_checkpoint restores, checked directly: the weights, both Adam moments, the step count, the learning rate, the scheduler
    from litemkd_amd import trainloop as TL
    ps = TT.build_parser()
    args = TT.args_check(ps, ps.parse_args(flags))
    saved_ck = torch.load(os.path.join(ck, "checkpoint.pt"), map_location="cpu")
    torch.manual_seed(99)      # another initialisation than the checkpoint's run
    fresh = TT.build_model(args, dev)
    fopt = TL.FusedOptimizer(fresh, args.opt, args.learning_rate)
    fsch = TL.MultiStepLR(fopt, args.sch, episodes_per_step=1)
    assert fopt.steps == 0 and float(fopt.m.abs().max()) == 0.0
    assert TT.load_checkpoint(fresh, fopt, fsch, ck) == 2
    so = saved_ck["optimizer_state_dict"]
    assert fopt.steps == so["steps"] == 1 and fopt.lr == so["lr"]
    assert torch.equal(fopt.m.cpu(), so["exp_avg"].cpu()) and torch.equal(fopt.v.cpu(), so["exp_avg_sq"].cpu())
    assert float(fopt.m.abs().max()) > 0 and float(fopt.v.abs().max()) > 0
    assert (fsch.n, fsch.base) == (saved_ck["scheduler"]["n"], saved_ck["scheduler"]["base"]) and fsch.n > 0
    for k, v in fresh.state_dict().items():
        assert torch.equal(v.cpu(), saved_ck["model_state_dict"][k]), k
    del fresh, fopt, fsch
    torch.cuda.empty_cache()
    losses, accs, model, opt = TT.main(flags + ["--resume_from_checkpoint"])
    # continues counting at the checkpoint's label: iterations 3 and 4 run, the optimizer steps once more (at iteration 3)
    assert len(losses) == 2 and opt.steps == 2 and all(math.isfinite(v) for v in losses)
    saved = torch.load(os.path.join(ck, "checkpoint.pt"), map_location="cpu")["model_state_dict"]
    final = torch.load(os.path.join(ck, "checkpoint_final.pt"), map_location="cpu")
    k = "three_fusion.f1.weight"
    step = (final[k] - saved[k]).abs()
    assert 0.5 * LR < float(step.max()) < 1.5 * LR      # one Adam step from the checkpoint's weights, with its moments loaded
