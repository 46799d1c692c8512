"""tests/_pool_ref.py, the numpy statement of the stem and head pooling stages, checked without a GPU:
  * anchored to torch's CPU kernels in fp64 on the tie-heavy grid inputs (the same arg-max positions, the same gradient routing);
  * the pooled-side BatchNorm backward (pooled_bn_stats -> stem_unpool_bn_bwd) equals torch's gradient of
    max_pool2d(relu(batch_norm(c))) on non-dyadic inputs with true batch statistics;
  * on the grid inputs fp32 and fp64 evaluation agree in every bit, so no operation rounds and the GPU tests may ask for equality;
  * the grid inputs contain the ties and the zero-maximum windows those tests exist for."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pool_ref as R  # noqa: E402

STEM_CASES = R.STEM_CASES      # the cases of tests/test_gpu_pool.py, with its seeds
HEAD_HW = [(h, w) for h in range(1, 9) for w in range(1, 9)]


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _bn(c, stats, N0):
    """relu(c * scale + shift) per frame segment, float64"""
    _, _, scale, shift, _ = R._rows(stats, c.shape[0], N0, c.dtype)
    return np.maximum(c * scale + shift, 0.0)


# ---- anchor: torch's CPU pooling kernels ----
@pytest.mark.parametrize("H,W", [(h, w) for h in range(1, 10) for w in range(1, 9)] + [(17, 35), (31, 29)])
def test_stem_reference_picks_torchs_argmax_and_routes_its_gradient(H, W):
    N, C, N0 = 3, 16, 1
    c, dy, stats, _ = R.grid_inputs(11, N, H, W, C, N0)
    y, idx, cmax = R.bn_relu_maxpool(c, stats, N0)
    v = nchw(_bn(c, stats, N0)).requires_grad_()
    ty, tpos = F.max_pool2d(v, 3, 2, 1, return_indices=True)
    assert np.array_equal(y, nhwc(ty.detach()))
    # tap number -> flat position h * W + w of the input plane, torch's index convention
    OH, OW = y.shape[1:3]
    oh, ow = np.arange(OH)[None, :, None, None], np.arange(OW)[None, None, :, None]
    h, w = 2 * oh - 1 + idx // 3, 2 * ow - 1 + idx % 3
    assert (h >= 0).all() and (h < H).all() and (w >= 0).all() and (w < W).all()      # never a tap in the padding
    assert np.array_equal(h * W + w, nhwc(tpos))
    assert np.array_equal(cmax, np.take_along_axis(c.reshape(N, H * W, C), (h * W + w).reshape(N, -1, C), 1).reshape(y.shape))
    ty.backward(nchw(dy))
    assert np.array_equal(R.maxpool_bwd(dy, idx, H, W), nhwc(v.grad))


@pytest.mark.parametrize("H,W", HEAD_HW)
def test_head_reference_picks_torchs_argmax_and_routes_its_gradient(H, W):
    Fr, C = 3, 16
    x, dy = R.head_grid_inputs(5, Fr, H, W, C)
    v = nchw(x).requires_grad_()
    ty, tpos = F.adaptive_max_pool2d(v, (4, 4), return_indices=True)
    assert np.array_equal(R.head_argmax(x), tpos.permute(2, 3, 0, 1).reshape(16, Fr, C).numpy())
    out = ty.mean((2, 3))
    assert np.array_equal(R.head_pool(x), out.detach().numpy())      # 16 dyadic terms: the mean is exact in any order
    out.backward(torch.from_numpy(dy))
    assert np.array_equal(R.head_pool_bwd(x, dy), nhwc(v.grad))


def test_head_windows_are_the_adaptive_pooling_windows():
    assert R.head_windows(2) == [(0, 1), (0, 1), (1, 2), (1, 2)]
    assert R.head_windows(3) == [(0, 1), (0, 2), (1, 3), (2, 3)]
    assert R.head_windows(7) == [(0, 2), (1, 4), (3, 6), (5, 7)]
    assert R.head_windows(8) == [(0, 2), (2, 4), (4, 6), (6, 8)]


def test_round_bf16_is_torchs_rounding():
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(4096, generator=g) * 3, torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0, 44.0, 257.0 / 256])])
    assert np.array_equal(R.round_bf16(x.numpy()), x.to(torch.bfloat16).float().numpy())


# ---- chain: the pooled-side identity against autograd ----
@pytest.mark.parametrize("N,H,W,C,N0", [(4, 9, 12, 8, 4), (5, 14, 11, 8, 2), (3, 6, 5, 16, 1)])
def test_pooled_side_bn_backward_equals_autograd(N, H, W, C, N0):
    """non-dyadic c, true batch statistics per frame segment: dc, dgamma, dbeta of pooled_bn_stats -> stem_unpool_bn_bwd against torch's
    fp64 gradient of max_pool2d(relu(batch_norm(c))), 1e-12 relative - the sums over windows equal the sums over pre-pooling pixels"""
    rng = np.random.default_rng(N * 100 + H)
    c = rng.standard_normal((N, H, W, C)) * 1.5 + rng.standard_normal(C) * 0.5
    gamma, beta = 1 + 0.3 * rng.standard_normal(C), 0.3 * rng.standard_normal(C)
    gamma[1] = -gamma[1]
    beta[0] -= 2.0      # a channel that is mostly masked
    dy = rng.standard_normal((N, R.pooled_size(H), R.pooled_size(W), C))
    eps = 1e-5
    two = N0 < N
    tabs = []
    for a, b in ([(0, N0), (N0, N)] if two else [(0, N)]):
        x = c[a:b].reshape(-1, C)
        mean, var = x.mean(0), x.var(0)
        invstd = 1.0 / np.sqrt(var + eps)
        tabs.append(np.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd, var]))
    stats = np.stack(tabs) if two else tabs[0]
    y, idx, cmax = R.bn_relu_maxpool(c, stats, N0)
    prow, crow = y.shape[1] * y.shape[2], H * W
    sg, sgx, coef = R.pooled_bn_stats(dy, cmax, stats, gamma, N * crow, N0 * prow if two else 0, N0 * crow if two else 0, round_coef=False)
    dc = R.stem_unpool_bn_bwd(dy, idx, c, stats, coef, N0)
    if two:
        assert np.array_equal(coef[:, 3], sgx) and np.array_equal(coef[:, 4], sg)
        sg, sgx = sg.sum(0), sgx.sum(0)
    tc = nchw(c).requires_grad_()
    tg, tb = torch.from_numpy(gamma).requires_grad_(), torch.from_numpy(beta).requires_grad_()
    parts = [F.batch_norm(tc[a:b], None, None, tg, tb, True, 0.1, eps) for a, b in ([(0, N0), (N0, N)] if two else [(0, N)])]
    ty = F.max_pool2d(F.relu(torch.cat(parts)), 3, 2, 1)
    assert np.allclose(y, nhwc(ty.detach()), rtol=1e-13, atol=1e-13)
    ty.backward(nchw(dy))
    for name, got, ref in (("dc", dc, nhwc(tc.grad)), ("dgamma", sgx, tg.grad.numpy()), ("dbeta", sg, tb.grad.numpy())):
        err = np.abs(got - ref).max() / np.abs(ref).max()
        assert err <= 1e-12, (name, err)


# ---- exactness of the grid ----
def _f32(*arrays):
    return [np.asarray(a).astype(np.float32) for a in arrays]


def _same(a32, a64):
    assert a32.dtype == np.float32 and a64.dtype == np.float64
    assert np.array_equal(a32.astype(np.float64), a64)


def _bf16_exact(a):
    a = np.asarray(a).astype(np.float32)
    assert np.array_equal(R.round_bf16(a), a)


@pytest.mark.parametrize("N,H,W,C,N0", STEM_CASES)
def test_stem_grid_is_exact_in_fp32(N, H, W, C, N0):
    """every function on the grid inputs, evaluated in fp32 and in fp64: identical, so nothing rounds; every tensor a bf16 kernel instance
    reads or writes (except dc) is bf16-representable"""
    c, dy, stats, coef = R.grid_inputs(R.STEM_SEED, N, H, W, C, N0)
    gamma = R.grid_gamma(R.STEM_SEED, C)
    c32, dy32, st32, cf32, ga32 = _f32(c, dy, stats, coef, gamma)
    for a, b in ((c32, c), (dy32, dy), (st32, stats), (cf32, coef), (ga32, gamma)):
        _same(a, b)
    for a in (c, dy):
        _bf16_exact(a)
    y, idx, cmax = R.bn_relu_maxpool(c, stats, N0)
    y32, idx32, cmax32 = R.bn_relu_maxpool(c32, st32, N0)
    _same(y32, y), _same(cmax32, cmax)
    assert np.array_equal(idx32, idx) and idx.dtype == np.uint8 and idx.max() <= 8
    g, g32 = R.maxpool_bwd(dy, idx, H, W), R.maxpool_bwd(dy32, idx, H, W)
    _same(g32, g)
    for a in (y, cmax, g):
        _bf16_exact(a)
    two = 0 < N0 < N
    prow, crow = y.shape[1] * y.shape[2], H * W
    seg = (N0 * prow, N0 * crow) if two else (0, 0)
    sg, sgx, kc = R.pooled_bn_stats(dy, cmax, stats, gamma, N * crow, *seg)
    sg32, sgx32, kc32 = R.pooled_bn_stats(dy32, cmax32, st32, ga32, N * crow, *seg)
    _same(sg32, sg), _same(sgx32, sgx)
    assert kc.dtype == np.float32 and np.array_equal(kc, kc32)
    # the parameter gradients of two segments are the fp32 sums of the fp32 rows 3 / 4: exact as well
    if two:
        assert np.array_equal((kc[0, 3] + kc[1, 3]).astype(np.float64), sgx.sum(0)) and np.array_equal((kc[0, 4] + kc[1, 4]).astype(np.float64), sg.sum(0))
    _same(R.stem_unpool_bn_bwd(dy32, idx, c32, st32, cf32, N0), R.stem_unpool_bn_bwd(dy, idx, c, stats, coef, N0))


@pytest.mark.parametrize("H,W", HEAD_HW)
def test_head_grid_is_exact_in_fp32(H, W):
    for C in (4, 8, 64):
        x, dy = R.head_grid_inputs(R.HEAD_SEED, 3, H, W, C)
        x32, dy32 = _f32(x, dy)
        _same(x32, x), _same(dy32, dy)
        _bf16_exact(x)
        _same(R.head_pool(x32), R.head_pool(x))
        dx = R.head_pool_bwd(x, dy)
        _same(R.head_pool_bwd(x32, dy32), dx)
        _bf16_exact(dx)      # k * dy / 16 with k <= 4
        k = dx / np.where(dy == 0, 1.0, dy / 16.0)[:, None, None, :]
        if H >= 2 and W >= 2:      # the backward kernel's domain: at most two overlapping windows per axis
            assert k.max() <= 4
            if H <= 3 and W <= 3:
                assert k.max() == 4      # the third bit plane of the kernel's per-position counter is in use


# ---- the inputs contain what the tests are for ----
@pytest.mark.parametrize("N,H,W,C,N0", STEM_CASES)
def test_stem_grid_has_ties_zero_windows_and_distinct_tables(N, H, W, C, N0):
    c, _, stats, _ = R.grid_inputs(R.STEM_SEED, N, H, W, C, N0)
    assert (np.asarray(stats)[..., 2, :] < 0).any()      # negative scale occurs
    if 0 < N0 < N:
        flipped = np.sign(stats[0, 2]) != np.sign(stats[1, 2])
        assert flipped.any()
        # reading the wrong table changes arg-max bytes
        if H * W > 1:
            assert not np.array_equal(R.bn_relu_maxpool(c, stats, N0)[1], R.bn_relu_maxpool(c, stats, 3 - N0)[1])
    pos_tie, zero = R.window_tie_shares(c, stats, N0)
    if R.pooled_size(H) * R.pooled_size(W) >= 100:
        assert pos_tie >= 0.10 and zero >= 0.03, (pos_tie, zero)
        zc = R.window_tie_shares(c[..., R.ZERO_CHANNEL::8], np.asarray(stats)[..., R.ZERO_CHANNEL::8], N0)[1]
        assert zc > 0.5, zc      # the shifted channels: most windows have maximum 0


@pytest.mark.parametrize("H,W", HEAD_HW)
def test_head_grid_has_ties(H, W):
    for C in (4, 8, 64):
        x, _ = R.head_grid_inputs(R.HEAD_SEED, 3, H, W, C)
        if x.size >= 1000:
            assert 0.28 <= (x == 0).mean() <= 0.39      # about a third zeros
        share = R.head_tie_share(x)      # over the windows that hold more than one element
        assert (share is None) == (H in (1, 2, 4) and W in (1, 2, 4))
        if share is not None:
            assert share >= 0.10, (C, share)
