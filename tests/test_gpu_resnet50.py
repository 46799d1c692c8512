"""GPU: the ResNet-50 training path (BASELINE configs[4]) under the fp64-anchored criterion of tests/_anchor.py at its REAL map sizes -
every distinct convolution of the trunk at 224 x 224 (the kernels, tiles and XCD orders of the 200-frame call: tests/_r50_shapes.py) and
every kind of Bottleneck block (ops.ResBlockFn with three stages, hand-scheduled backward) with the HIP path's own ReLU masks imposed on both references.
Nothing here reads more than a few dozen frames; the measured (HIP, CPU-fp32) pairs go to $LMKD_PARITY_LOG."""
import pytest
import torch
import torch.nn.functional as F

import _r50_shapes as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    torch.set_num_threads(max(1, min(32, len(__import__("os").sched_getaffinity(0)))))
    return torch.device("cuda", 0)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


class _MaskedReLU(torch.autograd.Function):
    """ReLU with an imposed 0/1 mask (forward t * mask, backward g * mask)"""

    @staticmethod
    def forward(ctx, t, mask):
        ctx.save_for_backward(mask)
        return t * mask

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * mask, None


# (N, cin, width, H, stride): real ResNet-50 blocks at their 224^2 map size, the fewest frames that leave several row tiles and a
# ragged last one
BOTTLENECK_CASES = [
    (6, 64, 64, 56, 1),         # layer1.0: downsample at stride 1 - both data gradients of x on the patch kernel, the second accumulating; 64-column two-plane tile
    (6, 256, 64, 56, 1),        # layer1.1: no downsample - conv1's gradient accumulated onto g
    (8, 256, 128, 56, 2),       # layer2.0: 3x3 stride 2 inside the block, 1x1 stride-2 downsample accumulating onto a quarter of the pixels
    (24, 1024, 512, 14, 2),     # layer4.0: Cout 2048 / K 1024 - column-slice XCD order; 2048-channel BatchNorm on 7x7
    (40, 2048, 512, 7, 1),      # layer4.2: K = 2048 reduce; 49-pixel maps (1960 rows: 15.3 tiles)
]
_CASE_REF = {}      # the references of the case in flight, shared by its three modes: {"case", "inputs", "natural", "masked": (masks, run32, run64)}


def _bottleneck_ref(case, dt, masks):
    """one torchvision Bottleneck (v1.5) forward + backward on the CPU in dtype dt, training-mode BatchNorm; masks: None (natural ReLUs)
    or the three imposed ones.  -> y, {gradients of x and every parameter}, the three pre-activations"""
    N, cin, width, H, stride = case
    x0, gy, params = _CASE_REF["inputs"]
    x = x0.clone().to(dt).requires_grad_()
    ref = {k: v.clone().to(dt).requires_grad_() for k, v in params.items()}

    def bn(t, pre):
        c = t.shape[1]
        return F.batch_norm(t, torch.zeros(c, dtype=dt), torch.ones(c, dtype=dt), ref[pre + ".weight"], ref[pre + ".bias"], True, 0.1, 1e-5)

    def relu(t, i):
        return F.relu(t) if masks is None else _MaskedReLU.apply(t, masks[i].to(dt))
    pre1 = bn(F.conv2d(x, ref["conv1.weight"]), "bn1")
    pre2 = bn(F.conv2d(relu(pre1, 0), ref["conv2.weight"], None, stride, 1), "bn2")
    out = bn(F.conv2d(relu(pre2, 1), ref["conv3.weight"]), "bn3")
    idn = x
    if "downsample.0.weight" in ref:
        idn = bn(F.conv2d(x, ref["downsample.0.weight"], None, stride, 0), "downsample.1")
    pre3 = out + idn
    y = relu(pre3, 2)
    y.backward(gy.to(dt))
    g = {k: v.grad for k, v in ref.items()}
    g["x"] = x.grad
    return y.detach(), g, (pre1.detach(), pre2.detach(), pre3.detach())


@pytest.mark.parametrize("mode", ["fp32x3", "fp32h2", "fp32"])
@pytest.mark.parametrize("N,cin,width,H,stride", BOTTLENECK_CASES)
def test_bottleneck_isolated(dev, N, cin, width, H, stride, mode):
    """one Bottleneck (ops.ResBlockFn, three stages) forward + backward on identical inputs - the twin of test_gpu_ops.test_block_isolated, same
    structure, same numbers.  The hand-scheduled backward (BatchNorm-backward sums in the 1x1 data gradient's epilogue, in-place dx_out,
    conv1's gradient accumulated onto g, the downsample gradient accumulated at stride 1 and at stride 2, loader-side BatchNorm in
    fp32x3 / fp32 against the materialised activations of fp32h2) is judged per tensor against an fp64 evaluation: error at most 3 x
    torch-CPU-fp32's own + 2e-6, with the HIP path's three ReLU masks imposed on both references after checking that they differ from
    the natural fp64 masks at no more than max(4, numel // 200000) elements per site, each with |fp64 pre-activation| < 1e-5 max|pre|
    (a condition on the inputs: torch's own fp32 flips none at any site of these cases)."""
    import litemkd_amd
    from litemkd_amd import ops
    from litemkd_amd.model.backbone import resnet as R
    from _anchor import anchored, anchored_dict, record
    case = (N, cin, width, H, stride)
    if _CASE_REF.get("case") != case:
        _CASE_REF.clear()
        torch.manual_seed(0)
        blk = R._Bottleneck(cin, width, stride)
        x0 = torch.relu(torch.randn(N, cin, H, H))
        gy = torch.randn(N, 4 * width, H // stride, H // stride)
        _CASE_REF.update(case=case, inputs=(x0, gy, {k: v.detach().clone() for k, v in blk.named_parameters()}), block=blk)
        _CASE_REF["natural"] = _bottleneck_ref(case, torch.float64, None)[2]
    x0, gy, params = _CASE_REF["inputs"]
    blk = R._Bottleneck(cin, width, stride)
    blk.load_state_dict(_CASE_REF["block"].state_dict())
    blk = blk.to(dev).train()
    ops.set_conv_compute_dtype(mode)
    n0 = litemkd_amd.lib().value("lmkd_conv_h2_launches")
    try:
        xd = nhwc(x0).to(dev).requires_grad_()
        if mode == "fp32h2":      # inside the trunk the block's input carries the maximum its producer recorded
            ops.amax_compute(xd)
        ops.BLOCK_TAPS = []
        try:
            yd = blk(xd)
            tap = ops.BLOCK_TAPS[0]
        finally:
            ops.BLOCK_TAPS = None
        yd.backward(nhwc(gy).to(dev))
        # fmaf(c, scale, shift) > 0: what the backward recomputes (mask mode 2), and the block output's own sign
        masks = (nchw(ops.bn_apply(tap["c1"], tap["st1"], True) > 0).cpu(), nchw(ops.bn_apply(tap["c2"], tap["st2"], True) > 0).cpu(),
                 nchw(yd.detach() > 0).cpu())
        hip = {k: v.grad.cpu() for k, v in blk.named_parameters()}
        hip["x"] = nchw(xd.grad).cpu()
        y_hip = nchw(yd.detach()).cpu()
        if mode == "fp32h2":
            assert litemkd_amd.lib().value("lmkd_conv_h2_launches") > n0, "the two-plane kernels did not run"
    finally:
        ops.reset_compute_dtypes()
    flips = 0
    for site, (m, pre) in enumerate(zip(masks, _CASE_REF["natural"])):
        diff = m != (pre > 0)
        flips += int(diff.sum())
        lim = 1e-5 * float(pre.abs().max())
        cap = max(4, m.numel() // 200000)
        assert int(diff.sum()) <= cap and (not bool(diff.any()) or float(pre[diff].abs().max()) < lim), \
            "ReLU mask %d of the HIP path differs from fp64 at %d elements (|pre| up to %.2e, limit %.2e)" % (
                site + 1, int(diff.sum()), float(pre[diff].abs().max()), lim)
    cached = _CASE_REF.get("masked")
    if cached is None or not all(torch.equal(a, b) for a, b in zip(cached[0], masks)):
        cached = _CASE_REF["masked"] = (masks, _bottleneck_ref(case, torch.float32, masks)[:2], _bottleneck_ref(case, torch.float64, masks)[:2])
    (y32, g32), (y64, g64) = cached[1], cached[2]
    assert set(hip) == set(g64)
    ey = anchored("block y", y_hip, y32, y64, 3.0, 2e-6)
    worst = anchored_dict(hip, g32, g64, 3.0, 2e-6)
    record("bottleneck N=%d %d->%d->%d H=%d s=%d [%s]" % (N, cin, width, 4 * width, H, stride, mode), {"y": ey, "worst grad (%s)" % worst[1]: worst[2:]})
    print("bottleneck gradients (HIP masks imposed, %d flips vs fp64), y (hip, cpu):" % flips, ey, "worst HIP/CPU error ratio vs fp64:", worst)


SEEN50 = {"gemm": set(), "wgrad": set(), "x3": set(), "x3w": set()}      # NOT test_gpu_fullsize.SEEN: its assertions are about the ResNet-18 shapes


@pytest.mark.parametrize("mode", ["fp32x3", "fp32h2"])
@pytest.mark.parametrize("shape", T.RESNET50, ids=[s[0] for s in T.RESNET50])
def test_resnet50_conv_shapes_vs_fp64(dev, shape, mode):
    """the 19 distinct ResNet-50 convolutions at their 224^2 map sizes (1x1 with K and Cout up to 2048, 1x1 stride 2 from 256 ... 1024
    channels, 3x3 stride 2 at 128 / 256 / 512) through test_gpu_fullsize._run_shape: forward and data gradient within 3 x torch-CPU-fp32's
    error vs fp64 + 1e-6, weight gradient + 2e-6, the BatchNorm partial sums of the forward epilogue.  Frame counts and tile pins come from
    tests/_r50_shapes.py; that they put every launch on the 200-frame call's kernel (tile, XCD tile order, parity classes, family) is
    asserted from lmkd_conv2d_plan first."""
    import litemkd_amd
    from litemkd_amd import ops
    from test_gpu_fullsize import _run_shape
    ops.set_conv_compute_dtype(mode)
    try:
        tiles = T.assert_same_kernels(litemkd_amd.lib(), shape)
        _run_shape(dev, *shape, N=T.frames(shape), seen=SEEN50, tiles=tiles)
    finally:
        ops.reset_compute_dtypes()


def test_persistent_two_plane_1x1_equals_one_workgroup_per_tile(dev):
    """the 1x1 twin of test_gpu_h2.test_persistent_layer1_kernel_equals_one_workgroup_per_tile (3x3 only): r50.l1.reduce256 (256 -> 64, 56 x 56)
    in fp32h2 at 37 frames takes the two-plane 32x32x16 kernel with halo 0 and persistent workgroups; its forward (BatchNorm partial sums,
    recorded maximum) and the 64-column data gradient of the matching expand convolution (plain, accumulating, with the BatchNorm-backward
    sums in its epilogue - the da of the last stage in ResBlockFn.backward) are bit-identical to one workgroup per tile (lmkd_conv_set_persistent(0))."""
    import litemkd_amd
    from litemkd_amd import ops
    L = litemkd_amd.lib()
    g = torch.Generator(device=dev).manual_seed(5)
    frames, H, Ck, C = 37, 56, 256, 64
    x = torch.relu(torch.randn(frames, H, H, Ck, device=dev, generator=g))
    w = torch.randn(C, Ck, 1, 1, device=dev, generator=g) * (2.0 / Ck) ** 0.5              # reduce: 256 -> 64
    dy = torch.randn(frames, H, H, Ck, device=dev, generator=g) * 1e-2                      # gradient of the expand convolution's output
    w2 = torch.randn(Ck, C, 1, 1, device=dev, generator=g) * (2.0 / C) ** 0.5              # expand: 64 -> 256; its data gradient has 64 columns
    res = torch.randn(frames, H, H, C, device=dev, generator=g)
    ops.set_conv_compute_dtype("fp32h2")
    try:
        ops.amax_compute(x)
        ops.amax_compute(dy)
        wp, wd = ops._pack_weights(w, Ck, 0), ops._pack_weights(w2, C, 1)
        assert T.plan(L, 0, frames, ("reduce256", H, Ck, Ck, C, 1, 1, 0))[::4] == (11, 1)
        gam, bet = 1 + 0.1 * torch.randn(C, device=dev, generator=g), 0.1 * torch.randn(C, device=dev, generator=g)
        c, st = ops._conv_bn_train_or_eval(x, w, Ck, 1, 0, gam, bet, torch.zeros(C, device=dev), torch.ones(C, device=dev), True)      # the BatchNorm whose backward sums ride in the data gradient

        def run():
            words = ops._amax_slot(dev)
            y, p = ops.conv_fwd(x, wp, C, 1, 1, 1, 0, True, amax_out=words)[:2]
            dx = ops.conv_bwd_data(dy, wd, (frames, H, H, C), Ck, 1, 1, 1, 0)
            acc = res.clone()
            ops.conv_bwd_data(dy, wd, (frames, H, H, C), Ck, 1, 1, 1, 0, out=acc, accumulate=True)
            dxb, pb = ops.conv_bwd_data(dy, wd, (frames, H, H, C), Ck, 1, 1, 1, 0, bn=(c, st))
            torch.cuda.synchronize()
            return y, p, float(words.view(torch.float32).view(2, 64, 16)[0, :, 0].max()), dx, acc, dxb, pb
        n0 = L.value("lmkd_conv_h2_launches")
        a = run()
        ran = L.value("lmkd_conv_h2_launches") - n0
        L.call("lmkd_conv_set_persistent", 0)
        b = run()
    finally:
        L.call("lmkd_conv_set_persistent", 1)
        ops.reset_compute_dtypes()
    assert ran == 4 and a[6] is not None, (ran, a[6])      # every launch took the two-plane form, the last one with the fused sums
    for u, v in zip(a, b):
        assert torch.equal(u, v) if torch.is_tensor(u) else u == v
    y64 = F.conv2d(nchw(x).cpu().double(), w.cpu().double())
    assert float((nchw(a[0]).cpu().double() - y64).norm() / y64.norm()) < 1.5e-6
