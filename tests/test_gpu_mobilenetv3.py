"""GPU: the MobileNetV3-Large students (moblienetv3_fc2 / moblienetv3) - every kernel of csrc/mobile.hip against torch-CPU in fp64
(anchored: no worse than 3 x torch's own fp32 CPU error), the whole backbone and whole episodes against the restatement in
tests/_mnv3_ref.py, run-to-run determinism, and the training loop / evaluator with the new backbone."""
import pytest
import torch
import torch.nn.functional as F

from _anchor import anchored, anchored_dict
import _mnv3_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from litemkd_amd import ops
    ops.reset_compute_dtypes()
    return torch.device("cuda", 0)


def _lib():
    from litemkd_amd._lib import lib
    return lib()


def _s():
    from litemkd_amd import ops
    return ops._stream()


def _p(t):
    import ctypes
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _both(fn, *cpu_inputs):
    """fn evaluated on fp32 and fp64 copies of the CPU inputs (leaves with grad) -> ((out32, leaves32), (out64, leaves64))"""
    res = []
    for dt in (torch.float32, torch.float64):
        leaves = [t.detach().to(dt).requires_grad_() for t in cpu_inputs]
        res.append((fn(*leaves), leaves))
    return res


# every (K, stride, C, H) of the network's depthwise layers, + odd sizes at stride 2 (7 -> 4, 14 -> 7, 37 -> 19)
DW_CASES = [(3, 1, 16, 112), (3, 2, 64, 112), (3, 1, 72, 56), (5, 2, 72, 56), (5, 1, 120, 28), (3, 2, 240, 28), (3, 1, 200, 14),
            (3, 1, 184, 14), (3, 1, 480, 14), (3, 1, 672, 14), (5, 2, 672, 14), (5, 1, 960, 7),
            (3, 2, 24, 7), (5, 2, 40, 14), (5, 2, 16, 7), (3, 2, 120, 37)]


@pytest.mark.parametrize("K,S,C,H", DW_CASES)
def test_depthwise_fwd_dgrad_wgrad(dev, K, S, C, H):
    N = 3
    g = torch.Generator().manual_seed(K * 1000 + S * 100 + C + H)
    x = torch.randn(N, C, H, H, generator=g)
    w = torch.randn(C, 1, K, K, generator=g) * 0.3
    P = (K - 1) // 2
    Ho = (H + 2 * P - K) // S + 1
    dy = torch.randn(N, C, Ho, Ho, generator=g)
    (y32, l32), (y64, l64) = _both(lambda a, b: F.conv2d(a, b, None, S, P, 1, C), x, w)
    y32.backward(dy)
    y64.backward(dy.double())
    L = _lib()
    xd, wd, dyd = nhwc(x).to(dev), w.to(dev), nhwc(dy).to(dev)
    T = L.value("lmkd_mnv3_stat_tiles", N * Ho * Ho)
    y = torch.empty(N, Ho, Ho, C, device=dev)
    part = torch.empty(T, C, 2, device=dev)
    L.call("lmkd_dw_conv_fwd", _p(xd), _p(wd), _p(y), _p(part), N, H, H, C, K, S, _s())
    dx = torch.empty_like(xd)
    L.call("lmkd_dw_conv_bwd_data", _p(dyd), _p(wd), _p(dx), N, H, H, C, K, S, _s())
    ws = torch.empty(L.value("lmkd_dw_conv_bwd_weight_workspace", N, H, H, C, K, S), dtype=torch.uint8, device=dev)
    dw = torch.full_like(wd, float("nan"))
    L.call("lmkd_dw_conv_bwd_weight", _p(xd), _p(dyd), _p(dw), _p(ws), ws.numel(), N, H, H, C, K, S, 0, _s())
    dw2 = torch.ones_like(wd)
    L.call("lmkd_dw_conv_bwd_weight", _p(xd), _p(dyd), _p(dw2), _p(ws), ws.numel(), N, H, H, C, K, S, 1, _s())
    torch.cuda.synchronize()
    anchored("dw fwd", nchw(y), y32, y64)
    anchored("dw dgrad", nchw(dx), l32[0].grad, l64[0].grad)
    anchored("dw wgrad", dw, l32[1].grad, l64[1].grad)
    assert torch.equal(dw2, dw + 1.0) or float((dw2 - dw - 1).abs().max()) <= 1e-6 * float(dw.abs().max() + 1)
    # the BatchNorm partial sums of the epilogue: column sums and sums of squares of y
    ps = part.double().sum(0).cpu()
    ref = torch.stack([y64.detach().sum((0, 2, 3)), (y64.detach() ** 2).sum((0, 2, 3))], 1)
    assert float((ps - ref).abs().max() / ref.abs().max()) < 1e-5


def _bn_ref(act, res_flag):
    def f(x, gamma, beta, *res):
        y = F.batch_norm(x, None, None, gamma, beta, True, 0.01, 1e-3)
        y = F.relu(y) if act == 1 else (F.hardswish(y) if act == 2 else y)
        return y + res[0] if res_flag else y
    return f


@pytest.mark.parametrize("act,res,C", [(0, True, 24), (1, False, 72), (2, False, 40), (2, False, 960), (0, False, 16)])
def test_bn_act_train_fwd_bwd(dev, act, res, C):
    from litemkd_amd import ops
    N, H = 4, 14
    g = torch.Generator().manual_seed(act * 10 + C)
    x = torch.randn(N, C, H, H, generator=g) * 2 + 0.5
    gamma = torch.rand(C, generator=g) * 2 + 0.2
    beta = torch.randn(C, generator=g)
    r = torch.randn(N, C, H, H, generator=g)
    dy = torch.randn(N, C, H, H, generator=g)
    ins = (x, gamma, beta) + ((r,) if res else ())
    (o32, l32), (o64, l64) = _both(_bn_ref(act, res), *ins)
    o32.backward(dy)
    o64.backward(dy.double())
    xd = nhwc(x).to(dev)
    rows = N * H * H
    part = torch.empty(_lib().value("lmkd_mnv3_stat_tiles", rows), C, 2, device=dev)
    _lib().call("lmkd_col_stats", _p(xd), _p(part), rows, C, _s())
    upd = []
    rm, rv, nbt = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros((), dtype=torch.long, device=dev)
    stats = ops._mnv3_bn_stats(part, rows, (gamma.to(dev), beta.to(dev), rm, rv, nbt), True, upd)
    y = ops.mnv3_bn_act(xd, stats, act, nhwc(r).to(dev) if res else None)
    dx, dgamma, dbeta = ops.mnv3_bn_act_bwd(nhwc(dy).to(dev), xd, stats, gamma.to(dev), act)
    ops.mnv3_running_update(upd, [])
    torch.cuda.synchronize()
    anchored("bn_act fwd", nchw(y), o32, o64)
    anchored("bn_act dx", nchw(dx), l32[0].grad, l64[0].grad)
    anchored("bn_act dgamma", dgamma, l32[1].grad, l64[1].grad)
    anchored("bn_act dbeta", dbeta, l32[2].grad, l64[2].grad)
    x64 = x.double()
    m, v = x64.mean((0, 2, 3)), x64.var((0, 2, 3), unbiased=True)
    assert torch.allclose(rm.cpu().double(), 0.01 * m, rtol=1e-5, atol=1e-7)
    assert torch.allclose(rv.cpu().double(), 0.99 + 0.01 * v, rtol=1e-5, atol=1e-7)
    assert int(nbt) == 1


def test_hardswish_boundaries_and_eval_mode(dev):
    from litemkd_amd import ops
    C = 16
    vals = torch.tensor([-3.0, 3.0, -3.0001, 2.9999, 0.0, -4.0, 5.0, 1.5])
    x = vals.repeat(4 * C).reshape(4 * 8, C)      # rows x C, each value in every channel
    L = _lib()
    # a table that makes the BatchNorm the identity (mean 0, invstd 1, scale 1, shift 0): the activation sees x exactly
    st = torch.zeros(5, C)
    st[1], st[2], st[4] = 1.0, 1.0, 1.0
    xd, std = x.to(dev), st.to(dev)
    y = ops.mnv3_bn_act(xd, std, ops.ACT_HARDSWISH)
    assert torch.equal(y.cpu()[x == 3.0], torch.full_like(y.cpu()[x == 3.0], 3.0))
    assert torch.equal(y.cpu()[x == -3.0].abs(), torch.zeros_like(y.cpu()[x == -3.0]))
    assert float((y.cpu().double() - F.hardswish(x.double())).abs().max()) < 1e-6
    # backward: g = dy hardswish'(x) with aten's end points (0 at -3, 1 at +3), then the train-mode BatchNorm formula with this table
    dy = torch.randn(x.shape, generator=torch.Generator().manual_seed(4))
    dx, dgamma, dbeta = ops.mnv3_bn_act_bwd(dy.to(dev), xd, std, torch.ones(C, device=dev), ops.ACT_HARDSWISH)
    xx = x.double().requires_grad_()
    F.hardswish(xx).backward(dy.double())
    gref = xx.grad
    assert float(gref[x == -3.0].abs().max()) == 0.0 and torch.equal(gref[x == 3.0], dy.double()[x == 3.0])
    n = x.shape[0]
    ref = gref - gref.sum(0) / n - x.double() * (gref * x.double()).sum(0) / n
    assert float((dx.cpu().double() - ref).abs().max()) < 1e-5
    assert float((dbeta.cpu().double() - gref.sum(0)).abs().max()) < 1e-5
    assert float((dgamma.cpu().double() - (gref * x.double()).sum(0)).abs().max()) < 1e-5
    # eval mode: the table from the running statistics (eps 1e-3)
    g = torch.Generator().manual_seed(6)
    C = 40
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    xe = torch.randn(2, C, 9, 9, generator=g) * 3
    stats = ops._mnv3_bn_stats(None, 0, (gamma.to(dev), beta.to(dev), rm.to(dev), rv.to(dev), None), False, None)
    ye = ops.mnv3_bn_act(nhwc(xe).to(dev), stats, ops.ACT_HARDSWISH)
    r32 = F.hardswish(F.batch_norm(xe, rm, rv, gamma, beta, False, 0.01, 1e-3))
    r64 = F.hardswish(F.batch_norm(xe.double(), rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.01, 1e-3))
    anchored("bn_act eval", nchw(ye), r32, r64)


def _se_ref(a, w1, b1, w2, b2):
    s = a.mean((2, 3), keepdim=True)
    s = F.hardsigmoid(F.conv2d(F.relu(F.conv2d(s, w1, b1)), w2, b2))
    return a * s


@pytest.mark.parametrize("N,H,C,Q", [(16, 28, 72, 24), (8, 14, 480, 120), (16, 7, 960, 240)])
def test_squeeze_excitation(dev, N, H, C, Q):
    from litemkd_amd import ops
    g = torch.Generator().manual_seed(C)
    a = torch.randn(N, C, H, H, generator=g).abs()
    w1, b1 = torch.randn(Q, C, 1, 1, generator=g) * C ** -0.5, torch.randn(Q, generator=g) * 0.1
    w2, b2 = torch.randn(C, Q, 1, 1, generator=g) * Q ** -0.5 * 3, torch.randn(C, generator=g)
    dy = torch.randn(N, C, H, H, generator=g)
    (o32, l32), (o64, l64) = _both(_se_ref, a, w1, b1, w2, b2)
    o32.backward(dy)
    o64.backward(dy.double())
    ins = [nhwc(a).to(dev).requires_grad_()] + [t.to(dev).requires_grad_() for t in (w1, b1, w2, b2)]
    y = ops.MnvSEFn.apply(*ins)
    y.backward(nhwc(dy).to(dev))
    torch.cuda.synchronize()
    anchored("se fwd", nchw(y), o32, o64)
    anchored("se da", nchw(ins[0].grad), l32[0].grad, l64[0].grad)
    for i, name in enumerate(("w1", "b1", "w2", "b2")):
        anchored("se d" + name, ins[i + 1].grad, l32[i + 1].grad, l64[i + 1].grad)


@pytest.mark.parametrize("N,H", [(2, 224), (3, 37)])
def test_stem_fwd_and_wgrad(dev, N, H):
    g = torch.Generator().manual_seed(H)
    x = torch.rand(N, 3, H, H, generator=g)
    w = torch.randn(16, 3, 3, 3, generator=g) * 0.3
    Ho = (H - 1) // 2 + 1
    dy = torch.randn(N, 16, Ho, Ho, generator=g)
    (y32, l32), (y64, l64) = _both(lambda a, b: F.conv2d(a, b, None, 2, 1), x, w)
    y32.backward(dy)
    y64.backward(dy.double())
    L = _lib()
    x4 = torch.zeros(N, H, H, 4)
    x4[..., :3] = nhwc(x)
    x4, wd, dyd = x4.to(dev), w.to(dev), nhwc(dy).to(dev)
    y = torch.empty(N, Ho, Ho, 16, device=dev)
    part = torch.empty(L.value("lmkd_mnv3_stat_tiles", N * Ho * Ho), 16, 2, device=dev)
    L.call("lmkd_stem3x3_fwd", _p(x4), _p(wd), _p(y), _p(part), N, H, H, _s())
    ws = torch.empty(L.value("lmkd_stem3x3_bwd_weight_workspace", N, H, H), dtype=torch.uint8, device=dev)
    dw = torch.empty_like(wd)
    L.call("lmkd_stem3x3_bwd_weight", _p(x4), _p(dyd), _p(dw), _p(ws), ws.numel(), N, H, H, 0, _s())
    torch.cuda.synchronize()
    anchored("stem fwd", nchw(y), y32, y64)
    anchored("stem wgrad", dw, l32[1].grad, l64[1].grad)
    ps = part.double().sum(0).cpu()
    ref = torch.stack([y64.detach().sum((0, 2, 3)), (y64.detach() ** 2).sum((0, 2, 3))], 1)
    assert float((ps - ref).abs().max() / ref.abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------------------------------------
# whole backbone / episodes against the restatement
# ------------------------------------------------------------------------------------------------------------------------------
def _params(module, dtype):
    out = {}
    for k, v in module.state_dict().items():
        v = v.detach().cpu().clone()
        if v.is_floating_point():
            v = v.to(dtype)
            if "running" not in k and not k.endswith("pe.pe"):
                v.requires_grad_()
        out[k] = v
    return out


def _grads(params):
    return {k: v.grad for k, v in params.items() if torch.is_tensor(v) and v.is_leaf and v.requires_grad and v.grad is not None}


# Whole-episode gradients and running statistics: the 1x1 convolutions and the heads are GEMMs in the library's three-bf16-plane
# arithmetic and make up most of this network; against torch-CPU (which accumulates its CPU reductions in double) their error measured
# up to 4.2 x torch's fp32 error (fc2.weight at 400 frames; 3.0 on a BatchNorm bias gradient at 80 frames, 3.7 on an exactly-zero running
# mean).  The ResNet episode tests' factor 3 is therefore 5 here; every kernel of csrc/mobile.hip is held to factor 3 above.
EPISODE_FACTOR = 5.0


def _grads_match(hip, g32, g64):
    """anchored_dict over every parameter gradient, except those whose exact value is zero: the bias gradient of a BatchNorm whose
    output reaches nothing but train-mode BatchNorms through linear layers (the project BatchNorm of block 1 feeding block 2's expand
    convolution, ...) vanishes identically, so both fp32 evaluations of it are pure rounding residue - sums of up to 400 x 112^2 rounding
    errors of the incoming gradient, whose size depends on the arithmetic of the GEMM that produced it (three truncated bf16 planes here,
    round-to-nearest fp32 in torch).  Those are held to an absolute bound instead: 1e-6 of the largest gradient, or 4 x torch's residue."""
    gmax = max(float(v.abs().max()) for v in g64.values())
    zero = {k for k, v in g64.items() if float(v.abs().max()) <= 1e-9 * gmax}
    for k in zero:
        bound = max(1e-6 * gmax, 4 * float(g32[k].abs().max()))
        assert float(hip[k].abs().max()) <= bound, (k, float(hip[k].abs().max()), float(g32[k].abs().max()), gmax)
    keep = [k for k in g64 if k not in zero]
    assert len(keep) > len(zero)
    anchored_dict({k: hip[k] for k in keep}, {k: g32[k] for k in keep}, {k: g64[k] for k in keep}, factor=EPISODE_FACTOR)


def _check_running(module, p32, p64, refprefix=""):
    """running mean / var of every BatchNorm of the trunk against the restatement's updated copies (key of module + refprefix), and
    num_batches_tracked == 2 (the episode's two trunk calls)"""
    n = 0
    for k, v in module.state_dict().items():
        if ".mobile." not in "." + k:
            continue
        if "running" in k:
            # running_mean of a BatchNorm fed by a 1x1 convolution of a BatchNorm output is exactly zero (a linear map of zero-mean
            # channels): judged on an absolute floor of 1e-6
            anchored(k, v, p32[refprefix + k], p64[refprefix + k], factor=EPISODE_FACTOR, floor=2e-6, abs_floor=1e-6)
            n += 1
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 2 and int(p64[refprefix + k]) == 2, k
    assert n == 2 * 46       # 46 BatchNorm layers


def test_backbone_train_two_calls_small(dev):
    """mobile_large_2fc alone, 2 videos x 8 frames of 224^2 per call: output, every parameter gradient, running statistics and
    num_batches_tracked after the episode's two trunk calls"""
    from litemkd_amd.model.model_select import Student
    from litemkd_amd.options import default_args
    torch.manual_seed(11)
    args = default_args(device=dev, model_backbone="moblienetv3_fc2")
    bb = Student(args).backbone.to(dev)
    g = torch.Generator().manual_seed(12)
    ctx, tgt = torch.rand(16, 3, 224, 224, generator=g), torch.rand(16, 3, 224, 224, generator=g)
    wts = {k: torch.randn(2, 8, 2048, generator=g) for k in ("c1", "c2", "t1", "t2")}
    p32, p64 = _params(bb, torch.float32), _params(bb, torch.float64)
    c, t = bb(ctx.to(dev), None, tgt.to(dev))
    loss = sum((o * wts[n].to(dev)).sum() for o, n in ((c["context_features_1"], "c1"), (c["context_features_2"], "c2"),
                                                         (t["target_features_1"], "t1"), (t["target_features_2"], "t2")))
    loss.backward()
    torch.cuda.synchronize()
    refs, bps = [], []
    for p, dt in ((p32, torch.float32), (p64, torch.float64)):
        bp = {"backbone." + k: v for k, v in p.items()}
        rc, rt = R.backbone_2fc(ctx.to(dt), tgt.to(dt), bp)
        bps.append(bp)
        rl = sum((o * wts[n].to(dt)).sum() for o, n in ((rc["context_features_1"], "c1"), (rc["context_features_2"], "c2"),
                                                          (rt["target_features_1"], "t1"), (rt["target_features_2"], "t2")))
        rl.backward()
        refs.append((rc, rt))
    for key in ("context_features_1", "context_features_2"):
        anchored(key, c[key], refs[0][0][key], refs[1][0][key])
    for key in ("target_features_1", "target_features_2"):
        anchored(key, t[key], refs[0][1][key], refs[1][1][key])
    hip = {k: v.grad for k, v in bb.named_parameters()}
    anchored_dict(hip, _grads(p32), _grads(p64))
    assert len(hip) == len(_grads(p64))
    _check_running(bb, bps[0], bps[1], "backbone.")


def _episode_ref(ep, p, way, shot, two_heads=True):
    from oracle import ref_cpu as O
    cp = {k[len("classifier.transformers."):]: v for k, v in p.items() if k.startswith("classifier.transformers.")}
    if two_heads:
        ctx, tgt = R.backbone_2fc(ep["support_set"], ep["target_set"], p)
        return O.clf_TRX_2fcsup(ctx, ep["support_labels"], tgt, cp, way, shot)
    ctx, tgt = R.backbone_1fc(ep["support_set"], ep["target_set"], p)
    return O.trx_logits(ctx, ep["support_labels"], tgt, cp, way)


def _dbl(ep):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in ep.items()}


@pytest.mark.parametrize("shot,query,img", [(5, 5, 224)])
def test_full_episode_moblienetv3_fc2(dev, shot, query, img):
    """moblienetv3_fc2 + TRX_2fcsup + fc_2_sup_dist, 5-way 5-shot, 400 frames of 224^2: loss, every parameter gradient, running
    statistics and num_batches_tracked against the restatement (fp32 and fp64 on the CPU)"""
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from oracle import ref_cpu as O
    torch.manual_seed(21)
    args = default_args(shot=shot, query_per_class=query, img_size=img, trans_dropout=0.0, device=dev, model_backbone="moblienetv3_fc2")
    student, teacher = Student(args).to(dev), Teacher(args).to(dev)
    ep = O.make_episode(2024, 5, shot, query, img=img)
    labels = ep["target_labels"].long()
    p32, p64 = _params(student, torch.float32), _params(student, torch.float64)
    tp = {k[len("classifier.transformers."):]: v.detach().cpu() for k, v in teacher.state_dict().items() if k.startswith("classifier.transformers.")}
    out = student(ep["support_set"].to(dev), ep["support_labels"].to(dev), ep["target_set"].to(dev))
    tl = teacher(ep["support_set_feature_teacher"].to(dev), ep["support_labels"].to(dev), ep["target_set_feature_teacher"].to(dev))["logits"]
    loss = Distiller("fc_2_sup_dist", args.cfg, dev).fc_2_sup_dist(out["logits"], tl, labels.to(dev))["loss"]
    loss.backward()
    torch.cuda.synchronize()
    losses = []
    for p, e, tpp in ((p32, ep, tp), (p64, _dbl(ep), {k: v.double() for k, v in tp.items()})):
        lg = _episode_ref(e, p, 5, shot)
        t_l = O.clf_TRX_2fcsup_fixed(e["support_set_feature_teacher"], e["support_labels"], e["target_set_feature_teacher"], tpp, 5, shot)
        rl = O.distill_fc_2_sup_dist(lg, t_l, labels)["loss"]
        rl.backward()
        losses.append(rl)
    # a scalar: torch's fp32 error on it may be far below rounding level by chance, so the floor is smoke()'s 1e-5 relative
    anchored("loss", loss.reshape(1), losses[0].detach().reshape(1), losses[1].detach().reshape(1), floor=1e-5)
    hip = {k: v.grad for k, v in student.named_parameters() if v.grad is not None}
    assert len(hip) == len(_grads(p64))
    _grads_match(hip, _grads(p32), _grads(p64))
    _check_running(student, p32, p64)


def test_episode_moblienetv3_trx(dev):
    """moblienetv3 (one head, two tensors) + TRX: logits and every parameter gradient"""
    from litemkd_amd.model.model_select import Student
    from litemkd_amd.options import default_args
    from oracle import ref_cpu as O
    torch.manual_seed(31)
    args = default_args(shot=1, query_per_class=1, img_size=112, trans_dropout=0.0, device=dev, model_backbone="moblienetv3",
                        model_classifier="TRX")
    student = Student(args).to(dev)
    ep = O.make_episode(77, 5, 1, 1, img=112)
    labels = ep["target_labels"].long()
    p32, p64 = _params(student, torch.float32), _params(student, torch.float64)
    out = student(ep["support_set"].to(dev), ep["support_labels"].to(dev), ep["target_set"].to(dev))
    logits = out["logits"]
    assert torch.is_tensor(logits) and tuple(out["context_features"].shape) == (5, 8, 2048)
    F.cross_entropy(logits, labels.to(dev)).backward()
    torch.cuda.synchronize()
    refs = []
    for p, e in ((p32, ep), (p64, _dbl(ep))):
        lg = _episode_ref(e, p, 5, 1, two_heads=False)
        F.cross_entropy(lg, labels).backward()
        refs.append(lg)
    anchored("logits", logits, refs[0], refs[1])
    _grads_match({k: v.grad for k, v in student.named_parameters() if v.grad is not None}, _grads(p32), _grads(p64))
    _check_running(student, p32, p64)


def test_determinism_bit_identical(dev):
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from oracle import ref_cpu as O
    torch.manual_seed(41)
    args = default_args(shot=2, query_per_class=1, img_size=160, trans_dropout=0.0, device=dev, model_backbone="moblienetv3_fc2")
    student, teacher = Student(args).to(dev), Teacher(args).to(dev)
    sd0 = {k: v.clone() for k, v in student.state_dict().items()}
    ep = O.make_episode(5, 5, 2, 1, img=160)
    runs = []
    for _ in range(2):
        student.load_state_dict(sd0)
        student.zero_grad(set_to_none=True)
        out = student(ep["support_set"].to(dev), ep["support_labels"].to(dev), ep["target_set"].to(dev))
        tl = teacher(ep["support_set_feature_teacher"].to(dev), ep["support_labels"].to(dev), ep["target_set_feature_teacher"].to(dev))["logits"]
        loss = Distiller("fc_2_sup_dist", args.cfg, dev).fc_2_sup_dist(out["logits"], tl, ep["target_labels"].long().to(dev))["loss"]
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), {k: v.grad.clone() for k, v in student.named_parameters() if v.grad is not None},
                     {k: v.clone() for k, v in student.state_dict().items() if "running" in k}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert len(runs[0][1]) > 150 and runs[0][1].keys() == runs[1][1].keys()
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k


def test_train_loop_and_evaluator(dev, tmp_path):
    from litemkd_amd import trainloop as TL
    from litemkd_amd.evaluate import Evaluator
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from litemkd_amd.utils import aggregate_accuracy
    cfg = default_args(shot=1, query_per_class=1, img_size=112, device=dev, training_iterations=4, tasks_per_batch=2,
                       learning_rate=1e-2, print_freq=100, model_backbone="moblienetv3_fc2", save_dir=str(tmp_path), num_test_tasks=2)
    torch.manual_seed(3)
    student, teacher = Student(cfg).to(dev), Teacher(cfg).to(dev)
    opt = TL.FusedOptimizer(student, "sgd", cfg.learning_rate)
    sch = TL.MultiStepLR(opt, cfg.sch)
    w0 = opt.bucket.flat.clone()
    src = TL.SyntheticEpisodes(cfg, base_seed=5, device=dev)
    losses, accs = TL.train(student, teacher, src, Distiller(cfg.distill_name, cfg.cfg, dev), opt, sch, aggregate_accuracy, cfg)
    assert len(losses) == 4 and all(l == l for l in losses)
    assert opt.steps == 2
    assert float((opt.bucket.flat - w0).abs().max()) > 0
    nbt = student.state_dict()["backbone.mobile.0.16.1.num_batches_tracked"]
    assert int(nbt) == 8          # two trunk calls per episode
    acc = TL.test(student, TL.SyntheticEpisodes(cfg, base_seed=9, device=dev, train=False), aggregate_accuracy, cfg)
    assert 0.0 <= acc[cfg.dataset]["accuracy"] <= 100.0
    assert int(student.state_dict()["backbone.mobile.0.16.1.num_batches_tracked"]) == 8      # eval: running statistics untouched
    path = TL.save_checkpoint(student, 3, cfg)
    ecfg = default_args(**{**vars(cfg), "test_model": "student", "test_model_path": path})
    res = Evaluator(ecfg, log=lambda s: None).test()
    assert 0.0 <= res[cfg.dataset]["accuracy"] <= 100.0
