"""GPU: the teacher's pretraining and feature extraction - the three kernels of csrc/clipcls.hip, Action_Recognition_Resnet50 forward and
backward, the pretraining loop and both extraction stages end to end.  Every tolerance is tests/_anchor.anchored's: the HIP error
against an fp64 evaluation is at most 3 x torch-CPU-fp32's own error against it, plus 2e-6.  Tensors whose exact value is zero are
asserted to be exactly zero."""
import argparse
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pretrain_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    return torch.device("cuda", 0)


def _lib():
    import litemkd_amd
    return litemkd_amd.lib()


# ---------------------------------------------------------------------------------------------------------------------------------
# global average pool
# ---------------------------------------------------------------------------------------------------------------------------------
POOL_CASES = [(8, 7, 7, 2048, 1), (8, 7, 7, 2048, 8), (6, 2, 2, 256, 3), (4, 1, 1, 64, 2), (64, 7, 7, 2048, 8)]      # (F, H, W, C, G)


@pytest.mark.parametrize("act", ["fp32", "bf16"])
@pytest.mark.parametrize("F_,H,W,C,G", POOL_CASES)
def test_global_avgpool_vs_fp64(dev, F_, H, W, C, G, act):
    """forward and backward through the C entry points into NaN-filled outputs, twice (bit-identical), and through ops.GlobalAvgPoolFn.
    In bf16 the input is a bf16 tensor and the fp64 reference reads the same rounded values; the input gradient is stored as bf16, so
    the torch-CPU comparator rounds its fp32 result to bf16 once too, as anything that stores that type must."""
    from litemkd_amd import ops
    from _anchor import anchored
    from litemkd_amd.ops import _p, _stream
    L = _lib()
    g = torch.Generator().manual_seed(F_ * 131 + C + G)
    x = torch.randn(F_, H, W, C, generator=g) + 0.5
    dy = torch.randn(F_ // G, C, generator=g)
    if act == "bf16":
        ops.set_conv_compute_dtype("bf16")
        ops.set_activation_dtype("bf16")
        x = x.to(torch.bfloat16)
    try:
        xd, dyd = x.to(dev), dy.to(dev)
        outs = []
        for _ in range(2):
            y = torch.full((F_ // G, C), float("nan"), device=dev)
            dx = torch.full((F_, H, W, C), float("nan"), device=dev).to(xd.dtype)
            L.call("lmkd_global_avgpool_fwd", _p(xd), _p(y), F_, H, W, C, G, _stream())
            L.call("lmkd_global_avgpool_bwd", _p(dyd), _p(dx), F_, H, W, C, G, _stream())
            outs.append((y.cpu(), dx.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        xa = xd.clone().requires_grad_()
        ya = ops.GlobalAvgPoolFn.apply(xa, G)
        ya.backward(dy.to(dev))
        assert torch.equal(ya.detach().cpu(), outs[0][0]) and torch.equal(xa.grad.cpu(), outs[0][1]) and xa.grad.dtype == xd.dtype
    finally:
        ops.reset_compute_dtypes()
    y_hip, dx_hip = outs[0]
    assert bool(torch.isfinite(y_hip).all()) and bool(torch.isfinite(dx_hip.float()).all())
    P = G * H * W

    def ref(dt):
        v = x.to(dt).reshape(F_ // G, P, C)
        return v.mean(dim=1), (dy.to(dt) / P).reshape(F_ // G, 1, C).expand(-1, P, -1).reshape(F_, H, W, C)
    y32, dx32 = ref(torch.float32)
    y64, dx64 = ref(torch.float64)
    if act == "bf16":
        dx32 = dx32.to(torch.bfloat16)
    ey = anchored("pool y", y_hip, y32, y64)
    edx = anchored("pool dx", dx_hip, dx32, dx64)
    # the clip feature in one pass against the mean over frames of per-frame means
    mm32 = x.float().mean(dim=(1, 2)).reshape(F_ // G, G, C).mean(dim=1)
    mm64 = x.double().mean(dim=(1, 2)).reshape(F_ // G, G, C).mean(dim=1)
    emm = anchored("pool vs mean of means", y_hip, mm32, mm64)
    print("pool", (F_, H, W, C, G), act, "y", ey, "dx", edx, "mean of means", emm)


def test_global_avgpool_refuses_the_wrong_storage_type(dev):
    from litemkd_amd import ops
    with pytest.raises(RuntimeError, match="storage type"):
        ops.GlobalAvgPoolFn.apply(torch.zeros(2, 2, 2, 8, device=dev, dtype=torch.bfloat16), 1)
    with pytest.raises(RuntimeError, match="no multiple"):
        ops.GlobalAvgPoolFn.apply(torch.zeros(3, 2, 2, 8, device=dev), 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# softmax cross-entropy
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels_on", ["host", "device"])
@pytest.mark.parametrize("R_,C", [(1, 1), (8, 5), (8, 64), (8, 65), (13, 101), (3, 1000)])
def test_softmax_ce_vs_fp64(dev, R_, C, labels_on):
    from litemkd_amd import ops
    from _anchor import anchored
    g = torch.Generator().manual_seed(R_ * 1009 + C)
    logits = 100.0 * torch.randn(R_, C, generator=g)
    labels = torch.randint(0, C, (R_,), generator=g)
    if C >= 5:      # two equal maxima in one row, the label on the second: the prediction is the first, the row counts as a miss
        r = R_ // 2
        top = float(logits[r].max()) + 1.0
        logits[r, 1] = logits[r, C - 2] = top
        labels[r] = C - 2
    if R_ > 1:      # and one certain hit
        labels[0] = int(logits[0].argmax())
    ld = logits.to(dev).requires_grad_()
    lab = labels if labels_on == "host" else labels.to(dev)
    outs = []
    for _ in range(2):
        ld.grad = None
        loss, acc, pred = ops.softmax_ce(ld, lab, with_pred=True)
        loss.backward()
        outs.append((loss.detach().cpu(), acc.cpu(), pred.cpu(), ld.grad.cpu().clone()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))      # fixed summation order
    loss_hip, acc_hip, pred_hip, g_hip = outs[0]
    loss32, g32, _, _ = R.cross_entropy_parts(logits, labels)
    loss64, g64, pred64, acc64 = R.cross_entropy_parts(logits.double(), labels)
    assert torch.equal(pred_hip, pred64), (pred_hip, pred64)
    assert float(acc_hip) == pytest.approx(float(acc64), abs=1e-6)
    if C >= 5:
        assert int(pred_hip[R_ // 2]) == 1 and float(acc_hip) < 1.0
    if C == 1:      # one class: the loss and its gradient are exactly zero
        assert float(loss_hip) == 0.0 and float(g_hip.abs().max()) == 0.0 and float(acc_hip) == 1.0
        return
    el = anchored("ce loss", loss_hip.reshape(1), loss32.reshape(1), loss64.reshape(1))
    eg = anchored("ce gradient", g_hip, g32, g64)
    print("softmax_ce", (R_, C), labels_on, "loss", el, "gradient", eg)


def test_softmax_ce_labels_outside_the_range(dev):
    """host labels are refused before anything is launched; device labels are not read back: the kernel indexes with none outside the range
    and that row's loss is NaN (the gradient of the other rows is what it is without it)"""
    from litemkd_amd import ops
    logits = torch.randn(4, 6, device=dev)
    for bad in (6, -1):
        with pytest.raises(RuntimeError, match="outside"):
            ops.softmax_ce(logits, torch.tensor([1, bad, 0, 2]))
    loss, acc = ops.softmax_ce(logits, torch.tensor([6, 1, 0, 2], device=dev))
    assert math.isnan(float(loss)) and 0.0 <= float(acc) <= 0.75
    # a non-contiguous slice (the classifier drops the padding logits) goes through a copy
    wide = torch.randn(4, 8, device=dev).requires_grad_()
    l2, _ = ops.softmax_ce(wide[:, :6], torch.tensor([1, 5, 0, 2]))
    l2.backward()
    ref = F.cross_entropy(wide.detach().cpu().double()[:, :6], torch.tensor([1, 5, 0, 2]))
    assert float(l2.detach()) == pytest.approx(float(ref), rel=1e-5) and float(wide.grad[:, 6:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# SGD with momentum
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1028, 2 ** 20 + 4])
def test_sgd_momentum_vs_torch_fp64(dev, n):
    """5 steps of lmkd_sgd_momentum_step against torch.optim.SGD(momentum=0.9): `first` takes the gradient as the buffer whatever the
    buffer held (NaN here), the gradient is zeroed only when asked"""
    from _anchor import anchored
    from litemkd_amd.ops import _p, _stream, _f32
    L = _lib()
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(5)]
    lr, mom = 1e-2, 0.9
    p, buf = p0.to(dev), torch.full((n,), float("nan"), device=dev)
    for i, gr in enumerate(grads):
        gd = gr.to(dev)
        zero = i % 2
        L.call("lmkd_sgd_momentum_step", _p(p), _p(gd), _p(buf), _f32(lr), _f32(mom), n, int(i == 0), zero, _stream())
        assert (float(gd.abs().max()) == 0.0) if zero else torch.equal(gd.cpu(), gr)
    p32, b32 = torch.nn.Parameter(p0.clone()), None
    opt = torch.optim.SGD([p32], lr=lr, momentum=mom)
    for gr in grads:
        p32.grad = gr.clone()
        opt.step()
    b32 = opt.state[p32]["momentum_buffer"]
    p64, b64 = R.sgd_momentum(p0, grads, lr, mom)
    ep = anchored("sgd parameters", p.cpu(), p32.detach(), p64)
    eb = anchored("sgd momentum buffer", buf.cpu(), b32, b64)
    eu = anchored("sgd update", p.cpu().double() - p0.double(), p32.detach().double() - p0.double(), p64 - p0.double())
    print("sgd momentum n=%d" % n, "p", ep, "buffer", eb, "update", eu)


class _TwoPart(nn.Module):
    def __init__(self):
        super().__init__()
        self.convnet = nn.Sequential(nn.Linear(6, 5), nn.Linear(5, 3))
        self.fc = nn.Linear(3, 7)


def test_two_groups_over_one_model_keep_to_their_own_parameters(dev):
    from litemkd_amd import trainloop as TL
    from _anchor import anchored
    torch.manual_seed(3)
    model = _TwoPart().to(dev)
    lrs = {"convnet": 1e-6, "fc": 1e-2}
    opt = TL.MomentumSGD(model, {k: (k + ".", v, 0.9) for k, v in lrs.items()})
    names = [k for k, _ in model.named_parameters()]
    p0 = {k: v.detach().cpu().clone() for k, v in model.named_parameters()}
    g = torch.Generator().manual_seed(4)
    steps = [{k: torch.randn(p0[k].shape, generator=g) for k in names} for _ in range(3)]
    for i, gs in enumerate(steps):
        for k, prm in model.named_parameters():
            prm.grad.copy_(gs[k].to(dev))
        opt.step(zero_grad=(i == 1))
        zeroed = float(opt.bucket.grad.abs().max()) == 0.0
        assert zeroed == (i == 1)
    assert [grp["steps"] for grp in opt.groups.values()] == [3, 3]
    for k in names:
        lr = lrs[k.split(".")[0]]
        p64, _ = R.sgd_momentum(p0[k], [s[k] for s in steps], lr, 0.9)
        p32 = torch.nn.Parameter(p0[k].clone())
        o = torch.optim.SGD([p32], lr=lr, momentum=0.9)
        for s in steps:
            p32.grad = s[k].clone()
            o.step()
        got = dict(model.named_parameters())[k].detach().cpu()
        anchored(k, got, p32.detach(), p64)
        # the update itself, on its own scale: a trunk parameter stepped with fc's rate would be 10^4 off
        anchored(k + " update", got.double() - p0[k].double(), p32.detach().double() - p0[k].double(), p64 - p0[k].double())
    st = opt.state("fc")
    assert st["steps"] == 3 and st["momentum_buffer"].numel() == 32 and float(st["momentum_buffer"].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the model at 64 px
# ---------------------------------------------------------------------------------------------------------------------------------
class _MaskedReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, mask):
        ctx.save_for_backward(mask)
        return t * mask

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * mask, None


def test_model_forward_backward_and_extract_feature(dev):
    """2 videos x 4 frames of 64 x 64, 70 classes: logits, loss and every parameter gradient against the restatement over the oracle's
    ResNet-50 trunk in fp64, with the HIP path's ReLU masks and stem-pool selections imposed on both oracle runs as
    test_gpu_ops.test_resnet50_trunk_forward_backward imposes them (each checked to differ from the natural one only within rounding).
    Then extract_feature in eval mode: one video alone and inside a call of three videos, both against the fp64 eval forward."""
    from litemkd_amd import ops
    from litemkd_amd.teacher.action_recognition import Action_Recognition_Resnet50
    from oracle import ref_cpu as O
    from _anchor import anchored, anchored_dict, near_zero_limit
    from test_gpu_episode import _hip_relu_masks, _hip_pool_choices
    B, T, NC = 2, 4, 70
    g = torch.Generator().manual_seed(21)
    sd = O.init_trunk_from_shapes(O.resnet50_trunk_param_shapes(), g)
    fc_w, fc_b = torch.randn(NC, 2048, generator=g) / 2048 ** 0.5, 0.1 * torch.randn(NC, generator=g)
    model = Action_Recognition_Resnet50(argparse.Namespace(num_classes=NC))
    model.load_state_dict({**{"convnet." + k: v for k, v in sd.items()}, "fc.weight": fc_w, "fc.bias": fc_b}, strict=True)
    model = model.to(dev).train()
    x = torch.rand(B * T, 3, 64, 64, generator=g)
    labels = torch.tensor([69, 3])
    ops.BLOCK_TAPS = []
    try:
        logits = model(x.view(B, T, 3, 64, 64).to(dev))
        taps = ops.split_block_taps(ops.BLOCK_TAPS)
    finally:
        ops.BLOCK_TAPS = None
    assert tuple(logits.shape) == (B, NC)
    loss, acc = ops.softmax_ce(logits, labels)
    loss.backward()
    ops.join_all_streams()
    torch.cuda.synchronize()
    masks, pools = _hip_relu_masks(taps), _hip_pool_choices(taps)
    assert len(masks) == 1 + 3 * 16 and len(pools) == 1
    flips, ref32 = [0, 0], {}

    def oracle(dt):
        osd = {k: (v.clone().to(dt).requires_grad_() if v.is_floating_point() and "running" not in k else
                   (v.clone().to(dt) if v.is_floating_point() else v.clone())) for k, v in sd.items()}
        w, b = fc_w.clone().to(dt).requires_grad_(), fc_b.clone().to(dt).requires_grad_()
        site = [0]

        def hook(t):
            m = masks[site[0]]
            site[0] += 1
            if dt == torch.float32:
                ref32["relu", site[0]] = t.detach()
            else:
                diff = m != (t.detach() > 0)
                flips[0] += int(diff.sum())
                flips[1] += m.numel()
                assert not bool(diff.any()) or float(t.detach()[diff].abs().max()) < near_zero_limit(t.detach(), ref32["relu", site[0]]), site[0]
            return _MaskedReLU.apply(t, m.to(dt))

        def pool_hook(kind, t):
            assert kind == "stem"      # the classifier's pool is an average: no selection
            idx = pools[0][kind]
            v = t.flatten(2).gather(2, idx.flatten(2)).reshape(idx.shape)
            if dt == torch.float32:
                ref32[kind] = t.detach()
            else:
                d = F.max_pool2d(t.detach(), 3, 2, 1) - v.detach()
                assert float(d.max()) <= near_zero_limit(t.detach(), ref32[kind]), float(d.max())
            return v
        O.RELU_HOOK, O.POOL_HOOK = hook, pool_hook
        try:
            lg, _ = R.clip_logits(lambda a, s, tr: O.resnet50_trunk(a, s, tr, True), osd, x.to(dt), T, w, b, True)
        finally:
            O.RELU_HOOK = O.POOL_HOOK = None
        assert site[0] == len(masks)
        ls = F.cross_entropy(lg, labels)
        ls.backward()
        grads = {"convnet." + k: v.grad for k, v in osd.items() if v.requires_grad}
        grads.update({"fc.weight": w.grad, "fc.bias": b.grad})
        return lg.detach(), ls.detach(), grads, osd
    lg32, ls32, g32, osd32 = oracle(torch.float32)
    lg64, ls64, g64, _ = oracle(torch.float64)
    assert flips[0] <= max(8, flips[1] // 100000), flips
    hip = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}
    assert set(hip) == set(g64)
    e_lg = anchored("logits", logits.detach().cpu(), lg32, lg64)
    e_ls = anchored("loss", loss.detach().cpu().reshape(1), ls32.reshape(1), ls64.reshape(1))
    worst = anchored_dict(hip, g32, g64)
    print("model 64 px: logits", e_lg, "loss", e_ls, "worst gradient ratio", worst, "mask flips", flips)

    # extract_feature, eval mode, with the running statistics the training forward left
    model.eval()
    state = {k[len("convnet."):]: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith("convnet.")}
    vids = torch.rand(3 * T, 3, 64, 64, generator=g)
    alone = model.extract_feature(vids[T:2 * T].to(dev)).cpu()
    three = model.extract_feature(vids.to(dev)).cpu()
    nchw4 = model.extract_feature(F.pad(vids[T:2 * T].permute(0, 2, 3, 1), (0, 1)).contiguous().to(dev)).cpu()      # the frame transform's layout
    assert tuple(alone.shape) == (T, 2048) and tuple(three.shape) == (3 * T, 2048) and torch.equal(nchw4, alone)
    with torch.no_grad():
        f32 = O.resnet50_trunk(vids, state, False).mean(dim=(2, 3))
        f64 = O.resnet50_trunk(vids.double(), {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}, False).mean(dim=(2, 3))
    e3 = anchored("features of 3 videos", three, f32, f64)
    e1 = anchored("features of the video alone", alone, f32[T:2 * T], f64[T:2 * T])
    print("extract_feature: 3 videos", e3, "alone", e1, "alone bit-identical to its rows of the call of 3:", torch.equal(alone, three[T:2 * T]),
          "max abs difference", float((alone - three[T:2 * T]).abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# the loop and the tools
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pretrained(dev, tmp_path_factory):
    """python -m litemkd_amd.pretrain's main() for 2 epochs on 6 videos of 3 classes (one batch per epoch), 4 frames of 64 x 64"""
    from litemkd_amd import pretrain as PT
    root = tmp_path_factory.mktemp("pretrain")
    rgb, lists, ck = str(root / "rgb"), str(root / "lists"), str(root / "ck")
    entries = R.write_jpeg_tree(rgb, lists)
    flags = ["--path", rgb, "--traintestlist", lists, "--checkpoint_dir", ck, "--mode", "train", "--seq_len", "4", "--img_size", "64",
             "--num_classes", "3", "--epochs", "2", "--lr_1", "1e-4", "--lr_2", "1e-2", "--seed", "5", "--model", "Action_Recognition_Resnet50"]
    hist, model, opt = PT.main(flags)
    torch.cuda.synchronize()
    return dict(root=root, rgb=rgb, lists=lists, ck=ck, entries=entries, flags=flags, hist=hist, model=model, opt=opt)


def test_pretraining_loop_and_resume(dev, pretrained):
    from litemkd_amd import pretrain as PT
    from litemkd_amd import trainloop as TL
    h, opt, model, ck = pretrained["hist"], pretrained["opt"], pretrained["model"], pretrained["ck"]
    assert len(h["losses"]) == 2 and len(h["eval"]) == 2 and all(math.isfinite(v) and v > 0 for v in h["losses"])
    assert all(0.0 <= a <= 1.0 for a in h["accuracies"])
    assert all(min(abs(a - i / 8) for i in range(7)) < 1e-6 for a in h["eval"])      # 0 .. 6 right answers over the 8 of a batch
    assert [grp["steps"] for grp in opt.groups.values()] == [2, 2]
    assert opt.groups["convnet"]["lr"] == 1e-4 and opt.groups["fc"]["lr"] == 1e-2
    assert os.path.exists(os.path.join(ck, "best_checkpoint.pt")) == (h["best"] > 0)
    # the checkpoint the loop writes, in a state with lowered rates: 11 epochs on the schedulers
    s1, s2 = TL.StepLR(opt, "convnet", 10, 0.1), TL.StepLR(opt, "fc", 10, 0.1)
    for _ in range(11):
        s1.step()
        s2.step()
    PT.save_checkpoint(model, opt, s1, s2, 2, ck)
    saved = torch.load(os.path.join(ck, "best_checkpoint.pt"), map_location="cpu")
    assert set(saved) == {"iteration", "model_state_dict", "optimizer1_state_dict", "optimizer2_state_dict", "scheduler1", "scheduler2"}
    assert saved["iteration"] == 2 and float(saved["optimizer1_state_dict"]["momentum_buffer"].abs().max()) > 0
    _, model2, opt2 = PT.main(pretrained["flags"] + ["--resume", "True", "--epochs", "0"])
    assert torch.equal(opt2.buf.cpu(), opt.buf.cpu()) and torch.equal(opt2.bucket.flat.cpu(), opt.bucket.flat.cpu())
    for k, v in model.state_dict().items():
        assert torch.equal(model2.state_dict()[k].cpu(), v.cpu()), k
    for name, base in (("convnet", 1e-4), ("fc", 1e-2)):
        assert opt2.groups[name]["steps"] == 2 and opt2.groups[name]["lr"] == opt.groups[name]["lr"]
        assert opt2.groups[name]["lr"] == pytest.approx(base * 0.1, rel=1e-12)


def test_frames_to_a_student_end_to_end(dev, pretrained):
    """extract --stage modality three times over the tree -> FeatureTreeEpisodes reads the trees -> extract --stage fusion with a fresh
    ThreeTRXShiftLoopTime checkpoint written by train_teacher.save_checkpoint (and with the bare state dict) -> JpegFrameEpisodes reads
    the fused features through teacher_path and draws an episode"""
    from litemkd_amd import extract as E
    from litemkd_amd import pretrain as PT
    from litemkd_amd import train_teacher as TT
    from litemkd_amd.options import default_args
    from litemkd_amd.train import JpegFrameEpisodes
    root, rgb, lists, ck = pretrained["root"], pretrained["rgb"], pretrained["lists"], pretrained["ck"]
    PT.save_checkpoint(pretrained["model"], pretrained["opt"], types.SimpleNamespace(state=lambda: {}), types.SimpleNamespace(state=lambda: {}), 2, ck)
    feats, fused = str(root / "feats"), str(root / "fused")
    for i, m in enumerate(("rgb", "depth", "flow")):
        flags = ["--stage", "modality", "--path", rgb, "--traintestlist", lists, "--mode", "test", "--modality", m, "--out", feats,
                 "--checkpoint_dir", ck if i else os.path.join(ck, "best_checkpoint.pt"), "--seq_len", "4", "--img_size", "64",
                 "--videos_per_call", "4", "--num_classes", "64"]      # the class count comes from the checkpoint's fc (3), not the flag
        rec = E.main(flags)
        assert (rec["written"], rec["skipped"], rec["model_calls"]) == (6, 0, 2)
    a = np.load(os.path.join(feats, "rgb", pretrained["entries"][0], "feature.npy"))
    assert a.dtype == np.float32 and a.shape == (4, 2048) and np.isfinite(a).all() and a.std() > 0
    assert np.array_equal(a, np.load(os.path.join(feats, "flow", pretrained["entries"][0], "feature.npy")))      # centre crop: reproducible
    assert E.main(flags + ["--resume"])["skipped"] == 6
    # the trees open in train_teacher's reader
    p = TT.build_parser()
    targs = TT.args_check(p, p.parse_args(["--way", "3", "--shot", "1", "--query_per_class", "1", "--seq_len", "4", "--trans_num", "1",
                                           "--feature_save_path", feats, "--no_save"]))
    targs.device = dev
    ep = TT.FeatureTreeEpisodes(targs, feats, None, 3, dev).episode()
    assert tuple(ep["context_features"]["depth"].shape) == (3, 4, 2048) and tuple(ep["target_features"]["flow"].shape) == (3, 4, 2048)
    # a fresh teacher, saved the way the trainer saves it
    teacher = TT.build_model(targs, dev)
    tck = str(root / "teacher_ck")
    TT.save_checkpoint(teacher, types.SimpleNamespace(opt="sgd", lr=1e-4, steps=0), types.SimpleNamespace(n=0, base=1e-4), 5, tck)
    fflags = ["--stage", "fusion", "--feature_save_path", feats, "--out", fused, "--seq_len", "4", "--trans_num", "4"]      # depth from the file
    rec = E.main(fflags + ["--checkpoint_dir", os.path.join(tck, "checkpoint5.pt")])
    assert (rec["written"], rec["skipped"]) == (6, 0)
    f0 = np.load(os.path.join(fused, pretrained["entries"][0], "feature.npy"))
    assert f0.dtype == np.float32 and f0.shape == (4, 2048) and np.isfinite(f0).all()
    teacher.eval()
    want = teacher.extract_feature({m: torch.from_numpy(a).unsqueeze(0).to(dev) for m in ("rgb", "depth", "flow")}).reshape(4, 2048).cpu().numpy()
    assert np.array_equal(f0, want)
    final = os.path.join(tck, "checkpoint_final.pt")
    torch.save({k: v.detach().cpu() for k, v in teacher.state_dict().items()}, final)
    os.remove(os.path.join(fused, pretrained["entries"][3], "feature.npy"))
    rec = E.main(fflags + ["--checkpoint_dir", final, "--resume"])
    assert (rec["written"], rec["skipped"]) == (1, 5)
    del teacher
    torch.cuda.empty_cache()
    # and the student's loader reads them
    cfg = default_args(way=3, shot=1, query_per_class=1, query_per_class_test=1, seq_len=4, img_size=84, device=dev)
    task = JpegFrameEpisodes(cfg, rgb, None, fused, device=dev).episode()
    assert tuple(task["support_set_feature_teacher"].shape) == (1, 3, 4, 2048) and tuple(task["support_set"].shape) == (1, 12, 84, 84, 4)
    assert bool(torch.isfinite(task["target_set_feature_teacher"]).all())
