"""GPU: attention maps (csrc/cam.hip, litemkd_amd.cam, litemkd_amd.heatmap).  The Grad-CAM / HiResCAM kernel against the fp64 statement
of tests/_cam_ref.py (anchored: no worse than 3 x torch's fp32 CPU evaluation, floor 2e-6) and bit-identical from call to call; the
overlay bit for bit against PIL's resampler + the integer colour table and blend; cam.grad_cam end to end against autograd through the
oracle's pooled head and matcher restatements carried from the recorded maps; the state a call must leave untouched; the CLI."""
import os

import numpy as np
import pytest
import torch

from _anchor import anchored
import _cam_ref as R

pytestmark = pytest.mark.gpu

WAY, SHOT, L, IMG, OUT = 3, 2, 4, 64, 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from litemkd_amd import ops
    ops.reset_compute_dtypes()
    return torch.device("cuda", 0)


# ---- the kernel ----
KERNEL_SHAPES = [(3, 7, 7, 512), (2, 7, 7, 2048), (2, 7, 7, 960), (5, 2, 2, 512), (2, 3, 4, 40), (1, 1, 1, 64)]


@pytest.mark.parametrize("mode", [0, 1], ids=["gradcam", "hirescam"])
@pytest.mark.parametrize("F,h,w,C", KERNEL_SHAPES)
def test_gradcam_kernel(dev, F, h, w, C, mode):
    from litemkd_amd import ops
    g = torch.Generator().manual_seed(F * 100000 + h * 10000 + w * 1000 + C + mode)
    A = torch.randn(F, h, w, C, generator=g)
    dA = torch.randn(F, h, w, C, generator=g) * 1e-2
    if F > 1:
        A[-1], dA[-1] = A[-1].abs(), -dA[-1].abs()          # the last frame: nothing survives the ReLU, the map is all zero
    elif float((dA.sum((1, 2)) * A).sum()) < 0:
        dA = -dA                                            # the single 1 x 1 frame keeps a positive raw value (its normalised map is 0)
    w64, raw64, cam64 = (torch.from_numpy(t) for t in R.gradcam(A.double().numpy(), dA.double().numpy(), mode))
    w32, raw32, cam32 = R.gradcam_torch(A, dA, mode)
    Ad, dAd = A.to(dev), dA.to(dev)
    got = ops.gradcam(Ad, dAd, mode)
    again = ops.gradcam(Ad, dAd, mode)
    torch.cuda.synchronize()
    for name, a, b in zip(("weights", "raw", "cam"), got, again):
        assert torch.equal(a, b), name + ": two calls differ"
    wts, raw, cam = got
    assert tuple(wts.shape) == (F, C) and tuple(raw.shape) == (F, h, w) and tuple(cam.shape) == (F, h, w)
    for name, a, b, r in (("weights", wts, w32, w64), ("raw", raw, raw32, raw64), ("cam", cam, cam32, cam64)):
        if float(r.abs().max()) == 0.0:          # (HW = 1: the normalised map is exactly zero in every evaluation)
            assert float(a.abs().max()) == 0.0 and float(b.abs().max()) == 0.0, name
            continue
        e = anchored("%s mode %d %s" % (name, mode, (F, h, w, C)), a, b, r)
        print("%-8s hip %.3e cpu %.3e" % (name, *e))
    if F > 1:
        assert float(raw[-1].abs().max()) == 0.0 and float(cam[-1].abs().max()) == 0.0
    else:
        assert float(raw64.max()) > 0 and float(raw.max()) > 0
    assert float(raw.min()) >= 0.0 and float(cam.min()) >= 0.0 and float(cam.max()) <= 1.0
    if F > 1 and h * w > 1:
        assert float(raw64[:-1].max()) > 0
        spread = (raw64.amax((1, 2)) - raw64.amin((1, 2))) > 1e-3          # frames with a real range reach 1 - 1e-7 / range
        assert bool(spread.any()) and float(cam.cpu().amax((1, 2))[spread].min()) > 0.999


def test_gradcam_op_refusals(dev):
    from litemkd_amd import ops
    a = torch.zeros(1, 2, 2, 16, device=dev)
    with pytest.raises(RuntimeError, match="mode 2"):
        ops.gradcam(a, a, 2)
    with pytest.raises(RuntimeError, match=r"C 12\b"):
        ops.gradcam(a[..., :12].contiguous(), a[..., :12].contiguous(), 0)
    ops.set_conv_compute_dtype("bf16")
    ops.set_activation_dtype("bf16")
    try:
        with pytest.raises(RuntimeError, match="fp32 activations only"):
            ops.gradcam(a, a, 0)
        with pytest.raises(RuntimeError, match="fp32 activations only"):
            ops.cam_overlay(a[..., 0].contiguous(), None, (8, 8))
    finally:
        ops.reset_compute_dtypes()


# ---- the overlay ----
@pytest.mark.parametrize("alpha256", [0, 128, 256])
@pytest.mark.parametrize("h,w,Ho,Wo", [(7, 7, 224, 224), (2, 2, 64, 64), (3, 4, 96, 128)])
def test_overlay_is_pil_bit_for_bit(dev, h, w, Ho, Wo, alpha256):
    from litemkd_amd import ops
    F = 3
    g = torch.Generator().manual_seed(h * 1000 + w * 100 + alpha256)
    m = torch.randint(0, 1025, (F, h, w), generator=g)
    m[0].view(-1)[:2] = torch.tensor([0, 1024])
    cam = m.float() / 1024.0          # cam * 255 + 0.5 is exact in fp32 for these, fused or not
    frames = torch.randint(0, 256, (F, Ho, Wo, 3), generator=g, dtype=torch.uint8)
    lut = ops.jet_lut()
    assert np.array_equal(lut.numpy(), R.jet_lut())
    for fr in (frames, None):
        want = R.overlay(cam.numpy(), None if fr is None else fr.numpy(), (Ho, Wo), alpha256)
        got = ops.cam_overlay(cam.to(dev), None if fr is None else fr.to(dev), (Ho, Wo), image_weight=alpha256 / 256.0)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (F, Ho, Wo, 3)
        diff = int((got.cpu().numpy() != want).sum())
        assert diff == 0, "%d of %d bytes differ (frames: %s)" % (diff, want.size, fr is not None)
    # a caller's table: grey ramp
    ramp = torch.arange(256, dtype=torch.uint8)[:, None].repeat(1, 3)
    got = ops.cam_overlay(cam.to(dev), None, (Ho, Wo), lut=ramp.to(dev))
    assert np.array_equal(got.cpu().numpy(), R.overlay(cam.numpy(), None, (Ho, Wo), 0, lut=ramp.numpy()))


# ---- end to end ----
def _student(dev, backbone, classifier, seed):
    from litemkd_amd.model.model_select import Student
    from litemkd_amd.options import default_args
    args = default_args(way=WAY, shot=SHOT, query_per_class=1, query_per_class_test=1, seq_len=L, img_size=IMG, trans_linear_out_dim=OUT,
                        trans_dropout=0.0, model_backbone=backbone, model_classifier=classifier, device=dev)
    torch.manual_seed(seed)
    student = Student(args).to(dev)
    with torch.no_grad():                      # non-trivial running statistics, as the eval tests fill them
        for n, b in student.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(torch.randn_like(b) * 0.1)
            elif n.endswith("running_var"):
                b.copy_(torch.rand_like(b) + 0.5)
    return student, args


def _episode(dev, seed):
    g = torch.Generator().manual_seed(seed)
    sup = torch.rand(WAY * SHOT * L, 3, IMG, IMG, generator=g)
    qry = torch.rand(WAY * L, 3, IMG, IMG, generator=g)
    sl = torch.arange(WAY).repeat_interleave(SHOT).float()
    return sup.to(dev), sl.to(dev), qry.to(dev)


def _reference_maps(student, out, labels, target, query, two_heads, method):
    """the kept maps through the oracle's pooled head and TRX restatement with the student's own parameters, in fp64 and fp32: autograd's
    gradient of the same score, then the numpy Grad-CAM -> {dtype: {"support" | "query": (raw, cam, grad)}}"""
    from oracle import ref_cpu as O
    sd = {k: v.detach().cpu() for k, v in student.state_dict().items()}
    res = {}
    for dt in (torch.float64, torch.float32):
        bp = {k[len("backbone."):]: v.to(dt) for k, v in sd.items() if k.startswith("backbone.") and v.is_floating_point()}
        tp = {k[len("classifier.transformers."):]: v.to(dt) for k, v in sd.items() if k.startswith("classifier.transformers.")}
        fm = {n: out[n]["map"].cpu().to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_() for n in ("support", "query")}
        lab = labels.cpu()
        if two_heads:
            c, t = O.head_2fc(fm["support"], fm["query"], bp, seq_len=L)
            z = (O.trx_logits(c["context_features_1"], lab, t["target_features_1"], tp, WAY, L, OUT)
                 + O.trx_logits(c["context_features_2"], lab, t["target_features_2"], tp, WAY, L, OUT))
        else:
            lin = lambda f: torch.nn.functional.linear(O.pooled_frame_features(f), bp["res18_2048.weight"], bp["res18_2048.bias"])      # noqa: E731
            z = O.trx_logits(lin(fm["support"]).reshape(-1, L, 2048), lab, lin(fm["query"]).reshape(-1, L, 2048), tp, WAY, L, OUT)
        picked = z.gather(1, target.cpu()[:, None])[:, 0]
        score = picked.sum() if query is None else picked[query]
        gs, gq = torch.autograd.grad(score, [fm["support"], fm["query"]])
        res[dt] = {"z": z.detach()}
        for n, g_ in (("support", gs), ("query", gq)):
            A, dA = fm[n].detach().permute(0, 2, 3, 1).contiguous().numpy(), g_.permute(0, 2, 3, 1).contiguous().numpy()
            _, raw, cam = R.gradcam(A, dA, 0 if method == "gradcam" else 1)
            res[dt][n] = (torch.from_numpy(raw), torch.from_numpy(cam), torch.from_numpy(dA))
    return res


@pytest.mark.parametrize("backbone,classifier,seed", [("resnet18_2fc", "TRX_2fcsup", 11), ("resnet18_student", "TRX", 12)])
@pytest.mark.parametrize("how", ["predicted", "explicit", "query1", "hirescam"])
def test_grad_cam_against_autograd_through_the_oracle_head(dev, backbone, classifier, seed, how):
    from litemkd_amd import cam
    student, args = _student(dev, backbone, classifier, seed)
    sup, sl, qry = _episode(dev, seed + 100)
    target = torch.tensor([2, 0, 1], device=dev) if how == "explicit" else None
    query = 1 if how == "query1" else None
    method = "hirescam" if how == "hirescam" else "gradcam"
    out = cam.grad_cam(student, sup, sl, qry, target=target, query=query, method=method, keep=True)
    torch.cuda.synchronize()
    h = IMG // 32
    assert tuple(out["logits"].shape) == (WAY, WAY) and tuple(out["target"].shape) == (WAY,)
    assert tuple(out["support"]["cam"].shape) == (WAY * SHOT * L, h, h) and tuple(out["query"]["raw"].shape) == (WAY * L, h, h)
    if target is None:
        assert torch.equal(out["target"], out["logits"].argmax(-1))
    else:
        assert torch.equal(out["target"], target)
    ref = _reference_maps(student, out, sl, out["target"], query, backbone == "resnet18_2fc", method)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    anchored("scored logits", out["scored_logits"], r32["z"], r64["z"])
    assert float(r64["query"][0].amax((1, 2)).max()) > 0, "the fp64 reference's query maps are empty: pick another seed"
    for n in ("support", "query"):
        for i, what in enumerate(("raw", "cam")):
            e = anchored("%s %s %s" % (backbone, n, what), out[n][what], r32[n][i], r64[n][i])
            print("%-8s %-4s hip %.3e cpu %.3e" % (n, what, *e))
        e = anchored("%s %s grad" % (backbone, n), out[n]["grad"], r32[n][2], r64[n][2])
        print("%-8s grad hip %.3e cpu %.3e" % (n, *e))
    if query is not None:          # the other queries' frames receive no gradient
        gq = out["query"]["grad"].reshape(WAY, L, -1)
        assert float(gq[[0, 2]].abs().max()) == 0.0 and float(gq[1].abs().max()) > 0
        assert float(out["query"]["raw"].reshape(WAY, -1)[[0, 2]].abs().max()) == 0.0


@pytest.mark.parametrize("backbone,classifier,seed", [("resnet50_2fc", "TRX_2fcsup", 21), ("moblienetv3_fc2", "TRX_2fcsup", 22)])
def test_grad_cam_other_backbones(dev, backbone, classifier, seed):
    from litemkd_amd import cam, _audit
    student, args = _student(dev, backbone, classifier, seed)
    sup, sl, qry = _episode(dev, seed + 100)
    audit = backbone == "resnet50_2fc"
    if audit:          # the stream-lifetime audit over the whole call; a suite that runs audited throughout gets its own state back
        before = (_audit.ON, _audit.STRICT, _audit.ARMED, _audit._installed[0])
        _audit.enable(True)
        kept = _audit.findings(clear=True)
        _audit.arm()
    try:
        out = cam.grad_cam(student, sup, sl, qry, keep=True)
        torch.cuda.synchronize()
        found = _audit.findings(clear=True) if audit else []
    finally:
        if audit:
            _audit.arm(before[2])
            _audit.enable(before[0], before[1])
            _audit._findings.extend(kept)
            if not before[3]:
                _audit.uninstall()          # torch's own factories back: `with torch.device(...)` in later tests knows them by identity
    assert found == [], found
    if audit:
        assert (_audit.ON, _audit.STRICT, _audit.ARMED, _audit._installed[0]) == before
    for n in ("support", "query"):
        A, dA = out[n]["map"].cpu(), out[n]["grad"].cpu()
        assert A.shape[-1] == (2048 if backbone == "resnet50_2fc" else 960)
        _, raw64, cam64 = (torch.from_numpy(t) for t in R.gradcam(A.double().numpy(), dA.double().numpy(), 0))
        _, raw32, cam32 = R.gradcam_torch(A, dA, 0)
        anchored(n + " raw", out[n]["raw"], raw32, raw64)
        anchored(n + " cam", out[n]["cam"], cam32, cam64)
        if n == "query":
            assert float(raw64.amax((1, 2)).max()) > 0, "the fp64 reference's query maps are empty: pick another seed"
    student.eval()
    with torch.no_grad():
        plain = student(sup, sl, qry)["logits"]
        plain = plain["kl"] + plain["ce"]
    # the returned logits are the evaluator's: test_eval_bn_fused_in_conv_epilogue's bound
    dev_plain = float((out["logits"] - plain).abs().max())
    print("%s: logits differ from the plain forward's by %.3e of max |logit| %.3e" % (backbone, dev_plain, float(plain.abs().max())))
    assert dev_plain <= 1e-5 * float(plain.abs().max())
    assert torch.equal(out["target"], plain.argmax(-1))
    # the forward that gave the maps sums its heads' GEMMs in blocks (cam.K_BLOCK): its logits and the gradient at the recorded maps
    # against the fp64 evaluation of the same heads from those maps, the oracle's fp32 CPU evaluation as the yardstick
    ref = _reference_maps(student, out, sl, out["target"], None, True, "gradcam")
    r64, r32 = ref[torch.float64], ref[torch.float32]
    e = anchored(backbone + " scored logits", out["scored_logits"], r32["z"], r64["z"])
    print("scored logits hip %.3e cpu %.3e; differ from the plain forward's by %.3e" % (*e, float((out["scored_logits"] - plain).abs().max())))
    for n in ("support", "query"):
        e = anchored("%s %s grad" % (backbone, n), out[n]["grad"], r32[n][2], r64[n][2])
        print("%-8s grad hip %.3e cpu %.3e" % (n, *e))


# ---- state ----
def test_a_call_leaves_the_student_as_it_was(dev):
    from litemkd_amd import cam, ops
    student, args = _student(dev, "resnet18_2fc", "TRX_2fcsup", 31)
    sup, sl, qry = _episode(dev, 131)
    frozen = [p for n, p in student.named_parameters() if n.endswith("fc2.bias") or "norm_v" in n]
    for p in frozen:
        p.requires_grad_(False)

    def train_step():
        student.train()
        for p in student.parameters():
            p.grad = None
        lg = student(sup, sl, qry)["logits"]
        (lg["kl"] + lg["ce"]).sum().backward()
        torch.cuda.synchronize()
        return lg["kl"].detach().clone(), {n: p.grad.clone() for n, p in student.named_parameters() if p.grad is not None}

    for mode in (True, False):
        student.train(mode)
        student.classifier.train(not mode)          # a mixed state must come back as it was
        buffers = {n: b.clone() for n, b in student.named_buffers()}
        flags = {n: p.requires_grad for n, p in student.named_parameters()}
        for p in student.parameters():
            p.grad = None
        cam.grad_cam(student, sup, sl, qry)
        torch.cuda.synchronize()
        assert student.training is mode and student.classifier.training is (not mode) and student.backbone.training is mode
        assert {n: p.requires_grad for n, p in student.named_parameters()} == flags and not any(p.requires_grad for p in frozen)
        assert all(p.grad is None for p in student.parameters())
        for n, b in student.named_buffers():
            assert torch.equal(b, buffers[n]), n
        assert ops._CAM_TAP[0] is None and not any("gemm_k_block" in m.__dict__ for m in student.modules())
    # a forward that raises: the tap, the mode and the flags come back all the same
    student.train()
    orig = student.classifier.forward

    def boom(*a, **k):
        raise RuntimeError("boom")
    student.classifier.forward = boom
    try:
        with pytest.raises(RuntimeError, match="boom"):
            cam.grad_cam(student, sup, sl, qry)
    finally:
        student.classifier.forward = orig
    assert ops._CAM_TAP[0] is None and not any("gemm_k_block" in m.__dict__ for m in student.modules())
    assert student.training and all(p.requires_grad for p in student.parameters() if all(p is not f for f in frozen))
    assert not any(p.requires_grad for p in frozen)
    # training before and after a call: the same bits
    kl_a, grads_a = train_step()
    for p in student.parameters():
        p.grad = None
    cam.grad_cam(student, sup, sl, qry)
    assert all(p.grad is None for p in student.parameters())
    kl_b, grads_b = train_step()
    assert torch.equal(kl_a, kl_b) and sorted(grads_a) == sorted(grads_b) and len(grads_a) > 60
    for n in grads_a:
        assert torch.equal(grads_a[n], grads_b[n]), n


def test_refusals_on_the_device(dev):
    from litemkd_amd import cam
    student, args = _student(dev, "resnet18_student", "TRX_sup", 41)
    sup, sl, qry = _episode(dev, 141)
    with pytest.raises(ValueError, match="logits_fn"):
        cam.grad_cam(student, sup, sl, qry)
    out = cam.grad_cam(student, sup, sl, qry, logits_fn=lambda d: d["query"])
    assert tuple(out["logits"].shape) == (WAY, WAY) and float(out["query"]["cam"].max()) > 0
    with pytest.raises(ValueError, match="method"):
        cam.grad_cam(student, sup, sl, qry, method="gradcam++", logits_fn=lambda d: d["query"])
    # a class outside [0, way) is refused on the host, on whichever device the tensor lives, and leaves the student as it was
    student.train()
    for bad in ([0, 1, WAY], torch.tensor([0, -1, 1], device=dev), [0, 1], torch.tensor([0.0, 1.0, 2.0])):
        with pytest.raises(ValueError, match="target"):
            cam.grad_cam(student, sup, sl, qry, target=bad, logits_fn=lambda d: d["query"])
    with pytest.raises(ValueError, match="query 3"):
        cam.grad_cam(student, sup, sl, qry, query=3, logits_fn=lambda d: d["query"])
    torch.cuda.synchronize()
    assert student.training and all(p.requires_grad for p in student.parameters())


# ---- CLI ----
def test_heatmap_cli_writes_overlays_and_reproducible_maps(dev, tmp_path):
    from PIL import Image
    from litemkd_amd import heatmap
    argv = ("--episodes 2 --way %d --shot %d --seq_len %d --img_size %d --trans_linear_out_dim %d --who both --seed 5" % (WAY, SHOT, L, IMG, OUT)).split()
    runs = []
    for name in ("a", "b"):
        out_dir = str(tmp_path / name)
        dirs = heatmap.main(argv + ["--out_dir", out_dir])
        assert sorted(os.listdir(out_dir)) == ["ep0", "ep1"]
        for k in (0, 1):
            ep = os.path.join(out_dir, "ep%d" % k)
            names = sorted(os.listdir(ep))
            q = [n for n in names if n.startswith("q")]
            s = [n for n in names if n.startswith("s")]
            assert "maps.npz" in names and len(q) == WAY and len(s) == WAY * SHOT and len(names) == 1 + len(q) + len(s)
            maps = np.load(os.path.join(ep, "maps.npz"))
            for i in range(WAY):
                d = "q%d_true%d_pred%d" % (i, int(maps["query_labels"][i]), int(maps["target"][i]))
                assert d in q, (d, q)
                assert sorted(os.listdir(os.path.join(ep, d))) == ["frame%d.png" % j for j in range(L)]
                im = Image.open(os.path.join(ep, d, "frame0.png"))
                assert im.size == (IMG, IMG) and im.mode == "RGB"
            assert maps["query_cam"].shape == (WAY * L, IMG // 32, IMG // 32) and maps["support_raw"].shape == (WAY * SHOT * L, IMG // 32, IMG // 32)
            assert maps["logits"].shape == (WAY, WAY) and float(maps["query_cam"].max()) > 0
        assert len(dirs) == 2 * (WAY + WAY * SHOT)
        runs.append({(k, f): np.load(os.path.join(out_dir, "ep%d" % k, "maps.npz"))[f] for k in (0, 1)
                     for f in ("logits", "target", "query_raw", "query_cam", "support_raw", "support_cam")})
    for key in runs[0]:
        assert np.array_equal(runs[0][key], runs[1][key]), key
    assert not np.array_equal(runs[0][(0, "query_raw")], runs[0][(1, "query_raw")])


def test_heatmap_cli_takes_an_evaluator_command_line_over_a_jpeg_tree(dev, tmp_path):
    """the evaluator's flags as they stand (those that concern a teacher or count its tasks are accepted and unused), the test split of a
    JPEG frame tree read by --rgb_path / --traintestlist / --split (its transform knows 84- and 224-px crops: 84 here, a 3 x 3 map)"""
    img = 84
    import io
    from PIL import Image
    from litemkd_amd import heatmap
    rgb, lists = tmp_path / "rgb", tmp_path / "lists"
    lists.mkdir()
    rng = np.random.default_rng(3)
    split = {"train": [], "test": []}
    for c in range(WAY):
        for v in range(SHOT + 2):          # the first video of a class trains, the others (shot + one query) test
            name = "V%d_c%d" % (v, c)
            split["train" if v == 0 else "test"].append("Cls%d/%s.avi 1" % (c, name))
            d = rgb / ("Cls%d" % c) / name
            d.mkdir(parents=True)
            for f in range(L + 1):
                y, x = np.mgrid[0:72, 0:88]
                a = np.stack([90 + 60 * np.sin(x / 9.0 + c + f), 120 + 50 * np.cos(y / 7.0 - v), 100 + 40 * np.sin((x + y) / 5.0)], -1)
                b = io.BytesIO()
                Image.fromarray(np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)).save(b, "JPEG", quality=75)
                (d / ("img_%05d.jpg" % (f + 1))).write_bytes(b.getvalue())
    for k, v in split.items():
        (lists / ("%slist03.txt" % k)).write_text("\n".join(v) + "\n")
    out_dir = str(tmp_path / "maps")
    argv = ("--test_model student --model_teacher test_teacher_TRX_2fcsup_fixed --num_test_tasks 7 --teacher_path %s --split 3 "
            "--way %d --shot %d --query_per_class_test 1 --seq_len %d --img_size %d --trans_linear_out_dim %d --seed 2 --image_weight 1.0"
            % (tmp_path / "none", WAY, SHOT, L, img, OUT)).split()
    argv += ["--rgb_path", str(rgb), "--traintestlist", str(lists), "--out_dir", out_dir]
    dirs = heatmap.main(argv)
    assert os.listdir(out_dir) == ["ep0"] and len(dirs) == WAY
    maps = np.load(os.path.join(out_dir, "ep0", "maps.npz"))
    assert maps["query_cam"].shape == (WAY * L, 3, 3) and sorted(maps["query_labels"].tolist()) == list(range(WAY))
    frames = []
    for i in range(WAY):
        d = os.path.join(out_dir, "ep0", "q%d_true%d_pred%d" % (i, int(maps["query_labels"][i]), int(maps["target"][i])))
        assert sorted(os.listdir(d)) == ["frame%d.png" % j for j in range(L)]
        frames.append(np.asarray(Image.open(os.path.join(d, "frame0.png"))))
        assert frames[-1].shape == (img, img, 3)
    # --image_weight 1.0: the overlay is the frame itself, and these frames are the tree's (channel means as written above), not noise
    mean = np.stack(frames).reshape(-1, 3).mean(0)
    assert np.all(np.abs(mean - np.array([90.0, 120.0, 100.0])) < 25), mean
    with pytest.raises(SystemExit):
        heatmap.main(["--test_model", "teacher", "--out_dir", out_dir])
