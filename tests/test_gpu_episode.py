"""GPU: whole-episode parity (student + teacher + D2M loss + backward) against the CPU oracle on the same
seeded episode and weights; loop semantics on the real modules; size-independent properties at the
benchmark size."""
import math

import pytest
import torch
import torch.nn.functional as F

from _anchor import anchored, anchored_dict, near_zero_limit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@pytest.mark.parametrize("shot,query,img,clf,dist,bb,mode", [(1, 1, 96, "TRX_2fcsup", "fc_2_sup_dist", "resnet18_2fc", "fp32"),
                                                             (2, 1, 64, "e_dist_fc2_sup", "fc_2_sup_dist", "resnet18_2fc", "fp32"),
                                                             (1, 1, 64, "TRX_2fcsup", "fc_2_sup_dist", "resnet50_2fc", "fp32"),
                                                             (1, 1, 96, "TRX_2fcsup", "fc_2_sup_dist", "resnet18_2fc", "fp32x3"),
                                                             (2, 1, 64, "e_dist_fc2_sup", "fc_2_sup_dist", "resnet18_2fc", "fp32x3"),
                                                             (1, 1, 64, "TRX_2fcsup", "fc_2_sup_dist", "resnet50_2fc", "fp32x3"),
                                                             (1, 1, 96, "TRX_2fcsup", "fc_2_sup_dist", "resnet18_2fc", "fp32h2"),
                                                             (2, 1, 64, "e_dist_fc2_sup", "fc_2_sup_dist", "resnet18_2fc", "fp32h2"),
                                                             # BASELINE configs[4]'s student in the arithmetic its benchmark line runs
                                                             (1, 1, 64, "TRX_2fcsup", "fc_2_sup_dist", "resnet50_2fc", "fp32h2"),
                                                             (1, 1, 96, "TRX_2fcsup", "fc_2_sup_dist", "resnet18_2fc", "bf16"),
                                                             (1, 1, 96, "TRX_2fcsup", "fc_2_sup_dist", "resnet18_2fc", "bf16act"),
                                                             # BASELINE configs[1] at FULL SIZE in the benchmark's arithmetic: 400 frames of
                                                             # 224^2, forward, loss and every parameter gradient (three oracle runs, ~2 min)
                                                             (5, 5, 224, "TRX_2fcsup", "fc_2_sup_dist", "resnet18_2fc", "fp32x3"),
                                                             # ... and in bench.py's headline arithmetic (two fp16 planes in the 3x3 kernels)
                                                             (5, 5, 224, "TRX_2fcsup", "fc_2_sup_dist", "resnet18_2fc", "fp32h2"),
                                                             # ... with the statistics of a TRAINED network: BatchNorm
                                                             # |gamma| ~ U(0.2, 3) of either sign, beta ~ N(0, 1), convolution weights with a 2^6
                                                             # spread of per-output-channel scales
                                                             (5, 5, 224, "TRX_2fcsup", "fc_2_sup_dist", "resnet18_2fc", "fp32h2+trained")])
def test_episode_matches_oracle(dev, shot, query, img, clf, dist, bb, mode):
    """mode fp32h2 (bench.py's headline arithmetic): fp32x3 with the 3x3 convolutions on two fp16 planes (csrc/conv_patch16.h); the test
    asserts that those kernels ran.
    mode fp32x3 (the library default): the convolutions (forward, data and weight gradient) in the 3xbf16 arithmetic, under the same fp32 criteria.
    mode bf16 (BASELINE configs[2]): against the ORACLE RUN ON BF16-ROUNDED CONVOLUTION OPERANDS (oracle.CONV_BF16: forward
    conv(r(x), r(w)), data gradient from r(dy), r(w), weight gradient from r(x), r(dy), fp32 everywhere else) - the same
    arithmetic on the CPU, not the GPU's own fp32 run."""
    from litemkd_amd import ops
    from oracle import ref_cpu as O
    trained = mode.endswith("+trained")
    mode = mode.split("+")[0]
    ops.set_conv_compute_dtype("bf16" if mode == "bf16act" else mode)
    if mode == "bf16act":      # + every stored activation / activation gradient of the trunk as bf16: oracle.ACT_BF16 rounds at the same places
        ops.set_activation_dtype("bf16")
        O.ACT_BF16 = True
    import litemkd_amd
    h2_before = litemkd_amd.lib().value("lmkd_conv_h2_launches")
    try:
        _episode_matches_oracle(dev, shot, query, img, clf, dist, bb, mode in ("bf16", "bf16act"), trained=trained)
        if mode == "fp32h2":      # 16 forward + 16 data-gradient + 13 weight-gradient launches per trunk call (one merged call here)
            n_h2 = litemkd_amd.lib().value("lmkd_conv_h2_launches") - h2_before
            import os
            if os.environ.get("LMKD_PARITY_LOG"):
                with open(os.environ["LMKD_PARITY_LOG"], "a") as f:
                    f.write("two-plane launches %s %dpx: %d\n" % (bb, img, n_h2))
            # ResNet-18: 16 forward + 16 data-gradient + 13 weight-gradient launches per trunk call (one merged call at 224 px).  ResNet-50 (two
            # trunk calls; its Bottlenecks keep the materialised activations in this mode, so every operand carries a maximum): per call the
            # stem's forward + weight gradient, the 3x3 and the same-size 1x1 convolutions' forward / data gradient on the patch kernel and
            # every weight gradient
            need = 45 if img == 224 else (150 if bb == "resnet50_2fc" else 20)
            assert n_h2 >= need, "the two-plane kernels did not run: %d launches" % n_h2
    finally:
        O.ACT_BF16 = False
        ops.set_activation_dtype("fp32")
        ops.reset_compute_dtypes()


class _MaskedReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, mask):
        ctx.save_for_backward(mask)
        return t * mask

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * mask, None


def _hip_relu_masks(taps):
    """ReLU masks of the HIP trunk calls in the oracle's ReLU order (stem, relu1, relu2 per BasicBlock, relu1, relu2, relu3 per
    Bottleneck; support call, then query), NCHW bool on the CPU.  relu1 = fmaf(c1, scale, shift) > 0 (Bottleneck: relu2 from c2 likewise),
    exactly what the kernels compute (lmkd_bn_apply)."""
    from litemkd_amd import ops
    masks = []
    for t in taps:
        if "stem_c" in t:
            masks.append((ops.bn_apply(t["stem_c"], t["stem_st"], True) > 0).permute(0, 3, 1, 2).cpu())
        else:
            masks.append((ops.bn_apply(t["c1"], t["st1"], True) > 0).permute(0, 3, 1, 2).cpu())
            if "c2" in t:      # Bottleneck entry: three masks
                masks.append((ops.bn_apply(t["c2"], t["st2"], True) > 0).permute(0, 3, 1, 2).cpu())
            masks.append((t["y"] > 0).permute(0, 3, 1, 2).cpu())
    return masks


def _hip_pool_choices(taps):
    """the arg-max selections of the HIP trunk calls in the oracle's order: per call ("stem": flat index into the H x W plane of the
    pooling input for every [n, c, oh, ow], from the kernel's own arg-max bytes; "head": the same for AdaptiveMaxPool2d((4, 4)) on
    the call's last block output - torch's kernel on the HIP tensor picks, like lmkd_adaptive_maxpool_mean, the first maximum in scan
    order)"""
    import torch.nn.functional as F
    calls, cur = [], None
    for t in taps:
        if "stem_c" in t:
            cur = {}
            calls.append(cur)
            N, Hc, Wc, C = t["stem_c"].shape
            k = t["stem_idx"].permute(0, 3, 1, 2).long()                       # [N, C, OH, OW], window position kh * 3 + kw
            OH, OW = k.shape[2], k.shape[3]
            oh = torch.arange(OH, device=k.device).view(1, 1, OH, 1)
            ow = torch.arange(OW, device=k.device).view(1, 1, 1, OW)
            cur["stem"] = ((2 * oh - 1 + k // 3) * Wc + (2 * ow - 1 + k % 3)).cpu()
        else:
            cur["last_y"] = t["y"]
    for c in calls:
        y = c.pop("last_y").float().permute(0, 3, 1, 2).contiguous()
        c["head"] = F.adaptive_max_pool2d(y, (4, 4), return_indices=True)[1].cpu()
    return calls


def _trained_like_(student, seed=77):
    """in place: the trunk's BatchNorm tables and convolution weights as a trained network has them (the reference starts from ImageNet
    weights, resnet18_2fc.py:30) - |gamma| ~ U(0.2, 3) of either sign, beta ~ N(0, 1), a 2^6 spread of per-output-channel weight scales"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in student.named_parameters():
            if not n.startswith("backbone.resnet."):
                continue
            if p.dim() == 4:
                p.mul_(torch.exp2(6.0 * torch.rand(p.shape[0], 1, 1, 1, generator=g) - 3.0).to(p.device))
            elif n.endswith(".weight"):
                sg = torch.where(torch.randn(p.shape, generator=g) < 0, -1.0, 1.0)
                p.copy_(((0.2 + 2.8 * torch.rand(p.shape, generator=g)) * sg).to(p.device))
            elif n.endswith(".bias"):
                p.copy_(torch.randn(p.shape, generator=g).to(p.device))


def _episode_matches_oracle(dev, shot, query, img, clf, dist, bb, bf16=False, trained=False):
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from litemkd_amd import ops
    from litemkd_amd.model.backbone import resnet as R
    from oracle import ref_cpu as O
    impose = bb in ("resnet18_2fc", "resnet50_2fc")      # the oracle runs with the HIP path's own ReLU masks and pooling selections imposed
    args = default_args(shot=shot, query_per_class=query, img_size=img, trans_dropout=0.0, device=dev, model_classifier=clf,
                        model_backbone=bb)
    torch.manual_seed(1)
    student, teacher = Student(args).to(dev), Teacher(args).to(dev)
    if trained:
        _trained_like_(student)
    ep = O.make_episode(900 + shot, 5, shot, query, img=img)
    sp = {k: v.detach().cpu().clone() for k, v in student.state_dict().items()}
    tp = {k[len("classifier.transformers."):]: v.detach().cpu().clone() for k, v in teacher.state_dict().items()
          if k.startswith("classifier.transformers.")}
    labels = ep["target_labels"].long()
    overlap = R.OVERLAP_TRUNK_CALLS
    R.OVERLAP_TRUNK_CALLS = False          # support call, then query call: the taps come out in the oracle's order
    ops.BLOCK_TAPS = [] if impose else None
    try:
        out = student(ep["support_set"].to(dev), ep["support_labels"].to(dev), ep["target_set"].to(dev))
        taps = ops.split_block_taps(ops.BLOCK_TAPS) if impose else None      # merged trunk call (the default): per-call entries, oracle order
    finally:
        R.OVERLAP_TRUNK_CALLS, ops.BLOCK_TAPS = overlap, None
    tl = teacher(ep["support_set_feature_teacher"].to(dev), ep["support_labels"].to(dev), ep["target_set_feature_teacher"].to(dev))["logits"]
    loss = getattr(Distiller(dist, args.cfg, dev), dist)(out["logits"], tl, labels.to(dev))["loss"]
    loss.backward()
    acc, pred = ops.accuracy(out["logits"]["kl"], out["logits"]["ce"], labels.to(dev))
    masks = _hip_relu_masks(taps) if impose else None
    pools = _hip_pool_choices(taps) if impose else None
    flips = [0, 0]
    pflips = [0, 0]
    deep = bb == "resnet50_2fc"      # the fp32 oracle run (masks imposed) leaves its pre-activations / pooling inputs here for the fp64 run's limits
    ref32 = {}

    def oracle(dt, imposed):
        p = {k: (v.clone().to(dt) if v.is_floating_point() else v.clone()) for k, v in sp.items()}
        for k, v in p.items():
            if v.is_floating_point() and "running" not in k and not k.endswith("pe.pe"):
                v.requires_grad_()
        e = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in ep.items()}
        site = [0]

        def hook(t):
            m = masks[site[0]]
            site[0] += 1
            if deep and dt == torch.float32:
                ref32["relu", site[0]] = t.detach()
            if dt == torch.float64:        # a mask may differ from the fp64 one only where the pre-activation is within rounding of 0
                diff = m != (t.detach() > 0)
                flips[0] += int(diff.sum())
                flips[1] += m.numel()
                # bf16 mode: an activation within fp32 rounding of a bf16 rounding boundary rounds the other way in the other
                # implementation (1 bf16 ulp = 0.4 %), so downstream pre-activations agree to ~1e-4, not 1e-6
                # Bottleneck trunks (50 layers): or within 3 x the fp32 oracle's own deviation from fp64 at this site (_anchor.near_zero_limit)
                lim = near_zero_limit(t.detach(), ref32.get(("relu", site[0])), (3e-2 if O.ACT_BF16 else 1e-2) if bf16 else 1e-5)
                assert not bool(diff.any()) or float(t.detach()[diff].abs().max()) < lim, site[0]
            return _MaskedReLU.apply(t, m.to(dt))
        psite = {"stem": 0, "head": 0}

        def pool_hook(kind, t):
            """the pooling with the HIP path's selection imposed (a gather: differentiable); in fp64 the selection may differ from
            the natural arg-max only where the two candidates are within rounding of each other"""
            idx = pools[psite[kind]][kind]
            psite[kind] += 1
            v = t.flatten(2).gather(2, idx.flatten(2)).reshape(idx.shape)
            if deep and dt == torch.float32:
                ref32[kind, psite[kind]] = t.detach()
            if dt == torch.float64:
                nat = (F.max_pool2d(t.detach(), 3, 2, 1) if kind == "stem" else F.adaptive_max_pool2d(t.detach(), (4, 4)))
                d = (nat - v.detach())
                pflips[0] += int((d > 0).sum())
                pflips[1] += d.numel()
                lim = near_zero_limit(t.detach(), ref32.get((kind, psite[kind])), (3e-2 if O.ACT_BF16 else 1e-2) if bf16 else 1e-5)
                assert float(d.max()) <= lim, (kind, float(d.max()), lim)
            return v
        O.RELU_HOOK = hook if imposed else None
        O.POOL_HOOK = pool_hook if imposed else None
        O.CONV_BF16 = bf16
        try:
            o = O.student_forward(e, p, 5, shot, classifier=clf, backbone=bb)
        finally:
            O.RELU_HOOK = None
            O.POOL_HOOK = None
            O.CONV_BF16 = False
        ot = O.clf_TRX_2fcsup_fixed(e["support_set_feature_teacher"], e["support_labels"], e["target_set_feature_teacher"],
                                    {k: v.to(dt) for k, v in tp.items()}, 5, shot)
        ol = O.distill_fc_2_sup_dist(o["logits"], ot, labels)["loss"]
        ol.backward()
        return p, o, ot, ol
    _, o, ot, ol = oracle(torch.float32, False)                  # forward values, logits, loss: the plain oracle
    sp32, _, _, _ = oracle(torch.float32, impose)               # gradients: both precisions with the HIP masks imposed
    sp64, o64, ot64, ol64 = oracle(torch.float64, impose)
    assert flips[0] <= max(8, flips[1] // ((500 if O.ACT_BF16 else 2000) if bf16 else 100000)), flips
    if bf16:
        # bf16 convolution operands: two fp32 implementations of this arithmetic agree only to ~1e-4 RMS (an activation within
        # fp32 rounding of a bf16 rounding boundary rounds the other way: 1 bf16 ulp = 0.4 % of that element), so the forward is
        # ANCHORED like the gradients: error against the oracle in fp64 (exact accumulation of the same bf16-rounded products) at
        # most 3x the error of the oracle's own fp32 run
        _, o64, ot64, ol64u = oracle(torch.float64, False)
        for k in ("context_features_1", "context_features_2"):
            anchored(k, out["context_features"][k], o["context_features"][k], o64["context_features"][k], 3.0, 1e-5)
        for k in ("kl", "ce", "sup"):
            anchored("logits " + k, out["logits"][k], o["logits"][k], o64["logits"][k], 3.0, 1e-5)
        assert abs(loss.item() - ol64u.item()) <= 3 * abs(ol.item() - ol64u.item()) + 1e-3 * abs(ol64u.item()), (loss.item(), ol.item(), ol64u.item())
    else:
        # round 4: the forward is fp64-ANCHORED like the gradients (before: features rel 2e-3, logits 2e-3 / 2e-2, loss 1e-3 - twenty times
        # looser than what is measured): per tensor, relative-L2 error against the oracle in fp64 <= 3 x the fp32 oracle's own + 1e-5.  (The
        # fp64 run carries the HIP path's ReLU masks / pooling selections where they are imposed: they differ from the natural ones only at
        # values within 1e-5 of zero / of a tie - checked above - which moves no forward value by more than that.)
        fwd = {}
        for k in ("context_features_1", "context_features_2"):
            fwd[k] = anchored(k, out["context_features"][k], o["context_features"][k], o64["context_features"][k], 3.0, 1e-5)
        for k in ("kl", "ce", "sup"):
            fwd["logits " + k] = anchored("logits " + k, out["logits"][k], o["logits"][k], o64["logits"][k], 3.0, 1e-5)
            if k != "ce":
                anchored("teacher logits " + k, tl[k], ot[k], ot64[k], 3.0, 1e-5)
        assert abs(loss.item() - ol64.item()) <= 3 * abs(ol.item() - ol64.item()) + 1e-5 * abs(ol64.item()), (loss.item(), ol.item(), ol64.item())
        from _anchor import record as _rec
        _rec("episode forward %d-shot %d-query %dpx %s %s [%s%s]" % (shot, query, img, clf, bb, ops.get_conv_compute_dtype(),
                                                                    ", trained-like statistics" if trained else ""), fwd)
    # argmax bit-exact wherever the oracle's top-2 margin exceeds the logit tolerance
    lg = o["logits"]["kl"].detach() + o["logits"]["ce"].detach()
    srt = torch.sort(lg, -1).values
    clear = (srt[:, -1] - srt[:, -2]) > (1.0 if bf16 else 5e-2)
    assert torch.equal(pred.cpu()[clear], torch.argmax(lg, -1)[clear])
    # gradients of every parameter, fp64-anchored (tests/_anchor.py): per tensor, the HIP gradient's relative-L2 error against
    # the oracle run in fp64 is at most 3x the error of the oracle's own fp32 run.  Both oracle runs use
    # the HIP path's own ReLU masks (checked above to differ from fp64's only at pre-activations within rounding of zero): one
    # flipped mask moves a small-map channel gradient by 1e-3 of the tensor norm in EITHER fp32 evaluation, which a fixed budget
    # can only absorb by being loose enough to hide a scheduling bug.
    # Tensors whose exact gradient is 0 (biases that cancel in q - s differences) are judged on an absolute floor.
    names = [k for k, p in student.named_parameters() if sp64[k].grad is not None]
    for k, p in student.named_parameters():
        if sp64[k].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    # trunk tensors: factor 3.  Head / matcher tensors (fc1, fc2, TRX projections): factor 6 - their gradients come through the
    # TRX distance -|q - prototype|^2 (a cancellation over 28 x 1152 terms) that the HIP path evaluates with two 2048-wide
    # per-frame projections instead of the reference's 4096-wide tuple Linear: same value, different fp32 rounding pattern
    # (measured 1.2e-4 vs 4e-5 relative to fp64 on fc2.weight).
    pg = dict(student.named_parameters())
    trunk = [k for k in names if k.startswith("backbone.resnet.")]
    head = [k for k in names if not k.startswith("backbone.resnet.")]
    gmax = max(float(sp64[k].grad.abs().max()) for k in names)
    worst = (0.0, "")
    for group, factor in ((trunk, 3.0), (head, 6.0)):
        for k in group:
            # floor 5e-5: the max-pool / adaptive-max-pool argmax choices are NOT imposed; a near-tie resolved differently moves
            # one gradient value to a neighbouring pixel (measured 3.5e-5 on the stem weight in one configuration)
            # (round 3: 1e-4 - with another arithmetic mode or another summation order in the stem's BatchNorm backward the near-ties
            # fall differently; measured up to 7.6e-5 on layer-1 / stem BatchNorm parameters in the 64-px episodes, while the block
            # tests, where every mask is imposed, hold the 2e-6 floor at 200 frames in the same arithmetic)
            # (round 3, later: the pooling selections ARE imposed now for the BasicBlock trunks - _hip_pool_choices / oracle.POOL_HOOK -
            # so what remains there is a linear map; the ResNet-50 cases, whose masks and selections were not imposed then, kept 1e-4)
            # (round 6: imposed for the Bottleneck trunks too - ops.ResBlockFn taps, oracle.resnet50_trunk through the hooks: the CPU pair
            # of the 64-px ResNet-50 episodes drops from 4e-3 ... 7e-3 to the 1e-5 class, so factor 3 binds there as well)
            e_hip, e_cpu = anchored(k, pg[k].grad, sp32[k].grad, sp64[k].grad, factor, 1e-4, 1e-7 * gmax)
            worst = max(worst, (e_hip / (e_cpu + 1e-6), k, e_hip, e_cpu))
    print("worst HIP/CPU gradient error ratio vs fp64:", worst, "loss", loss.item(), ol.item(), ol64.item(), "mask flips vs fp64:", flips,
          "pooling selections that differ from fp64's:", pflips)
    from _anchor import record
    record("episode %d-shot %d-query %dpx %s %s [%s%s%s]" % (shot, query, img, clf, bb, ops.get_conv_compute_dtype(),
                                                            ", bf16 tensors" if ops.get_activation_dtype() == "bf16" else "",
                                                            ", trained-like statistics" if trained else ""),
           {"worst parameter gradient (%s)" % worst[1]: worst[2:], "loss (hip, oracle fp32) vs fp64 abs": (abs(loss.item() - ol64.item()), abs(ol.item() - ol64.item()))})


def test_train_loop_runs_and_steps(dev):
    """real modules through trainloop.train: SGD step every (iteration+1)%tasks_per_batch, weights change only then"""
    from litemkd_amd import trainloop as TL
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from litemkd_amd.utils import aggregate_accuracy
    cfg = default_args(shot=1, query_per_class=1, img_size=64, device=dev, training_iterations=5, tasks_per_batch=3,
                       learning_rate=1e-2, print_freq=100)
    torch.manual_seed(2)
    student, teacher = Student(cfg).to(dev), Teacher(cfg).to(dev)
    opt = TL.FusedOptimizer(student, "sgd", cfg.learning_rate)
    sch = TL.MultiStepLR(opt, cfg.sch)
    w0 = opt.bucket.flat.clone()
    src = TL.SyntheticEpisodes(cfg, base_seed=5, device=dev)
    losses, accs = TL.train(student, teacher, src, Distiller(cfg.distill_name, cfg.cfg, dev), opt, sch, aggregate_accuracy, cfg)
    assert len(losses) == 5 and all(l == l for l in losses)          # finite
    assert opt.steps == 3                                            # iterations 2 and 5 ((it+1)%3==0) and 4 (= total-1)
    assert float((opt.bucket.flat - w0).abs().max()) > 0
    assert float(opt.bucket.grad.abs().max()) == 0.0 or opt.steps >= 2
    # eval path: running statistics, no grad
    acc = TL.test(student, TL.SyntheticEpisodes(cfg, base_seed=9, device=dev, train=False), aggregate_accuracy,
                  default_args(**{**vars(cfg), "num_test_tasks": 2}))
    assert 0.0 <= acc[cfg.dataset]["accuracy"] <= 100.0


def test_train_loop_checkpoint_and_test_iters(dev, tmp_path):
    """trainwandb.py:171-187: a checkpoint {'iteration','model_state_dict'} every save_freq iterations that load_student
    (model_select.py:138-153) reads back — also with DataParallel's `module.` prefix on the trunk keys — and the in-training
    test() call at test_iters; the reloaded student scores the same test episodes identically."""
    import glob
    from litemkd_amd import trainloop as TL
    from litemkd_amd.model.model_select import Student, Teacher, load_student
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from litemkd_amd.utils import aggregate_accuracy
    cfg = default_args(shot=1, query_per_class=1, img_size=64, device=dev, training_iterations=4, tasks_per_batch=2,
                       learning_rate=1e-2, print_freq=100, save_freq=3, test_iters=[2], num_test_tasks=2, save_dir=str(tmp_path))
    torch.manual_seed(4)
    student, teacher = Student(cfg).to(dev), Teacher(cfg).to(dev)
    opt = TL.FusedOptimizer(student, "sgd", cfg.learning_rate)
    logged = []
    src = TL.SyntheticEpisodes(cfg, base_seed=6, device=dev)
    TL.train(student, teacher, src, Distiller(cfg.distill_name, cfg.cfg, dev), opt, TL.MultiStepLR(opt, cfg.sch),
             aggregate_accuracy, cfg, log=lambda it, a, b: logged.append((it, a, b)))
    assert any(isinstance(a, dict) and it == 1 for it, a, _ in logged)          # test() ran at iteration+1 == 2
    files = glob.glob(str(tmp_path / "*.pt"))
    assert len(files) == 1 and files[0].endswith("%s2.pt" % cfg.mode)            # (iteration+1) % 3 == 0 -> iteration 2
    ck = torch.load(files[0], map_location="cpu")
    assert ck["iteration"] == 2 and set(ck["model_state_dict"]) == set(student.state_dict())
    # the reference saves DataParallel-wrapped trunks: backbone.resnet.module.N... -> must load too
    dp = {k.replace("backbone.resnet.", "backbone.resnet.module."): v for k, v in ck["model_state_dict"].items()}
    torch.save({"iteration": 2, "model_state_dict": dp}, str(tmp_path / "dp.pt"))
    cfg2 = default_args(**{**vars(cfg), "test_model_path": str(tmp_path / "dp.pt")})
    restored = load_student(cfg2).to(dev)
    for k, v in ck["model_state_dict"].items():
        assert torch.equal(restored.state_dict()[k].cpu(), v), k
    ev = TL.SyntheticEpisodes(cfg, base_seed=11, device=dev, train=False)
    student.load_state_dict(ck["model_state_dict"])
    a1 = TL.test(student, ev, aggregate_accuracy, cfg)
    a2 = TL.test(restored, ev, aggregate_accuracy, cfg)
    assert a1 == a2


def test_kl_feature_episode_and_evaluator(dev, tmp_path):
    """(1) the KL_feature training branch (trainwandb.py:209-226,243-244): single-head student (resnet18_student + TRX), the
    features packed into the logits dicts, loss = CE/16 + KL + MSE vs the oracle on the same episode;  (2) the stand-alone
    evaluator (test.py:65-299 + select_test): a saved student checkpoint scores the same test episodes as trainloop.test, and a
    teacher checkpoint in the MFM key layout loads through load_teacher."""
    from litemkd_amd import trainloop as TL
    from litemkd_amd.evaluate import Evaluator
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from litemkd_amd.utils import aggregate_accuracy
    from oracle import ref_cpu as O
    cfg = default_args(shot=1, query_per_class=1, img_size=64, trans_dropout=0.0, device=dev, model_backbone="resnet18_student",
                       model_classifier="TRX", model_teacher="train_teacher", distill_name="KL_feature", save_dir=str(tmp_path),
                       num_test_tasks=3)
    torch.manual_seed(8)
    student, teacher = Student(cfg).to(dev), Teacher(cfg).to(dev)
    ep = O.make_episode(515, 5, 1, 1, img=64)
    loss, acc, _ = TL.train_task({k: v.unsqueeze(0) for k, v in ep.items()}, student, teacher, Distiller("KL_feature", cfg.cfg, dev),
                                 aggregate_accuracy, cfg)
    sp = {k: v.detach().cpu() for k, v in student.state_dict().items()}
    tp = {k[len("classifier.transformers."):]: v.detach().cpu() for k, v in teacher.state_dict().items()}
    o = O.student_forward(ep, sp, 5, 1, classifier="TRX", backbone="resnet18_student", update_running=False)
    t_log = O.trx_logits(ep["support_set_feature_teacher"], ep["support_labels"], ep["target_set_feature_teacher"], tp)
    ref = O.distill_KL_feature({"logits": o["logits"], "feature": torch.cat([o["context_features"], o["target_features"]], 0)},
                               {"logits": t_log, "feature": torch.cat([ep["support_set_feature_teacher"], ep["target_set_feature_teacher"]], 0)},
                               ep["target_labels"].long())["loss"]
    assert abs(float(loss) - float(ref)) < 1e-3 * max(1.0, abs(float(ref))), (float(loss), float(ref))
    assert torch.isfinite(loss) and sum(1 for p in student.parameters() if p.grad is not None) > 60
    # evaluator on a student checkpoint
    path = TL.save_checkpoint(student, 7, cfg)
    ecfg = default_args(**{**vars(cfg), "test_model": "student", "test_model_path": path})
    lines = []
    res = Evaluator(ecfg, log=lines.append).test()
    ref_acc = TL.test(student, TL.SyntheticEpisodes(cfg, base_seed=777, device=dev, train=False), aggregate_accuracy, cfg)
    assert res == ref_acc and len(lines) == 4 and 0.0 <= res[cfg.dataset]["accuracy"] <= 100.0
    # evaluator on a teacher: MFM checkpoint layout `bracnch.transformers.0.*` (model_select.py:105-117)
    tsd = {"bracnch.transformers.0." + k[len("classifier.transformers."):]: v.detach().cpu() for k, v in teacher.state_dict().items()}
    torch.save({"iteration": 1, "model_state_dict": tsd}, str(tmp_path / "teacher.pt"))
    tcfg = default_args(**{**vars(cfg), "test_model": "teacher", "teacher_checkpoint": str(tmp_path / "teacher.pt")})
    ev = Evaluator(tcfg, log=lambda s: None)
    for k, v in teacher.classifier.transformers.state_dict().items():
        assert torch.equal(ev.model.transformers.state_dict()[k].cpu(), v.cpu()), k
    assert 0.0 <= ev.test()[cfg.dataset]["accuracy"] <= 100.0


def test_live_mfm_episode_resnet50(dev):
    """BASELINE configs[4] shape in the loop: ResNet-50 student (resnet50_2fc) + the MFM fusion computing the teacher features of
    the episode LIVE from rgb / depth / flow per-modality features (ThreeTRXShiftLoopTime.extract_feature at its full width 2048,
    teacher/code/model.py:1648-1664), frozen TRX_2fcsup_fixed teacher on them, fc_2_sup_dist, backward.  The fused features equal
    the oracle's MFM on the same weights and the teacher logits the oracle's TRX on them; the student side is finite and complete."""
    import argparse
    from litemkd_amd import trainloop as TL
    from litemkd_amd.teacher import ThreeTRXShiftLoopTime
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from litemkd_amd.utils import aggregate_accuracy
    from oracle import ref_cpu as O
    cfg = default_args(shot=1, query_per_class=1, img_size=64, trans_dropout=0.0, device=dev, model_backbone="resnet50_2fc")
    torch.manual_seed(13)
    student, teacher = Student(cfg).to(dev), Teacher(cfg).to(dev)
    with torch.device(dev):
        mfm = ThreeTRXShiftLoopTime(argparse.Namespace(seq_len=8, trans_num=2, shirt_num=1)).eval()
    p = O.make_mfm_params(5)
    mfm.load_state_dict(p, strict=True)
    rgb, depth, flow = O.make_mfm_inputs(6, 10)
    fused = mfm.extract_feature({"rgb": rgb.to(dev), "depth": depth.to(dev), "flow": flow.to(dev)})
    with torch.no_grad():
        ref = O.mfm_extract_feature(rgb, depth, flow, p, 1, 2)
    assert float((fused.cpu() - ref).abs().max()) < 2e-4 * float(ref.abs().max()) + 2e-4
    ep = O.make_episode(321, 5, 1, 1, img=64)
    ep = dict(ep, support_set_feature_teacher=fused[:5].cpu(), target_set_feature_teacher=fused[5:].cpu())
    loss, acc, _ = TL.train_task({k: v.unsqueeze(0) for k, v in ep.items()}, student, teacher, Distiller("fc_2_sup_dist", cfg.cfg, dev),
                                 aggregate_accuracy, cfg)
    assert torch.isfinite(loss) and 0.0 <= float(acc) <= 1.0
    tp = {k[len("classifier.transformers."):]: v.detach().cpu() for k, v in teacher.state_dict().items() if k.startswith("classifier.transformers.")}
    tl = teacher(fused[:5], ep["support_labels"].to(dev), fused[5:])["logits"]
    ot = O.clf_TRX_2fcsup_fixed(ref[:5], ep["support_labels"], ref[5:], tp, 5, 1)
    for k in ("kl", "sup"):
        assert torch.allclose(tl[k].cpu(), ot[k], rtol=2e-3, atol=5e-2), (k, float((tl[k].cpu() - ot[k]).abs().max()))
    g = [q.grad for q in student.parameters() if q.grad is not None]
    assert len(g) > 150 and all(torch.isfinite(x).all() for x in g)


def test_full_size_properties(dev):
    """BASELINE size (5-way 5-shot, 8x224^2): properties that need no oracle —
    BN batch independence of the two trunk calls, permutation equivariance over frames, determinism."""
    from litemkd_amd.model.backbone.resnet import ResNet18Trunk
    from litemkd_amd import ops
    torch.manual_seed(3)
    trunk = ResNet18Trunk().to(dev).train()
    x = torch.rand(200, 3, 224, 224, device=dev)
    with torch.no_grad():
        f1 = ops.PoolHeadFn.apply(trunk(x))
        f2 = ops.PoolHeadFn.apply(trunk(x))
        perm = torch.randperm(200, device=dev)
        f3 = ops.PoolHeadFn.apply(trunk(x[perm].contiguous()))
    assert torch.equal(f1, f2)                                        # deterministic (no float atomics)
    # batch statistics are permutation invariant up to fp32 summation order
    assert float((f3 - f1[perm]).abs().max()) < 1e-3 * float(f1.abs().max())
    assert torch.isfinite(f1).all()


def test_packed_weight_cache_follows_optimizer(dev):
    """the packed conv weights are cached between optimizer steps; after a fused SGD step (raw-pointer update) and after
    an in-place torch update the next forward must see the new weights"""
    from litemkd_amd import trainloop as TL
    from litemkd_amd.model.backbone.resnet import ResNet18Trunk
    torch.manual_seed(5)
    trunk = ResNet18Trunk().to(dev).train()
    x = torch.rand(4, 3, 64, 64, device=dev)
    opt = TL.FusedOptimizer(trunk, "sgd", 0.05)
    y0 = trunk(x)
    y0.sum().backward()
    opt.step()                                   # weights change through the flat buffer
    y1 = trunk(x)
    fresh = ResNet18Trunk().to(dev).train()
    fresh.load_state_dict(trunk.state_dict())    # same weights, no cached packs
    for m in fresh.modules():
        if hasattr(m, "running_mean"):
            pass
    # running statistics do not enter train-mode outputs, so the two forwards must agree exactly
    y2 = fresh(x)
    assert float((y1 - y0).abs().max()) > 0
    assert torch.equal(y1, y2)
    with torch.no_grad():
        getattr(trunk, "4")[0].conv1.weight.mul_(1.5)      # in-place torch update bumps _version
    fresh.load_state_dict(trunk.state_dict())
    assert torch.equal(trunk(x), fresh(x))


_FULL64 = {}


@pytest.mark.parametrize("mode", ["fp32h2", "fp32x3", "fp32"])
def test_full_size_episode_matches_oracle(dev, mode):
    """BASELINE configs[1] at full size (5-way 5-shot, 5 queries/class, 400 frames of 224x224): logits, loss and class
    predictions of the HIP path against the CPU oracle on the same episode and weights (~10 s of oracle time), in the library
    default arithmetic (fp32x3 = what bench.py times) and in the native fp32 MFMA mode.  (The gradients at this size:
    test_episode_matches_oracle[5-5-224-...-fp32x3].)"""
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from litemkd_amd import ops
    from oracle import ref_cpu as O
    ops.set_conv_compute_dtype(mode)
    args = default_args(trans_dropout=0.0, device=dev)
    torch.manual_seed(11)
    student, teacher = Student(args).to(dev), Teacher(args).to(dev)
    ep = O.make_episode(4242, 5, 5, 5)
    sp = {k: v.detach().cpu().clone() for k, v in student.state_dict().items()}
    tp = {k[len("classifier.transformers."):]: v.detach().cpu().clone() for k, v in teacher.state_dict().items()
          if k.startswith("classifier.transformers.")}
    labels = ep["target_labels"].long()
    with torch.no_grad():
        out = student(ep["support_set"].to(dev), ep["support_labels"].to(dev), ep["target_set"].to(dev))
        tl = teacher(ep["support_set_feature_teacher"].to(dev), ep["support_labels"].to(dev), ep["target_set_feature_teacher"].to(dev))["logits"]
        loss = Distiller("fc_2_sup_dist", args.cfg, dev).fc_2_sup_dist(out["logits"], tl, labels.to(dev))["loss"]
        acc, pred = ops.accuracy(out["logits"]["kl"], out["logits"]["ce"], labels.to(dev))
        o = O.student_forward(ep, sp, 5, 5)
        ot = O.clf_TRX_2fcsup_fixed(ep["support_set_feature_teacher"], ep["support_labels"], ep["target_set_feature_teacher"], tp, 5, 5)
        ol = O.distill_fc_2_sup_dist(o["logits"], ot, labels)["loss"]
        # the same forward in fp64 (once per session: both arithmetic modes start from the same seeded weights and episode)
        if "o64" not in _FULL64:
            e64 = {k: (v.double() if v.is_floating_point() else v) for k, v in ep.items()}
            o64 = O.student_forward(e64, {k: (v.double() if v.is_floating_point() else v) for k, v in sp.items()}, 5, 5)
            ot64 = O.clf_TRX_2fcsup_fixed(e64["support_set_feature_teacher"], e64["support_labels"], e64["target_set_feature_teacher"],
                                          {k: v.double() for k, v in tp.items()}, 5, 5)
            _FULL64.update(o64=o64, ol64=O.distill_fc_2_sup_dist(o64["logits"], ot64, labels)["loss"], w0=sp["backbone.resnet.0.weight"].clone())
        assert torch.equal(_FULL64["w0"], sp["backbone.resnet.0.weight"])
        o64, ol64 = _FULL64["o64"], _FULL64["ol64"]
    # fp64-anchored (round 4; before: 2e-3 / 2e-2 / 1e-3): relative-L2 error vs fp64 <= 3 x the fp32 oracle's own + 1e-5
    from _anchor import anchored, record
    fwd = {}
    for k in ("context_features_1", "context_features_2"):
        fwd[k] = anchored(k, out["context_features"][k], o["context_features"][k], o64["context_features"][k], 3.0, 1e-5)
    for k in ("kl", "ce", "sup"):
        fwd["logits " + k] = anchored("logits " + k, out["logits"][k], o["logits"][k], o64["logits"][k], 3.0, 1e-5)
    assert abs(loss.item() - ol64.item()) <= 3 * abs(ol.item() - ol64.item()) + 1e-5 * abs(ol64.item()), (loss.item(), ol.item(), ol64.item())
    fwd["loss abs"] = (abs(loss.item() - ol64.item()), abs(ol.item() - ol64.item()))
    record("full-size episode forward (400 frames of 224^2) [%s]" % mode, fwd)
    lg = o["logits"]["kl"] + o["logits"]["ce"]
    srt = torch.sort(lg, -1).values
    clear = (srt[:, -1] - srt[:, -2]) > 5e-2
    assert int(clear.sum()) >= 20                                       # the margin guard must not hide the test
    assert torch.equal(pred.cpu()[clear], torch.argmax(lg, -1)[clear])   # bit-exact class indices
    assert abs(float(acc) - float(O.aggregate_accuracy(lg, labels))) < 1e-6 or not bool(clear.all())
    # running statistics after the two deferred updates (support first, then query) equal the serial reference order
    assert _rel(student.state_dict()["backbone.resnet.1.running_mean"], sp["backbone.resnet.1.running_mean"]) < 1e-3
    assert _rel(student.state_dict()["backbone.resnet.7.1.bn2.running_var"], sp["backbone.resnet.7.1.bn2.running_var"]) < 1e-3


@pytest.mark.parametrize("clf,dist,teacher", [("TRX", "KD", "train_teacher"), ("TRX_2fc", "fc_2", "train_teacher"),
                                             ("e_dist_1fc_sup", "e_dist_1fc_sup", "e_dist_fc2_sup")])
def test_other_plugin_combinations_run(dev, clf, dist, teacher):
    """registry combinations from the reference's scripts other than the default: forward + loss + backward produce
    finite values, and the single-head TRX path equals the 'kl' head of TRX_2fcsup on the same features"""
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from oracle import ref_cpu as O
    bb = "resnet18_student" if clf in ("TRX", "e_dist_1fc_sup") else "resnet18_2fc"
    args = default_args(shot=1, query_per_class=1, img_size=64, trans_dropout=0.0, device=dev, model_classifier=clf,
                        model_backbone=bb, model_teacher=teacher, distill_name=dist)
    torch.manual_seed(3)
    student, tch = Student(args).to(dev), Teacher(args).to(dev)
    ep = O.make_episode(77, 5, 1, 1, img=64)
    out = student(ep["support_set"].to(dev), ep["support_labels"].to(dev), ep["target_set"].to(dev))
    tl = tch(ep["support_set_feature_teacher"].to(dev), ep["support_labels"].to(dev), ep["target_set_feature_teacher"].to(dev))["logits"]
    loss = getattr(Distiller(dist, args.cfg, dev), dist)(out["logits"], tl, ep["target_labels"].long().to(dev))["loss"]
    loss.backward()
    assert torch.isfinite(loss)
    g = [p.grad for p in student.parameters() if p.grad is not None]
    assert len(g) > 60 and all(torch.isfinite(x).all() for x in g)
    if clf == "TRX":
        sp = {k: v.detach().cpu() for k, v in student.state_dict().items()}
        cp = {k[len("classifier.transformers."):]: v for k, v in sp.items() if k.startswith("classifier.transformers.")}
        ref = O.trx_logits(out["context_features"].detach().cpu(), ep["support_labels"], out["target_features"].detach().cpu(), cp)
        assert torch.allclose(out["logits"].detach().cpu(), ref, rtol=1e-4, atol=2e-2)


def test_side_stream_weight_gradients_identical(dev):
    """ops.SIDE_WGRAD: conv weight gradients launched on their own stream and accumulated into weight.grad there.  After one
    backward pass they are bit-identical to the autograd path (same kernels, same order); over two passes they agree to fp32
    rounding (autograd sums the two trunk calls' gradients of a pass in its input buffer before adding them to .grad, the side
    stream adds them one by one).  Checked with and without the end-of-backward wait (then after wait_weight_grads())."""
    from litemkd_amd import ops
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from oracle import ref_cpu as O
    args = default_args(shot=1, query_per_class=1, img_size=64, trans_dropout=0.0, device=dev)
    torch.manual_seed(5)
    student, teacher = Student(args).to(dev), Teacher(args).to(dev)
    ep = O.make_episode(77, 5, 1, 1, img=64)
    labels = ep["target_labels"].long().to(dev)

    def grads(side, sync_at_end, passes):
        ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END = side, sync_at_end
        student.zero_grad(set_to_none=True)
        for _ in range(passes):
            out = student(ep["support_set"].to(dev), ep["support_labels"].to(dev), ep["target_set"].to(dev))
            tl = teacher(ep["support_set_feature_teacher"].to(dev), ep["support_labels"].to(dev), ep["target_set_feature_teacher"].to(dev))["logits"]
            Distiller("fc_2_sup_dist", args.cfg, dev).fc_2_sup_dist(out["logits"], tl, labels)["loss"].backward()
        if not sync_at_end:
            ops.wait_weight_grads()
        return {n: p.grad.clone() for n, p in student.named_parameters() if p.grad is not None}
    try:
        for passes in (1, 2):
            ref = grads(False, True, passes)
            for sync in (True, False):
                got = grads(True, sync, passes)
                assert set(got) == set(ref)
                for n in ref:
                    if passes == 1:
                        assert torch.equal(got[n], ref[n]), (n, sync)
                    else:
                        assert float((got[n] - ref[n]).abs().max()) <= 2e-6 * float(ref[n].abs().max()) + 1e-12, (n, sync)
    finally:
        ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END = False, True


def test_direct_param_grads_match_autograd_path(dev):
    """ops.DIRECT_PARAM_GRAD: BatchNorm / Linear / TRX parameter gradients added into .grad inside the HIP kernels (the side stream's
    share into FlatParams.shadow, folded by the optimizer) instead of returned to autograd.  After two accumulated episodes the
    flat gradient buffer equals the autograd path's to fp32 rounding (the same per-call gradients, added in a different order);
    the teacher head on its own stream (trainloop.TEACHER_STREAM) is exercised on the way."""
    from litemkd_amd import ops, trainloop as TL
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from litemkd_amd.utils import aggregate_accuracy
    cfg = default_args(shot=1, query_per_class=1, img_size=64, trans_dropout=0.0, device=dev)
    torch.manual_seed(21)
    student, teacher = Student(cfg).to(dev), Teacher(cfg).to(dev)
    opt = TL.FusedOptimizer(student, "sgd", 1e-3)
    distiller = Distiller(cfg.distill_name, cfg.cfg, dev)
    src = TL.SyntheticEpisodes(cfg, base_seed=31, device=dev)
    eps = [src.episode(e) for e in range(2)]

    def grads(direct, teacher_stream):
        prev = (ops.DIRECT_PARAM_GRAD, ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END, TL.TEACHER_STREAM)
        ops.DIRECT_PARAM_GRAD, ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END, TL.TEACHER_STREAM = direct, True, False, teacher_stream
        try:
            opt.zero_grad()
            losses = [TL.train_task(ep, student, teacher, distiller, aggregate_accuracy, cfg)[0] for ep in eps]
            ops.wait_weight_grads()
            if direct:
                assert float(opt.bucket.shadow.abs().max()) > 0          # the side stream's BatchNorm gradients went to the shadow
                opt.bucket.fold_shadow()
            torch.cuda.synchronize()
            return opt.bucket.grad.clone(), torch.stack(losses)
        finally:
            ops.DIRECT_PARAM_GRAD, ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END, TL.TEACHER_STREAM = prev
    g_ref, l_ref = grads(False, False)
    g_dir, l_dir = grads(True, True)
    assert torch.equal(l_ref, l_dir)                                   # the forward does not change
    assert float(g_ref.abs().max()) > 0
    scale = float(g_ref.abs().max())
    assert float((g_dir - g_ref).abs().max()) <= 2e-6 * scale, float((g_dir - g_ref).abs().max()) / scale
    # per parameter: relative L2
    for p, o in zip(opt.bucket.params, opt.bucket.offsets):
        a, b = g_dir[o:o + p.numel()].double(), g_ref[o:o + p.numel()].double()
        assert float((a - b).norm()) <= 1e-5 * float(b.norm()) + 1e-9 * scale, (o, float((a - b).norm() / (b.norm() + 1e-30)))
