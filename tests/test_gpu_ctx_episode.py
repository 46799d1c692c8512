"""GPU: whole episodes with the CTX head (resnet18_student + CTX, the CTX_fixed teacher loaded from a `bracnch.transformers.*` checkpoint
on seeded teacher features, KD) against the CPU oracle's ResNet-18 trunk with the restatement tests/_ctx_ref.py on top, the HIP path's
ReLU masks and pooling selections imposed the way tests/test_gpu_otam_episode.py imposes them; the default and bench schedules against
the serial one in the training loop; the other plain-logits distillers; the evaluator's command line.  Criterion of
test_gpu_otam_episode.py: logits and loss factor 3 with floor 1e-5, trunk parameter gradients factor 3, head parameter gradients
factor 6, floor 1e-4."""
import pytest
import torch
import torch.nn.functional as F

from _anchor import anchored, record
import _ctx_ref as R
from test_gpu_episode import _MaskedReLU, _hip_pool_choices, _hip_relu_masks

pytestmark = pytest.mark.gpu
NAMES = dict(model_backbone="resnet18_student", model_classifier="CTX", model_teacher="test_teacher_ctx", distill_name="KD")
HEAD = {"wk": "k_linear.weight", "bk": "k_linear.bias", "wv": "v_linear.weight", "bv": "v_linear.bias", "gamma": "norm_k.weight",
        "beta": "norm_k.bias"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def teacher_ckpt(tmp_path_factory):
    """a TwoCTXShuffleTime-layout checkpoint: a seeded head under `bracnch.`, norm_k off its default so the LayerNorm's affine part counts"""
    from litemkd_amd.model import classifiers as C
    from litemkd_amd.options import default_args
    torch.manual_seed(41)
    head = C.CTX(default_args(device=torch.device("cpu")))
    with torch.no_grad():
        head.transformers.norm_k.weight.add_(0.1 * torch.randn(1152))
        head.transformers.norm_k.bias.add_(0.1 * torch.randn(1152))
    path = str(tmp_path_factory.mktemp("ctx") / "two_ctx.pt")
    torch.save({"model_state_dict": {"bracnch." + k: v.clone() for k, v in head.state_dict().items()}}, path)
    return path


def _head(p, pre, dt):
    out = {k: p[pre + name].to(dt) for k, name in HEAD.items()}      # (.to of a leaf already in dt is the leaf itself)
    out["pe"] = p[pre + "pe.pe"].detach()[0].to(dt)
    return out


def test_ctx_episode_matches_oracle(dev, teacher_ckpt):
    from litemkd_amd import ops
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.model import classifiers as C
    from litemkd_amd.model.backbone import resnet as RN
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.options import default_args
    from oracle import ref_cpu as O
    way, shot, query, img = 5, 1, 1, 96
    ops.set_conv_compute_dtype("fp32x3")
    args = default_args(shot=shot, query_per_class=query, img_size=img, trans_dropout=0.0, device=dev, teacher_checkpoint=teacher_ckpt, **NAMES)
    torch.manual_seed(1)
    student, teacher = Student(args).to(dev), Teacher(args).to(dev)
    assert type(student.classifier) is C.CTX and type(teacher.classifier) is C.CTX_fixed
    ep = O.make_episode(971, way, shot, query, img=img)
    sp = {k: v.detach().cpu().clone() for k, v in student.state_dict().items()}
    tp = {k: v.detach().cpu().clone() for k, v in teacher.state_dict().items()}
    labels, sup_labels = ep["target_labels"].long(), ep["support_labels"]
    overlap = RN.OVERLAP_TRUNK_CALLS
    RN.OVERLAP_TRUNK_CALLS = False
    ops.BLOCK_TAPS = []
    try:
        out = student(ep["support_set"].to(dev), ep["support_labels"].to(dev), ep["target_set"].to(dev))
        taps = ops.split_block_taps(ops.BLOCK_TAPS)
    finally:
        RN.OVERLAP_TRUNK_CALLS, ops.BLOCK_TAPS = overlap, None
    tl = teacher(ep["support_set_feature_teacher"].to(dev), ep["support_labels"].to(dev), ep["target_set_feature_teacher"].to(dev))["logits"]
    assert tl.grad_fn is None
    loss = Distiller("KD", args.cfg, dev).KD(out["logits"], tl, labels.to(dev))["loss"]
    loss.backward()
    torch.cuda.synchronize()
    ops.reset_compute_dtypes()
    masks, pools = _hip_relu_masks(taps), _hip_pool_choices(taps)
    flips = [0, 0]

    def oracle(dt):
        p = {k: (v.clone().to(dt) if v.is_floating_point() else v.clone()) for k, v in sp.items()}
        for k, v in p.items():
            if v.is_floating_point() and "running" not in k and not k.endswith("pe.pe"):
                v.requires_grad_()
        site, psite = [0], {"stem": 0, "head": 0}

        def hook(t):
            m = masks[site[0]]
            site[0] += 1
            if dt == torch.float64:      # a mask may differ from the fp64 one only where the pre-activation is within rounding of 0
                diff = m != (t.detach() > 0)
                flips[0] += int(diff.sum())
                flips[1] += m.numel()
                assert not bool(diff.any()) or float(t.detach()[diff].abs().max()) < 1e-5 * float(t.detach().abs().max()), site[0]
            return _MaskedReLU.apply(t, m.to(dt))

        def pool_hook(kind, t):
            idx = pools[psite[kind]][kind]
            psite[kind] += 1
            v = t.flatten(2).gather(2, idx.flatten(2)).reshape(idx.shape)
            if dt == torch.float64:      # ... and a selection only at a tie within rounding
                nat = F.max_pool2d(t.detach(), 3, 2, 1) if kind == "stem" else F.adaptive_max_pool2d(t.detach(), (4, 4))
                assert float((nat - v.detach()).max()) <= 1e-5 * float(t.detach().abs().max()), kind
            return v
        bp = {k[len("backbone."):]: v for k, v in p.items() if k.startswith("backbone.")}
        O.RELU_HOOK, O.POOL_HOOK = hook, pool_hook
        try:
            fs, fq = O.backbone_resnet18_student(ep["support_set"].to(dt), ep["target_set"].to(dt), bp)
        finally:
            O.RELU_HOOK = O.POOL_HOOK = None
        logits = R.ctx_head(fs, sup_labels, fq, way, **_head(p, "classifier.transformers.", dt))
        with torch.no_grad():
            ot = R.ctx_head(ep["support_set_feature_teacher"].to(dt), sup_labels, ep["target_set_feature_teacher"].to(dt), way,
                            **_head(tp, "classifier.transformers.", dt))
        ol = O.distill_method("KD", logits, ot, labels)
        ol.backward()
        return p, logits, ot, ol
    p32, l32, t32, ol32 = oracle(torch.float32)
    p64, l64, t64, ol64 = oracle(torch.float64)
    fwd = {"logits": anchored("logits", out["logits"], l32, l64, 3.0, 1e-5),
           "teacher logits": anchored("teacher logits", tl, t32, t64, 3.0, 1e-5)}
    assert abs(loss.item() - ol64.item()) <= 3 * abs(ol32.item() - ol64.item()) + 1e-5 * abs(ol64.item()), (loss.item(), ol32.item(), ol64.item())
    tag = "ctx episode %d-shot %d-query %dpx resnet18_student CTX KD [fp32x3]" % (shot, query, img)
    record(tag + " forward", fwd)
    pg = dict(student.named_parameters())
    names = [k for k in pg if p64[k].grad is not None]
    assert sum(k.startswith("classifier.transformers.") for k in names) == 6 and len(names) > 60
    for k, v in pg.items():
        if p64[k].grad is None:
            assert "norm_v" in k and v.grad is None, k
    gmax = max(float(p64[k].grad.abs().max()) for k in names)
    worst, grads = (0.0, ""), {}
    for k in names:
        factor = 3.0 if k.startswith("backbone.resnet.") else 6.0
        e_hip, e_cpu = anchored(k, pg[k].grad, p32[k].grad, p64[k].grad, factor, 1e-4, 1e-7 * gmax)
        grads[k] = (e_hip, e_cpu)
        worst = max(worst, (e_hip / (e_cpu + 1e-6), k, e_hip, e_cpu))
    print("worst HIP/CPU gradient error ratio vs fp64:", worst, "loss", loss.item(), ol32.item(), ol64.item(), "mask flips vs fp64:", flips)
    record(tag + " gradients", grads)


def _run(dev, sched, ckpt, episodes=3, lr=1e-2, seed=3):
    """tests/test_gpu_schedule.py::_run for the CTX student: `episodes` accumulated training episodes of trainloop's loop + one SGD step
    under `sched` -> (losses, flat gradient bucket before the step, flat weights after it)"""
    from litemkd_amd import ops, trainloop as TL
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from litemkd_amd.utils import aggregate_accuracy
    cfg = default_args(shot=1, query_per_class=1, img_size=64, trans_dropout=0.0, device=dev, opt="sgd", learning_rate=lr,
                       teacher_checkpoint=ckpt, **NAMES)
    with sched.applied():
        torch.manual_seed(seed)
        student, teacher = TL.init_model(cfg)
        distiller = Distiller(cfg.distill_name, cfg.cfg, dev)
        optim = TL.FusedOptimizer(student, "sgd", lr)
        optim.zero_grad()
        src = TL.SyntheticEpisodes(cfg, base_seed=78, device=dev)
        pool = [src.episode(e) for e in range(episodes)]
        losses = []
        if sched.pipeline_episodes:
            pipe = TL.PipelinedEpisodes(student, teacher, distiller, aggregate_accuracy, cfg)
            for ep in pool:
                r = pipe.push(ep)
                if r is not None:
                    losses.append(r[0])
            r = pipe.flush()
            losses += [x[0] for x in (r if isinstance(r, list) else [r])]
        else:
            for ep in pool:
                losses.append(TL.train_task(ep, student, teacher, distiller, aggregate_accuracy, cfg)[0])
        ops.join_all_streams()
        optim.bucket.fold_shadow()
        grad = optim.bucket.grad.clone()
        optim.step()
        optim.zero_grad()
        torch.cuda.synchronize()
        return torch.stack(losses).cpu(), grad, optim.bucket.flat.clone()


@pytest.fixture(scope="module")
def serial_run(dev, teacher_ckpt):
    from litemkd_amd.schedule import Schedule
    return _run(dev, Schedule.serial(), teacher_ckpt)


@pytest.mark.parametrize("which", ["default", "bench"])
def test_schedules_agree_with_the_serial_one(dev, teacher_ckpt, serial_run, which):
    """three accumulated episodes + one SGD step: losses identical, the gradient bucket within 5e-6 of its maximum and the weights after
    the step to that precision - test_gpu_otam_episode.py's comparison.  The schedules add the head's parameter gradients into .grad
    from the kernels (ops.DIRECT_PARAM_GRAD) and run its weight gradients on the weight-gradient stream; the serial one returns them."""
    from litemkd_amd.schedule import Schedule
    lr, tol = 1e-2, 5e-6
    la, ga, wa = serial_run
    lb, gb, wb = _run(dev, Schedule() if which == "default" else Schedule.bench(), teacher_ckpt, lr=lr)
    assert bool(torch.isfinite(la).all()) and float(ga.abs().max()) > 0
    assert torch.equal(la, lb), (la, lb)
    gmax = float(ga.abs().max())
    assert float((ga - gb).abs().max()) <= tol * gmax, float((ga - gb).abs().max()) / gmax
    assert float((wa - wb).abs().max()) <= lr * tol * gmax + 1.2e-7 * float(wa.abs().max()), float((wa - wb).abs().max())


@pytest.mark.parametrize("distill", ["Dist_KD", "ce", "wsl"])
def test_other_logits_distillers_run(dev, teacher_ckpt, distill):
    """the other distillers that take plain logits tensors: forward + loss + backward through the CTX head are finite and reach the trunk"""
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.options import default_args
    from oracle import ref_cpu as O
    args = default_args(shot=1, query_per_class=1, img_size=64, trans_dropout=0.0, device=dev, teacher_checkpoint=teacher_ckpt,
                        **{**NAMES, "distill_name": distill})
    torch.manual_seed(3)
    student, tch = Student(args).to(dev), Teacher(args).to(dev)
    ep = O.make_episode(78, 5, 1, 1, img=64)
    out = student(ep["support_set"].to(dev), ep["support_labels"].to(dev), ep["target_set"].to(dev))
    tl = tch(ep["support_set_feature_teacher"].to(dev), ep["support_labels"].to(dev), ep["target_set_feature_teacher"].to(dev))["logits"]
    loss = getattr(Distiller(distill, args.cfg, dev), distill)(out["logits"], tl, ep["target_labels"].long().to(dev))["loss"]
    loss.backward()
    assert torch.isfinite(loss)
    g = [p.grad for p in student.parameters() if p.grad is not None]
    assert len(g) > 60 and all(torch.isfinite(x).all() for x in g) and max(float(x.abs().max()) for x in g) > 0


def test_evaluator_command_line_reads_a_ctx_student_checkpoint(dev, tmp_path):
    from litemkd_amd import evaluate, trainloop as TL
    from litemkd_amd.model.model_select import Student
    from litemkd_amd.options import default_args
    from litemkd_amd.utils import aggregate_accuracy
    cfg = default_args(shot=1, query_per_class=1, img_size=64, trans_dropout=0.0, device=dev, save_dir=str(tmp_path), num_test_tasks=3, **NAMES)
    torch.manual_seed(8)
    student = Student(cfg).to(dev)
    path = TL.save_checkpoint(student, 7, cfg)
    res = evaluate.main(("--test_model student --test_model_path %s --model_backbone resnet18_student --model_classifier CTX "
                         "--distill_name KD --num_test_tasks 3 --shot 1 --img_size 64" % path).split())
    ref_acc = TL.test(student, TL.SyntheticEpisodes(cfg, base_seed=777, device=dev, train=False), aggregate_accuracy, cfg)
    assert res == ref_acc and 0.0 <= res[cfg.dataset]["accuracy"] <= 100.0
