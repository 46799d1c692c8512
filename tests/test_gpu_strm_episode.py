"""GPU: whole STRM episodes (student + frozen TRX_2fcsup teacher + distiller + backward) against the CPU oracle's ResNet-18 trunk with
the restatement tests/_strm_ref.py on top of it, on the same seeded episode and weights, with the HIP path's ReLU masks, pooling and
minimum selections and dropout masks imposed the way tests/test_gpu_episode.py imposes them for the trunk.  Criterion of
test_gpu_episode.py: features and logits factor 3 with floor 1e-5, trunk parameter gradients factor 3, head parameter gradients
factor 6, floor 1e-4."""
import pytest
import torch
import torch.nn.functional as F

from _anchor import anchored, record
import _strm_ref as R
from test_gpu_episode import _MaskedReLU, _hip_pool_choices, _hip_relu_masks
from test_gpu_strm import _imposed_relu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.mark.parametrize("backbone,classifier,distill,shot,query,img,mode", [
    ("strm18_student", "strm_res18_sup", "strm_fc_2_sup_dist", 5, 5, 224, "fp32h2"),      # the 400-frame episode in bench.py's arithmetic
    ("strmbackbone", "strmclassifiers", "strm", 1, 1, 96, "fp32x3"),
])
def test_strm_episode_matches_oracle(dev, backbone, classifier, distill, shot, query, img, mode):
    from litemkd_amd import ops
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.model.backbone import resnet as RN
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.options import default_args
    from oracle import ref_cpu as O
    way = 5
    ops.set_conv_compute_dtype(mode)
    args = default_args(shot=shot, query_per_class=query, img_size=img, trans_dropout=0.0, device=dev, model_backbone=backbone,
                        model_classifier=classifier, distill_name=distill)
    torch.manual_seed(1)
    student, teacher = Student(args).to(dev), Teacher(args).to(dev)
    with torch.no_grad():
        student.backbone.attn_pat.gamma.fill_(R.GAMMA)
    ep = O.make_episode(950 + shot, way, shot, query, img=img)
    sp = {k: v.detach().cpu().clone() for k, v in student.state_dict().items()}
    tp = {k[len("classifier.transformers."):]: v.detach().cpu().clone() for k, v in teacher.state_dict().items()
          if k.startswith("classifier.transformers.")}
    labels = ep["target_labels"].long()
    sup_labels = ep["support_labels"].long()
    ns = way * shot
    overlap = RN.OVERLAP_TRUNK_CALLS
    RN.OVERLAP_TRUNK_CALLS = False
    ops.BLOCK_TAPS, ops.STRM_TAPS = [], {}
    try:
        torch.manual_seed(3)
        out = student(ep["support_set"].to(dev), ep["support_labels"].to(dev), ep["target_set"].to(dev))
        taps, st = ops.split_block_taps(ops.BLOCK_TAPS), ops.STRM_TAPS
    finally:
        RN.OVERLAP_TRUNK_CALLS, ops.BLOCK_TAPS, ops.STRM_TAPS = overlap, None, None
    tl = teacher(ep["support_set_feature_teacher"].to(dev), ep["support_labels"].to(dev), ep["target_set_feature_teacher"].to(dev))["logits"]
    loss = getattr(Distiller(distill, args.cfg, dev), distill)(out["logits"], tl, labels.to(dev))["loss"]
    loss.backward()
    torch.cuda.synchronize()
    ops.reset_compute_dtypes()
    trunk_masks, pools = _hip_relu_masks(taps), _hip_pool_choices(taps)
    head_masks = [m.cpu() for m in st["relu"]]
    pool_idx = torch.cat([t.cpu().long() for t in st["pool"]])
    sel = st["dist"][0].cpu().long()
    drop = [m.cpu() for m in st["dropout"]]
    assert len(drop) == 3 and len(head_masks) == 5
    flips = [0, 0]

    def oracle(dt):
        p = {k: (v.clone().to(dt) if v.is_floating_point() else v.clone()) for k, v in sp.items()}
        for k, v in p.items():
            if v.is_floating_point() and "running" not in k and not k.endswith("pe.pe"):
                v.requires_grad_()
        site, psite = [0], [0]

        def hook(t):
            m = trunk_masks[site[0]]
            site[0] += 1
            if dt == torch.float64:
                diff = m != (t.detach() > 0)
                flips[0] += int(diff.sum())
                flips[1] += m.numel()
                assert not bool(diff.any()) or float(t.detach()[diff].abs().max()) < 1e-5 * float(t.detach().abs().max()), site[0]
            return _MaskedReLU.apply(t, m.to(dt))

        def pool_hook(kind, t):
            assert kind == "stem"
            idx = pools[psite[0]]["stem"]
            psite[0] += 1
            v = t.flatten(2).gather(2, idx.flatten(2)).reshape(idx.shape)
            if dt == torch.float64:
                d = F.max_pool2d(t.detach(), 3, 2, 1) - v.detach()
                assert float(d.max()) <= 1e-5 * float(t.detach().abs().max())
            return v
        sd = {k[len("backbone.resnet."):]: v for k, v in p.items() if k.startswith("backbone.resnet.")}
        bp = {k[len("backbone."):]: v for k, v in p.items() if k.startswith("backbone.") and not k.startswith("backbone.resnet.")}
        cp = {k[len("classifier."):]: v for k, v in p.items() if k.startswith("classifier.")}
        O.RELU_HOOK, O.POOL_HOOK = hook, pool_hook
        try:
            fs = O.resnet18_trunk(ep["support_set"].to(dt), sd, True, True)
            fq = O.resnet18_trunk(ep["target_set"].to(dt), sd, True, True)
        finally:
            O.RELU_HOOK = O.POOL_HOOK = None
        fmap = torch.cat([fs, fq], 0).permute(0, 2, 3, 1)
        if dt == torch.float64:      # the imposed pooling selection differs from the natural one only at ties within rounding
            nat = R.patch_pool(fmap.detach())[0]
            got = R.patch_pool(fmap.detach(), pool_idx)[0]
            assert float((nat - got).max()) <= 1e-5 * float(fmap.detach().abs().max())
        masks = {"attn": drop[0], "mix": drop[1], "dist": drop[2]}
        with _imposed_relu(head_masks, dt, flips):
            feats, _ = R.backbone_head(fmap, bp, 8, backbone, pool_idx, masks)
            f_s = {k: v[:ns] for k, v in feats.items()}
            f_q = {k: v[ns:] for k, v in feats.items()}
            logits, _ = R.classifier(f_s, sup_labels, f_q, cp, way, shot, 8, masks["dist"], sel)
        ot = O.clf_TRX_2fcsup_fixed(ep["support_set_feature_teacher"].to(dt), ep["support_labels"], ep["target_set_feature_teacher"].to(dt),
                                    {k: v.to(dt) for k, v in tp.items()}, way, shot)
        ol = O.distill_method(distill, logits, ot, labels)
        ol.backward()
        return p, feats, logits, ol
    p32, f32, l32, ol32 = oracle(torch.float32)
    p64, f64, l64, ol64 = oracle(torch.float64)
    fwd = {}
    for k in f64:
        hip = torch.cat([out["context_features"][k], out["target_features"][k]], 0)
        fwd[k] = anchored("features " + k, hip, f32[k], f64[k], 3.0, 1e-5)
    for k in l64:
        fwd["logits " + k] = anchored("logits " + k, out["logits"][k], l32[k], l64[k], 3.0, 1e-5)
    assert abs(loss.item() - ol64.item()) <= 3 * abs(ol32.item() - ol64.item()) + 1e-5 * abs(ol64.item()), (loss.item(), ol32.item(), ol64.item())
    tag = "strm episode %d-shot %d-query %dpx %s %s %s [%s]" % (shot, query, img, backbone, classifier, distill, mode)
    record(tag + " forward", fwd)
    pg = dict(student.named_parameters())
    names = [k for k in pg if p64[k].grad is not None]
    for k, v in pg.items():
        if p64[k].grad is None:
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, k
    gmax = max(float(p64[k].grad.abs().max()) for k in names)
    worst, grads = (0.0, ""), {}
    for k in names:
        factor = 3.0 if k.startswith("backbone.resnet.") else 6.0
        print("grad %-48s" % k, end=" ")
        e_hip, e_cpu = anchored(k, pg[k].grad, p32[k].grad, p64[k].grad, factor, 1e-4, 1e-7 * gmax)
        print("hip %.3e cpu %.3e" % (e_hip, e_cpu))
        grads[k] = (e_hip, e_cpu)
        worst = max(worst, (e_hip / (e_cpu + 1e-6), k, e_hip, e_cpu))
    print("worst HIP/CPU gradient error ratio vs fp64:", worst, "loss", loss.item(), ol32.item(), ol64.item(), "mask flips vs fp64:", flips)
    record(tag + " gradients", grads)
