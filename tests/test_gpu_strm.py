"""GPU: the STRM student family (strm18_student / strmbackbone with strm_res18_sup / strmclassifiers / strm_res18) - every new operator
of csrc/strm.hip forward and backward against the plain-torch restatement tests/_strm_ref.py in fp64 (anchored: the HIP error is at most
3 x the error torch's CPU fp32 makes on the same inputs), the selections of the pooling and of the patch-distance head, the whole head
against the reference's own outputs (tests/golden/strm.npz), determinism, dropout, the training loop and the evaluator."""
import os

import numpy as np
import pytest
import torch

from _anchor import anchored, record
import _strm_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from litemkd_amd import ops
    ops.reset_compute_dtypes()
    return torch.device("cuda", 0)


def _mask(shape, seed, p=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) >= p).float() / (1.0 - p)


def _two(fn, inputs):
    """fn on fp32 and fp64 copies of the CPU tensors in `inputs` (dict), each a leaf with grad -> [(out, leaves)] for (fp32, fp64)"""
    res = []
    for dt in (torch.float32, torch.float64):
        leaves = {k: v.detach().to(dt).requires_grad_() for k, v in inputs.items()}
        res.append((fn(leaves), leaves))
    return res


def _check(name, hip, runs, pairs, key):
    (o32, l32), (o64, l64) = runs
    pairs[key] = anchored("%s %s" % (name, key), hip, l32[key].grad if key in l32 else o32, l64[key].grad if key in l64 else o64, 3.0)


# ----------------------------------------------------------------------------------------------------------------------------------
# single operators
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,masked", [(400, False), (400, True), (8, True), (8, False)])
def test_patch_pooling(dev, frames, masked):
    """indices equal torch's return_indices exactly on a post-ReLU map with whole windows of zeros; values and the gather backward"""
    from litemkd_amd import ops
    x = R.make_fmaps(frames, frames)
    x[::2, :2, :3] = 0
    x[1::3, 5:, 3:] = 0
    table = R.pe_table(512, 24)
    mask = _mask((frames, 16, 512), 3) if masked else None
    dy = torch.randn(frames, 16, 512, generator=torch.Generator().manual_seed(1))
    want, widx = torch.nn.functional.adaptive_max_pool2d(x.permute(0, 3, 1, 2), (4, 4), return_indices=True)
    widx = widx.permute(0, 2, 3, 1).reshape(frames, 16, 512)
    xd = x.to(dev).requires_grad_()
    md = mask.to(dev) if masked else None
    y, idx = ops.strm_patchpool_fwd(xd.detach(), table[0, :16].contiguous().to(dev), md)
    assert torch.equal(idx.cpu().long(), widx)
    runs = _two(lambda l: R.add_table(R.patch_pool(l["x"], widx)[0], table, mask), {"x": x})
    for (o, _), g in zip(runs, (dy, dy.double())):
        o.backward(g)
    pairs = {"y": anchored("patch pooling y", y, runs[0][0], runs[1][0], 3.0)}
    assert torch.equal(y.cpu(), runs[0][0].detach())      # max is exact, the add and the mask are single roundings
    out = ops.PatchPoolFn.apply(xd, table[0, :16].contiguous().to(dev), md)
    out.backward(dy.to(dev))
    pairs["dx"] = anchored("patch pooling dx", xd.grad, runs[0][1]["x"].grad, runs[1][1]["x"].grad, 3.0)
    low = ops.strm_patchpool_bwd(dy.to(dev), md, idx, 7, 7)
    assert torch.equal(low, xd.grad)
    record("strm patch pooling F=%d mask=%s" % (frames, masked), pairs)


@pytest.mark.parametrize("frames", [400, 8])
def test_patch_attention(dev, frames):
    """projections (one GEMM), energies, softmax, attn V, gamma * out + x with gamma = 0.3: forward and every gradient"""
    from litemkd_amd import ops
    g = torch.Generator().manual_seed(frames)
    p = R.make_backbone_params(7)
    names = ["attn_pat.%s.%s" % (m, w) for m in ("query_proj", "key_proj", "value_conv") for w in ("weight", "bias")] + ["attn_pat.gamma"]
    inputs = {"x": torch.relu(torch.randn(frames, 16, 512, generator=g)) + R.pe_table(512, 24)[0, :16]}
    inputs.update({k: p[k] for k in names})
    dy = torch.randn(frames, 16, 512, generator=g)
    runs = _two(lambda l: R.patch_attention(l["x"], l), inputs)
    for (o, _), gg in zip(runs, (dy, dy.double())):
        o.backward(gg)
    d = {k: v.to(dev).requires_grad_() for k, v in inputs.items()}
    y = ops.PatchAttnFn.apply(d["x"], *[d[k] for k in names])
    y.backward(dy.to(dev))
    pairs = {"y": anchored("patch attention y", y, runs[0][0], runs[1][0], 3.0)}
    for k in inputs:
        _check("patch attention d", d[k].grad, runs, pairs, k)
    record("strm patch attention F=%d" % frames, pairs)


@pytest.mark.parametrize("videos,masked", [(50, True), (50, False), (1, True), (1, False)])
def test_token_mlp(dev, videos, masked):
    from litemkd_amd import ops
    g = torch.Generator().manual_seed(videos)
    p = R.make_backbone_params(8)
    table = R.pe_table(2048, 12)
    mask = _mask((videos * 8, 2048), 4) if masked else None
    names = ["fr_enrich.Tok_MLP.%s.%s" % (m, w) for m in ("inp_fc", "out_fc") for w in ("weight", "bias")]
    inputs = {"x": torch.randn(videos, 8, 2048, generator=g)}
    inputs.update({k: p[k] for k in names})
    dy = torch.randn(videos, 8, 2048, generator=g)
    runs = _two(lambda l: R.token_mlp(R.add_table(l["x"], table, mask), *[l[k] for k in names]), inputs)
    for (o, _), gg in zip(runs, (dy, dy.double())):
        o.backward(gg)
    d = {k: v.to(dev).requires_grad_() for k, v in inputs.items()}
    y = ops.TokenMLPFn.apply(d["x"], table[0, :8].contiguous().to(dev), mask.to(dev) if masked else None, *[d[k] for k in names])
    y.backward(dy.to(dev))
    pairs = {"y": anchored("token MLP y", y, runs[0][0], runs[1][0], 3.0)}
    for k in inputs:
        _check("token MLP d", d[k].grad, runs, pairs, k)
    record("strm token MLP V=%d mask=%s" % (videos, masked), pairs)


@pytest.mark.parametrize("way,shot,query,masked", [(5, 5, 5, False), (5, 5, 5, True), (3, 2, 4, True), (3, 2, 4, False)])
def test_patch_distance(dev, way, shot, query, masked):
    """logits, the stored arg-min against fp64 on every row whose two smallest fp64 distances differ by more than 1e-4 relative (at most
    2 % of the rows may be left out), and the backward with the fp64 selections passed in.
    The left-out share is a property of the inputs alone (fp64 gaps; about 1.2 % on unit-normal features), so the odd-size case carries
    four query videos per class: 1008 (row, class) entries, where 2 % is 2.4 standard deviations above that rate - with one query video
    per class (252 entries) the cap would sit 1 standard deviation above it and fail one seed in eight whatever the kernel does."""
    from litemkd_amd import ops
    ns, nq, L = way * shot, way * query, 8
    g = torch.Generator().manual_seed(way * 100 + shot)
    cp = R.make_classifier_params(9)
    perm = torch.randperm(ns, generator=g)
    labels = torch.arange(way).repeat_interleave(shot)[perm]
    mask = _mask(((ns + nq) * L, 2048), 5) if masked else None
    inputs = {"sup": torch.randn(ns, L, 2048, generator=g), "qry": torch.randn(nq, L, 2048, generator=g),
              "w": cp["DistanceLoss.clsW.weight"], "b": cp["DistanceLoss.clsW.bias"]}
    gl = torch.randn(nq, way, generator=g)
    with torch.no_grad():
        _, sel64 = R.patch_distance(inputs["sup"].double(), labels, inputs["qry"].double(), inputs["w"].double(), inputs["b"].double(), way, mask)
        ms = None if mask is None else (mask[:ns * L].double(), mask[ns * L:].double())
        sup_m = inputs["sup"].double() if ms is None else inputs["sup"].double() * ms[0].reshape(ns, L, -1)
        qry_m = inputs["qry"].double() if ms is None else inputs["qry"].double() * ms[1].reshape(nq, L, -1)
        gaps = R.min_gaps(sup_m, labels, qry_m, inputs["w"].double(), inputs["b"].double(), way)
    runs = _two(lambda l: R.patch_distance(l["sup"], labels, l["qry"], l["w"], l["b"], way, mask, sel64)[0], inputs)
    for (o, _), gg in zip(runs, (gl, gl.double())):
        o.backward(gg)
    plan = ops.ClassPlan(labels.float().to(dev), way, labels.float())
    d = {k: v.to(dev) for k, v in inputs.items()}
    md = mask.to(dev) if masked else None
    X = torch.cat([d["sup"].reshape(-1, 2048), d["qry"].reshape(-1, 2048)], 0)
    Xd = X * md if masked else X
    P, E = ops.strm_patchdist_embed(Xd, d["w"], d["b"], L)
    logits, dist, idx = ops.strm_patchdist_fwd(E, plan, ns, nq, L)
    clear = gaps > 1e-4
    left_out = 1.0 - float(clear.float().mean())
    print("patch distance: rows left out %.4f" % left_out)
    assert left_out <= 0.02, left_out
    assert torch.equal(idx.cpu().long()[clear], sel64[clear]), int((idx.cpu().long() != sel64)[clear].sum())
    with torch.no_grad():
        free32 = R.patch_distance(inputs["sup"], labels, inputs["qry"], inputs["w"], inputs["b"], way, mask)[0]
        free64 = R.patch_distance(inputs["sup"].double(), labels, inputs["qry"].double(), inputs["w"].double(), inputs["b"].double(), way, mask)[0]
    pairs = {"logits": anchored("patch distance logits", logits, free32, free64, 3.0)}
    # the Function end to end (its own selections) gives the same logits
    leaf = {k: v.clone().requires_grad_() for k, v in d.items()}
    out = ops.PatchDistFn.apply(leaf["sup"], leaf["qry"], leaf["w"], leaf["b"], md, plan)
    assert torch.equal(out, logits)
    out.backward(gl.to(dev))
    # backward on the fp64 selections: distances of the imposed rows from the HIP embeddings
    T = L * (L - 1) // 2
    Es, Eq = E[:ns * T].reshape(ns, T, -1), E[ns * T:]
    dist_i = torch.empty_like(dist)
    for c in range(way):
        members = torch.nonzero(labels == c).reshape(-1).to(dev)
        ec = Es[members].reshape(-1, E.shape[1])
        dist_i[:, c] = (Eq.double() - ec[sel64[:, c].to(dev)].double()).pow(2).sum(-1).sqrt().float()
    dX, dw, db = ops.strm_patchdist_grads(Xd, d["w"], E, plan, dist_i, sel64.to(dev).int().contiguous(), gl.to(dev), md, ns, nq, L)
    hip = {"sup": dX[:ns * L].reshape(ns, L, -1), "qry": dX[ns * L:].reshape(nq, L, -1), "w": dw, "b": db}
    for k in inputs:
        _check("patch distance d", hip[k], runs, pairs, k)
    if bool((idx.cpu().long() == sel64).all()):      # the Function's own backward (its stored distances) agrees to rounding of the distances
        for k in inputs:
            assert float((leaf[k].grad.reshape(hip[k].shape) - hip[k]).norm() / hip[k].norm()) < 1e-5, k
    record("strm patch distance %d-way %d-shot %d-query mask=%s" % (way, shot, query, masked), pairs)


def test_patch_distance_zero_distance_has_zero_gradient(dev):
    """a query video equal to a support video: distance 0 on every pair row of that class, gradient 0 there (as cdist's backward)"""
    from litemkd_amd import ops
    way, shot, L = 2, 1, 8
    g = torch.Generator().manual_seed(0)
    cp = R.make_classifier_params(9)
    sup = torch.randn(2, L, 2048, generator=g)
    qry = torch.stack([sup[1], torch.randn(L, 2048, generator=g)])
    labels = torch.tensor([0.0, 1.0])
    plan = ops.ClassPlan(labels.to(dev), way, labels)
    leaf = [t.to(dev).requires_grad_() for t in (sup, qry, cp["DistanceLoss.clsW.weight"], cp["DistanceLoss.clsW.bias"])]
    out = ops.PatchDistFn.apply(*leaf, None, plan)
    assert float(out[0, 1].detach()) == 0.0
    out[0, 1].backward()
    for t in leaf:
        assert torch.isfinite(t.grad).all() and float(t.grad.abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------------------
# whole head and whole students
# ----------------------------------------------------------------------------------------------------------------------------------
def _student(dev, backbone, classifier, seed, **kw):
    """Student with the seeded head parameters of tests/_strm_ref.py (the trunk keeps its own initialisation)"""
    from litemkd_amd.model.model_select import Student
    from litemkd_amd.options import default_args
    args = default_args(model_backbone=backbone, model_classifier=classifier, device=dev, **kw)
    torch.manual_seed(seed)
    s = Student(args)
    sd = {"backbone." + k: v for k, v in R.make_backbone_params(seed, backbone).items()}
    sd.update({"classifier." + k: v for k, v in R.make_classifier_params(seed).items()})
    missing = s.load_state_dict(sd, strict=False)
    assert all(k.startswith("backbone.resnet.") for k in missing.missing_keys) and not missing.unexpected_keys
    return s.to(dev), args


class _imposed_relu:
    """every ReLU of the restatement takes the HIP path's mask (in evaluation order); in fp64 a mask may differ from the natural one only
    where the pre-activation is within rounding of zero"""

    def __init__(self, masks, dt, flips):
        self.masks, self.dt, self.flips, self.site = masks, dt, flips, 0

    def hook(self, t):
        m = self.masks[self.site].reshape(t.shape).bool()
        self.site += 1
        if self.dt == torch.float64:
            diff = m != (t.detach() > 0)
            self.flips[0] += int(diff.sum())
            self.flips[1] += m.numel()
            assert not bool(diff.any()) or float(t.detach()[diff].abs().max()) < 1e-5 * float(t.detach().abs().max()), self.site
        return t * m.to(t.dtype)

    def __enter__(self):
        R.RELU = self.hook

    def __exit__(self, *a):
        R.RELU = None
        if a[0] is None:
            assert self.site == len(self.masks), (self.site, len(self.masks))


def _head_only(student, fmap, n_support_frames, labels):
    """the student's head on given trunk outputs (NHWC, support frames first): the trunk is bypassed"""
    from litemkd_amd.model.backbone import strm as S
    real = S.trunk_features
    S.trunk_features = lambda trunk, head, c, t: (torch.cat([head(c), head(t)], 0), c.shape[0])
    try:
        return student(fmap[:n_support_frames], labels, fmap[n_support_frames:])
    finally:
        S.trunk_features = real


@pytest.mark.parametrize("case", [0, 1, 2])
def test_head_matches_the_reference(dev, case):
    """patches in, logits out, eval mode, against the reference's own fp32 CPU outputs: anchored on the fp64 restatement"""
    G = np.load(os.path.join(GOLD, "strm.npz"))
    pre = "c%d_" % case
    seed, way, shot, query = (int(G[pre + k]) for k in ("seed", "way", "shot", "query"))
    backbone = str(G[pre + "backbone"])
    classifier = {0: "strm_res18_sup", 1: "strm_res18", 2: "strmclassifiers"}[case]
    student, args = _student(dev, backbone, classifier, seed, way=way, shot=shot, query_per_class=query)
    student.eval()
    ns = way * shot
    fm = R.make_fmaps(seed, (ns + way * query) * 8)
    labels = torch.arange(way).repeat_interleave(shot)
    fd = fm.to(dev).requires_grad_()
    from litemkd_amd import ops
    ops.STRM_TAPS = taps = {}
    try:
        out = _head_only(student, fd, ns * 8, labels.float().to(dev))["logits"]
    finally:
        ops.STRM_TAPS = None
    bp, cp = R.make_backbone_params(seed, backbone), R.make_classifier_params(seed)
    bp64, cp64 = R.cast(bp, torch.float64), R.cast(cp, torch.float64)
    with torch.no_grad():
        l64, pool64, sel64 = R.head(fm.double(), ns, labels, bp64, cp64, way, shot, backbone=backbone)
    pairs = {}
    for k, v in l64.items():      # forward: against the reference's own fp32 outputs
        pairs[k] = anchored("head logits " + k, out[k], torch.from_numpy(G[pre + "logits_" + k]), v, 3.0, 1e-5)
    # the selections the HIP path made: pooling exactly the natural ones (max is exact); the minimum may differ from fp64's only on rows
    # whose two smallest fp64 distances are within 1e-4 relative of each other
    assert torch.equal(torch.cat([t.cpu().long() for t in taps["pool"]]), pool64)
    sel = taps["dist"][0].cpu().long()
    differ = sel != sel64
    if bool(differ.any()):
        with torch.no_grad():
            f = R.backbone_head(fm.double(), bp64, 8, backbone)[0]["distance"]
            gaps = R.min_gaps(f[:ns], labels, f[ns:], cp64["DistanceLoss.clsW.weight"], cp64["DistanceLoss.clsW.bias"], way)
        assert float(gaps[differ].max()) <= 1e-4, gaps[differ]
    # gradients: both precisions of the restatement on the HIP path's selections and ReLU masks (a pre-activation within rounding of zero
    # flips a mask in ANY fp32 evaluation and moves one video's gradient by 1e-3; tests/test_gpu_episode.py does the same for the trunk)
    masks = [m.cpu() for m in taps["relu"]]
    grads, flips = {}, [0, 0]
    for dt in (torch.float32, torch.float64):
        leaf = fm.detach().to(dt).clone().requires_grad_()
        with _imposed_relu(masks, dt, flips):
            lg = R.head(leaf, ns, labels, R.cast(bp, dt), R.cast(cp, dt), way, shot, backbone=backbone, sel=sel)[0]
        R.fixture_loss(lg).backward()
        grads[dt] = leaf.grad
    R.fixture_loss({k: v.double() for k, v in out.items()}).backward()
    for name, sl in (("g_support", slice(0, ns * 8)), ("g_query", slice(ns * 8, None))):
        pairs[name] = anchored("head " + name, fd.grad[sl], grads[torch.float32][sl], grads[torch.float64][sl], 3.0, 1e-5)
        if flips[0] == 0 and not bool(differ.any()):      # natural masks and selections: the reference's own digests hold as well
            anchored("head digest " + name, R.gsum(fd.grad[sl].cpu()), torch.from_numpy(G[pre + name]), R.gsum(grads[torch.float64][sl]), 3.0, 1e-5)
    print("head case %d: ReLU masks that differ from fp64's: %s, selections: %d" % (case, flips, int(differ.sum())))
    record("strm head vs reference, case %d (%s)" % (case, backbone), pairs)


def _episode(dev, args, seed):
    from litemkd_amd import trainloop as TL
    return TL.SyntheticEpisodes(args, base_seed=seed, device=dev).episode(0)


def _teacher(dev, args):
    from litemkd_amd.model.model_select import Teacher
    torch.manual_seed(17)
    return Teacher(args).to(dev)


def _run_episode(dev, student, teacher, args, ep, distill="strm_fc_2_sup_dist"):
    """one train-mode episode under the caller's RNG state (the dropout seeds are drawn from torch's generator)"""
    from litemkd_amd import trainloop as TL
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.utils import aggregate_accuracy
    cfg = TL._with(args, distill_name=distill)
    student.zero_grad(set_to_none=True)
    loss, acc, _ = TL.train_task(ep, student, teacher, Distiller(distill, cfg.cfg, dev), aggregate_accuracy, cfg)
    torch.cuda.synchronize()
    return loss.clone(), acc.clone(), {k: v.grad.clone() for k, v in student.named_parameters() if v.grad is not None}


@pytest.mark.parametrize("backbone,classifier,distill,teacher", [("strm18_student", "strm_res18_sup", "strm_fc_2_sup_dist", "test_teacher_TRX_2fcsup_fixed")])
def test_episode_runs_are_bit_identical_and_dropout_follows_the_seed(dev, backbone, classifier, distill, teacher):
    """eval-free train-mode episode (dropout 0.1 at five sites): the same seed repeats bit for bit, another seed differs; every parameter
    beyond the unused ones receives a gradient, gamma included"""
    student, args = _student(dev, backbone, classifier, 21, shot=1, query_per_class=1, img_size=64, model_teacher=teacher, distill_name=distill)
    student.train()
    ep = _episode(dev, args, 31)
    bn = {k: v.clone() for k, v in student.state_dict().items() if "running" in k or "num_batches" in k}
    runs = []
    tch = _teacher(dev, args)
    for seed in (5, 5, 6):
        student.load_state_dict(bn, strict=False)
        torch.manual_seed(seed)
        runs.append(_run_episode(dev, student, tch, args, ep, distill))
    assert torch.equal(runs[0][0], runs[1][0])
    assert runs[0][2].keys() == runs[1][2].keys()
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    assert not torch.equal(runs[0][0], runs[2][0])
    got = set(runs[0][2])
    for k, p in student.named_parameters():
        if "norm_v" in k:      # unused by the reference's forward too
            continue
        assert k in got and float(runs[0][2][k].abs().max()) > 0, k
    assert float(runs[0][2]["backbone.attn_pat.gamma"].abs().max()) > 0


def test_one_call_head_equals_two_calls(dev):
    """every new operator is per frame or per video: the head over support and query frames together equals the reference's two calls
    bit for bit (eval mode)"""
    student, args = _student(dev, "strm18_student", "strm_res18_sup", 23, shot=2, query_per_class=1)
    from litemkd_amd import ops
    student.eval()
    b = student.backbone
    fm = R.make_fmaps(5, 15 * 8).to(dev)
    ns = 10 * 8
    with torch.no_grad():
        both = _head_only(student, fm, ns, torch.arange(5).repeat_interleave(2).float().to(dev))

        def alone(x):
            xp = b.attn_pat(ops.PatchPoolFn.apply(x, b.attn_pat.pe.pe[0, :16].contiguous(), None))
            dist = b.res18_2048(ops.PatchMeanFn.apply(xp)).view(-1, 8, 2048)
            fr = b.fr_enrich(dist)
            return dist, b.fc1(fr.view(-1, 2048)).view(-1, 8, 2048), b.fc2(fr.view(-1, 2048)).view(-1, 8, 2048)
        cs, ct = alone(fm[:ns]), alone(fm[ns:])
    for i, k in enumerate(("distance", "trx1", "trx2")):
        assert torch.equal(both["context_features"][k], cs[i]), k
        assert torch.equal(both["target_features"][k], ct[i]), k


def test_strmbackbone_episode_and_accuracy_rule(dev):
    """strmbackbone + strmclassifiers + the `strm` distiller: one train-mode episode end to end; accuracy on 0.1 * pat + fr"""
    from litemkd_amd import trainloop as TL
    student, args = _student(dev, "strmbackbone", "strmclassifiers", 25, shot=1, query_per_class=1, img_size=64, distill_name="strm",
                             model_teacher="test_teacher_TRX_2fcsup_fixed")
    student.train()
    ep = _episode(dev, args, 33)
    loss, acc, grads = _run_episode(dev, student, _teacher(dev, args), args, ep, "strm")
    assert torch.isfinite(loss) and 0.0 <= float(acc) <= 1.0
    assert "backbone.fc1.weight" not in grads or float(grads["backbone.fc1.weight"].abs().max()) == 0.0      # unused, as in the reference
    assert float(grads["backbone.attn_pat.gamma"].abs().max()) > 0
    fr = torch.tensor([[1.0, 1.05], [0.0, 3.0]], device=dev)
    pat = torch.tensor([[1.0, 0.0], [0.0, 0.0]], device=dev)
    lab = torch.tensor([0, 1], device=dev)
    from litemkd_amd.utils import aggregate_accuracy
    assert float(aggregate_accuracy(TL.strm_accuracy_logits("strm", {"pat": pat, "fr": fr}), lab)) == 1.0
    assert float(aggregate_accuracy(fr, lab)) == 0.5


def test_pipelined_episodes_equal_the_sequential_loop(dev):
    """trainloop.PipelinedEpisodes over four STRM episodes (dropout active, an optimizer step in the middle): losses, accuracies, the
    accumulated gradient and the weights are bit-identical to the sequential loop"""
    from litemkd_amd import ops, trainloop as TL
    from litemkd_amd.options import default_args
    cfg = default_args(shot=1, query_per_class=1, img_size=64, trans_dropout=0.1, device=dev, learning_rate=1e-2, model_backbone="strm18_student",
                       model_classifier="strm_res18_sup", distill_name="strm_fc_2_sup_dist")
    src = TL.SyntheticEpisodes(cfg, base_seed=177, device=dev)
    eps = [src.episode(e) for e in range(4)]

    def run(pipelined):
        torch.manual_seed(91)
        student, teacher, _, distiller, accuracy_fn, _, opt, _ = TL.make(cfg)
        with torch.no_grad():
            student.backbone.attn_pat.gamma.fill_(0.3)
        prev = (ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END, ops.DIRECT_PARAM_GRAD)
        ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END, ops.DIRECT_PARAM_GRAD = True, False, True
        out = []
        try:
            torch.manual_seed(5)
            pipe = TL.PipelinedEpisodes(student, teacher, distiller, accuracy_fn, cfg) if pipelined else None
            for i, ep in enumerate(eps):
                if pipelined:
                    r = pipe.push(ep)
                    if r is not None:
                        out.append(r)
                else:
                    loss, acc, _ = TL.train_task(ep, student, teacher, distiller, accuracy_fn, cfg)
                    out.append((loss, acc))
                if i == 1:
                    if pipelined:
                        out.append(pipe.flush())
                    opt.step()
                    opt.zero_grad()
            if pipelined:
                out.append(pipe.flush())
            ops.wait_weight_grads()
            opt.bucket.fold_shadow()
            torch.cuda.synchronize()
        finally:
            ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END, ops.DIRECT_PARAM_GRAD = prev
        return [(float(l), float(a)) for l, a in out], opt.bucket.grad.clone(), opt.bucket.flat.clone()
    o_s, g_s, w_s = run(False)
    o_p, g_p, w_p = run(True)
    assert len(o_p) == len(eps) and o_s == o_p, (o_s, o_p)
    assert torch.equal(w_s, w_p)
    assert torch.equal(g_s, g_p), float((g_s - g_p).abs().max())


def test_graphed_episode_bit_identical_to_eager(dev):
    """trainloop.GraphedEpisode (train.py / bench.py --graph) captures an STRM episode - five dropout seeds in device slots, the class
    plan with its class-sorted order in device memory - and replays it bit-identically to the eager loop (bench.py's arithmetic)"""
    from litemkd_amd import ops, trainloop as TL
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from litemkd_amd.utils import aggregate_accuracy
    ops.set_conv_compute_dtype("fp32h2")
    cfg = default_args(shot=1, query_per_class=1, img_size=64, trans_dropout=0.1, device=dev, learning_rate=1e-2, model_backbone="strm18_student",
                       model_classifier="strm_res18_sup", distill_name="strm_fc_2_sup_dist")
    src = TL.SyntheticEpisodes(cfg, base_seed=77, device=dev)
    pool = [src.episode(e) for e in range(2)]
    order = [0, 1, 0, 1, 0, 1]

    def run(graph):
        torch.manual_seed(91)
        student, teacher = Student(cfg).to(dev), Teacher(cfg).to(dev)
        with torch.no_grad():
            student.backbone.attn_pat.gamma.fill_(0.3)
        opt = TL.FusedOptimizer(student, "sgd", cfg.learning_rate)
        distiller = Distiller(cfg.distill_name, cfg.cfg, dev)
        runner = TL.GraphedEpisode(student, teacher, distiller, aggregate_accuracy, cfg, max_graphs=2) if graph else None
        prev = (ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END, ops.DIRECT_PARAM_GRAD)
        ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END, ops.DIRECT_PARAM_GRAD = True, False, True
        out = []
        try:
            torch.manual_seed(5)
            for i, e in enumerate(order):
                loss, acc, _ = runner(pool[e]) if graph else TL.train_task(pool[e], student, teacher, distiller, aggregate_accuracy, cfg)
                out.append((float(loss), float(acc)))
                if i == 3:
                    opt.step()
                    opt.zero_grad()
            ops.wait_weight_grads()
            opt.bucket.fold_shadow()
            torch.cuda.synchronize()
        finally:
            ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END, ops.DIRECT_PARAM_GRAD = prev
        return out, opt.bucket.grad.clone(), opt.bucket.flat.clone(), runner
    try:
        o_e, g_e, w_e, _ = run(False)
        o_g, g_g, w_g, runner = run(True)
    finally:
        ops.reset_compute_dtypes()
    assert runner.replays == len(order) - 2 and len(runner.graphs) == 2, (runner.replays, runner.eager)
    assert o_e == o_g, (o_e, o_g)
    assert torch.equal(w_e, w_g)
    assert torch.equal(g_e, g_g), float((g_e - g_g).abs().max())
    assert len({l for l, _ in o_e}) > 3


def test_train_loop_checkpoint_and_evaluator(dev, tmp_path):
    """three optimizer steps through trainloop.train change every parameter the forward uses, gamma included; the checkpoint loads into
    load_student and evaluate.Evaluator scores it with the 0.2 * pat + fr1 + fr2 rule"""
    from litemkd_amd import trainloop as TL
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.evaluate import Evaluator
    from litemkd_amd.model.model_select import Student, Teacher, load_student
    from litemkd_amd.options import default_args
    from litemkd_amd.utils import aggregate_accuracy
    cfg = default_args(shot=1, query_per_class=1, img_size=64, device=dev, training_iterations=6, tasks_per_batch=2, learning_rate=1e-2,
                       print_freq=100, model_backbone="strm18_student", model_classifier="strm_res18_sup", distill_name="strm_fc_2_sup_dist",
                       save_dir=str(tmp_path), num_test_tasks=2)
    torch.manual_seed(3)
    student, teacher = Student(cfg).to(dev), Teacher(cfg).to(dev)
    with torch.no_grad():
        student.backbone.attn_pat.gamma.fill_(0.3)
    opt = TL.FusedOptimizer(student, "sgd", cfg.learning_rate)
    sch = TL.MultiStepLR(opt, cfg.sch)
    before = {k: v.detach().clone() for k, v in student.named_parameters()}
    losses, accs = TL.train(student, teacher, TL.SyntheticEpisodes(cfg, base_seed=5, device=dev), Distiller(cfg.distill_name, cfg.cfg, dev), opt, sch,
                            aggregate_accuracy, cfg)
    assert len(losses) == 6 and all(l == l for l in losses) and opt.steps == 3
    for k, v in student.named_parameters():
        if "norm_v" in k:
            continue
        assert not torch.equal(v.detach(), before[k]), k
    assert float(student.backbone.attn_pat.gamma.detach()) != pytest.approx(0.3, abs=0)
    acc = TL.test(student, TL.SyntheticEpisodes(cfg, base_seed=9, device=dev, train=False), aggregate_accuracy, cfg)
    assert 0.0 <= acc[cfg.dataset]["accuracy"] <= 100.0
    path = TL.save_checkpoint(student, 5, cfg)
    ecfg = default_args(**{**vars(cfg), "test_model": "student", "test_model_path": path})
    restored = load_student(ecfg)
    for k, v in student.state_dict().items():
        assert torch.equal(restored.state_dict()[k], v.cpu()), k
    res = Evaluator(ecfg, log=lambda s: None).test()
    assert 0.0 <= res[cfg.dataset]["accuracy"] <= 100.0


def test_train_and_evaluate_command_lines(dev, tmp_path):
    """python -m litemkd_amd.train with the STRM plugin names trains and writes a checkpoint with the reference's keys;
    python -m litemkd_amd.evaluate --distill_name strm_fc_2_sup_dist scores it"""
    import glob
    from litemkd_amd import evaluate as E, train as T
    ck = tmp_path / "ckpt"
    names = ["--model_backbone", "strm18_student", "--model_classifier", "strm_res18_sup", "--distill_name", "strm_fc_2_sup_dist"]
    losses, accs = T.main(names + ["--model_teacher", "test_teacher_TRX_2fcsup_fixed", "--shot", "1", "--query_per_class", "1", "--img_size", "64",
                                   "--tasks_per_batch", "2", "--training_iterations", "4", "--print_freq", "2", "--checkpoint_dir", str(ck),
                                   "--learning_rate", "0.001", "--test_iters", "100"])
    assert len(losses) == 4 and all(np.isfinite(losses))
    files = glob.glob(str(ck / "*.pt"))
    assert len(files) == 1
    sd = torch.load(files[0])["model_state_dict"]
    for k in ("backbone.attn_pat.gamma", "backbone.attn_pat.pe.pe", "backbone.fr_enrich.Tok_MLP.inp_fc.weight", "classifier.DistanceLoss.clsW.weight"):
        assert k in sd, k
    res = E.main(["--test_model", "student", "--test_model_path", files[0], "--num_test_tasks", "2", "--img_size", "64", "--shot", "1"] + names)
    assert 0.0 <= list(res.values())[0]["accuracy"] <= 100.0


def test_bf16_activations_are_refused_on_the_device(dev):
    from litemkd_amd import ops
    student, args = _student(dev, "strm18_student", "strm_res18_sup", 27, shot=1, query_per_class=1, img_size=64)
    ep = _episode(dev, args, 35)
    ops.set_conv_compute_dtype("bf16")
    ops.set_activation_dtype("bf16")
    try:
        with pytest.raises(RuntimeError, match="fp32 activations only"):
            student(ep["support_set"][0], ep["support_labels"][0].to(dev), ep["target_set"][0])
    finally:
        ops.reset_compute_dtypes()
