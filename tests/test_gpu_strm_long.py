"""GPU: the STRM student family on clips of 9-16 frames - the token-MLP family templated on the clip length against the
fp64 restatement tests/_strm_ref.py (anchored: the HIP error is at most 3 x the error torch's CPU fp32 makes on the same inputs), the
patch-distance head at long clips, the LDS-tiled minimum-distance kernel bit for bit against the one-wave kernel, the whole head against
the reference's own outputs at 12 frames (tests/golden/strm_long.npz), and the episode loop, graph capture, pipelining and the command
lines at seq_len 12."""
import os

import numpy as np
import pytest
import torch

from _anchor import anchored, record
import _strm_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STRM = dict(model_backbone="strm18_student", model_classifier="strm_res18_sup", distill_name="strm_fc_2_sup_dist")


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
# token MLP, 2 <= L <= 16
# ----------------------------------------------------------------------------------------------------------------------------------
TOK_CASES = [(L, V, D, m) for L in (2, 9, 12, 16) for (V, D) in ((1, 2048), (3, 136)) for m in (False, True)] + [(12, 50, 2048, True)]


@pytest.mark.parametrize("L,videos,D,masked", TOK_CASES)
def test_token_mlp_long(dev, L, videos, D, masked):
    """y, dx, dW1, db1, dW2, db2 of the family templated on L.  V = 3, D = 136 is 408 lanes: the second workgroup is partly dead, and
    its dead lanes must add nothing to the parameter sums."""
    from litemkd_amd import ops
    g = torch.Generator().manual_seed(videos * 100 + L)
    p = R.make_backbone_params(8, seq_len=L)
    table = R.pe_table(D, int(1.5 * L))
    mask = _mask((videos * L, D), 4) if masked else None
    names = ["fr_enrich.Tok_MLP.%s.%s" % (m, w) for m in ("inp_fc", "out_fc") for w in ("weight", "bias")]
    assert tuple(p[names[0]].shape) == (L, L)
    inputs = {"x": torch.randn(videos, L, D, generator=g)}
    inputs.update({k: p[k] for k in names})
    dy = torch.randn(videos, L, D, generator=g)
    runs = _two(lambda l: R.token_mlp(R.add_table(l["x"], table, mask), *[l[k] for k in names]), inputs)
    for (o, _), gg in zip(runs, (dy, dy.double())):
        o.backward(gg)
    d = {k: v.to(dev).requires_grad_() for k, v in inputs.items()}
    y = ops.TokenMLPFn.apply(d["x"], table[0, :L].contiguous().to(dev), mask.to(dev) if masked else None, *[d[k] for k in names])
    y.backward(dy.to(dev))
    pairs = {"y": anchored("token MLP y", y, runs[0][0], runs[1][0], 3.0)}
    for k in inputs:
        assert d[k].grad.shape == inputs[k].shape
        _check("token MLP d", d[k].grad, runs, pairs, k)
    record("strm token MLP L=%d V=%d D=%d mask=%s" % (L, videos, D, masked), pairs)


# ----------------------------------------------------------------------------------------------------------------------------------
# patch distance at long clips
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,masked", [(9, False), (9, True), (12, False), (12, True), (16, False), (16, True)])
def test_patch_distance_long(dev, L, masked):
    """the scheme of test_gpu_strm.py::test_patch_distance at 3-way 2-shot, 4 queries per class: the stored arg-min equals fp64's on
    every (row, class) whose two smallest fp64 distances differ by more than 1e-4 relative (at most 2 % of the entries may be left out - a
    property of the inputs: 1.1 - 1.6 % at these seeds, masked or not), then logits and all four gradients on the fp64 selections."""
    from litemkd_amd import ops
    way, shot, query = 3, 2, 4
    ns, nq = way * shot, way * query
    g = torch.Generator().manual_seed(way * 100 + shot)
    cp = R.make_classifier_params(9, seq_len=L)
    perm = torch.randperm(ns, generator=g)
    labels = torch.arange(way).repeat_interleave(shot)[perm]
    mask = _mask(((ns + nq) * L, 2048), 5) if masked else None
    inputs = {"sup": torch.randn(ns, L, 2048, generator=g), "qry": torch.randn(nq, L, 2048, generator=g),
              "w": cp["DistanceLoss.clsW.weight"], "b": cp["DistanceLoss.clsW.bias"]}
    gl = torch.randn(nq, way, generator=g)
    with torch.no_grad():
        free64, sel64 = R.patch_distance(inputs["sup"].double(), labels, inputs["qry"].double(), inputs["w"].double(), inputs["b"].double(), way, mask)
        ms = None if mask is None else (mask[:ns * L].double(), mask[ns * L:].double())
        sup_m = inputs["sup"].double() if ms is None else inputs["sup"].double() * ms[0].reshape(ns, L, -1)
        qry_m = inputs["qry"].double() if ms is None else inputs["qry"].double() * ms[1].reshape(nq, L, -1)
        gaps = R.min_gaps(sup_m, labels, qry_m, inputs["w"].double(), inputs["b"].double(), way)
    plan = ops.ClassPlan(labels.float().to(dev), way, labels.float())
    d = {k: v.to(dev) for k, v in inputs.items()}
    md = mask.to(dev) if masked else None
    X = torch.cat([d["sup"].reshape(-1, 2048), d["qry"].reshape(-1, 2048)], 0)
    Xd = X * md if masked else X
    P, E = ops.strm_patchdist_embed(Xd, d["w"], d["b"], L)
    logits, dist, idx = ops.strm_patchdist_fwd(E, plan, ns, nq, L)
    # the gradients' restatement runs on the HIP path's ReLU mask, as test_head_matches_the_reference does: at 16 frames there are
    # 2160 x 1024 pre-activations, and one of them within fp32 rounding of zero takes a different sign in ANY fp32 evaluation and moves
    # the support gradient by 3e-5 (measured at L = 16 unmasked: 1 sign of 2211840 differs from fp64's, 0 in the five other cases; without
    # the imposed mask the support gradient stood at 3.5e-5 against torch-CPU-fp32's 4.2e-7).  _imposed_relu asserts that the mask
    # differs from fp64's own only where |pre-activation| < 1e-5 max |pre-activation|; selections, bounds and cases are unchanged.
    relu_mask, flips, runs = [(E > 0).cpu()], [0, 0], []
    for dt, gg in ((torch.float32, gl), (torch.float64, gl.double())):
        leaves = {k: v.detach().to(dt).requires_grad_() for k, v in inputs.items()}
        with _imposed_relu(relu_mask, dt, flips):
            o = R.patch_distance(leaves["sup"], labels, leaves["qry"], leaves["w"], leaves["b"], way, mask, sel64)[0]
        o.backward(gg)
        runs.append((o, leaves))
    print("patch distance L=%d: ReLU signs that differ from fp64's: %d of %d" % (L, flips[0], flips[1]))
    clear = gaps > 1e-4
    left_out = 1.0 - float(clear.float().mean())
    print("patch distance L=%d: entries %d, left out %.4f" % (L, clear.numel(), left_out))
    assert left_out <= 0.02, left_out
    assert torch.equal(idx.cpu().long()[clear], sel64[clear]), int((idx.cpu().long() != sel64)[clear].sum())
    with torch.no_grad():
        free32 = R.patch_distance(inputs["sup"], labels, inputs["qry"], inputs["w"], inputs["b"], way, mask)[0]
    pairs = {"logits": anchored("patch distance logits", logits, free32, free64, 3.0)}
    leaf = {k: v.clone().requires_grad_() for k, v in d.items()}
    out = ops.PatchDistFn.apply(leaf["sup"], leaf["qry"], leaf["w"], leaf["b"], md, plan)
    assert torch.equal(out, logits)
    out.backward(gl.to(dev))
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
    if bool((idx.cpu().long() == sel64).all()):
        for k in inputs:
            assert float((leaf[k].grad.reshape(hip[k].shape) - hip[k]).norm() / hip[k].norm()) < 1e-5, k
    record("strm patch distance L=%d 3-way 2-shot 4-query mask=%s" % (L, masked), pairs)


@pytest.mark.parametrize("L", [7, 8, 12, 16])
@pytest.mark.parametrize("way,shot,query", [(3, 2, 4), (2, 1, 1), (3, 3, 1)])
def test_tiled_kernel_equals_plain_kernel(dev, L, way, shot, query):
    """set_patchdist_tiled(0) against (1): dist, idx and logits bit for bit.  (3, 3, 1) has Nq * T = 84 / 198 / 360 rows, no multiple of
    the 16-row query tile, and a last support block that is not full; L = 7 (T = 21) ends a class on a single support row, the kernel's
    odd tail.  Two support rows of every class are copies of earlier ones, and one query row equals a support row, so exact ties and a zero
    distance occur: the first row in (member, t) order must win in both kernels."""
    from litemkd_amd import ops
    ns, nq, T = way * shot, way * query, L * (L - 1) // 2
    g = torch.Generator().manual_seed(1000 * L + 100 * way + 10 * shot + query)
    E = torch.relu(torch.randn((ns + nq) * T, 1024, generator=g))
    Es = E[:ns * T].reshape(ns, T, 1024)
    Es[:, T - 1] = Es[:, 0]      # a tie inside every support video
    if shot > 1:
        Es[1, 2] = Es[0, 2]      # and across two videos (of one class or two, as the permutation has it)
    E[ns * T + 1] = Es[ns - 1, 1]      # distance 0
    perm = torch.randperm(ns, generator=g)
    labels = torch.arange(way).repeat_interleave(shot)[perm].float()
    plan = ops.ClassPlan(labels.to(dev), way, labels)
    Ed = E.to(dev)
    got = {}
    try:
        for mode in (0, 1):
            ops.set_patchdist_tiled(mode)
            got[mode] = ops.strm_patchdist_fwd(Ed, plan, ns, nq, L)
    finally:
        ops.set_patchdist_tiled(-1)
    for a, b, name in zip(got[0], got[1], ("logits", "dist", "idx")):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert float(got[1][1].min()) == 0.0
    auto = ops.strm_patchdist_fwd(Ed, plan, ns, nq, L)
    assert all(torch.equal(a, b) for a, b in zip(auto, got[0]))


# ----------------------------------------------------------------------------------------------------------------------------------
# whole head and whole students at 12 frames
# ----------------------------------------------------------------------------------------------------------------------------------
SEQ = 12


def _student(dev, backbone, classifier, seed, **kw):
    """Student with the seeded head parameters of tests/_strm_ref.py at 12 frames (the trunk keeps its own initialisation)"""
    from litemkd_amd.model.model_select import Student
    from litemkd_amd.options import default_args
    args = default_args(model_backbone=backbone, model_classifier=classifier, device=dev, seq_len=SEQ, **kw)
    torch.manual_seed(seed)
    s = Student(args)
    sd = {"backbone." + k: v for k, v in R.make_backbone_params(seed, backbone, seq_len=SEQ).items()}
    sd.update({"classifier." + k: v for k, v in R.make_classifier_params(seed, seq_len=SEQ).items()})
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
def test_head_matches_the_reference_at_12_frames(dev, case):
    """patches in, logits out, eval mode, against the reference's own fp32 CPU outputs at seq_len 12: anchored on the fp64 restatement"""
    from litemkd_amd import ops
    G = np.load(os.path.join(GOLD, "strm_long.npz"))
    assert int(G["seq_len"]) == SEQ
    pre = "c%d_" % case
    seed, way, shot, query = (int(G[pre + k]) for k in ("seed", "way", "shot", "query"))
    backbone = str(G[pre + "backbone"])
    classifier = {0: "strm_res18_sup", 1: "strm_res18", 2: "strmclassifiers"}[case]
    student, args = _student(dev, backbone, classifier, seed, way=way, shot=shot, query_per_class=query)
    student.eval()
    ns = way * shot
    fm = R.make_fmaps(seed, (ns + way * query) * SEQ)
    np.testing.assert_allclose(R.gsum(fm).numpy()[::64], G[pre + "in_digest"], rtol=1e-6, atol=1e-6,
                               err_msg="the seeded inputs differ from the generator's: regenerate the fixture")
    labels = torch.arange(way).repeat_interleave(shot)
    fd = fm.to(dev).requires_grad_()
    ops.STRM_TAPS = taps = {}
    try:
        out = _head_only(student, fd, ns * SEQ, labels.float().to(dev))["logits"]
    finally:
        ops.STRM_TAPS = None
    bp, cp = R.make_backbone_params(seed, backbone, seq_len=SEQ), R.make_classifier_params(seed, seq_len=SEQ)
    bp64, cp64 = R.cast(bp, torch.float64), R.cast(cp, torch.float64)
    with torch.no_grad():
        l64, pool64, sel64 = R.head(fm.double(), ns, labels, bp64, cp64, way, shot, seq_len=SEQ, backbone=backbone)
    pairs = {}
    assert sorted(l64) == sorted(k[len(pre) + 7:] for k in G.files if k.startswith(pre + "logits_"))
    for k, v in l64.items():      # forward: against the reference's own fp32 outputs
        pairs[k] = anchored("head logits " + k, out[k], torch.from_numpy(G[pre + "logits_" + k]), v, 3.0, 1e-5)
    assert torch.equal(torch.cat([t.cpu().long() for t in taps["pool"]]), pool64)
    sel = taps["dist"][0].cpu().long()
    differ = sel != sel64
    if bool(differ.any()):
        with torch.no_grad():
            f = R.backbone_head(fm.double(), bp64, SEQ, backbone)[0]["distance"]
            gaps = R.min_gaps(f[:ns], labels, f[ns:], cp64["DistanceLoss.clsW.weight"], cp64["DistanceLoss.clsW.bias"], way)
        assert float(gaps[differ].max()) <= 1e-4, gaps[differ]
    masks = [m.cpu() for m in taps["relu"]]
    grads, flips = {}, [0, 0]
    for dt in (torch.float32, torch.float64):
        leaf = fm.detach().to(dt).clone().requires_grad_()
        with _imposed_relu(masks, dt, flips):
            lg = R.head(leaf, ns, labels, R.cast(bp, dt), R.cast(cp, dt), way, shot, seq_len=SEQ, backbone=backbone, sel=sel)[0]
        R.fixture_loss(lg).backward()
        grads[dt] = leaf.grad
    R.fixture_loss({k: v.double() for k, v in out.items()}).backward()
    for name, sl in (("g_support", slice(0, ns * SEQ)), ("g_query", slice(ns * SEQ, None))):
        pairs[name] = anchored("head " + name, fd.grad[sl], grads[torch.float32][sl], grads[torch.float64][sl], 3.0, 1e-5)
        if flips[0] == 0 and not bool(differ.any()):      # natural masks and selections: the reference's own digests hold as well
            anchored("head digest " + name, R.gsum(fd.grad[sl].cpu()), torch.from_numpy(G[pre + name]), R.gsum(grads[torch.float64][sl]), 3.0, 1e-5)
    print("head case %d at %d frames: ReLU masks that differ from fp64's: %s, selections: %d" % (case, SEQ, flips, int(differ.sum())))
    record("strm head vs reference at %d frames, case %d (%s)" % (SEQ, case, backbone), pairs)


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


def test_episode_runs_are_bit_identical_and_dropout_follows_the_seed_at_12_frames(dev):
    from litemkd_amd import trainloop as TL
    from litemkd_amd.model.model_select import Teacher
    student, args = _student(dev, "strm18_student", "strm_res18_sup", 21, shot=1, query_per_class=1, img_size=64,
                             model_teacher="test_teacher_TRX_2fcsup_fixed", distill_name="strm_fc_2_sup_dist")
    student.train()
    ep = TL.SyntheticEpisodes(args, base_seed=31, device=dev).episode(0)
    assert ep["support_set"][0].shape[0] == 5 * SEQ
    bn = {k: v.clone() for k, v in student.state_dict().items() if "running" in k or "num_batches" in k}
    torch.manual_seed(17)
    tch = Teacher(args).to(dev)
    runs = []
    for seed in (5, 5, 6):
        student.load_state_dict(bn, strict=False)
        torch.manual_seed(seed)
        runs.append(_run_episode(dev, student, tch, args, ep))
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
    assert tuple(runs[0][2]["backbone.fr_enrich.Tok_MLP.inp_fc.weight"].shape) == (SEQ, SEQ)


def _loop_cfg(dev):
    from litemkd_amd.options import default_args
    return default_args(shot=1, query_per_class=1, img_size=64, trans_dropout=0.1, device=dev, learning_rate=1e-2, seq_len=SEQ, **STRM)


class _side_wgrad:
    def __enter__(self):
        from litemkd_amd import ops
        self.prev = (ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END, ops.DIRECT_PARAM_GRAD)
        ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END, ops.DIRECT_PARAM_GRAD = True, False, True

    def __exit__(self, *a):
        from litemkd_amd import ops
        ops.SIDE_WGRAD, ops.SYNC_WGRAD_AT_BACKWARD_END, ops.DIRECT_PARAM_GRAD = self.prev


def test_pipelined_episodes_equal_the_sequential_loop_at_12_frames(dev):
    """trainloop.PipelinedEpisodes over three 12-frame STRM episodes (dropout active, an optimizer step in the middle): losses,
    accuracies, the accumulated gradient and the weights are bit-identical to the sequential loop"""
    from litemkd_amd import ops, trainloop as TL
    cfg = _loop_cfg(dev)
    src = TL.SyntheticEpisodes(cfg, base_seed=177, device=dev)
    eps = [src.episode(e) for e in range(3)]

    def run(pipelined):
        torch.manual_seed(91)
        student, teacher, _, distiller, accuracy_fn, _, opt, _ = TL.make(cfg)
        with torch.no_grad():
            student.backbone.attn_pat.gamma.fill_(0.3)
        out = []
        with _side_wgrad():
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
        return [(float(l), float(a)) for l, a in out], opt.bucket.grad.clone(), opt.bucket.flat.clone()
    o_s, g_s, w_s = run(False)
    o_p, g_p, w_p = run(True)
    assert len(o_p) == len(eps) and o_s == o_p, (o_s, o_p)
    assert torch.equal(w_s, w_p)
    assert torch.equal(g_s, g_p), float((g_s - g_p).abs().max())


def test_graphed_episode_bit_identical_to_eager_at_12_frames(dev):
    """trainloop.GraphedEpisode captures a 12-frame STRM episode and replays it bit-identically to the eager loop"""
    from litemkd_amd import ops, trainloop as TL
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.utils import aggregate_accuracy
    ops.set_conv_compute_dtype("fp32h2")
    cfg = _loop_cfg(dev)
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
        out = []
        with _side_wgrad():
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


@pytest.mark.parametrize("backbone,classifier,distill,teacher", [
    ("strm18_student", "strm_res18_sup", "strm_fc_2_sup_dist", "test_teacher_TRX_2fcsup_fixed"),
    ("strmbackbone", "strmclassifiers", "strm", "test_teacher_TRX_2fcsup_fixed"),
    ("strmbackbone", "strm_res18", "strm_KD", "test_teacher_otam")])      # strm_KD distils from one logit tensor, not from a dict of heads
def test_train_and_evaluate_command_lines_at_12_frames(dev, tmp_path, backbone, classifier, distill, teacher):
    """python -m litemkd_amd.train --seq_len 12 with the STRM plugin names trains 4 iterations and writes a checkpoint whose token MLP is
    12 x 12 and whose positional tables have 18 rows; python -m litemkd_amd.evaluate --seq_len 12 scores it on 2 tasks"""
    import glob
    from litemkd_amd import evaluate as E, train as T
    ck = tmp_path / "ckpt"
    names = ["--model_backbone", backbone, "--model_classifier", classifier, "--distill_name", distill, "--seq_len", str(SEQ)]
    losses, accs = T.main(names + ["--model_teacher", teacher, "--shot", "1", "--query_per_class", "1", "--img_size", "64",
                                   "--tasks_per_batch", "2", "--training_iterations", "4", "--print_freq", "2", "--checkpoint_dir", str(ck),
                                   "--learning_rate", "0.001", "--test_iters", "100"])
    assert len(losses) == 4 and all(np.isfinite(losses))
    files = glob.glob(str(ck / "*.pt"))
    assert len(files) == 1
    sd = torch.load(files[0])["model_state_dict"]
    assert tuple(sd["backbone.fr_enrich.Tok_MLP.inp_fc.weight"].shape) == (SEQ, SEQ)
    assert tuple(sd["backbone.fr_enrich.pe.pe"].shape) == (1, 18, 2048) and tuple(sd["classifier.transformers.pe.pe"].shape) == (1, 18, 2048)
    res = E.main(["--test_model", "student", "--test_model_path", files[0], "--num_test_tasks", "2", "--img_size", "64", "--shot", "1"] + names)
    assert 0.0 <= list(res.values())[0]["accuracy"] <= 100.0


def test_seventeen_frames_are_refused_with_the_limit(dev):
    from litemkd_amd import ops
    x = torch.zeros(1, 17, 256, device=dev)
    w = torch.zeros(17, 17, device=dev)
    b = torch.zeros(17, device=dev)
    with pytest.raises(RuntimeError, match=r"2 <= L <= 16.*got 17"):
        ops.strm_tokmlp_fwd(x, torch.zeros(17, 256, device=dev), None, w, b, w, b)
