"""GPU: frame-tuple cardinalities of the temporal cross-transformer.  The tuple kernels with a device table against the
pair kernels they generalise (bit for bit) and against torch; TRX / TRX_fixed heads with temp_set [2, 3] and [3] against fixtures made by
the reference's own modules (tests/golden/trx_card.npz, tools/gen_trx_card_golden.py) at the criteria test_gpu_ops.py::_trx_golden
applies to pairs; the ragged path; one whole training episode with both cardinalities."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

import _trx_card_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    return torch.device("cuda", 0)


def close(a, b, rtol, atol, msg=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    print("%-28s max abs err %.3e (ref max %.3e, atol %.3e)" % (msg, float(err.max()), float(b.abs().max()), atol))
    assert not bad.any(), "%s: %d/%d elements differ, max abs err %.3e (ref max %.3e)" % (
        msg, int(bad.sum()), bad.numel(), float(err.max()), float(b.abs().max()))


def _tuple_inputs(NV, L, card, D, seed):
    g = torch.Generator().manual_seed(seed)
    T = math.comb(L, card)
    t = {"P": torch.randn(NV * L, 2 * card * D, generator=g), "bk": torch.randn(D, generator=g), "bv": torch.randn(D, generator=g),
         "gamma": 1 + 0.1 * torch.randn(D, generator=g), "beta": 0.1 * torch.randn(D, generator=g),
         "dK": torch.randn(NV * T, D, generator=g), "dV": torch.randn(NV * T, D, generator=g)}
    return T, t


def _run_tuples(dev, t, rowmap, NV, L, card, T, D, new):
    """-> Kn, Khat, V, rstd, dP of the pair entry points (new = False) or of the table entry points, outputs pre-filled with NaN"""
    from litemkd_amd import ops
    from litemkd_amd._lib import lib
    d = {k: v.to(dev) for k, v in t.items()}
    rm = torch.tensor(rowmap, dtype=torch.int32, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)      # noqa: E731
    Kn, Khat, V, rstd, dP = nan(NV * T, D), nan(NV * T, D), nan(NV * T, D), nan(NV * T), nan(NV * L, 2 * card * D)
    p, st = ops._p, ops._stream()
    if new:
        tab = ops.trx_tuple_table(L, card, dev)
        assert tab.dtype == torch.int32 and tab.cpu().tolist() == [list(c) for c in itertools.combinations(range(L), card)]
        lib().call("lmkd_trx_tuples_ln_fwd", p(d["P"]), p(d["bk"]), p(d["bv"]), p(d["gamma"]), p(d["beta"]), p(rm), p(tab), p(Kn), p(Khat),
                   p(V), p(rstd), NV, L, card, T, D, ops._f32(1e-5), st)
        lib().call("lmkd_trx_tuples_bwd_gather", p(d["dK"]), p(d["dV"]), p(rm), p(tab), p(dP), NV, L, card, T, D, st)
    else:
        lib().call("lmkd_trx_tuple_ln_fwd", p(d["P"]), p(d["bk"]), p(d["bv"]), p(d["gamma"]), p(d["beta"]), p(rm), p(Kn), p(Khat), p(V),
                   p(rstd), NV, L, D, ops._f32(1e-5), st)
        lib().call("lmkd_trx_tuple_bwd_gather", p(d["dK"]), p(d["dV"]), p(rm), p(dP), NV, L, D, st)
    torch.cuda.synchronize()
    return [x.cpu() for x in (Kn, Khat, V, rstd, dP)]


@pytest.mark.parametrize("D", [96, 1152])      # a row shorter than the 256-thread workgroup; a row with a partial last pass
def test_table_entry_points_equal_the_pair_entry_points(dev, D):
    NV, L, card = 3, 8, 2
    T, t = _tuple_inputs(NV, L, card, D, 7 + D)
    old = _run_tuples(dev, t, [2, 0, 1], NV, L, card, T, D, new=False)
    new = _run_tuples(dev, t, [2, 0, 1], NV, L, card, T, D, new=True)
    for name, a, b in zip(("Kn", "Khat", "V", "rstd", "dP"), old, new):
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("D", [96, 1152])
@pytest.mark.parametrize("L", [3, 4, 8])       # T = 1, 4, 56
def test_triples_kernels_alone(dev, L, D):
    NV, card = 3, 3
    T, t = _tuple_inputs(NV, L, card, D, 100 * L + D)
    assert T == {3: 1, 4: 4, 8: 56}[L]
    rowmap = [1, 2, 0]
    Kn, Khat, V, rstd, dP = _run_tuples(dev, t, rowmap, NV, L, card, T, D, new=True)
    inv = torch.tensor(rowmap).repeat_interleave(T) * T + torch.arange(T).repeat(NV)      # output row of input row n * T + t
    Kn, Khat, V, rstd = Kn[inv], Khat[inv], V[inv], rstd[inv]
    _, _, v32, _ = R.tuples_combine(t["P"], t["bk"], t["bv"], t["gamma"], t["beta"], L, card)
    assert torch.equal(V, v32)                                                           # ((a + b) + c) + bias in fp32, exactly
    d = {k: v.double() for k, v in t.items()}
    kn64, khat64, _, rstd64 = R.tuples_combine(d["P"], d["bk"], d["bv"], d["gamma"], d["beta"], L, card)
    # LayerNorm over at most 1152 fp32 terms: rounding about sqrt(D) * 2^-24 = 2e-6 of the largest value; 1e-5 leaves about 5x
    for name, a, r in (("Kn", Kn, kn64), ("Khat", Khat, khat64), ("rstd", rstd, rstd64)):
        err = float((a.double() - r).abs().max())
        print("L %d D %d %s: max err %.3e of max %.3e" % (L, D, name, err, float(r.abs().max())))
        assert err <= 1e-5 * float(r.abs().max()), name
    # the gather: the transpose of the forward's selection, every output the sum of at most C(7, 2) = 21 terms in ascending tuple order
    assert torch.equal(dP, R.tuples_gather(t["dK"][inv], t["dV"][inv], NV, L, card))      # video n reads rows rowmap[n] * T ..


def test_entry_points_check_their_arguments(dev):
    from litemkd_amd import ops
    from litemkd_amd._lib import lib
    x = torch.zeros(8 * 6 * 32, device=dev)
    tab = ops.trx_tuple_table(8, 3, dev)
    p, st = ops._p, ops._stream()
    for card, L, T, table in ((4, 8, 70, tab), (3, 2, 0, tab), (3, 8, 28, tab), (3, 8, 56, None)):
        with pytest.raises(RuntimeError, match="lmkd_trx_tuples_ln_fwd"):
            lib().call("lmkd_trx_tuples_ln_fwd", p(x), p(x), p(x), p(x), p(x), None, p(table), p(x), None, p(x), None, 1, L, card, T, 32, ops._f32(1e-5), st)
        with pytest.raises(RuntimeError, match="lmkd_trx_tuples_bwd_gather"):
            lib().call("lmkd_trx_tuples_bwd_gather", p(x), p(x), None, p(table), p(x), 1, L, card, T, 32, st)


def _case_args(dev, way, L, ts):
    from litemkd_amd.options import default_args
    return default_args(device=dev, way=way, shot=1, query_per_class=1, seq_len=L, temp_set=ts)


def _load(clf, params, ts):
    sd = clf.state_dict()
    for i, p in enumerate(params):
        pre = "transformers.%d." % i if len(ts) > 1 else "transformers."
        for k, v in p.items():
            sd[pre + k].copy_(v)


@pytest.mark.parametrize("proj", ["gemm", "conv"])
@pytest.mark.parametrize("case", [0, 1, 2])
def test_trx_card_golden(dev, golden_dir, case, proj):
    """TRX (with gradients) and TRX_fixed with the cases' temp_set against the reference's own modules, forward and backward, on both
    projection paths; the criteria of test_gpu_ops.py::_trx_golden: logits rtol 1e-4 / atol 2e-2, input-gradient chunk sums 2e-3 of the
    reference's maximum, parameter gradients 5e-3."""
    from litemkd_amd import ops
    from litemkd_amd.model import classifiers as C
    G = np.load(os.path.join(golden_dir, "trx_card.npz"))
    pre = "c%d_" % case
    way, L, ts, params, sup, lab, qry = R.case_data(case)
    assert np.array_equal(R.gsum(torch.cat([sup.reshape(-1), qry.reshape(-1)])).numpy()[::64], G[pre + "in_digest"])
    args = _case_args(dev, way, L, ts)
    was = ops.TRX_PROJ_ON_CONV
    ops.TRX_PROJ_ON_CONV = proj == "conv"
    try:
        clf = C.TRX(args)
        _load(clf, params, ts)
        clf = clf.to(dev).eval()
        s, q = sup.to(dev).requires_grad_(), qry.to(dev).requires_grad_()
        out = clf(s, lab.to(dev), q)["logits"]
        ref = torch.from_numpy(G[pre + "logits"])
        close(out, ref, 1e-4, 2e-2, "logits")
        if case == 1:
            assert float(out[:, 1].abs().max()) == 0.0
        R.fixture_loss(out).backward()
        fx = C.TRX_fixed(args)
        _load(fx, params, ts)
        close(fx.to(dev).eval()(sup.to(dev), lab.to(dev), qry.to(dev))["logits"], ref, 1e-4, 2e-2, "fixed logits")
        torch.cuda.synchronize()
    finally:
        ops.TRX_PROJ_ON_CONV = was
    for name, x in (("g_support", s), ("g_query", q)):
        r = torch.from_numpy(G[pre + name])
        close(R.gsum(x.grad.cpu()), r, 2e-3, 2e-3 * float(r.abs().max()), name)
    mods = list(clf.transformers) if len(ts) > 1 else [clf.transformers]
    for i, tr in enumerate(mods):
        for name, gt in (("kb", tr.k_linear.bias.grad), ("vb", tr.v_linear.bias.grad), ("nkw", tr.norm_k.weight.grad),
                         ("nkb", tr.norm_k.bias.grad), ("kw_sum", tr.k_linear.weight.grad.sum(1)), ("vw_sum", tr.v_linear.weight.grad.sum(1))):
            r = torch.from_numpy(G[pre + "g%d_%s" % (i, name)])
            # (the v-bias gradient is exactly 0 in exact arithmetic: softmax rows sum to 1 - compare against an absolute floor)
            close(gt, r, 5e-3, 5e-3 * max(float(r.abs().max()), 1e-4), "card %d %s" % (ts[i], name))


def test_triples_ragged_classes(dev):
    """unequal shots per class and a missing class through trx_logits_nograd with cardinality 3, against the fp64 restatement"""
    from litemkd_amd import ops
    way, L, ts, params, sup, lab, qry = R.case_data(1)
    p = params[0]
    ref = R.trx_logits(sup.double(), lab, qry.double(), R.cast(p, torch.float64), way, L, 3)
    plan = ops.ClassPlan(lab.to(dev), way)
    assert plan.counts == [2, 3] and not plan.uniform
    pd = {k: v.to(dev) for k, v in p.items()}
    out = ops.trx_logits_nograd(sup.to(dev), qry.to(dev), plan, pd["k_linear.weight"], pd["k_linear.bias"], pd["v_linear.weight"],
                                pd["v_linear.bias"], pd["norm_k.weight"], pd["norm_k.bias"], pd["pe.pe"][0, :L].contiguous())
    close(out, ref, 1e-4, 2e-2, "ragged triples")
    assert float(out[:, 1].abs().max()) == 0.0


def _episode(dev, temp_set, record=None):
    """one 64-px 5-way 1-shot 1-query training episode in train mode, trans_dropout 0.1 -> (loss, {parameter: gradient}, student)"""
    from litemkd_amd import ops
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.options import default_args
    from oracle import ref_cpu as O
    kw = {} if temp_set is None else {"temp_set": temp_set}
    args = default_args(shot=1, query_per_class=1, img_size=64, trans_dropout=0.1, device=dev, model_backbone="resnet18_2fc",
                        model_classifier="TRX_2fcsup", model_teacher="test_teacher_TRX_2fcsup_fixed", distill_name="fc_2_sup_dist", **kw)
    torch.manual_seed(0)
    student, teacher = Student(args).to(dev).train(), Teacher(args).to(dev).train()
    ep = O.make_episode(321, way=5, shot=1, query=1, img=64)
    real = ops.dropout_mask
    if record is not None:
        def spy(*a, **k):
            m = real(*a, **k)
            record.append(m)
            return m
        ops.dropout_mask = spy
    try:
        torch.manual_seed(1)
        out = student(ep["support_set"].to(dev), ep["support_labels"].to(dev), ep["target_set"].to(dev))
        tl = teacher(ep["support_set_feature_teacher"].to(dev), ep["support_labels"].to(dev), ep["target_set_feature_teacher"].to(dev))["logits"]
        loss = Distiller("fc_2_sup_dist", args.cfg, dev).fc_2_sup_dist(out["logits"], tl, ep["target_labels"].long().to(dev))["loss"]
        loss.backward()
        ops.wait_weight_grads()
        torch.cuda.synchronize()
    finally:
        ops.dropout_mask = real
    return loss.detach().cpu(), {k: (None if v.grad is None else v.grad.detach().cpu().clone()) for k, v in student.named_parameters()}, student


def test_episode_with_pairs_and_triples(dev):
    masks = []
    loss, grads, student = _episode(dev, [2, 3], masks)
    assert torch.isfinite(loss)
    keys = list(grads)
    assert any(k.startswith("classifier.transformers.0.") for k in keys) and any(k.startswith("classifier.transformers.1.") for k in keys)
    assert tuple(student.classifier.transformers[1].k_linear.weight.shape) == (1152, 6144)
    for k, g in grads.items():
        if ".norm_v." in k:      # unused by forward, as in the reference
            continue
        assert g is not None and torch.isfinite(g).all(), k
    for n in ("k_linear.weight", "k_linear.bias", "v_linear.weight", "norm_k.weight", "norm_k.bias"):
        for i in (0, 1):
            assert float(grads["classifier.transformers.%d.%s" % (i, n)].abs().max()) > 0.0, (i, n)
    # student: 2 heads x 2 cardinalities, teacher: 2 cardinalities - six masks, each module's own draw
    assert len(masks) == 6
    host = [m.cpu() for m in masks]
    for a, b in itertools.combinations(range(6), 2):
        assert host[a].shape == host[b].shape and not torch.equal(host[a], host[b]), (a, b)
    for m in host:
        assert 0.05 < float((m == 0).float().mean()) < 0.15


def test_pairs_alone_equal_the_default_construction(dev):
    """temp_set [2] is today's module: loss and every gradient bit-identical to arguments that carry no temp_set at all"""
    from litemkd_amd.options import default_args
    l0, g0, s0 = _episode(dev, None)
    l1, g1, s1 = _episode(dev, [2])
    assert default_args().temp_set == [2] and list(g0) == list(g1)
    assert torch.equal(l0, l1)
    for k in g0:
        assert (g0[k] is None) == (g1[k] is None) and (g0[k] is None or torch.equal(g0[k], g1[k])), k

