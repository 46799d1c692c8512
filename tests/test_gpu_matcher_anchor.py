"""GPU: the matcher heads (csrc/trx.hip behind ops.TRXLogitsFn / TRXSupFn / EDistFn / SupportDKFn) held to an fp64 evaluation of
tests/_matcher_ref.py, element by element, forward and backward, on the class layouts whose backward nothing else runs: unequal shots
(the per-class GEMM loop), classes without support, the padded layout of ops._trx_class_slots (4, 5 or 6 frames), both together, sixteen
segments, a softmax segment longer than the workgroup.  Then the kernels of the heads alone through the C ABI, at their limits.

Widths are reduced (128 -> 96: a row shorter than the 256-thread workgroup; one case at 288: a partial second pass), so a case costs
milliseconds and an fp64 reference is affordable per element.

Two criteria for every output and every gradient, both relative to what torch's CPU fp32 evaluation of the SAME reference does on the
same inputs (nothing here is derived from what the kernels give):
  1. _anchor.anchored / anchored_dict: relative L2 against fp64 at most 3 x the CPU-fp32 one + 2e-6;
  2. per element: max |hip - ref64| <= 3 x max |cpu32 - ref64| + 1e-5 x max |ref64| (the per-element fp32 bound of
     test_gpu_trx_card.py::test_triples_kernels_alone).  A tensor whose exact gradient is 0 (v_linear.bias: every softmax row sums to 1;
     fp64 leaves 1e-16 of it) is judged against 1e-5 x the largest gradient of its set.
Every measured pair is appended to $LMKD_PARITY_LOG (profiles/matcher_anchor_parity_errors.txt is such a run)."""
import math

import pytest
import torch

import _anchor as A
import _matcher_ref as M
import _trx_card_ref as R

pytestmark = pytest.mark.gpu

DIN = 128
GRAD_KEYS = ("k_linear.weight", "k_linear.bias", "v_linear.weight", "v_linear.bias", "norm_k.weight", "norm_k.bias")

# name -> (seed, way, support labels, shuffle them, queries, frames, cardinality)
LAYOUTS = {
    "a": (61, 3, [0, 0, 1, 1, 2, 2], True, 4, 8, 2),          # uniform: the batched GEMMs
    "b": (62, 4, [2, 0, 0, 2, 2], False, 2, 8, 3),            # ragged, classes 1 and 3 absent, nothing padded (T = 56)
    "c": (63, 3, [0, 1, 2], False, 3, 4, 2),                  # uniform and padded: T = 6, one shot takes two video positions
    "d": (64, 4, [0, 1, 1, 2, 2, 2], False, 3, 4, 2),         # ragged and padded: positions 2 / 2 / 4, class 3 absent
    "e": (65, 3, [1, 0, 2, 0, 1, 0, 0], False, 2, 6, 2),      # T = 15: counts 4 / 2 / 1 all take 4 positions; labels interleaved
    "f": (66, 16, list(range(16)), False, 2, 4, 3),           # LMKD_MAX_SEG segments, T = 4
    "g": (67, 2, [0] * 10 + [1], False, 1, 8, 2),             # a 280-column softmax segment (> 256 threads) beside a 28-column one
}
SLOTS = {"a": [2, 2, 2], "b": [2, 3], "c": [2, 2, 2], "d": [2, 2, 4], "e": [4, 4, 4], "f": [1] * 16, "g": [10, 1]}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    return torch.device("cuda", 0)


# ---- the two criteria ----
def _per_element(name, hip, cpu32, ref64, scale=None):
    r = ref64.detach().double()
    top = float(r.abs().max()) if scale is None else scale
    e_hip = float((hip.detach().cpu().double() - r).abs().max())
    e_cpu = float((cpu32.detach().double() - r).abs().max())
    print("%-40s per element: hip %.3e cpu %.3e of %.3e" % (name, e_hip, e_cpu, top))
    assert e_hip <= 3.0 * e_cpu + 1e-5 * top, "%s: max |hip - fp64| %.3e > 3 x max |cpu32 - fp64| %.3e + 1e-5 x %.3e" % (name, e_hip, e_cpu, top)


def _both(name, hip, cpu32, ref64):
    """one tensor against both criteria -> (rel-L2 hip, rel-L2 cpu)"""
    assert hip.shape == ref64.shape, (name, hip.shape, ref64.shape)
    assert torch.isfinite(hip).all(), name
    pair = A.anchored(name, hip, cpu32, ref64)
    _per_element(name, hip, cpu32, ref64)
    return pair


def _both_dict(name, hip, cpu32, ref64):
    """a set of gradients against both criteria -> {key: (rel-L2 hip, rel-L2 cpu)} (on anchored_dict's scale)"""
    for k in ref64:
        assert hip[k] is not None and hip[k].shape == ref64[k].shape and torch.isfinite(hip[k]).all(), (name, k)
    A.anchored_dict(hip, cpu32, ref64)
    gmax = max(float(v.abs().max()) for v in ref64.values())
    pairs = {}
    for k, r in ref64.items():
        zero = float(r.abs().max()) <= 1e-10 * gmax      # exactly 0 in exact arithmetic
        _per_element("%s %s" % (name, k), hip[k], cpu32[k], r, gmax if zero else None)
        add = 1e-7 * gmax * math.sqrt(max(1, r.numel()))
        pairs[k] = (A.rel_l2(hip[k], r, add), A.rel_l2(cpu32[k], r, add))
    return pairs


# ---- whole TRX heads ----
_DATA, _REF = {}, {}


def _data(name, D=96, masked=False):
    """seeded parameters, inputs, loss weights (and a dropout-style mask) of a layout; made once, never changed"""
    key = (name, D, masked)
    if key not in _DATA:
        seed, way, labels, shuffle, nq, L, card = LAYOUTS[name]
        p = R.make_params(seed, card, L, out_dim=D, in_dim=DIN)
        sup, lab, qry = R.make_inputs(seed, labels, nq, L, shuffle, in_dim=DIN)
        g = torch.Generator().manual_seed(seed + 9000)
        d = {"way": way, "L": L, "card": card, "p": p, "sup": sup, "lab": lab, "qry": qry, "w": torch.randn(nq, way, generator=g),
             "w2": torch.randn(nq, way, way, generator=g), "mask": None,
             "absent": [c for c in range(way) if c not in labels]}
        if masked:      # entries 0 or 1 / (1 - p), p = 0.1, drawn on the host
            d["mask"] = (torch.rand(len(labels) + nq, L, DIN, generator=g) >= 0.1).float() / 0.9
        _DATA[key] = d
    return _DATA[key]


def _ref_run(d, dtype, with_sim, w=None, w2=None):
    p = R.cast(d["p"], dtype)
    leaf = {k: p[k].clone().requires_grad_() for k in GRAD_KEYS}
    p.update(leaf)
    s, q = d["sup"].to(dtype).clone().requires_grad_(), d["qry"].to(dtype).clone().requires_grad_()
    logits, sim = M.trx(s, d["lab"], q, p, d["way"], d["L"], d["card"], d["mask"])
    loss = (logits * (d["w"] if w is None else w).to(dtype)).sum()
    if with_sim:
        loss = loss + (sim * (d["w2"] if w2 is None else w2).to(dtype)).sum()
    loss.backward()
    grads = {"support": s.grad, "queries": q.grad}
    grads.update({k: v.grad for k, v in leaf.items()})
    return {"logits": logits.detach(), "sim": sim.detach(), "grads": grads}


def _ref(name, D, masked, with_sim):
    """(CPU fp32, fp64) evaluations of tests/_matcher_ref.trx and its gradients: computed once, shared by both GEMM modes"""
    key = (name, D, masked, with_sim)
    if key not in _REF:
        d = _data(name, D, masked)
        _REF[key] = (_ref_run(d, torch.float32, with_sim), _ref_run(d, torch.float64, with_sim))
    return _REF[key]


def _hip_run(dev, d, mode, with_sim, w=None, w2=None):
    import litemkd_amd
    from litemkd_amd import ops
    p = {k: v.to(dev) for k, v in d["p"].items()}
    leaf = {k: p[k].clone().requires_grad_() for k in GRAD_KEYS}
    s, q = d["sup"].to(dev).requires_grad_(), d["qry"].to(dev).requires_grad_()
    plan = ops.ClassPlan(d["lab"].to(dev), d["way"], cpu_copy=d["lab"])
    pe = p["pe.pe"][0, :d["L"]].contiguous()
    mask = None if d["mask"] is None else d["mask"].reshape(-1, DIN).contiguous().to(dev)
    args = (s, q, leaf["k_linear.weight"], leaf["k_linear.bias"], leaf["v_linear.weight"], leaf["v_linear.bias"], leaf["norm_k.weight"],
            leaf["norm_k.bias"], pe, mask, plan)
    lib = litemkd_amd.lib()
    lib.call("lmkd_gemm_set_mode", mode)
    try:
        if with_sim:
            logits, sim = ops.TRXSupFn.apply(*args)
            loss = (logits * (d["w"] if w is None else w).to(dev)).sum() + (sim * (d["w2"] if w2 is None else w2).to(dev)).sum()
        else:
            logits, sim = ops.TRXLogitsFn.apply(*args), None
            loss = (logits * (d["w"] if w is None else w).to(dev)).sum()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        lib.call("lmkd_gemm_set_mode", -1)
    grads = {"support": s.grad.cpu(), "queries": q.grad.cpu()}
    grads.update({k: (None if v.grad is None else v.grad.cpu()) for k, v in leaf.items()})
    return {"logits": logits.detach().cpu(), "sim": None if sim is None else sim.detach().cpu(), "grads": grads, "plan": plan}


def _check_head(dev, name, D, mode, with_sim, masked=False):
    from litemkd_amd import ops
    d = _data(name, D, masked)
    T = math.comb(d["L"], d["card"])
    cpu32, ref64 = _ref(name, D, masked, with_sim)
    hip = _hip_run(dev, d, mode, with_sim)
    if D == 96:      # the layout the case is here for
        assert ops._trx_class_slots(hip["plan"].counts, T) == SLOTS[name]
    tag = "%s %s D %d mode %d%s" % ("trx_sup" if with_sim else "trx", name, D, mode, " masked" if masked else "")
    pairs = {"logits": _both(tag + " logits", hip["logits"], cpu32["logits"], ref64["logits"])}
    if with_sim:
        pairs["sim"] = _both(tag + " sim", hip["sim"], cpu32["sim"], ref64["sim"])
    pairs.update(_both_dict(tag, hip["grads"], cpu32["grads"], ref64["grads"]))
    A.record(tag, pairs)
    for c in d["absent"]:      # exactly 0, not merely small
        assert float(hip["logits"][:, c].abs().max()) == 0.0, c
        if with_sim:
            assert float(hip["sim"][:, c, :].abs().max()) == 0.0 and float(hip["sim"][:, :, c].abs().max()) == 0.0, c
    if d["absent"]:      # and nothing of the loss at an absent class reaches any gradient: the same bits with other weights there
        g = torch.Generator().manual_seed(77)
        w, w2 = d["w"].clone(), d["w2"].clone()
        for c in d["absent"]:
            w[:, c] = torch.randn(w.shape[0], generator=g) * 10
            w2[:, c, :] = torch.randn(w2.shape[0], w2.shape[2], generator=g) * 10
            w2[:, :, c] = torch.randn(w2.shape[0], w2.shape[1], generator=g) * 10
        again = _hip_run(dev, d, mode, with_sim, w, w2)
        assert torch.equal(hip["logits"], again["logits"])
        for k, v in hip["grads"].items():
            assert torch.equal(v, again["grads"][k]), k
    return hip


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,D", [("a", 96), ("a", 288), ("b", 96), ("c", 96), ("d", 96), ("e", 96), ("f", 96), ("g", 96)])
def test_trx_logits_head(dev, name, D, mode):
    """TRXLogitsFn on every layout, logits and all eight gradients per element, under lmkd_gemm_set_mode 0 (every product on the fp32 MFMA
    kernel) and 1 (the three-plane kernel - for the products with M * N * K >= 2^18 only: at these sizes the projections and their
    gradients in every case, the score product and its gradients in (a), (b), (e), (g), the prototype products in (a), (b), (g); the
    rest stays on the fp32 kernel in both modes)."""
    _check_head(dev, name, D, mode, False)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["a", "b", "d", "e"])
def test_trx_sup_head(dev, name, mode):
    """TRXSupFn (way <= TRXS_MAXW): the loss reads the logits and the prototype similarities, so the similarity's backward kernel feeds
    every gradient; the similarity rows and columns of absent classes are exactly 0"""
    _check_head(dev, name, 96, mode, True)


@pytest.mark.parametrize("with_sim", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
def test_trx_heads_through_a_dropout_mask(dev, mode, with_sim):
    """layout (d) with an explicit mask of 0 / (1 / 0.9) entries: lmkd_add_pe's mask branch forward, lmkd_mul on the input gradient"""
    hip = _check_head(dev, "d", 96, mode, with_sim, masked=True)
    d0, d1 = _ref("d", 96, False, with_sim)[1], _ref("d", 96, True, with_sim)[1]
    assert not torch.equal(d0["logits"], d1["logits"])      # the mask does change the case
    m = _data("d", 96, True)["mask"]
    assert 0.05 < float((m == 0).float().mean()) < 0.15
    for g in (d1["grads"], hip["grads"]):                   # a dropped input entry has no gradient, exactly
        assert float(g["support"][m[:6] == 0].abs().max()) == 0.0 and float(g["queries"][m[6:] == 0].abs().max()) == 0.0


def test_seventeen_classes_are_refused(dev):
    """one class more than LMKD_MAX_SEG: a RuntimeError that names the segment limit, raised by the forward before any result exists"""
    from litemkd_amd import ops
    L, card, way = 4, 3, 17
    p = {k: v.to(dev) for k, v in R.make_params(68, card, L, out_dim=96, in_dim=DIN).items()}
    sup, lab, qry = R.make_inputs(68, list(range(way)), 1, L, False, in_dim=DIN)
    plan = ops.ClassPlan(lab.to(dev), way, cpu_copy=lab)
    with pytest.raises(RuntimeError, match=r"1\.\.16 segments"):
        ops.TRXLogitsFn.apply(sup.to(dev), qry.to(dev), p["k_linear.weight"], p["k_linear.bias"], p["v_linear.weight"], p["v_linear.bias"],
                              p["norm_k.weight"], p["norm_k.bias"], p["pe.pe"][0, :L].contiguous(), None, plan)
    torch.cuda.synchronize()


# ---- the Euclidean matcher and the support prototype distances ----
def _grad_run(fn, tensors, w):
    """fn(*leaves) -> out; loss (out * w).sum() -> (out, [gradients]) on the CPU"""
    leaves = [t.clone().requires_grad_() for t in tensors]
    out = fn(*leaves)
    (out * w.to(out)).sum().backward()
    if out.is_cuda:
        torch.cuda.synchronize()
    return out.detach().cpu(), [t.grad.cpu() for t in leaves]


@pytest.mark.parametrize("nq,labels,way", [(7, [2, 0, 2], 4), (2, [5, 5, 1, 1, 1, 19, 0, 0, 5], 20)])
def test_edist_head(dev, nq, labels, way):
    """EDistFn with more query than support rows and the reverse (both row kinds of edist_bwd_kernel's max(Nq, Ns) grid run with idle
    rows), absent classes, more than 16 ways, 3 frames of 100 features, and one coincident pair: queries[0] is support[1], the distance
    is exactly 0 and adds nothing to either gradient (the subgradient the kernel and torch.cdist both state)"""
    from litemkd_amd import ops
    ns, L, D = len(labels), 3, 100
    g = torch.Generator().manual_seed(500 + nq)
    sup, qry = torch.randn(ns, L, D, generator=g), torch.randn(nq, L, D, generator=g)
    qry[0] = sup[1]
    lab = torch.tensor(labels, dtype=torch.float32)
    w = torch.randn(nq, way, generator=g)
    ref = lambda s, q: M.e_dist(s, lab, q, way)      # noqa: E731
    o32, g32 = _grad_run(ref, (sup, qry), w)
    o64, g64 = _grad_run(ref, (sup.double(), qry.double()), w)
    plan = ops.ClassPlan(lab.to(dev), way, cpu_copy=lab)
    out, gh = _grad_run(lambda s, q: ops.EDistFn.apply(s, q, plan), (sup.to(dev), qry.to(dev)), w)
    tag = "edist Nq %d Ns %d way %d" % (nq, ns, way)
    pairs = {"logits": _both(tag + " logits", out, o32, o64)}
    pairs.update(_both_dict(tag, dict(zip(("support", "queries"), gh)), dict(zip(("support", "queries"), g32)), dict(zip(("support", "queries"), g64))))
    A.record(tag, pairs)
    for c in range(way):
        if c not in labels:
            assert float(out[:, c].abs().max()) == 0.0, c
    # the coincident pair alone: support video 1's gradient without query 0 is what the other queries give it
    others = [i for i in range(nq) if i != 0]
    if labels.count(labels[1]) == 1 and others:      # (class of its own: its column is minus the distance itself)
        sm, qm = sup.double().mean(1), qry.double().mean(1)
        want = sum(w[i, labels[1]].double() * (qm[i] - sm[1]) / (qm[i] - sm[1]).norm() for i in others) / L
        assert float((gh[0][1].double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("way,shot,L,D", [(5, 3, 4, 100), (7, 2, 3, 260)])
def test_supportdk_head(dev, way, shot, L, D):
    """SupportDKFn: way 5 takes the compile-time instance of supportdk_partial_kernel, way 7 the run-time one; L * D = 400 and 780
    elements: two and four workgroups, the last one partly idle"""
    from litemkd_amd import ops
    g = torch.Generator().manual_seed(600 + way)
    sup = torch.randn(way * shot, L, D, generator=g)
    w = torch.randn(way, way - 1, generator=g)
    ref = lambda s: M.support_dk(s, way, shot)      # noqa: E731
    o32, g32 = _grad_run(ref, (sup,), w)
    o64, g64 = _grad_run(ref, (sup.double(),), w)
    out, gh = _grad_run(lambda s: ops.SupportDKFn.apply(s, way, shot), (sup.to(dev),), w)
    tag = "supportdk way %d shot %d L %d D %d" % (way, shot, L, D)
    pairs = {"out": _both(tag + " out", out, o32, o64), "support": _both(tag + " support", gh[0], g32[0], g64[0])}
    A.record(tag, pairs)


# ---- the kernels alone, through the C ABI; every output is the test's own tensor, pre-filled with NaN or a sentinel ----
SENTINEL = -7777.0


def _softmax_case():
    """3 rows of pitch 304, segments [0, 5) [8, 288) [300, 301), sentinels between them.  Scores spread over +-60 (exp overflows without
    the subtraction of the maximum); row 1's long segment is one constant; row 2 holds its largest scores past the segment's first 256 columns,
    which only a lane's second pass reaches."""
    g = torch.Generator().manual_seed(701)
    off, cnt, ld = [0, 8, 300], [5, 280, 1], 304
    S = torch.full((3, ld), SENTINEL)
    for o, c in zip(off, cnt):
        S[:, o:o + c] = (torch.rand(3, c, generator=g) * 2 - 1) * 60
    S[1, 8:288] = 41.5
    S[2, 8 + 256:288] += 30
    dP = torch.full((3, ld), SENTINEL)
    for o, c in zip(off, cnt):
        dP[:, o:o + c] = torch.randn(3, c, generator=g)
    return S, dP, off, cnt, ld


def test_segment_softmax_alone(dev):
    from litemkd_amd import ops
    from litemkd_amd._lib import lib
    S, dP, off, cnt, ld = _softmax_case()
    p, st = ops._p, ops._stream()
    Sd = S.to(dev)
    lib().call("lmkd_segment_softmax_fwd", p(Sd), 3, ld, 3, ops._ints(off), ops._ints(cnt), st)
    torch.cuda.synchronize()
    P = Sd.cpu()
    inside = torch.zeros(ld, dtype=torch.bool)
    pairs = {}
    for i, (o, c) in enumerate(zip(off, cnt)):
        inside[o:o + c] = True
        pairs["fwd seg %d" % i] = _both("softmax fwd segment %d" % i, P[:, o:o + c], torch.softmax(S[:, o:o + c], -1),
                                        torch.softmax(S[:, o:o + c].double(), -1))
    assert torch.equal(P[:, ~inside], S[:, ~inside])                       # the gaps: bit-unchanged
    assert torch.equal(P[:, 300], torch.ones(3))                           # one column: exactly 1
    assert float((P[1, 8:288].double() - 1 / 280).abs().max()) <= 1e-9      # the constant segment: 1 / 280 to fp32 rounding of it
    # backward on the probabilities the forward left, against P * (dP - sum(P * dP)) in fp64 of the same fp32 inputs
    dd = dP.to(dev)
    lib().call("lmkd_segment_softmax_bwd", p(Sd), p(dd), 3, ld, 3, ops._ints(off), ops._ints(cnt), st)
    torch.cuda.synchronize()
    dS = dd.cpu()
    assert torch.equal(Sd.cpu(), P)
    for i, (o, c) in enumerate(zip(off, cnt)):
        pr, dr = P[:, o:o + c], dP[:, o:o + c]
        f = lambda a, b: a * (b - (a * b).sum(-1, keepdim=True))      # noqa: E731
        if c == 1:
            assert float(dS[:, o:o + c].abs().max()) == 0.0                # one column: exactly 0
        else:
            pairs["bwd seg %d" % i] = _both("softmax bwd segment %d" % i, dS[:, o:o + c], f(pr, dr), f(pr.double(), dr.double()))
    assert torch.equal(dS[:, ~inside], dP[:, ~inside])
    A.record("segment softmax alone", pairs)


def test_segment_softmax_segment_limit(dev):
    """16 segments run, 17 are refused on the host (nothing is launched)"""
    from litemkd_amd import ops
    from litemkd_amd._lib import lib
    g = torch.Generator().manual_seed(702)
    S = torch.randn(2, 68, generator=g)
    off, cnt = [4 * i for i in range(17)], [3] * 17
    p, st = ops._p, ops._stream()
    Sd, dd = S.to(dev), torch.randn(2, 68, generator=g).to(dev)
    lib().call("lmkd_segment_softmax_fwd", p(Sd), 2, 68, 16, ops._ints(off[:16]), ops._ints(cnt[:16]), st)
    torch.cuda.synchronize()
    P = Sd.cpu()
    for i in range(16):
        _per_element("segment %d of 16" % i, P[:, 4 * i:4 * i + 3], torch.softmax(S[:, 4 * i:4 * i + 3], -1), torch.softmax(S[:, 4 * i:4 * i + 3].double(), -1))
    assert torch.equal(P[:, 3:64:4], S[:, 3:64:4]) and torch.equal(P[:, 64:], S[:, 64:])
    lib().call("lmkd_segment_softmax_bwd", p(Sd), p(dd), 2, 68, 16, ops._ints(off[:16]), ops._ints(cnt[:16]), st)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="lmkd_segment_softmax_fwd"):
        lib().call("lmkd_segment_softmax_fwd", p(Sd), 2, 68, 17, ops._ints(off), ops._ints(cnt), st)
    with pytest.raises(RuntimeError, match="lmkd_segment_softmax_bwd"):
        lib().call("lmkd_segment_softmax_bwd", p(Sd), p(dd), 2, 68, 17, ops._ints(off), ops._ints(cnt), st)
    assert torch.equal(Sd.cpu(), P)


@pytest.mark.parametrize("T,D", [(6, 96), (28, 96)])      # 144 float4 for 256 threads; 672: a partial third pass
def test_trx_dist_alone(dev, T, D):
    from litemkd_amd import ops
    from litemkd_amd._lib import lib
    nq, way, col = 3, 5, [4, 0, 2]
    g = torch.Generator().manual_seed(710 + T)
    Qv, proto = torch.randn(nq * T, D, generator=g), torch.randn(len(col), nq * T, D, generator=g)
    gl = torch.randn(nq, way, generator=g)
    p, st = ops._p, ops._stream()
    Qd, Pd = Qv.to(dev), proto.to(dev)
    logits = torch.full((nq, way), SENTINEL, device=dev)
    lib().call("lmkd_trx_dist_fwd", p(Qd), p(Pd), p(logits), nq, way, T, D, len(col), ops._ints(col), st)
    torch.cuda.synchronize()
    out = logits.cpu()
    f = lambda q, pr: -(q.reshape(1, nq, T * D) - pr.reshape(len(col), nq, T * D)).pow(2).sum(-1).t() / T      # noqa: E731  [nq, segment]
    tag = "trx_dist T %d D %d" % (T, D)
    pairs = {"logits": _both(tag + " logits", out[:, col], f(Qv, proto), f(Qv.double(), proto.double()))}
    assert torch.equal(out[:, [1, 3]], torch.full((nq, 2), SENTINEL))      # columns of no segment: untouched
    assert torch.equal(Pd.cpu(), proto)
    dQv = torch.full((nq * T, D), float("nan"), device=dev)
    gd = gl.to(dev)
    lib().call("lmkd_trx_dist_bwd", p(Qd), p(Pd), p(gd), p(dQv), nq, way, T, D, len(col), ops._ints(col), st)
    torch.cuda.synchronize()

    def dp(q, pr, gg):      # (2 / T) g[q, col(segment)] (Qv - proto)
        cf = gg[:, col].t().reshape(len(col), nq, 1, 1) * (2.0 / T)
        return (cf * (q.reshape(1, nq, T, D) - pr.reshape(len(col), nq, T, D))).reshape(len(col), nq * T, D)
    pairs["dproto"] = _both(tag + " dproto", Pd.cpu(), dp(Qv, proto, gl), dp(Qv.double(), proto.double(), gl.double()))
    pairs["dQv"] = _both(tag + " dQv", dQv.cpu(), -dp(Qv, proto, gl).sum(0), -dp(Qv.double(), proto.double(), gl.double()).sum(0))
    A.record(tag, pairs)


def _sim_formula(P):
    """P [nseg, Nq, T * D] -> (sim [Nq, nseg, nseg], gram): the explicit formula of tests/_matcher_ref.trx"""
    Pq = P.permute(1, 0, 2)
    gram = Pq @ Pq.transpose(1, 2)
    n = torch.linalg.vector_norm(Pq, dim=-1)
    return gram / torch.clamp(n.unsqueeze(2) * n.unsqueeze(1), min=1e-8), gram


@pytest.mark.parametrize("col", [list(range(8)), [1, 4, 6]])
def test_trx_sup_sim_alone(dev, col):
    from litemkd_amd import ops
    from litemkd_amd._lib import lib
    nq, T, D, way, nseg = 2, 4, 96, 8, len(col)
    g = torch.Generator().manual_seed(720 + nseg)
    proto = torch.randn(nseg, nq * T, D, generator=g)
    proto[1] = 0.7 * proto[0] + 0.3 * proto[1]      # (not every pair near-orthogonal)
    dsim = torch.randn(nq, way, way, generator=g)
    p, st = ops._p, ops._stream()
    Pd = proto.to(dev)
    sim, gram = torch.full((nq, way, way), float("nan"), device=dev), torch.full((nq, nseg, nseg), float("nan"), device=dev)
    lib().call("lmkd_trx_sup_sim_fwd", p(Pd), ops._ints(col), p(sim), p(gram), nq, way, nseg, T, D, st)
    torch.cuda.synchronize()
    sim, gram = sim.cpu(), gram.cpu()
    assert torch.isfinite(sim).all() and torch.equal(sim, sim.transpose(1, 2))
    assert float((sim[:, col, col] - 1).abs().max()) <= 1e-6
    for c in range(way):
        if c not in col:
            assert float(sim[:, c, :].abs().max()) == 0.0 and float(sim[:, :, c].abs().max()) == 0.0, c
    P3 = proto.reshape(nseg, nq, T * D)
    s32, g32 = _sim_formula(P3)
    P64 = P3.double().requires_grad_()
    s64, g64 = _sim_formula(P64)
    tag = "trx_sup_sim %d of %d" % (nseg, way)
    sub = sim[:, col][:, :, col]
    pairs = {"sim": _both(tag + " sim", sub, s32, s64.detach()), "gram": _both(tag + " gram", gram, g32, g64.detach())}
    dsub = dsim[:, col][:, :, col]
    (s64 * dsub.double()).sum().backward()
    P32 = P3.clone().requires_grad_()
    (_sim_formula(P32)[0] * dsub).sum().backward()
    dproto = torch.full((nseg, nq * T, D), float("nan"), device=dev)
    gram_d, dsim_d = gram.to(dev), dsim.to(dev)
    lib().call("lmkd_trx_sup_sim_bwd", p(Pd), ops._ints(col), p(gram_d), p(dsim_d), p(dproto), nq, way, nseg, T, D, st)
    torch.cuda.synchronize()
    pairs["dproto"] = _both(tag + " dproto", dproto.cpu().reshape(nseg, nq, T * D), P32.grad, P64.grad)
    A.record(tag, pairs)
    assert torch.equal(Pd.cpu(), proto)
    # sim[a][a] is the constant 1: a loss weight on the diagonal (and one at an absent class) moves no gradient - the kernel sums over
    # b != a and never reads them, so the bits stay.  (With the diagonal summed in, its two terms cancel only to rounding.)
    other = dsim.clone()
    other.diagonal(dim1=1, dim2=2).mul_(-1000.0)
    for c in range(way):
        if c not in col:
            other[:, c, :] += 5.0
            other[:, :, c] -= 3.0
    other_d, again = other.to(dev), torch.full((nseg, nq * T, D), float("nan"), device=dev)
    lib().call("lmkd_trx_sup_sim_bwd", p(Pd), ops._ints(col), p(gram_d), p(other_d), p(again), nq, way, nseg, T, D, st)
    torch.cuda.synchronize()
    assert torch.equal(again.cpu(), dproto.cpu())


def test_trx_sup_sim_refuses_nine_ways(dev):
    from litemkd_amd import ops
    from litemkd_amd._lib import lib
    x = torch.zeros(9 * 2 * 4 * 96, device=dev)
    p, st = ops._p, ops._stream()
    with pytest.raises(RuntimeError, match="lmkd_trx_sup_sim_fwd"):
        lib().call("lmkd_trx_sup_sim_fwd", p(x), ops._ints(range(9)), p(x), p(x), 2, 9, 9, 4, 96, st)
    with pytest.raises(RuntimeError, match="lmkd_trx_sup_sim_bwd"):
        lib().call("lmkd_trx_sup_sim_bwd", p(x), ops._ints(range(9)), p(x), p(x), p(x), 2, 9, 9, 4, 96, st)
