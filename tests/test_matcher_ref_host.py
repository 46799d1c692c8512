"""CPU: tests/_matcher_ref.py, the restatement test_gpu_matcher_anchor.py holds the matcher heads to, against the restatements the project
already trusts - _trx_card_ref.trx_logits (pairs and triples, any width) and oracle.ref_cpu (the reference's own layout at 8 frames,
2048 -> 1152).  Two fp32 evaluations of one quantity: 1e-5 of its maximum, the bound test_triples_kernels_alone uses per element."""
import pytest
import torch
import torch.nn.functional as F

import _matcher_ref as M
import _trx_card_ref as R
from oracle import ref_cpu as O


def _close(a, b, name, rel=1e-5):
    err, top = float((a.double() - b.double()).abs().max()), float(b.double().abs().max())
    print("%-24s max err %.3e of max %.3e" % (name, err, top))
    assert a.shape == b.shape and err <= rel * top, "%s: max err %.3e > %g x %.3e" % (name, err, rel, top)


# (way, support labels, queries, frames, cardinality): ragged with absent classes, padded positions in the HIP layout, 15 tuples, triples of 4
LAYOUTS = [(4, [2, 0, 0, 2, 2], 2, 8, 3), (4, [0, 1, 1, 2, 2, 2], 3, 4, 2), (3, [1, 0, 2, 0, 1, 0, 0], 2, 6, 2), (5, [4, 0, 2, 0], 2, 4, 3),
           (3, [0, 0, 1, 1, 2, 2], 4, 8, 2)]


@pytest.mark.parametrize("case", range(len(LAYOUTS)))
def test_trx_equals_the_cardinality_restatement_in_fp32(case):
    way, labels, nq, L, card = LAYOUTS[case]
    p = R.make_params(300 + case, card, L, out_dim=96, in_dim=128)
    sup, lab, qry = R.make_inputs(300 + case, labels, nq, L, case == 4, in_dim=128)
    logits, sim = M.trx(sup, lab, qry, p, way, L, card)
    assert logits.dtype == torch.float32 and sim.shape == (nq, way, way)
    _close(logits, R.trx_logits(sup, lab, qry, p, way, L, card), "logits")
    absent = [c for c in range(way) if c not in labels]
    for c in absent:
        assert float(logits[:, c].abs().max()) == 0.0 and float(sim[:, c].abs().max()) == 0.0 and float(sim[:, :, c].abs().max()) == 0.0
    l64, s64 = M.trx(sup.double(), lab, qry.double(), R.cast(p, torch.float64), way, L, card)
    assert l64.dtype == torch.float64
    _close(logits, l64, "logits fp32 / fp64")
    _close(sim, s64, "sim fp32 / fp64")


def _oracle_case(seed, labels, nq):
    g = torch.Generator().manual_seed(seed)
    p = O.make_trx_params(g)
    p["norm_k.weight"] = 1 + 0.1 * torch.randn(1152, generator=g)
    p["norm_k.bias"] = 0.1 * torch.randn(1152, generator=g)
    sup = torch.randn(len(labels), 8, 2048, generator=g) * 0.5
    qry = torch.randn(nq, 8, 2048, generator=g) * 0.5
    return p, sup, torch.tensor(labels, dtype=torch.float32), qry


@pytest.mark.parametrize("way,labels", [(3, [1, 0, 2, 1]), (4, [3, 0, 3])])
def test_trx_equals_the_oracle_at_full_width(way, labels):
    p, sup, lab, qry = _oracle_case(17 + way, labels, 2)
    logits, sim = M.trx(sup, lab, qry, p, way, 8, 2)
    _close(logits, O.trx_logits(sup, lab, qry, p, way), "logits")
    o_logits, o_sim = O.trx_sup_logits(sup, lab, qry, p, way)      # (its similarity is F.cosine_similarity over the 28 * 1152 entries)
    _close(logits, o_logits, "sup logits")
    _close(sim, o_sim, "similarity")
    # and the similarity formula alone, on the prototypes' own scale and on tiny ones (eps matters only for a zero prototype)
    g = torch.Generator().manual_seed(5)
    P = torch.randn(2, 4, 300, generator=g, dtype=torch.float64)
    P[:, 2] = 0
    gram = P @ P.transpose(1, 2)
    n = gram.diagonal(dim1=1, dim2=2).sqrt()
    mine = gram / torch.clamp(n.unsqueeze(2) * n.unsqueeze(1), min=1e-8)
    ref = F.cosine_similarity(P.unsqueeze(1), P.unsqueeze(2), dim=-1)
    _close(mine, ref, "cosine", 1e-12)


def test_e_dist_and_support_dk_equal_the_oracle():
    g = torch.Generator().manual_seed(23)
    sup, qry = torch.randn(6, 8, 2048, generator=g), torch.randn(3, 8, 2048, generator=g)
    lab = torch.tensor([2, 0, 2, 3, 0, 2], dtype=torch.float32)
    out = M.e_dist(sup, lab, qry, 5)
    _close(out, O.e_dist_logits(sup, lab, qry, 5), "e_dist")
    assert float(out[:, 1].abs().max()) == 0.0 and float(out[:, 4].abs().max()) == 0.0
    _close(M.support_dk(sup, 3, 2), O.support_dk(sup, 3, 2), "support_dk")
    _close(M.support_dk(sup, 6, 1), O.support_dk(sup, 6, 1), "support_dk one shot")
    # any L, D
    s2 = torch.randn(6, 3, 100, generator=g, dtype=torch.float64)
    proto = s2.reshape(3, 2, 300).mean(1)
    assert abs(float(M.support_dk(s2, 3, 2)[2, 0]) + float((proto[2] - proto[0]).pow(2).sum()) / 3) < 1e-12


def test_e_dist_zero_distance_has_zero_subgradient():
    g = torch.Generator().manual_seed(29)
    sup = torch.randn(3, 3, 100, generator=g, dtype=torch.float64).requires_grad_()
    qry = torch.randn(2, 3, 100, generator=g, dtype=torch.float64)
    qry[0] = sup.detach()[1]
    qry.requires_grad_()
    lab = torch.tensor([2, 0, 2], dtype=torch.float32)
    out = M.e_dist(sup, lab, qry, 4)
    assert float(out.detach()[0, 0]) == 0.0
    out.sum().backward()
    assert torch.isfinite(sup.grad).all() and torch.isfinite(qry.grad).all()
    # support video 1 is class 0's only one: its gradient comes from query 1 alone
    d = (qry.detach()[1].mean(0) - sup.detach()[1].mean(0))
    assert torch.allclose(sup.grad[1], (d / d.norm() / 3).expand(3, 100), rtol=1e-12, atol=1e-15)


def test_mask_none_equals_a_mask_of_ones_bit_for_bit():
    way, labels, nq, L, card = LAYOUTS[1]
    p = R.make_params(41, card, L, out_dim=96, in_dim=128)
    sup, lab, qry = R.make_inputs(41, labels, nq, L, False, in_dim=128)
    a = M.trx(sup, lab, qry, p, way, L, card)
    b = M.trx(sup, lab, qry, p, way, L, card, mask=torch.ones(len(labels) + nq, L, 128))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    keep = (torch.rand(len(labels) + nq, L, 128, generator=torch.Generator().manual_seed(1)) >= 0.1).float() / 0.9
    c = M.trx(sup, lab, qry, p, way, L, card, mask=keep)
    assert not torch.equal(a[0], c[0])
    # the mask multiplies (x + pe): the same head on pre-masked inputs with the table taken out
    table = p["pe.pe"][:, :L]
    d = M.trx((sup + table) * keep[:len(labels)] - table, lab, (qry + table) * keep[len(labels):] - table, p, way, L, card)
    _close(c[0], d[0], "masked logits")
