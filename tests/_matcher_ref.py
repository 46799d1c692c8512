"""Plain-torch restatement of the matcher heads (csrc/trx.hip behind ops.TRXLogitsFn / TRXSupFn / EDistFn / SupportDKFn), written from their
description: the temporal cross-transformer over frame pairs or triples with its prototype similarity, the Euclidean matcher, the support
prototype distances.  The dtype follows the inputs (fp32 and fp64 on the CPU); every width is taken from the shapes it is given."""
import math
from itertools import combinations

import torch
import torch.nn.functional as F


def trx(support, labels, queries, p, way, seq_len, card, mask=None):
    """-> (logits [Nq, way], sim [Nq, way, way]).  p: one TemporalCrossTransformer's state_dict (keys without prefix, as
    _trx_card_ref.make_params makes it); mask [Ns + Nq, L, Din] (support videos first) multiplies (x + pe) elementwise, as lmkd_add_pe does.
    A class without support keeps a zero logit column and a zero prototype; sim[q, a, b] = <P_a, P_b> / max(|P_a| |P_b|, 1e-8) over the
    T * D entries of query q's class prototypes."""
    D = p["k_linear.weight"].shape[0]
    n_q, n_s = queries.shape[0], support.shape[0]
    table = p["pe.pe"][:, :seq_len].to(support.dtype)
    support, queries = support + table, queries + table
    if mask is not None:
        mask = mask.reshape(n_s + n_q, seq_len, -1).to(support.dtype)
        support, queries = support * mask[:n_s], queries * mask[n_s:]
    tuples = [list(c) for c in combinations(range(seq_len), card)]
    T = len(tuples)
    s = torch.stack([support[:, t, :].reshape(n_s, -1) for t in tuples], dim=1)      # [Ns, T, card * Din]
    q = torch.stack([queries[:, t, :].reshape(n_q, -1) for t in tuples], dim=1)

    def keys(x):
        return F.layer_norm(F.linear(x, p["k_linear.weight"], p["k_linear.bias"]), (D,), p["norm_k.weight"], p["norm_k.bias"], 1e-5)

    s_k, q_k = keys(s), keys(q)
    s_v = F.linear(s, p["v_linear.weight"], p["v_linear.bias"])
    q_v = F.linear(q, p["v_linear.weight"], p["v_linear.bias"])
    zero = torch.zeros((), dtype=support.dtype)
    cols, protos = [], []
    for c in range(way):
        idx = torch.nonzero(labels == c).reshape(-1)
        if idx.numel() == 0:
            cols.append(zero.expand(n_q))
            protos.append(zero.expand(n_q, T, D))
            continue
        # every query tuple attends over ALL tuples of ALL the class's videos: one softmax over count * T scores
        ck, cv = s_k[idx].reshape(-1, D), s_v[idx].reshape(-1, D)
        att = torch.softmax(torch.matmul(q_k, ck.t()) / math.sqrt(D), dim=-1)          # [Nq, T, count * T]
        proto = torch.matmul(att, cv)                                                  # [Nq, T, D]
        protos.append(proto)
        cols.append(-(q_v - proto).pow(2).sum(dim=(-2, -1)) / T)
    P = torch.stack(protos, 1).reshape(n_q, way, T * D)
    gram = torch.matmul(P, P.transpose(1, 2))
    norm = torch.linalg.vector_norm(P, dim=-1)      # (its subgradient at an absent class's zero prototype is 0, not 0 / 0)
    sim = gram / torch.clamp(norm.unsqueeze(2) * norm.unsqueeze(1), min=1e-8)
    return torch.stack(cols, 1), sim


def e_dist(support, labels, queries, way):
    """frame means, Euclidean distance of every query to every support video (direct differences: the subgradient at a zero distance is 0),
    the class mean negated; 0 for a class without support.  -> [Nq, way]"""
    sm, qm = support.mean(dim=1), queries.mean(dim=1)
    dist = torch.cdist(qm, sm, p=2.0, compute_mode="donot_use_mm_for_euclid_dist")
    cols = []
    for c in range(way):
        idx = torch.nonzero(labels == c).reshape(-1)
        cols.append(-dist[:, idx].mean(dim=1) if idx.numel() else torch.zeros(queries.shape[0], dtype=support.dtype))
    return torch.stack(cols, 1)


def support_dk(support, way, shot):
    """class-sorted support [way * shot, L, D] -> [way, way - 1]: -|P_i - P_j|^2 / L over the L * D prototype entries, j != i ascending"""
    L = support.shape[1]
    proto = support.reshape(way, shot, -1).mean(dim=1)
    d = -(proto.unsqueeze(1) - proto.unsqueeze(0)).pow(2).sum(-1) / L
    return torch.stack([torch.cat([d[i, :i], d[i, i + 1:]]) for i in range(way)])
