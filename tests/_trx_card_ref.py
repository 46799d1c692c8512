"""Plain-torch restatement of the TemporalCrossTransformer over frame tuples of cardinality 2 or 3 and of a head that averages several
cardinalities, written from their description.  Runs in fp32 and fp64 on the CPU (the dtype follows the inputs), dropout
off.  Also the seeded parameters / inputs that tools/gen_trx_card_golden.py and the tests share (the fixture stores no parameters)."""
import math
from itertools import combinations

import torch
import torch.nn.functional as F

from _strm_ref import gsum, pe_table      # noqa: F401  (the 64-wide chunk sums the fixtures store)

IN_DIM, OUT_DIM = 2048, 1152

# (seed, way, support labels, queries, seq_len, temp_set, shuffle the support)
CASES = [
    (51, 5, [0, 0, 1, 1, 2, 2, 3, 3, 4, 4], 5, 8, [2, 3], True),
    (52, 3, [2, 0, 0, 2, 2], 2, 8, [3], False),      # ragged, class 1 absent: its column stays 0
    (53, 2, [0, 1], 2, 4, [2, 3], False),
]


def _linear(g, p, name, fin, fout):
    b = 1.0 / math.sqrt(fin)
    p[name + ".weight"] = (torch.rand(fout, fin, generator=g) * 2 - 1) * b
    p[name + ".bias"] = (torch.rand(fout, generator=g) * 2 - 1) * b


def make_params(seed, card, seq_len=8, out_dim=OUT_DIM, in_dim=IN_DIM):
    """one TemporalCrossTransformer's state_dict (keys without prefix); a non-trivial LayerNorm affine so a test sees it"""
    g = torch.Generator().manual_seed(seed * 10 + card)
    p = {"pe.pe": pe_table(in_dim, int(seq_len * 1.5))}
    _linear(g, p, "k_linear", in_dim * card, out_dim)
    _linear(g, p, "v_linear", in_dim * card, out_dim)
    p["norm_k.weight"] = 1 + 0.1 * torch.randn(out_dim, generator=g)
    p["norm_k.bias"] = 0.1 * torch.randn(out_dim, generator=g)
    p["norm_v.weight"] = torch.ones(out_dim)
    p["norm_v.bias"] = torch.zeros(out_dim)
    return p


def make_inputs(seed, labels, n_query, seq_len, shuffle, in_dim=IN_DIM):
    """-> support [Ns, L, in_dim], labels float [Ns], queries [Nq, L, in_dim]: randn * 0.5"""
    g = torch.Generator().manual_seed(seed + 5000)
    lab = torch.tensor(labels, dtype=torch.float32)
    if shuffle:
        lab = lab[torch.randperm(lab.numel(), generator=g)]
    sup = torch.randn(lab.numel(), seq_len, in_dim, generator=g) * 0.5
    qry = torch.randn(n_query, seq_len, in_dim, generator=g) * 0.5
    return sup, lab, qry


def case_data(case):
    """-> (way, seq_len, temp_set, [params per cardinality], support, labels, queries)"""
    seed, way, labels, nq, L, ts, shuffle = CASES[case]
    return (way, L, ts, [make_params(seed, c, L) for c in ts]) + make_inputs(seed, labels, nq, L, shuffle)


def cast(p, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.items()}


def frame_tuples(seq_len, card):
    return [list(c) for c in combinations(range(seq_len), card)]


def trx_logits(support, labels, queries, p, way, seq_len, card):
    """TemporalCrossTransformer over the frame tuples of cardinality `card`, dropout off.  Classes without support keep 0."""
    out_dim = p["k_linear.weight"].shape[0]
    n_q, n_s = queries.shape[0], support.shape[0]
    table = p["pe.pe"][:, :seq_len].to(support.dtype)
    support, queries = support + table, queries + table
    tuples = frame_tuples(seq_len, card)
    T = len(tuples)
    s = torch.stack([support[:, t, :].reshape(n_s, -1) for t in tuples], dim=-2)
    q = torch.stack([queries[:, t, :].reshape(n_q, -1) for t in tuples], dim=-2)
    s_k = F.layer_norm(F.linear(s, p["k_linear.weight"], p["k_linear.bias"]), (out_dim,), p["norm_k.weight"], p["norm_k.bias"], 1e-5)
    q_k = F.layer_norm(F.linear(q, p["k_linear.weight"], p["k_linear.bias"]), (out_dim,), p["norm_k.weight"], p["norm_k.bias"], 1e-5)
    s_v = F.linear(s, p["v_linear.weight"], p["v_linear.bias"])
    q_v = F.linear(q, p["v_linear.weight"], p["v_linear.bias"])
    cols = []
    for c in range(way):
        idx = torch.nonzero(labels == c).reshape(-1)
        if idx.numel() == 0:
            cols.append(torch.zeros(n_q, dtype=support.dtype))
            continue
        sc = torch.matmul(q_k.unsqueeze(1), s_k[idx].transpose(-2, -1)) / math.sqrt(out_dim)
        sc = torch.softmax(sc.permute(0, 2, 1, 3).reshape(n_q, T, -1), dim=-1).reshape(n_q, T, -1, T).permute(0, 2, 1, 3)
        proto = torch.matmul(sc, s_v[idx]).sum(dim=1)
        cols.append(-(q_v - proto).pow(2).sum(dim=(-2, -1)) / T)
    return torch.stack(cols, 1)


def head_logits(support, labels, queries, params, way, seq_len, temp_set):
    """mean over the cardinalities of a head (one parameter dict per entry of temp_set)"""
    return torch.stack([trx_logits(support, labels, queries, p, way, seq_len, c) for p, c in zip(params, temp_set)], dim=-1).mean(dim=-1)


def fixture_loss(logits):
    """the scalar whose gradients the fixture digests"""
    return (logits * torch.linspace(-1, 1, logits.numel()).reshape(logits.shape).to(logits)).sum() * 1e-2


# ---- the tuple kernels alone ----
def tuples_combine(P, bk, bv, gamma, beta, L, card, eps=1e-5):
    """P [NV*L, 2*card*D] -> (Kn, Khat, V, rstd) rows n*T + t (no rowmap), left-to-right sums like the kernel"""
    D = bk.numel()
    NV = P.shape[0] // L
    Pf = P.reshape(NV, L, 2 * card, D)
    ks, vs = [], []
    for tup in frame_tuples(L, card):
        k = Pf[:, tup[0], 0] + Pf[:, tup[1], 1]
        v = Pf[:, tup[0], card] + Pf[:, tup[1], card + 1]
        if card == 3:
            k = k + Pf[:, tup[2], 2]
            v = v + Pf[:, tup[2], card + 2]
        ks.append(k + bk)
        vs.append(v + bv)
    K = torch.stack(ks, 1).reshape(-1, D)
    V = torch.stack(vs, 1).reshape(-1, D)
    mean = K.mean(1, keepdim=True)
    var = (K - mean).pow(2).mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    Khat = (K - mean) * rstd
    return Khat * gamma + beta, Khat, V, rstd.reshape(-1)


def tuples_gather(dK, dV, NV, L, card):
    """transpose of the forward's selection: dP [NV*L, 2*card*D], every sum in ascending tuple order"""
    D = dK.shape[1]
    tuples = frame_tuples(L, card)
    T = len(tuples)
    dP = torch.zeros(NV, L, 2 * card, D, dtype=dK.dtype)
    dK, dV = dK.reshape(NV, T, D), dV.reshape(NV, T, D)
    for t, tup in enumerate(tuples):
        for s, f in enumerate(tup):
            dP[:, f, s] = dP[:, f, s] + dK[:, t]
            dP[:, f, card + s] = dP[:, f, card + s] + dV[:, t]
    return dP.reshape(NV * L, 2 * card * D)
