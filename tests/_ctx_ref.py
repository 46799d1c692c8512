"""Plain-torch restatement of the CTX matcher head, written from its description: positional encoding (+ an optional
dropout mask), key and value projections, LayerNorm of the keys only, and per (query, class) a softmax over ALL support frames of the
class, the prototype A Vc and the negated squared distance over seq_len; a class in [0, way) without support keeps logit 0.  Runs in
fp32 and fp64 on the CPU.  Also the seeded inputs and parameters that tools/gen_ctx_golden.py and the tests share (nothing is stored)."""
import math

import torch
import torch.nn.functional as F

from _strm_ref import gsum      # noqa: F401  (the 64-wide chunk sums the fixtures store)

# (seed, way, support labels, queries, seq_len, Din, Dk, factor on norm_k.weight)
CASES = [
    (81, 2, [0, 1], 1, 2, 64, 4, 1.0),                                        # 0 the minimum
    (82, 3, [1, 2, 1, 0, 1, 2], 4, 4, 64, 32, 1.0),                           # 1 ragged (1, 3, 2), labels unsorted
    (83, 4, [2, 0, 2, 2, 3], 2, 3, 2048, 20, 1.0),                            # 2 class 1 absent: its column is 0; fixture
    (84, 2, [0, 0, 1, 1], 2, 1, 64, 8, 1.0),                                  # 3 seq_len 1: the softmax runs over the class's 2 entries only
    (85, 2, [0, 1], 2, 16, 64, 36, 1.0),                                      # 4 the largest seq_len: pe rows 0 .. 15 of 24
    # 5: the per-(query, class) kernels walk D 1024 columns at a time (CX_BIG lanes, one column each; CX_DTILE of the backward's score
    # kernel) and the row-gradient kernel in workgroups of 64 columns (CX_COLS); 1284 = 1024 + 4 x 64 + 4 leaves a partial tile of both
    (86, 2, [0, 1], 2, 2, 64, 1284, 1.0),
    (87, 2, [0] * 16 + [1], 2, 16, 64, 8, 1.0),                               # 6 class 0 at the limit of 256 support frames
    (88, 2, [0, 0, 1, 1], 2, 4, 2048, 32, 6.0),                               # 7 scores beyond 89: exp overflows without the row maximum; fixture
    (89, 5, [c for c in range(5) for _ in range(5)], 25, 8, 2048, 1152, 1.0),  # 8 the workload; fixture
]
FIXTURE_CASES = (2, 7, 8)
GRAD_KEYS = ("g_support", "g_query", "g_wk", "g_bk", "g_wv", "g_bv", "g_gamma", "g_beta")
KEYS = ("logits",) + GRAD_KEYS

# Bound of each comparison with tests/golden/ctx.npz (the reference's own CrossTransformer): 3 x the deviation of the fp32 restatement
# from the reference as tools/gen_ctx_golden.py measured it on the CPU, not below 3e-6 of the largest |value| of the reference's tensor.
# Logits: largest absolute difference; gradients: largest difference of the 64-wide chunk sums.  (measured deviation, largest |value|)
# beside each bound; the largest |value| is that of the gradient itself (chunk sums cancel where a gradient sums to 0 along D).  g_bv is
# 0 in exact arithmetic (every attention row sums to 1), the reference holds the rounding of its column sums there, and 3e-6 of that
# bounds nothing; its floor is 3 x sqrt(64 x rows) x 2^-24 x max |dV|, the rounding of a 64-wide chunk sum over the rows of dV (the
# second figure beside it is max |dV|).
FIXTURE_BOUNDS = {
    2: {
        "logits": 3.57e-05,   # (1.91e-06, 1.189e+01)
        "g_support": 2.42e-06,   # (8.05e-07, 1.939e-01)
        "g_query": 4.30e-06,   # (1.43e-06, 2.244e-01)
        "g_wk": 1.26e-04,   # (4.20e-05, 1.218e+01)
        "g_bk": 1.13e-05,   # (3.87e-07, 3.738e+00)
        "g_wv": 1.38e-04,   # (4.58e-05, 1.160e+01)
        "g_bv": 1.46e-05,   # (0.00e+00, 2.217e+00)
        "g_gamma": 1.81e-05,   # (6.02e-06, 3.313e+00)
        "g_beta": 5.77e-06,   # (8.34e-07, 1.922e+00)
    },
    7: {
        "logits": 8.23e-05,   # (1.34e-05, 2.741e+01)
        "g_support": 6.44e-05,   # (2.15e-05, 3.584e-01)
        "g_query": 8.30e-05,   # (2.77e-05, 3.669e-01)
        "g_wk": 4.08e-03,   # (1.36e-03, 1.880e+01)
        "g_bk": 9.75e-06,   # (1.67e-06, 3.249e+00)
        "g_wv": 5.15e-05,   # (1.72e-05, 2.517e+00)
        "g_bv": 5.58e-06,   # (5.59e-08, 7.949e-01)
        "g_gamma": 2.21e-05,   # (7.36e-06, 1.115e+00)
        "g_beta": 1.27e-06,   # (5.96e-08, 4.229e-01)
    },
    8: {
        "logits": 1.59e-03,   # (2.14e-04, 5.294e+02)
        "g_support": 8.02e-05,   # (2.67e-05, 2.704e+00)
        "g_query": 4.44e-05,   # (1.48e-05, 2.561e+00)
        "g_wk": 1.41e-03,   # (4.69e-04, 4.797e+01)
        "g_bk": 2.41e-04,   # (8.01e-05, 1.365e+01)
        "g_wv": 3.44e-04,   # (1.14e-04, 2.997e+01)
        "g_bv": 1.08e-04,   # (1.98e-05, 3.747e+00)
        "g_gamma": 3.44e-04,   # (1.14e-04, 2.196e+01)
        "g_beta": 1.72e-04,   # (5.72e-05, 9.560e+00)
    },
}


def positional_encoding(max_len, d_model, scale=0.1):
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2) * -(math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term) * scale
    pe[:, 1::2] = torch.cos(position * div_term) * scale
    return pe


def case_data(case):
    """-> dict(way, L, sup [Ns, L, Din], lab float [Ns], qry [Nq, L, Din], and the parameters wk, bk, wv, bv, gamma, beta, pe [1.5 L, Din]).
    Query i is the first support video of class i % (classes with support) plus 0.5 randn, so the softmax is not flat."""
    seed, way, labels, nq, L, Din, Dk, kscale = CASES[case]
    g = torch.Generator().manual_seed(seed + 9000)
    lab = torch.tensor(labels, dtype=torch.float32)
    sup = torch.randn(lab.numel(), L, Din, generator=g)
    classes = sorted(set(labels))
    first = [labels.index(classes[i % len(classes)]) for i in range(nq)]
    qry = sup[first] + 0.5 * torch.randn(nq, L, Din, generator=g)
    bound = 1.0 / math.sqrt(Din)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * bound      # noqa: E731  (nn.Linear's default range)
    P = {"wk": u(Dk, Din), "bk": u(Dk), "wv": u(Dk, Din), "bv": u(Dk),
         "gamma": (1 + 0.1 * torch.randn(Dk, generator=g)) * kscale, "beta": 0.1 * torch.randn(Dk, generator=g),
         "pe": positional_encoding(int(L * 1.5), Din)}
    return dict(way=way, L=L, sup=sup, lab=lab, qry=qry, **P)


def ctx_head(sup, lab, qry, way, wk, bk, wv, bv, gamma, beta, pe, mask=None, scores=None):
    """-> logits [Nq, way].  mask: [(Ns + Nq) L, Din] multiplier (dropout), support rows first.  scores: a list that receives the scaled
    score tensor of every class"""
    Ns, L, Din = sup.shape
    Dk = wk.shape[0]
    x = torch.cat([sup, qry]) + pe[:L]
    if mask is not None:
        x = x * mask.reshape(x.shape).to(x)
    k = F.layer_norm(x @ wk.t() + bk, (Dk,), gamma, beta, 1e-5)
    v = x @ wv.t() + bv
    kq, vq = k[Ns:], v[Ns:]
    cols = []
    for c in range(way):
        idx = torch.nonzero(lab == c).reshape(-1)
        if idx.numel() == 0:
            cols.append(torch.zeros(qry.shape[0], dtype=x.dtype))
            continue
        kc, vc = k[idx].reshape(-1, Dk), v[idx].reshape(-1, Dk)
        s = torch.einsum("qld,fd->qlf", kq, kc) / math.sqrt(Dk)
        if scores is not None:
            scores.append(s.detach())
        diff = vq - torch.softmax(s, dim=-1) @ vc
        cols.append(-(diff * diff).sum((1, 2)) / L)
    return torch.stack(cols, 1)


def fixture_weights(shape, seed=97):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def fixture_loss(logits):
    """the scalar whose gradients the fixture digests"""
    return (logits * fixture_weights(logits.shape).to(logits)).sum()


PARAMS = ("wk", "bk", "wv", "bv", "gamma", "beta")


def run(case, dtype, mask=None):
    """-> dict(logits, g_support, g_query, g_wk, g_bk, g_wv, g_bv, g_gamma, g_beta) of the restatement in `dtype`"""
    d = case_data(case)
    s, q = d["sup"].to(dtype).requires_grad_(), d["qry"].to(dtype).requires_grad_()
    P = {k: d[k].to(dtype).requires_grad_() for k in PARAMS}
    logits = ctx_head(s, d["lab"], q, d["way"], pe=d["pe"].to(dtype), mask=mask, **P)
    fixture_loss(logits).backward()
    out = {"logits": logits.detach(), "g_support": s.grad, "g_query": q.grad}
    out.update({"g_" + k: P[k].grad for k in PARAMS})
    return out


def fixture_error(key, value, ref):
    """the figure FIXTURE_BOUNDS bounds: logits by elements, gradients by their chunk sums; ref = the array stored in ctx.npz"""
    v = value.detach().cpu().double() if key == "logits" else gsum(value.detach().cpu()).double()
    return float((v - torch.as_tensor(ref).double()).abs().max())
