"""Plain-torch restatement of the OTAM matcher head, written from its description: frame cosine distances with the
0.01 added to the PRODUCT of the norms, the ordered alignment table in both directions with the soft minimum evaluated after its
minimum is subtracted, class means, softmax of the negated class distances.  Runs in fp32 and fp64 on the CPU (the dtype follows the
inputs).  Also the seeded inputs that tools/gen_otam_golden.py and the tests share (the fixture stores no inputs)."""
import torch

from _strm_ref import gsum      # noqa: F401  (the 64-wide chunk sums the fixtures store)

LBDA = 0.1
EPS = 0.01

# (seed, way, support labels, queries, seq_len, D, shuffle the support, queries near a same-class support video)
CASES = [
    (61, 5, [0, 0, 1, 1, 2, 2, 3, 3, 4, 4], 5, 8, 2048, True, True),                     # the register path
    (62, 3, [2, 0, 0, 2, 2, 1], 2, 8, 2048, False, True),                                # ragged counts, unsorted labels
    (63, 2, [0, 1], 2, 4, 64, False, True),                                              # the LDS path, small D
    (64, 5, [c for c in range(5) for _ in range(7)][:34], 3, 8, 256, False, True),       # 68 lanes: the block crosses a wavefront
    (65, 5, [c for c in range(5) for _ in range(5)], 25, 8, 2048, False, True),          # the workload's own shape
    (66, 2, [0, 0, 1], 2, 12, 128, False, False),                                        # randn: the reference is inf here
    (67, 2, [0, 1], 1, 16, 64, False, False),                                            # the largest seq_len
    # the sizes at which the kernels take another path
    (68, 2, [0] * 17 + [1] * 17, 2, 16, 64, False, False),                               # LDS path, 68 pair-directions in two rounds of 64 lanes
    (69, 2, [0] * 129 + [1] * 129, 1, 8, 64, False, True),                               # seq_len 8 past 256 supports: LDS path, two rounds
    (70, 2, [0, 1, 0], 2, 5, 8, False, False),                                           # Ns * L = 15: row pitch 16, zero pad rows in the GEMMs
]
FIXTURE_CASES = (0, 1, 2)      # the cases tests/golden/otam.npz holds: the reference alone is finite there (seq_len <= 8)


def make_inputs(seed, labels, n_query, seq_len, dim, shuffle, near):
    """-> support [Ns, L, D], labels float [Ns], queries [Nq, L, D].  near: query i is the first support video of class i % way plus
    0.5 * randn (cum then spans about 1.7 .. 14.5 and the softmax is not flat); otherwise plain randn."""
    g = torch.Generator().manual_seed(seed + 7000)
    lab = torch.tensor(labels, dtype=torch.float32)
    if shuffle:
        lab = lab[torch.randperm(lab.numel(), generator=g)]
    sup = torch.randn(lab.numel(), seq_len, dim, generator=g)
    noise = torch.randn(n_query, seq_len, dim, generator=g)
    if not near:
        return sup, lab, noise
    classes = sorted(set(int(v) for v in lab.tolist()))
    first = [int(torch.nonzero(lab == classes[i % len(classes)])[0]) for i in range(n_query)]
    return sup, lab, sup[first] + 0.5 * noise


def case_data(case):
    """-> (way, seq_len, support, labels, queries)"""
    seed, way, labels, nq, L, D, shuffle, near = CASES[case]
    return (way, L) + make_inputs(seed, labels, nq, L, D, shuffle, near)


def frame_dist(sup, qry):
    """-> d [Nq*L, Ns*L] = 1 - x.y / (|x| |y| + 0.01), rows the query frames"""
    x, y = qry.reshape(-1, qry.shape[-1]), sup.reshape(-1, sup.shape[-1])
    den = x.norm(dim=-1).unsqueeze(1) * y.norm(dim=-1).unsqueeze(0) + EPS
    return 1 - (x @ y.t()) / den


def softmin(*a):
    a = torch.stack(a, -1)
    m = a.min(dim=-1, keepdim=True).values.detach()
    return m.squeeze(-1) - LBDA * torch.log(torch.exp(-(a - m) / LBDA).sum(-1))


def align(B):
    """one direction over blocks B [..., L, L] (row = the sequence that advances one frame per table row) -> C[L-1][L+1]"""
    L = B.shape[-1]
    zero = torch.zeros_like(B[..., 0, 0])
    P = [[zero] + [B[..., l, k] for k in range(L)] + [zero] for l in range(L)]
    row = [zero]
    for m in range(1, L + 2):
        row.append(P[0][m] + row[m - 1])
    for l in range(1, L):
        new = [zero, P[l][1] + softmin(row[0], row[1], zero)]
        for m in range(2, L + 1):
            new.append(P[l][m] + softmin(row[m - 1], new[m - 1]))
        new.append(softmin(row[L], row[L + 1], new[L]))
        row = new
    return row[L + 1]


def otam(sup, labels, qry, way):
    """-> (logits [Nq, way] (probabilities, as in the reference), cum [Nq, Ns]); every class 0 .. way-1 needs a support video"""
    Ns, L, _ = sup.shape
    Nq = qry.shape[0]
    B = frame_dist(sup, qry).reshape(Nq, L, Ns, L).permute(0, 2, 1, 3)
    cum = align(B) + align(B.transpose(-1, -2))
    cols = []
    for c in range(way):
        idx = torch.nonzero(labels == c).reshape(-1)
        if idx.numel() == 0:
            raise ValueError("class %d has no support video" % c)
        cols.append(cum[:, idx].mean(1))
    return torch.softmax(-torch.stack(cols, 1), dim=1), cum


def fixture_weights(shape, seed=99):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def fixture_loss(logits):
    """the scalar whose gradients the fixture digests: seeded weights, because a plain sum of a softmax has zero gradient"""
    return (logits * fixture_weights(logits.shape).to(logits)).sum()


def run(case, dtype, loss=True):
    """-> dict(logits, cum, g_support, g_query) of the restatement in `dtype`"""
    way, L, sup, lab, qry = case_data(case)
    s, q = sup.to(dtype).requires_grad_(), qry.to(dtype).requires_grad_()
    logits, cum = otam(s, lab, q, way)
    out = {"logits": logits.detach(), "cum": cum.detach()}
    if loss:
        fixture_loss(logits).backward()
        out["g_support"], out["g_query"] = s.grad, q.grad
    return out
