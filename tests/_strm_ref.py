"""Plain-torch restatement of the STRM student family's head: 4 x 4 adaptive max pooling with the patches kept, patch
attention, the bottleneck MLPs, frame mixing and the patch-distance head, written from their description.  Runs in fp32 and fp64 on the
CPU (the dtype follows the inputs), takes optional dropout masks, and can have the pooling and minimum selections imposed, so that a
GPU result is compared on the same selections.  Also the seeded parameters / inputs that tools/gen_strm_golden.py and the tests share
(the fixtures store no parameters)."""
import math
from itertools import combinations

import torch
import torch.nn.functional as F

RELU = None      # tests: a callable(t) -> tensor replacing torch.relu at every ReLU of the head, in evaluation order (imposed masks)


def _relu(t):
    return torch.relu(t) if RELU is None else RELU(t)


GAMMA = 0.3      # attn_pat.gamma of the fixtures (the reference initialises it to 0, which hides the attention path)


def pe_table(d_model, max_len, scale=0.1):
    pe = torch.zeros(max_len, d_model)
    pos = torch.arange(0, max_len).unsqueeze(1)
    div = torch.exp(torch.arange(0, d_model, 2) * -(math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(pos * div) * scale
    pe[:, 1::2] = torch.cos(pos * div) * scale
    return pe.unsqueeze(0)


def gsum(g):
    """64-wide chunk sums of a gradient (the digest the fixtures store)"""
    g = g.detach().reshape(-1)
    pad = (-g.numel()) % 64
    if pad:
        g = torch.cat([g, g.new_zeros(pad)])
    return g.reshape(-1, 64).sum(1)


# ----------------------------------------------------------------------------------------------------------------------------------
# seeded parameters and inputs
# ----------------------------------------------------------------------------------------------------------------------------------
def _linear(g, p, name, fin, fout):
    b = 1.0 / math.sqrt(fin)
    p[name + ".weight"] = (torch.rand(fout, fin, generator=g) * 2 - 1) * b
    p[name + ".bias"] = (torch.rand(fout, generator=g) * 2 - 1) * b


def make_backbone_params(seed, backbone="strm18_student", seq_len=8):
    """every state_dict entry of the backbone beyond the trunk, by the reference's key names"""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for n in ("key_proj", "query_proj", "value_conv"):
        _linear(g, p, "attn_pat." + n, 512, 512)
    p["attn_pat.gamma"] = torch.full((1,), GAMMA)
    _linear(g, p, "attn_pat.Bot_MLP.inp_fc", 512, 256)
    _linear(g, p, "attn_pat.Bot_MLP.hid_fc", 256, 256)
    _linear(g, p, "attn_pat.Bot_MLP.out_fc", 256, 512)
    p["attn_pat.pe.pe"] = pe_table(512, 24)
    _linear(g, p, "fr_enrich.Tok_MLP.inp_fc", seq_len, seq_len)
    _linear(g, p, "fr_enrich.Tok_MLP.out_fc", seq_len, seq_len)
    _linear(g, p, "fr_enrich.Bot_MLP.inp_fc", 2048, 2048)
    _linear(g, p, "fr_enrich.Bot_MLP.out_fc", 2048, 2048)
    p["fr_enrich.pe.pe"] = pe_table(2048, int(seq_len * 1.5))
    _linear(g, p, "res18_2048", 512, 2048)
    fin = 2048 if backbone == "strm18_student" else 512
    _linear(g, p, "fc1", fin, 2048)
    _linear(g, p, "fc2", fin, 2048)
    return p


def make_classifier_params(seed, out_dim=1152, seq_len=8):
    g = torch.Generator().manual_seed(seed + 1000)
    p = {"transformers.pe.pe": pe_table(2048, int(seq_len * 1.5))}
    _linear(g, p, "transformers.k_linear", 4096, out_dim)
    _linear(g, p, "transformers.v_linear", 4096, out_dim)
    for n in ("norm_k", "norm_v"):
        p["transformers.%s.weight" % n] = torch.ones(out_dim)
        p["transformers.%s.bias" % n] = torch.zeros(out_dim)
    _linear(g, p, "DistanceLoss.clsW", 4096, 1024)
    return p


def make_fmaps(seed, frames, hw=7, channels=512):
    """post-ReLU trunk outputs [frames, hw, hw, channels] (NHWC): about half the entries are exactly 0"""
    g = torch.Generator().manual_seed(seed + 2000)
    return torch.relu(torch.randn(frames, hw, hw, channels, generator=g))


def cast(p, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.items()}


# ----------------------------------------------------------------------------------------------------------------------------------
# the operators
# ----------------------------------------------------------------------------------------------------------------------------------
def windows(n, parts=4):
    return [((i * n) // parts, -((-(i + 1) * n) // parts)) for i in range(parts)]


def patch_pool(x, idx=None):
    """x [F,H,W,C] -> (patches [F,16,C], idx int64 [F,16,C] = h * W + w of the first maximum in row-major window order).
    With `idx` given the selection is imposed: the patches gather x at those positions."""
    Fr, H, W, C = x.shape
    if idx is not None:
        return torch.gather(x.reshape(Fr, H * W, C), 1, idx.long()), idx
    flat = torch.arange(H * W).reshape(H, W)
    vals, sel = [], []
    for (h0, h1) in windows(H):
        for (w0, w1) in windows(W):
            win = x[:, h0:h1, w0:w1, :].reshape(Fr, -1, C)
            pos = flat[h0:h1, w0:w1].reshape(-1)
            m = win.max(dim=1, keepdim=True).values
            first = (win == m).to(torch.uint8).argmax(dim=1)      # argmax of a 0/1 tensor: the first maximum
            vals.append(m[:, 0])
            sel.append(pos[first])
    return torch.stack(vals, 1), torch.stack(sel, 1)


def add_table(x, table, mask=None):
    x = x + table[:, :x.shape[1]].to(x.dtype)
    return x if mask is None else x * mask.reshape(x.shape).to(x.dtype)


def patch_attention(xp, p, pre="attn_pat."):
    """xp [F,16,C] with the table (and dropout) applied -> gamma * softmax(Q K^T) V + xp   (unscaled energies)"""
    q = F.linear(xp, p[pre + "query_proj.weight"], p[pre + "query_proj.bias"])
    k = F.linear(xp, p[pre + "key_proj.weight"], p[pre + "key_proj.bias"])
    v = F.linear(xp, p[pre + "value_conv.weight"], p[pre + "value_conv.bias"])
    attn = torch.softmax(q @ k.transpose(1, 2), dim=-1)
    return p[pre + "gamma"] * (attn @ v) + xp


def bottleneck3(x, p, pre):
    h = _relu(F.linear(x, p[pre + "inp_fc.weight"], p[pre + "inp_fc.bias"]))
    h = _relu(F.linear(h, p[pre + "hid_fc.weight"], p[pre + "hid_fc.bias"]))
    return F.linear(h, p[pre + "out_fc.weight"], p[pre + "out_fc.bias"]) + x


def token_mlp(xp, w1, b1, w2, b2):
    """xp [V,L,D]: y = W2 relu(W1 xp + b1) + b2 + xp along the frame axis"""
    h = _relu(F.linear(xp.transpose(1, 2), w1, b1).transpose(1, 2))      # [V, L(hidden unit), D]
    return F.linear(h.transpose(1, 2), w2, b2).transpose(1, 2) + xp


def frame_mix(x, p, pre="fr_enrich.", mask=None):
    xp = add_table(x, p[pre + "pe.pe"], mask)
    y = token_mlp(xp, p[pre + "Tok_MLP.inp_fc.weight"], p[pre + "Tok_MLP.inp_fc.bias"], p[pre + "Tok_MLP.out_fc.weight"],
                  p[pre + "Tok_MLP.out_fc.bias"])
    h = _relu(F.linear(y, p[pre + "Bot_MLP.inp_fc.weight"], p[pre + "Bot_MLP.inp_fc.bias"]))
    return F.linear(h, p[pre + "Bot_MLP.out_fc.weight"], p[pre + "Bot_MLP.out_fc.bias"]) + y


def backbone_head(fmap, p, seq_len=8, backbone="strm18_student", pool_idx=None, masks=None):
    """fmap [F,H,W,512] NHWC trunk output -> dict of [V,L,2048] features: 'distance', and 'trx1' / 'trx2' (strm18_student) or 'trx'.
    masks: {'attn': [F,16,512], 'mix': [V*L,2048]} dropout masks (0 or 1 / (1 - p)) or None.  Also returns the pooling selection."""
    masks = masks or {}
    patches, idx = patch_pool(fmap, pool_idx)
    xp = add_table(patches, p["attn_pat.pe.pe"], masks.get("attn"))
    y = bottleneck3(patch_attention(xp, p), p, "attn_pat.Bot_MLP.")
    dist = F.linear(y.mean(dim=1), p["res18_2048.weight"], p["res18_2048.bias"]).reshape(-1, seq_len, 2048)
    fr = frame_mix(dist, p, mask=masks.get("mix"))
    if backbone == "strm18_student":
        out = {"distance": dist, "trx1": F.linear(fr, p["fc1.weight"], p["fc1.bias"]), "trx2": F.linear(fr, p["fc2.weight"], p["fc2.bias"])}
    else:
        out = {"distance": dist, "trx": fr}
    return out, idx


def pair_embed(x, w, b, mask=None):
    """x [N,L,D] -> relu(clsW([x_i | x_j])) for the frame pairs i < j in combinations order: [N * T, Hd]"""
    if mask is not None:
        x = x * mask.reshape(x.shape).to(x.dtype)
    N, L, D = x.shape
    rows = torch.stack([torch.cat([x[:, i], x[:, j]], -1) for i, j in combinations(range(L), 2)], 1)
    return _relu(F.linear(rows.reshape(-1, 2 * D), w, b))


def patch_distance(sup, labels, qry, w, b, way, mask=None, sel=None):
    """-> (logits [Nq, way], sel int64 [Nq * T, way]): per class the minimum Euclidean distance of every query pair row to the pair
    rows of the class's support videos (videos ascending, row = member * T + pair), mean over the pairs, negated.  `sel` imposes the
    selection.  mask: [(Ns + Nq) * L, D] dropout mask over support rows, then query rows."""
    Ns, L, D = sup.shape
    Nq = qry.shape[0]
    T = L * (L - 1) // 2
    e = pair_embed(torch.cat([sup, qry], 0), w, b, mask)      # support rows, then query rows: one ReLU site
    es, eq = e[:Ns * T].reshape(Ns, T, -1), e[Ns * T:]
    logits = torch.zeros(Nq, way, dtype=sup.dtype)
    chosen = torch.zeros(Nq * T, way, dtype=torch.long)
    cols = []
    for c in range(way):
        members = torch.nonzero(labels == c).reshape(-1)
        if members.numel() == 0:
            cols.append(logits[:, c])
            continue
        ec = es[members].reshape(-1, es.shape[-1])
        if sel is None:      # difference form, 64 query rows at a time
            with torch.no_grad():
                pick = torch.cat([(eq[i:i + 64].unsqueeze(1) - ec.unsqueeze(0)).pow(2).sum(-1).argmin(dim=1) for i in range(0, eq.shape[0], 64)])
        else:
            pick = sel[:, c].long()
        chosen[:, c] = pick
        diff = eq - ec[pick]
        d2 = diff.pow(2).sum(-1)
        d = torch.where(d2 > 0, torch.sqrt(torch.where(d2 > 0, d2, torch.ones_like(d2))), torch.zeros_like(d2))      # gradient 0 at distance 0
        cols.append(-d.reshape(Nq, T).mean(1))
    return torch.stack(cols, 1), chosen


def min_gaps(sup, labels, qry, w, b, way):
    """relative gap between the two smallest distances of every (query pair row, class): rows with a gap below a threshold have no
    well-defined selection in fp32"""
    Ns, L, D = sup.shape
    T = L * (L - 1) // 2
    es, eq = pair_embed(sup, w, b).reshape(Ns, T, -1), pair_embed(qry, w, b)
    gaps = []
    for c in range(way):
        ec = es[torch.nonzero(labels == c).reshape(-1)].reshape(-1, es.shape[-1])
        d = torch.cat([(eq[i:i + 64].unsqueeze(1) - ec.unsqueeze(0)).pow(2).sum(-1).sqrt() for i in range(0, eq.shape[0], 64)])
        two = torch.topk(d, 2, dim=1, largest=False).values
        gaps.append((two[:, 1] - two[:, 0]) / two[:, 1].clamp_min(1e-30))
    return torch.stack(gaps, 1)


def trx_logits(support, labels, queries, p, way, seq_len=8, pre="transformers."):
    """TemporalCrossTransformer over frame pairs, dropout off (the TRX_2fcsup family's head)"""
    out_dim = p[pre + "k_linear.weight"].shape[0]
    n_q, n_s = queries.shape[0], support.shape[0]
    table = p[pre + "pe.pe"][:, :seq_len].to(support.dtype)
    support, queries = support + table, queries + table
    tuples = [list(c) for c in combinations(range(seq_len), 2)]
    T = len(tuples)
    s = torch.stack([support[:, t, :].reshape(n_s, -1) for t in tuples], dim=-2)
    q = torch.stack([queries[:, t, :].reshape(n_q, -1) for t in tuples], dim=-2)
    s_k = F.layer_norm(F.linear(s, p[pre + "k_linear.weight"], p[pre + "k_linear.bias"]), (out_dim,), p[pre + "norm_k.weight"], p[pre + "norm_k.bias"], 1e-5)
    q_k = F.layer_norm(F.linear(q, p[pre + "k_linear.weight"], p[pre + "k_linear.bias"]), (out_dim,), p[pre + "norm_k.weight"], p[pre + "norm_k.bias"], 1e-5)
    s_v = F.linear(s, p[pre + "v_linear.weight"], p[pre + "v_linear.bias"])
    q_v = F.linear(q, p[pre + "v_linear.weight"], p[pre + "v_linear.bias"])
    cols = []
    for c in range(way):
        idx = torch.nonzero(labels == c).reshape(-1)
        sc = torch.matmul(q_k.unsqueeze(1), s_k[idx].transpose(-2, -1)) / math.sqrt(out_dim)
        sc = torch.softmax(sc.permute(0, 2, 1, 3).reshape(n_q, T, -1), dim=-1).reshape(n_q, T, -1, T).permute(0, 2, 1, 3)
        proto = torch.matmul(sc, s_v[idx]).sum(dim=1)
        cols.append(-(q_v - proto).pow(2).sum(dim=(-2, -1)) / T)
    return torch.stack(cols, 1)


def support_dk(support, way, shot, seq_len=8):
    proto = support.reshape(way, shot, seq_len, -1).mean(dim=1)
    return torch.stack([torch.stack([-(proto[i] - proto[n]).pow(2).sum() / seq_len for n in range(way) if n != i]) for i in range(way)])


def classifier(feats_s, labels, feats_q, p, way, shot, seq_len=8, dist_mask=None, sel=None):
    """the three STRM classifiers: {'pat','fr1','fr2','sup'} for strm18_student features, {'pat','fr'} for strmbackbone's"""
    pat, chosen = patch_distance(feats_s["distance"], labels, feats_q["distance"], p["DistanceLoss.clsW.weight"], p["DistanceLoss.clsW.bias"],
                                 way, dist_mask, sel)
    if "trx" in feats_s:
        return {"pat": pat, "fr": trx_logits(feats_s["trx"], labels, feats_q["trx"], p, way, seq_len)}, chosen
    return {"pat": pat, "fr1": trx_logits(feats_s["trx1"], labels, feats_q["trx1"], p, way, seq_len),
            "fr2": trx_logits(feats_s["trx2"], labels, feats_q["trx2"], p, way, seq_len),
            "sup": support_dk(feats_s["trx2"], way, shot, seq_len)}, chosen


def head(fmap, n_support, labels, bp, cp, way, shot, seq_len=8, backbone="strm18_student", pool_idx=None, masks=None, sel=None):
    """trunk outputs of all frames (support videos first) -> (logits dict, pooling selection, minimum selection)"""
    feats, idx = backbone_head(fmap, bp, seq_len, backbone, pool_idx, masks)
    fs = {k: v[:n_support] for k, v in feats.items()}
    fq = {k: v[n_support:] for k, v in feats.items()}
    logits, chosen = classifier(fs, labels, fq, cp, way, shot, seq_len, (masks or {}).get("dist"), sel)
    return logits, idx, chosen


def fixture_loss(logits):
    """the scalar whose input gradient the fixtures digest: every logit tensor takes part with a different weight"""
    return sum((i + 1) * (v * torch.linspace(0.5, 1.5, v.numel()).reshape(v.shape).to(v)).sum() for i, (k, v) in enumerate(sorted(logits.items())))
