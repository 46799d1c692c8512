"""MFM hierarchical multi-modal fusion of the teacher (reference: teacher/code/model.py —
TrainablePositionalEncoding :1135-1151, ThreeTransforTemproal :1300-1331, TwoTransforFusion :1361-1392,
ThreeTRXShiftLoopTime.extract_feature :1648-1664).  Inference (eval mode, no grad), which is how the student path
consumes it: rgb / depth / flow ResNet-50 features [N,L,2048] -> fused teacher feature [N,L,2048], L = seq_len <= ops.MFM_MAX_L = 16.

Training (the fusions' `forward`, :1317-1323 / :1376-1385, and ThreeTRXShiftLoopTime.forward :1597-1636): `_Fusion.forward` runs the same
arithmetic with autograd - LayerNorm and attention on the training kernels of csrc/mfm.hip through ops.MfmPosCatFn / MfmAttnFn /
MfmLayerNormFn, the five Linear layers on ops.LinearFn / LinearXFn - and the reference's dropouts as explicit masks.

Parameters live in the same torch containers as the reference (nn.Embedding, nn.LayerNorm,
nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model, nhead, batch_first=True)), nn.Linear) so the state_dict keys
(`three_fusion.transformer_encoder.layers.0.self_attn.in_proj_weight`, `fusion.f1.weight`, ...) match the reference's
checkpoints; the arithmetic runs on the HIP GEMM + LayerNorm + attention kernels (csrc/mfm.hip: one family up to 8 tokens, one up to 16)."""
import ctypes

import torch
import torch.nn as nn

from .. import ops
from .._lib import lib


def layernorm(x, gamma, beta, res=None, res_rows=0, out=None, ldy=None, col_off=0):
    rows, D = x.shape
    if out is None:
        out = torch.empty_like(x)
        ldy = D
    ops._chk(x, gamma, beta, res)
    lib().call("lmkd_layernorm_fwd", ops._p(x), ops._p(res), res_rows, ops._p(gamma), ops._p(beta), ctypes.c_void_p(ops._pw(out) + 4 * col_off), ldy,
               rows, D, ops._f32(1e-5), ops._stream())
    return out


class TrainablePositionalEncoding(nn.Module):
    """model.py:1135-1151: LayerNorm(x + Embedding(position)); dropout is identity at inference."""

    def __init__(self, max_position_embeddings, hidden_size, dropout=0.1):
        super().__init__()
        self.position_embeddings = nn.Embedding(max_position_embeddings, hidden_size)
        self.LayerNorm = nn.LayerNorm(hidden_size)
        self.dropout = nn.Dropout(dropout)

    def into(self, x2d, L, out, ld, col_off):
        """x2d [N*L, D] -> out[:, col_off:col_off+D] (row stride ld)"""
        emb = self.position_embeddings.weight[:L].contiguous()
        return layernorm(x2d, self.LayerNorm.weight, self.LayerNorm.bias, emb, L, out, ld, col_off)


def _encoder_layer(x, layer, L, nhead):
    """nn.TransformerEncoderLayer defaults: post-norm, ReLU, eps 1e-5, batch_first.  x [B*L, D]"""
    M, D = x.shape
    at = layer.self_attn
    # the four Linear layers: ops.linear_infer - the bf16-plane convolution kernels (1x1 convolution + bias / ReLU epilogue) in the
    # library's default arithmetic, the fp32 MFMA GEMM in the native mode
    qkv = ops.linear_infer(x, at.in_proj_weight, at.in_proj_bias)
    ctx = torch.empty_like(x)
    family, _ = ops.mfm_attn_family(L)
    lib().call("lmkd_mha_" + family, ops._p(qkv), ops._p(ctx), M // L, L, D, nhead, ops._stream())
    o = ops.linear_infer(ctx, at.out_proj.weight, at.out_proj.bias)
    x = layernorm(x, layer.norm1.weight, layer.norm1.bias, o, M)
    h = ops.linear_infer(x, layer.linear1.weight, layer.linear1.bias, relu=True)
    f = ops.linear_infer(h, layer.linear2.weight, layer.linear2.bias)
    return layernorm(x, layer.norm2.weight, layer.norm2.bias, f, M)


class _Fusion(nn.Module):
    def __init__(self, args, n_mod, in_channels, dropout):
        super().__init__()
        self.n_mod, self.in_channels = n_mod, in_channels
        for i in range(n_mod):
            setattr(self, "positionEncoding%d" % (i + 1), TrainablePositionalEncoding(args.seq_len, in_channels))
        encoder_layer = nn.TransformerEncoderLayer(d_model=in_channels * n_mod, nhead=n_mod, batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(encoder_layer, num_layers=args.trans_num)
        self.f1 = nn.Linear(in_channels * n_mod, in_channels)
        self.dropout = nn.Dropout(dropout)

    def check_features(self, x):
        """before any kernel runs: x is [N, L <= ops.MFM_MAX_L, in_channels]"""
        if x.dim() != 3 or x.shape[2] != self.in_channels or x.shape[1] > ops.MFM_MAX_L:
            raise ValueError("features %s: the fusion takes [N, L <= %d, %d]" % (tuple(x.shape), ops.MFM_MAX_L, self.in_channels))

    def dropout_shapes(self, N, L):
        """{site: (shape, p)} of every dropout of one forward over N videos of L tokens, in the order their seeds are drawn:
        "pe<i>" after each positional-encoding LayerNorm (model.py:1150), per layer "l<k>.attn" on the attention probabilities,
        "l<k>.dropout1" on the out_proj output, "l<k>.dropout" after the ReLU, "l<k>.dropout2" on the linear2 output (nn.TransformerEncoderLayer),
        "f1" after f1 (:1323 / :1385)"""
        d, D = self.in_channels, self.in_channels * self.n_mod
        sites = {}
        for i in range(self.n_mod):
            sites["pe%d" % (i + 1)] = ((N * L, d), getattr(self, "positionEncoding%d" % (i + 1)).dropout.p)
        for k, layer in enumerate(self.transformer_encoder.layers):
            sites["l%d.attn" % k] = ((N * self.n_mod, L, L), float(layer.self_attn.dropout))
            sites["l%d.dropout1" % k] = ((N * L, D), layer.dropout1.p)
            sites["l%d.dropout" % k] = ((N * L, layer.linear1.out_features), layer.dropout.p)
            sites["l%d.dropout2" % k] = ((N * L, D), layer.dropout2.p)
        sites["f1"] = ((N * L, d), self.dropout.p)
        return sites

    def draw_masks(self, N, L, device):
        """one seed per site and call from torch's default generator, as TemporalCrossTransformer.draw_dropout_seed() draws them"""
        from ..model.classifiers.TRX_2fcsup import TemporalCrossTransformer
        return {site: ops.dropout_mask(shape, p, TemporalCrossTransformer.draw_dropout_seed(), device)
                for site, (shape, p) in self.dropout_shapes(N, L).items() if p > 0.0}

    def forward(self, *mods, masks=None):
        """mods: n_mod tensors [N, L, d] -> fused [N, L, d], with autograd.  masks: {site: mask} over dropout_shapes() (values 0 or
        1/(1-p); a missing site has no dropout); None: in training mode the masks are drawn, in eval mode there is no dropout."""
        if len(mods) != self.n_mod:
            raise ValueError("%d modalities for a fusion of %d" % (len(mods), self.n_mod))
        self.check_features(mods[0])
        N, L, d = mods[0].shape
        if masks is None:
            masks = self.draw_masks(N, L, mods[0].device) if self.training else {}
        else:
            unknown = set(masks) - set(self.dropout_shapes(N, L))
            if unknown:
                raise KeyError("no dropout site %s" % sorted(unknown))
        a = []
        for i, m in enumerate(mods):
            pe = getattr(self, "positionEncoding%d" % (i + 1))
            a += [m.reshape(N * L, d), pe.position_embeddings.weight[:L], pe.LayerNorm.weight, pe.LayerNorm.bias, masks.get("pe%d" % (i + 1))]
        h = ops.MfmPosCatFn.apply(L, *a)
        for k, layer in enumerate(self.transformer_encoder.layers):
            pre = "l%d." % k
            h = ops.mfm_encoder_layer_train(h, layer, L, self.n_mod, {s: masks.get(pre + s) for s in ops.MFM_LAYER_SITES})
        out = ops.feature_dropout(ops.LinearFn.apply(h, self.f1.weight, self.f1.bias, ops.MFM_K_BLOCK), masks.get("f1"))
        return out.reshape(N, L, d)

    @torch.no_grad()
    def extract_feature(self, *mods):
        if self.training:
            raise NotImplementedError("the MFM fusion is on the hot path as a frozen feature extractor: call .eval()")
        self.check_features(mods[0])
        N, L, d = mods[0].shape
        D = d * self.n_mod
        cat = torch.empty((N * L, D), dtype=torch.float32, device=mods[0].device)
        for i, m in enumerate(mods):
            getattr(self, "positionEncoding%d" % (i + 1)).into(m.reshape(N * L, d).contiguous(), L, cat, D, i * d)
        h = cat
        for layer in self.transformer_encoder.layers:
            h = _encoder_layer(h, layer, L, self.n_mod)
        return ops.linear_infer(h, self.f1.weight, self.f1.bias).reshape(N, L, d)


class ThreeTransforTemproal(_Fusion):
    """model.py:1300-1331 (d_model 6144, 3 heads)."""

    def __init__(self, args, out_channels=None, dropout=0.1, in_channels=2048):
        super().__init__(args, 3, in_channels, dropout)


class TwoTransforFusion(_Fusion):
    """model.py:1361-1392 (d_model 4096, 2 heads)."""

    def __init__(self, args, out_channels=None, dropout=0.1, in_channels=2048):
        super().__init__(args, 2, in_channels, dropout)


class TrxBranch(nn.Module):
    """model.py:1094-1128: one TemporalCrossTransformer per entry of args.temp_set, logits averaged"""

    def __init__(self, args):
        super().__init__()
        from ..model.classifiers.TRX_2fcsup import TemporalCrossTransformer, temp_set_of
        self.transformers = nn.ModuleList([TemporalCrossTransformer(args, s) for s in temp_set_of(args)])

    def forward(self, context_features, target_features, context_labels):
        from ..model.classifiers.TRX_2fcsup import head_logits
        for t in self.transformers:      # the head's 2048- and 1152-term sums in blocks, like the fusions' 
            t.gemm_k_block = ops.MFM_K_BLOCK
        return {"logits": head_logits(self.transformers, context_features, context_labels, target_features)}


class ThreeTRXShiftLoopTime(nn.Module):
    """model.py:1588-1664.  The student path uses `three_fusion`, `fusion` and `extract_feature` (there `bracnch`, the teacher's own
    TRX head, is the TRX_2fcsup_fixed classifier of model_select).  head=True adds `bracnch` (keys `bracnch.transformers.<i>.*`) and with
    it `forward`, the teacher's training forward."""

    def __init__(self, args, in_channels=2048, head=False):
        super().__init__()
        self.args = args
        if head:
            if in_channels != 2048:
                raise ValueError("head=True: the TRX head reads features of width 2048, not in_channels = %d" % in_channels)
            self.bracnch = TrxBranch(args)
        self.fusion = TwoTransforFusion(args, in_channels=in_channels)
        self.three_fusion = ThreeTransforTemproal(args, in_channels=in_channels)

    def forward(self, context_features, context_labels, target_features):
        """model.py:1597-1636: dicts keyed by args.m1 / m2 / m3 -> {"logits": [Nq, way]}.  As there, the second modality is rolled by
        shirt_num for its fusion with the first, and the third is not: cat(x[:, :s], x[:, s:]) (:1613-1619) is x itself.  Every
        operation of the fusions is per video, so support and query videos share one call per fusion use; the shared `fusion`
        module is used twice and autograd sums its gradients."""
        if not hasattr(self, "bracnch"):
            raise RuntimeError("ThreeTRXShiftLoopTime.forward needs the TRX head: construct with head=True")
        a = self.args
        L, d, s = a.seq_len, self.three_fusion.in_channels, a.shirt_num
        c = [context_features[m].reshape(-1, L, d) for m in (a.m1, a.m2, a.m3)]
        t = [target_features[m].reshape(-1, L, d) for m in (a.m1, a.m2, a.m3)]
        ns = c[0].shape[0]
        first, second, third = (torch.cat((ci, ti), dim=0) for ci, ti in zip(c, t))
        second_shuffle = torch.cat((second[:, s:], second[:, :s]), dim=1)
        fused = ops.SumFn.apply(self.three_fusion(first, second, third), self.fusion(first, second_shuffle), self.fusion(first, third))
        return self.bracnch(fused[:ns], fused[ns:], context_labels)

    @torch.no_grad()
    def extract_feature(self, feature):
        L, d = self.args.seq_len, self.three_fusion.in_channels
        rgb = feature["rgb"].reshape(-1, L, d)
        depth = feature["depth"].reshape(-1, L, d)
        flow = feature["flow"].reshape(-1, L, d)
        s = self.args.shirt_num
        out = self.three_fusion.extract_feature(rgb, depth, flow)
        f2 = self.fusion.extract_feature(rgb, torch.cat((depth[:, s:], depth[:, :s]), dim=1).contiguous())
        f3 = self.fusion.extract_feature(rgb, torch.cat((flow[:, s:], flow[:, :s]), dim=1).contiguous())
        for f in (f2, f3):
            lib().call("lmkd_axpby", ops._p(f), ops._p(out), ops._f32(1.0), ops._f32(1.0), out.numel(), ops._stream())
        return out
