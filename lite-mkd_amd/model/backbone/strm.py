"""STRM student backbones (reference: model/backbone/strm18_student.py:207-310, strmbackbone.py:207-310): ResNet-18 trunk, the 16
max-pooled patches of every frame through patch attention (Self_Attn_Bot), mean over the patches, res18_2048, frame mixing
(MLP_Mix_Enrich).  Attribute names reproduce the reference's, so state_dict keys match its checkpoints key for key.

The head runs ONCE over the support and the query frames: every operator in it is per frame or per video, so the result is
bit-identical to the reference's two calls (tests/test_gpu_strm.py)."""
import torch
import torch.nn as nn

from ... import ops
from ..classifiers.TRX_2fcsup import PositionalEncoding, TemporalCrossTransformer
from .resnet import Linear, ResNet18Trunk, trunk_features


def _dropout_mask(module, pe, shape, device):
    """mask of a PositionalEncoding's nn.Dropout (train mode), drawn like the TRX heads' (capturable: ops.SEED_SLOTS)"""
    if not module.training or pe.p <= 0.0:
        return None
    seed = 0 if ops.SEED_SLOTS is not None else TemporalCrossTransformer.draw_dropout_seed()
    mask = ops.dropout_mask(shape, pe.p, seed, device)
    if ops.STRM_TAPS is not None:
        ops.STRM_TAPS.setdefault("dropout", []).append(mask)
    return mask


class Bottleneck_Perceptron_3_layer_res(nn.Module):
    """strm18_student.py:82-99: in -> in/2 -> in/2 -> in, ReLU between, residual"""

    def __init__(self, in_dim):
        super().__init__()
        self.inp_fc = nn.Linear(in_dim, in_dim // 2)
        self.hid_fc = nn.Linear(in_dim // 2, in_dim // 2)
        self.out_fc = nn.Linear(in_dim // 2, in_dim)

    def forward(self, x, seg=0):
        h = ops.LinearXFn.apply(x, self.inp_fc.weight, self.inp_fc.bias, True, None, seg)
        h = ops.LinearXFn.apply(h, self.hid_fc.weight, self.hid_fc.bias, True, None, seg)
        return ops.LinearXFn.apply(h, self.out_fc.weight, self.out_fc.bias, False, x, seg)


class Bottleneck_Perceptron_2_layer(nn.Module):
    """strm18_student.py:65-80; the caller's residual (:200) rides in the second GEMM"""

    def __init__(self, in_dim):
        super().__init__()
        self.inp_fc = nn.Linear(in_dim, in_dim)
        self.out_fc = nn.Linear(in_dim, in_dim)

    def forward(self, x, seg=0):
        h = ops.LinearXFn.apply(x, self.inp_fc.weight, self.inp_fc.bias, True, None, seg)
        return ops.LinearXFn.apply(h, self.out_fc.weight, self.out_fc.bias, False, x, seg)


class Token_Perceptron(nn.Module):
    """strm18_student.py:41-63: parameters only; evaluated inside ops.TokenMLPFn"""

    def __init__(self, in_dim):
        super().__init__()
        self.inp_fc = nn.Linear(in_dim, in_dim)
        self.out_fc = nn.Linear(in_dim, in_dim)


class Self_Attn_Bot(nn.Module):
    """strm18_student.py:101-166.  forward takes the patches with the table and dropout already applied (ops.PatchPoolFn)."""

    def __init__(self, in_dim, seq_len):
        super().__init__()
        self.chanel_in = in_dim
        self.key_proj = nn.Linear(in_dim, in_dim)
        self.query_proj = nn.Linear(in_dim, in_dim)
        self.value_conv = nn.Linear(in_dim, in_dim)
        self.gamma = nn.Parameter(torch.zeros(1))
        self.Bot_MLP = Bottleneck_Perceptron_3_layer_res(in_dim)
        self.pe = PositionalEncoding(in_dim, 0.1, int(seq_len * 1.5))

    def forward(self, xp, seg=0):
        """seg: number of support frames when xp holds both trunk calls (ops._row_segments)"""
        F_, NP, C = xp.shape
        y = ops.PatchAttnFn.apply(xp, self.query_proj.weight, self.query_proj.bias, self.key_proj.weight, self.key_proj.bias,
                                  self.value_conv.weight, self.value_conv.bias, self.gamma)
        return self.Bot_MLP(y.view(F_ * NP, C), seg * NP).view(F_, NP, C)


class MLP_Mix_Enrich(nn.Module):
    """strm18_student.py:168-202"""

    def __init__(self, in_dim, seq_len):
        super().__init__()
        self.Tok_MLP = Token_Perceptron(seq_len)
        self.Bot_MLP = Bottleneck_Perceptron_2_layer(in_dim)
        self.pe = PositionalEncoding(in_dim, 0.1, int(seq_len * 1.5))

    def forward(self, x, seg=0):
        """seg: number of support videos when x holds both trunk calls"""
        V, L, D = x.shape
        mask = _dropout_mask(self, self.pe, (V * L, D), x.device)
        t = self.Tok_MLP
        y = ops.TokenMLPFn.apply(x, self.pe.pe[0, :L].contiguous(), mask, t.inp_fc.weight, t.inp_fc.bias, t.out_fc.weight, t.out_fc.bias)
        return self.Bot_MLP(y.view(V * L, D), seg * L).view(V, L, D)


class _StrmBase(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.args.trans_linear_in_dim = 2048          # strm18_student.py:218
        self.num_patches = 16
        self.attn_pat = Self_Attn_Bot(512, self.num_patches)
        self.fr_enrich = MLP_Mix_Enrich(self.args.trans_linear_in_dim, self.args.seq_len)
        self.resnet = ResNet18Trunk()
        self.res18_2048 = Linear(512, 2048)

    def features(self, context_frames, target_frames):
        """-> (distance features [V,L,2048] (:263-267), frame-mixed features [V,L,2048] (:269-270), Ns): support videos first"""
        if ops.get_activation_dtype() != "fp32":
            raise RuntimeError("the STRM backbones run fp32 activations only; set_activation_dtype('%s') is not supported for them"
                               % ops.get_activation_dtype())
        a = self.attn_pat
        L, D = self.args.seq_len, self.args.trans_linear_in_dim
        F_ = context_frames.shape[0] + target_frames.shape[0]
        pe = a.pe.pe[0, :self.num_patches].contiguous()
        # one mask for all frames, drawn before the trunk is queued; the pooling launch of each trunk call takes its rows
        mask = _dropout_mask(a, a.pe, (F_, self.num_patches, 512), context_frames.device)
        if mask is not None and context_frames.is_cuda and ops.SEED_SLOTS is None:      # (a capture keeps its tensors for the graph's lifetime)
            mask.record_stream(ops.side_stream(context_frames.device))
        at = [0]

        def pool(y):
            m = None
            if mask is not None:
                m = mask[at[0]:at[0] + y.shape[0]]
            at[0] += y.shape[0]
            return ops.PatchPoolFn.apply(y, pe, m).flatten(1)

        X, Fs = trunk_features(self.resnet, pool, context_frames, target_frames)
        xp = X.view(F_, self.num_patches, 512)
        pooled = ops.PatchMeanFn.apply(a(xp, Fs))              # :254-255
        r = self.res18_2048
        dist = ops.LinearXFn.apply(pooled, r.weight, r.bias, False, None, Fs).view(F_ // L, L, D)      # :258-264
        return dist, self.fr_enrich(dist, Fs // L), Fs // L

    def distribute_model(self):
        """The reference wraps self.resnet in nn.DataParallel (strm18_student.py:304-310).  Multi-GPU here is episode-parallel
        (parallel.py): a no-op."""
        return None


class strm18_student(_StrmBase):
    """strm18_student.py:207-302: fc1 / fc2 on the frame-mixed features -> {'distance', 'trx1', 'trx2'}"""

    def __init__(self, args):
        super().__init__(args)
        self.fc1 = Linear(2048, 2048)
        self.fc2 = Linear(2048, 2048)

    def forward(self, context_feature, context_labels, target_feature):
        dist, fr, Ns = self.features(context_feature, target_feature)
        V, L, D = fr.shape
        x = fr.view(V * L, D)
        y1 = ops.LinearXFn.apply(x, self.fc1.weight, self.fc1.bias, False, None, Ns * L).view(V, L, D)      # :272-276
        y2 = ops.LinearXFn.apply(x, self.fc2.weight, self.fc2.bias, False, None, Ns * L).view(V, L, D)
        return ({"distance": dist[:Ns], "trx1": y1[:Ns], "trx2": y2[:Ns]}, {"distance": dist[Ns:], "trx1": y1[Ns:], "trx2": y2[Ns:]})


class strmbackbone(_StrmBase):
    """strmbackbone.py:207-298: the frame-mixed features are 'trx'; fc1 / fc2 (512 -> 2048) are parameters the forward never uses
    (:232-233), kept for the state_dict"""

    def __init__(self, args):
        super().__init__(args)
        self.fc1 = Linear(512, 2048)
        self.fc2 = Linear(512, 2048)

    def forward(self, context_feature, context_labels, target_feature):
        dist, fr, Ns = self.features(context_feature, target_feature)
        return {"distance": dist[:Ns], "trx": fr[:Ns]}, {"distance": dist[Ns:], "trx": fr[Ns:]}
