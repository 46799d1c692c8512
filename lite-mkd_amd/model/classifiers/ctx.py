"""CTX matcher head (reference: teacher/code/model.py:2840-2936 CrossTransformer, :3045-3081 CTXBranch - the head TwoCTXShuffleTime
puts on the fused teacher feature): the frame-level cross-transformer.  Every query frame attends over all support frames of a class;
the logit is the negated squared distance between the query's value rows and that prototype, over seq_len."""
import torch
import torch.nn as nn

from ... import ops
from .TRX_2fcsup import PositionalEncoding, TemporalCrossTransformer


class CrossTransformer(nn.Module):
    """model.py:2840-2924.  Standard containers, so the state_dict keys (pe.pe, k_linear.*, v_linear.*, norm_k.*, norm_v.*) and the
    default initialisation are the reference's; norm_v is never applied (:2881-2882), as there."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.pe = PositionalEncoding(2048, self.args.trans_dropout, max_len=int(self.args.seq_len * 1.5))
        self.k_linear = nn.Linear(2048, self.args.trans_linear_out_dim)
        self.v_linear = nn.Linear(2048, self.args.trans_linear_out_dim)
        self.norm_k = nn.LayerNorm(self.args.trans_linear_out_dim)
        self.norm_v = nn.LayerNorm(self.args.trans_linear_out_dim)

    def _mask(self, n_rows, width, device):
        """one seed per call, drawn exactly as TemporalCrossTransformer._mask draws it (none while a hipGraph capture fills ops.SEED_SLOTS)"""
        p = self.pe.p
        if not self.training or p <= 0.0:
            return None
        seed = 0 if ops.SEED_SLOTS is not None else TemporalCrossTransformer.draw_dropout_seed()
        return ops.dropout_mask((n_rows, width), p, seed, device)

    def forward(self, support_set, support_labels, queries):
        L = self.args.seq_len
        Din = self.k_linear.weight.shape[1]
        if support_set.dim() != 3 or support_set.shape[1] != L or support_set.shape[2] != Din or queries.shape[1:] != support_set.shape[1:]:
            raise RuntimeError("CrossTransformer expects [N,%d,%d] features" % (L, Din))
        plan = ops.get_plan(support_labels, self.args.way)
        pe = self.pe.pe[0, :L, :Din].contiguous()
        mask = self._mask((support_set.shape[0] + queries.shape[0]) * L, Din, support_set.device)
        a = (self.k_linear.weight, self.k_linear.bias, self.v_linear.weight, self.v_linear.bias, self.norm_k.weight, self.norm_k.bias, pe, mask)
        if torch.is_grad_enabled() and (support_set.requires_grad or self.k_linear.weight.requires_grad):
            return {"logits": ops.CtxLogitsFn.apply(support_set, queries, *a, plan)}
        return {"logits": ops.ctx_logits_nograd(support_set, queries, plan, *a)}


class CTX(nn.Module):
    """CTXBranch (:3045-3081) on [N, seq_len, D] features (or their flattened [N * seq_len, D] form) -> {'logits': [Nq, way]};
    keys `transformers.*`.  A class in [0, way) without a support video keeps logit 0, as the reference's torch.zeros does."""

    def __init__(self, args):
        super().__init__()
        self.train()
        self.args = args
        self.transformers = CrossTransformer(args)

    def forward(self, context_feature, context_labels, target_feature):
        if isinstance(context_feature, dict) or isinstance(target_feature, dict):
            raise NotImplementedError("classifier '%s' reads plain [N, seq_len, D] features, not the feature dict %s of a two-head or STRM backbone"
                                      % (type(self).__name__, sorted(context_feature) if isinstance(context_feature, dict) else sorted(target_feature)))
        D = context_feature.shape[-1]
        supports = context_feature.reshape(-1, self.args.seq_len, D)
        queries = target_feature.reshape(-1, self.args.seq_len, D)
        return {"logits": self.transformers(supports, context_labels, queries)["logits"]}


class CTX_fixed(CTX):
    """the same head as a frozen teacher: nothing flows back"""

    def forward(self, context_feature, context_labels, target_feature):
        with torch.no_grad():
            return super().forward(context_feature, context_labels, target_feature)
