"""STRM classifiers (reference: model/classifiers/strmclassifiers.py:257-288, strmclassifiers_res18.py:257-288,
strm_res18_sup.py:290-325): the patch-distance head on the 'distance' features beside the TRX head(s) the TRX_2fcsup family runs."""
import torch.nn as nn

from ... import ops
from .TRX_2fcsup import SupportDK, TemporalCrossTransformer


class DistanceLoss(nn.Module):
    """strm_res18_sup.py:162-255.  clsW (4096 -> 1024) is evaluated as two per-frame 2048-wide projections (ops.PatchDistFn)."""

    def __init__(self, args, temporal_set_size=2):
        super().__init__()
        if temporal_set_size != 2:
            raise NotImplementedError("only frame pairs (temporal_set_size=2) are on the hot path")
        self.args = args
        self.temporal_set_size = temporal_set_size
        self.p = 0.1
        self.clsW = nn.Linear(self.args.trans_linear_in_dim * temporal_set_size, self.args.trans_linear_in_dim // 2)
        self.tuples_len = self.args.seq_len * (self.args.seq_len - 1) // 2

    def forward(self, support_set, support_labels, queries):
        L, D = self.args.seq_len, self.args.trans_linear_in_dim
        if support_set.shape[1] != L or support_set.shape[2] != D:
            raise RuntimeError("DistanceLoss expects [N,%d,%d] features" % (L, D))
        plan = ops.get_plan(support_labels, self.args.way)
        mask = None
        if self.training:
            seed = 0 if ops.SEED_SLOTS is not None else TemporalCrossTransformer.draw_dropout_seed()
            mask = ops.dropout_mask(((support_set.shape[0] + queries.shape[0]) * L, D), self.p, seed, support_set.device)
            if ops.STRM_TAPS is not None:
                ops.STRM_TAPS.setdefault("dropout", []).append(mask)
        return {"logits": ops.PatchDistFn.apply(support_set, queries, self.clsW.weight, self.clsW.bias, mask, plan)}


def _need(features, keys, who):
    if not isinstance(features, dict) or any(k not in features for k in keys):
        raise NotImplementedError("classifier '%s' reads the feature dict %s of an STRM backbone" % (who, list(keys)))


class strmclassifiers_resnet18(nn.Module):
    """strmclassifiers_res18.py:257-288: {'pat', 'fr'} from a strmbackbone"""

    def __init__(self, args):
        super().__init__()
        self.train()
        self.args = args
        self.transformers = TemporalCrossTransformer(args, 2)
        self.DistanceLoss = DistanceLoss(args, 2)

    def forward(self, context_feature, context_labels, target_feature):
        _need(context_feature, ("distance", "trx"), type(self).__name__)
        pat = self.DistanceLoss(context_feature["distance"], context_labels, target_feature["distance"])["logits"]
        fr = self.transformers(context_feature["trx"], context_labels, target_feature["trx"])["logits"]
        return {"logits": {"pat": pat, "fr": fr}}


class strmclassifiers(strmclassifiers_resnet18):
    """strmclassifiers.py:257-288 (the same head under the ResNet-50 family's name)"""


class strmclassifiers_resnet18_sup(nn.Module):
    """strm_res18_sup.py:290-325: {'pat', 'fr1', 'sup', 'fr2'} from a strm18_student; one TemporalCrossTransformer shared by both heads"""

    def __init__(self, args):
        super().__init__()
        self.train()
        self.args = args
        self.transformers = TemporalCrossTransformer(args, 2)
        self.DistanceLoss = DistanceLoss(args, 2)
        self.SupportDK = SupportDK(args)

    def forward(self, context_feature, context_labels, target_feature):
        _need(context_feature, ("distance", "trx1", "trx2"), type(self).__name__)
        pat = self.DistanceLoss(context_feature["distance"], context_labels, target_feature["distance"])["logits"]
        fr1 = self.transformers(context_feature["trx1"], context_labels, target_feature["trx1"])["logits"]
        fr2 = self.transformers(context_feature["trx2"], context_labels, target_feature["trx2"])["logits"]
        sup = self.SupportDK(context_feature["trx2"], context_labels, target_feature["trx2"])["logits"]
        return {"logits": {"pat": pat, "fr1": fr1, "sup": sup, "fr2": fr2}}
