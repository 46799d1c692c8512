"""OTAM matcher head (reference: teacher/code/model.py:3260-3343 - cos_sim, OTAM_cum_dist, CNN_OTAM; the head of
OTAMThreeTRXShiftLoopTime on the fused teacher feature): frames matched in order by a soft dynamic-time alignment, no parameters."""
import torch
import torch.nn as nn

from ... import ops


class OTAM(nn.Module):
    """CNN_OTAM.forward (:3319-3343) on [N, seq_len, D] features -> {'logits': [Nq, way]}: as in the reference the "logits" are the
    softmax of the negated class distances.  Every class 0 .. way-1 needs a support video (ValueError otherwise: the reference returns a
    narrower tensor); non-finite features propagate (the reference's zeros of width 5 on NaN input are not reproduced)."""

    def __init__(self, args):
        super().__init__()
        self.train()
        self.args = args

    def forward(self, context_feature, context_labels, target_feature):
        if isinstance(context_feature, dict) or isinstance(target_feature, dict):
            raise NotImplementedError("classifier '%s' reads plain [N, seq_len, D] features, not the feature dict %s of a two-head or STRM backbone"
                                      % (type(self).__name__, sorted(context_feature) if isinstance(context_feature, dict) else sorted(target_feature)))
        D = context_feature.shape[-1]
        supports = context_feature.reshape(-1, self.args.seq_len, D)
        queries = target_feature.reshape(-1, self.args.seq_len, D)
        plan = ops.get_plan(context_labels, self.args.way)
        ops.otam_plan_check(plan)
        return {"logits": ops.OtamFn.apply(supports, queries, plan)[0]}


class OTAM_fixed(OTAM):
    """the same head on teacher features: nothing flows back"""

    def forward(self, context_feature, context_labels, target_feature):
        with torch.no_grad():
            return super().forward(context_feature, context_labels, target_feature)
