"""MobileNetV3-Large student backbones (reference: model/backbone/moblienetv3.py): mobile_large_2fc (`moblienetv3_fc2`, two
960 -> 2048 heads) and mobile_large (`moblienetv3`, one head).

The trunk is torchvision's mobilenet_v3_large().features, restated here (torchvision is not a dependency): `self.mobile` =
nn.Sequential(features), so state_dict keys read `mobile.0.<i>.…` exactly like the reference's
nn.Sequential(*list(mobilenet_v3_large().children())[:-2]).  The reference starts from the ImageNet weights (pretrained=True, a
download); here the modules are initialised as torchvision initialises them, and load_torchvision_features() takes a torchvision
state_dict from disk.  It never fetches anything."""
import torch
import torch.nn as nn

from ... import ops
from .resnet import Linear

# (in, kernel, expanded, out, squeeze-excitation, activation, stride) of features.1 .. 15 (torchvision _mobilenet_v3_conf("mobilenet_v3_large"))
LARGE_BLOCKS = [
    (16, 3, 16, 16, False, "RE", 1),
    (16, 3, 64, 24, False, "RE", 2),
    (24, 3, 72, 24, False, "RE", 1),
    (24, 5, 72, 40, True, "RE", 2),
    (40, 5, 120, 40, True, "RE", 1),
    (40, 5, 120, 40, True, "RE", 1),
    (40, 3, 240, 80, False, "HS", 2),
    (80, 3, 200, 80, False, "HS", 1),
    (80, 3, 184, 80, False, "HS", 1),
    (80, 3, 184, 80, False, "HS", 1),
    (80, 3, 480, 112, True, "HS", 1),
    (112, 3, 672, 112, True, "HS", 1),
    (112, 5, 672, 160, True, "HS", 2),
    (160, 5, 960, 160, True, "HS", 1),
    (160, 5, 960, 160, True, "HS", 1),
]
LAST_CHANNELS = 960
_ACT = {"RE": ops.ACT_RELU, "HS": ops.ACT_HARDSWISH, None: ops.ACT_NONE}


def make_divisible(v, divisor=8, min_value=None):
    """torchvision's _make_divisible: the squeeze width of SqueezeExcitation(C, _make_divisible(C // 4, 8))"""
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def _conv_weight(cout, cin, k):
    w = torch.empty(cout, cin, k, k)
    nn.init.kaiming_normal_(w, mode="fan_out")      # torchvision MobileNetV3.__init__
    return nn.Parameter(w)


class _Conv(nn.Module):
    """nn.Conv2d parameters (no bias) of a Conv2dNormActivation: key `weight`"""

    def __init__(self, cin, cout, k, groups=1):
        super().__init__()
        self.weight = _conv_weight(cout, cin // groups, k)


class _SEConv(nn.Module):
    """the 1x1 nn.Conv2d (with bias) of SqueezeExcitation.fc1 / fc2"""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = _conv_weight(cout, cin, 1)
        self.bias = nn.Parameter(torch.zeros(cout))


class _BN(nn.Module):
    """nn.BatchNorm2d(eps=0.001, momentum=0.01) parameters and buffers"""

    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    def args(self):
        return self.weight, self.bias, self.running_mean, self.running_var, self.num_batches_tracked


class ConvBNAct(nn.Sequential):
    """Conv2dNormActivation: children `0` (conv) and `1` (BatchNorm); the activation has no parameters.
    kind 'stem' (features.0), 'pw' (1x1) or 'dw' (depthwise)."""

    def __init__(self, cin, cout, k, stride, kind, act):
        super().__init__()
        self.add_module("0", _Conv(cin, cout, k, groups=cin if kind == "dw" else 1))
        self.add_module("1", _BN(cout))
        self.kind, self.k, self.stride, self.act = kind, k, stride, _ACT[act]

    def forward(self, x, updates=None, res=None):
        conv, bn = getattr(self, "0"), getattr(self, "1")
        if self.kind == "stem":
            return ops.MnvStemFn.apply(x, conv.weight, *bn.args(), self.training, updates)
        return ops.MnvConvBNActFn.apply(x, conv.weight, *bn.args(), res, (self.kind, self.k, self.stride, self.act), self.training, updates)


class SqueezeExcitation(nn.Module):
    def __init__(self, c, squeeze):
        super().__init__()
        self.fc1 = _SEConv(c, squeeze)
        self.fc2 = _SEConv(squeeze, c)

    def forward(self, x):
        return ops.MnvSEFn.apply(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias)


class InvertedResidual(nn.Module):
    """torchvision InvertedResidual: `block` = [expand 1x1] + depthwise + [SE] + project 1x1 (no activation), + x when stride 1 and in == out"""

    def __init__(self, cin, k, exp, cout, se, act, stride):
        super().__init__()
        layers = []
        if exp != cin:
            layers.append(ConvBNAct(cin, exp, 1, 1, "pw", act))
        layers.append(ConvBNAct(exp, exp, k, stride, "dw", act))
        if se:
            layers.append(SqueezeExcitation(exp, make_divisible(exp // 4, 8)))
        layers.append(ConvBNAct(exp, cout, 1, 1, "pw", None))
        self.block = nn.Sequential(*layers)
        self.use_res = stride == 1 and cin == cout

    def forward(self, x, updates=None):
        y = x
        mods = list(self.block)
        for m in mods[:-1]:
            y = m(y) if isinstance(m, SqueezeExcitation) else m(y, updates)
        return mods[-1](y, updates, res=x if self.use_res else None)


class MobileNetV3LargeFeatures(nn.Sequential):
    """torchvision mobilenet_v3_large().features: NHWC4 frames [F, H, W, 4] -> [F, H/32, W/32, 960] (7 x 7 at 224)"""

    def __init__(self):
        super().__init__()
        self.add_module("0", ConvBNAct(3, 16, 3, 2, "stem", "HS"))
        for i, cfg in enumerate(LARGE_BLOCKS):
            self.add_module(str(i + 1), InvertedResidual(*cfg))
        self.add_module(str(len(LARGE_BLOCKS) + 1), ConvBNAct(LARGE_BLOCKS[-1][3], 6 * LARGE_BLOCKS[-1][3], 1, 1, "pw", "HS"))

    def forward(self, x, updates=None):
        for m in self:
            x = m(x, updates)
        return x


def features_two_calls(mobile, context_frames, target_frames):
    """the reference's two trunk calls (moblienetv3.py:38-39): support frames, then query frames, each with its own train-mode BatchNorm
    batch; the running statistics are updated in that order, both calls' updates in one launch after the second call.
    -> pooled [F, 960] features of both calls (AdaptiveMaxPool2d((4, 4)) + mean over the 16 patches, :41-52)."""
    feats = getattr(mobile, "0")
    training = feats.training
    upd_s, upd_q = ([], []) if training else (None, None)
    cf = ops.pool_head(feats(context_frames, upd_s))
    tf = ops.pool_head(feats(target_frames, upd_q))
    if training:
        ops.mnv3_running_update(upd_s, upd_q)
    return cf, tf


def load_torchvision_features(backbone, state_dict):
    """copy the `features.*` entries of a torchvision mobilenet_v3_large state_dict (e.g. torch.load of the ImageNet weights file
    on local disk) into backbone.mobile.0.*; the classifier entries are ignored.  Every trunk tensor must be present with its shape."""
    if "state_dict" in state_dict and isinstance(state_dict["state_dict"], dict):
        state_dict = state_dict["state_dict"]
    own = {k: v for k, v in backbone.state_dict().items() if k.startswith("mobile.0.")}
    mapped = {"mobile.0." + k[len("features."):]: v for k, v in state_dict.items() if k.startswith("features.")}
    missing = sorted(set(own) - set(mapped))
    unexpected = sorted(set(mapped) - set(own))
    if missing or unexpected:
        raise KeyError("not a torchvision mobilenet_v3_large state_dict: missing %s, unexpected %s" % (missing[:5], unexpected[:5]))
    with torch.no_grad():
        for k, v in mapped.items():
            if tuple(own[k].shape) != tuple(v.shape):
                raise ValueError("%s: shape %s, expected %s" % (k, tuple(v.shape), tuple(own[k].shape)))
            own[k].copy_(v)
    return backbone


class _MobileBase(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.args.trans_linear_in_dim = 2048          # moblienetv3.py:25
        self.num_patches = 16
        self.mobile = nn.Sequential(MobileNetV3LargeFeatures())

    def load_torchvision(self, path_or_state_dict):
        """start from torchvision ImageNet weights on disk (the reference's pretrained=True, without the download)"""
        sd = path_or_state_dict
        if not isinstance(sd, dict):
            sd = torch.load(sd, map_location="cpu")
        return load_torchvision_features(self, sd)

    def distribute_model(self):
        """The reference wraps a nonexistent self.resnet in nn.DataParallel (moblienetv3.py:81-86).  Multi-GPU here is episode-parallel
        (parallel.py): a no-op.  parallel.EarlyAllReduce finds no `backbone.resnet.7.` parameters in this backbone and falls back to one
        all-reduce at the optimizer step, which is correct."""
        return None


class mobile_large_2fc(_MobileBase):
    def __init__(self, args):
        super().__init__(args)
        self.fc1 = Linear(LAST_CHANNELS, 2048)
        self.fc2 = Linear(LAST_CHANNELS, 2048)

    def forward(self, context_feature, context_labels, target_feature):
        cf, tf = features_two_calls(self.mobile, context_feature, target_feature)
        L, D = self.args.seq_len, self.args.trans_linear_in_dim
        c1, t1, c2, t2 = ops.two_head_linear_x(ops.stack_rows(cf, tf), cf.shape[0], self.fc1, self.fc2)      # :54-64
        context_feature_dict = {"context_features_1": c1.reshape(-1, L, D), "context_features_2": c2.reshape(-1, L, D)}
        target_features_dict = {"target_features_1": t1.reshape(-1, L, D), "target_features_2": t2.reshape(-1, L, D)}
        return context_feature_dict, target_features_dict


class mobile_large(_MobileBase):
    def __init__(self, args):
        super().__init__(args)
        self.fc = Linear(LAST_CHANNELS, 2048)

    def forward(self, context_feature, context_labels, target_feature):
        cf, tf = features_two_calls(self.mobile, context_feature, target_feature)
        L, D = self.args.seq_len, self.args.trans_linear_in_dim
        return self.fc(cf).reshape(-1, L, D), self.fc(tf).reshape(-1, L, D)      # :118-124
