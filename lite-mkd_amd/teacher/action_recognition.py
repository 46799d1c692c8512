"""The per-modality feature extractor of the teacher (reference: teacher/code/model.py:3345-3371 Action_Recognition_Resnet50): a
torchvision ResNet-50 up to and including its global average pool (`convnet`) and `fc = Linear(2048, num_classes)`, trained as a clip
classifier by litemkd_amd.pretrain and read out frame by frame by litemkd_amd.extract.

State-dict keys: `convnet.<i>.*` and `fc.*` - those of the reference's nn.Sequential(*children[:-1]): ResNet50Trunk numbers its children
like that Sequential (0 conv1, 1 bn1, 4..7 layer1..4) and the pool (child 8 there) holds no parameters, so a checkpoint loads with
strict=True in both directions.

The pool is lmkd_global_avgpool (ops.GlobalAvgPoolFn): per frame for extract_feature, over a whole clip for forward - the mean over a
clip's frames of per-frame means over equal H*W is the mean over T*H*W positions, one pass.  fc runs on the MFMA GEMM (ops.LinearFn);
the GEMM reads rows of 4 floats, so a class count that is no multiple of 4 is computed with zero rows appended to the weight and the
extra logits dropped (the parameters keep the reference's shapes)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..model.backbone.resnet import ResNet50Trunk

_TV_CHILD = {"conv1": "0", "bn1": "1", "layer1": "4", "layer2": "5", "layer3": "6", "layer4": "7"}


def map_torchvision_keys(sd):
    """the state dict of a torchvision resnet50 -> the keys of `convnet` (conv1 -> 0, bn1 -> 1, layer1..4 -> 4..7); fc.* is dropped"""
    out = {}
    for k, v in sd.items():
        head, _, rest = k.partition(".")
        if head == "fc":
            continue
        if head not in _TV_CHILD:
            raise KeyError("not a torchvision resnet50 key: %s" % k)
        out[_TV_CHILD[head] + "." + rest] = v
    return out


class Action_Recognition_Resnet50(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.convnet = ResNet50Trunk()
        self.fc = nn.Linear(2048, args.num_classes)

    def load_torchvision_resnet50(self, path):
        """what the reference's `pretrained=True` downloads, from a file: a torchvision resnet50 state dict onto convnet.*"""
        sd = torch.load(path, map_location="cpu")
        if isinstance(sd, dict) and "state_dict" in sd:
            sd = sd["state_dict"]
        with torch.no_grad():
            self.convnet.load_state_dict(map_torchvision_keys(sd), strict=True)
        ops.WEIGHT_EPOCH[0] += 1

    def _classify(self, feature):
        n = self.args.num_classes
        pad = -n % 4
        if not pad:
            return ops.LinearFn.apply(feature, self.fc.weight, self.fc.bias)
        w = F.pad(self.fc.weight, (0, 0, 0, pad))
        b = F.pad(self.fc.bias, (0, pad))
        return ops.LinearFn.apply(feature, w, b)[:, :n]

    def forward(self, x):
        """x: [B, T, 3, H, W], or [B, T, H, W, 4] (the frame transform's NHWC4) -> logits [B, num_classes]"""
        b, t = x.shape[:2]
        fm = self.convnet(x.reshape((b * t,) + tuple(x.shape[2:])).contiguous())
        return self._classify(ops.GlobalAvgPoolFn.apply(fm, t))

    @torch.no_grad()
    def extract_feature(self, x):
        """x: [T, 3, H, W] or NHWC4 [T, H, W, 4] -> [T, 2048].  In eval mode the frames are independent (BatchNorm uses its running
        statistics), so the frames of several videos may share one call."""
        return ops.GlobalAvgPoolFn.apply(self.convnet(x.contiguous()), 1)

    def distribute_model(self):
        return None
