"""Writes tests/golden/conv_plan.json.gz (gzip-compressed JSON): what the convolution plan entry points of liblmkd_hip.so report over
a sweep of shapes, arithmetic modes and dispatch switches.  tests/test_host_cpu.py replays every row against the library under test, so a change to the
host-side dispatch of csrc/conv.hip that changes a kernel choice, a grid or a buffer size shows up as a changed row.

    LMKD_LIB=<path of the library to record> python tools/gen_conv_plan_golden.py [out.json.gz]
    zcat tests/golden/conv_plan.json.gz | python -m json.tool      # to read it: {setting: {shape: [FIELDS values]}}

Pure host code: no GPU is needed.  Every switch is restored to the library default afterwards."""
import ctypes
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "conv_plan.json.gz")

# (name, H (= W), Cs, Cin, Cout, K, stride, pad): the ResNet-18 trunk (tests/test_gpu_fullsize.SHAPES) ...
TRUNK = [
    ("stem7x7", 224, 4, 3, 64, 7, 2, 3),
    ("layer1.3x3", 56, 64, 64, 64, 3, 1, 1),
    ("layer2.0.conv1", 56, 64, 64, 128, 3, 2, 1),
    ("layer2.3x3", 28, 128, 128, 128, 3, 1, 1),
    ("layer2.ds", 56, 64, 64, 128, 1, 2, 0),
    ("layer3.0.conv1", 28, 128, 128, 256, 3, 2, 1),
    ("layer3.3x3", 14, 256, 256, 256, 3, 1, 1),
    ("layer3.ds", 28, 128, 128, 256, 1, 2, 0),
    ("layer4.0.conv1", 14, 256, 256, 512, 3, 2, 1),
    ("layer4.3x3", 7, 512, 512, 512, 3, 1, 1),
    ("layer4.ds", 14, 256, 256, 512, 1, 2, 0),
]
# ... and the distinct convolutions of the ResNet-50 trunk (bottleneck blocks, stride on the 3x3) not among them
RESNET50 = [
    ("r50.l1.reduce64", 56, 64, 64, 64, 1, 1, 0),
    ("r50.l1.expand", 56, 64, 64, 256, 1, 1, 0),
    ("r50.l1.reduce256", 56, 256, 256, 64, 1, 1, 0),
    ("r50.l1.ds", 56, 64, 64, 256, 1, 1, 0),
    ("r50.l2.0.reduce", 56, 256, 256, 128, 1, 1, 0),
    ("r50.l2.0.3x3s2", 56, 128, 128, 128, 3, 2, 1),
    ("r50.l2.expand", 28, 128, 128, 512, 1, 1, 0),
    ("r50.l2.ds", 56, 256, 256, 512, 1, 2, 0),
    ("r50.l2.reduce", 28, 512, 512, 128, 1, 1, 0),
    ("r50.l3.0.reduce", 28, 512, 512, 256, 1, 1, 0),
    ("r50.l3.0.3x3s2", 28, 256, 256, 256, 3, 2, 1),
    ("r50.l3.expand", 14, 256, 256, 1024, 1, 1, 0),
    ("r50.l3.ds", 28, 512, 512, 1024, 1, 2, 0),
    ("r50.l3.reduce", 14, 1024, 1024, 256, 1, 1, 0),
    ("r50.l4.0.reduce", 14, 1024, 1024, 512, 1, 1, 0),
    ("r50.l4.0.3x3s2", 14, 512, 512, 512, 3, 2, 1),
    ("r50.l4.expand", 7, 512, 512, 2048, 1, 1, 0),
    ("r50.l4.ds", 14, 1024, 1024, 2048, 1, 2, 0),
    ("r50.l4.reduce", 7, 2048, 2048, 512, 1, 1, 0),
]
SHAPES = TRUNK + RESNET50
FRAMES = (200, 400)

# library defaults of the dispatch switches, and the values each is flipped to (one at a time)
DEFAULTS = {"patch": 1, "patch16": 1, "s2_patch": 1, "stem_patch": 1, "persistent": 1, "wgrad_planes": 1, "wgrad_win16": 1,
            "wgrad_window": 1, "wgrad_stem": 1, "xcd_mode": -1, "tile": 0}
FLIPS = [("patch", 0), ("patch16", 0), ("patch16", 2), ("s2_patch", 0), ("stem_patch", 0), ("persistent", 0), ("wgrad_planes", 0),
         ("wgrad_win16", 0), ("wgrad_window", 0), ("wgrad_window", 512), ("wgrad_stem", 0), ("xcd_mode", 0), ("xcd_mode", 1)]
# (compute dtype, activation dtype): modes 0 - 4, bf16 tensors with mode 1; and the tile overrides valid in each
MODES = [(0, 0), (1, 0), (1, 1), (2, 0), (3, 0), (4, 0)]


def tiles(mode):
    return list(range(1, 7)) if mode == 0 else (list(range(7, 15)) if mode == 1 else list(range(7, 13)))


def settings():
    for mode, act in MODES:
        yield mode, act, None, None
        for sw, v in FLIPS:
            yield mode, act, sw, v
        for t in tiles(mode):
            yield mode, act, "tile", t


def setting_key(mode, act, sw, v):
    return "mode=%d act=%d%s" % (mode, act, "" if sw is None else " %s=%d" % (sw, v))


def shape_key(shape, n):
    return "%s N=%d" % (shape[0], n)


def apply(L, mode, act, sw, v):
    L.cdll.lmkd_conv_set_compute_dtype(mode)
    L.cdll.lmkd_set_activation_dtype(act)
    for name, d in DEFAULTS.items():
        getattr(L.cdll, "lmkd_conv_set_" + name)(v if name == sw else d)


def restore(L):
    apply(L, 2, 0, None, None)


def record(L, shape, n):
    """-> the flat list of everything the entry points report for one shape at n frames (seg: the frames split in halves)"""
    _, H, Cs, Cin, Cout, K, s, p = shape
    seg = n // 2
    out = []
    info = (ctypes.c_int * 5)()
    for kind in (0, 1, 2):
        L.call("lmkd_conv2d_plan", kind, n, H, H, Cs if kind != 1 else Cin, Cin, Cout, K, K, s, p, info)
        out += list(info)
    t0 = (ctypes.c_int * 1)()
    v = L.cdll
    out.append(v.lmkd_conv2d_fwd_row_tiles(n, H, H, Cout, K, K, s, p))
    out.append(v.lmkd_conv2d_fwd_row_tiles_cs(n, H, H, Cs, Cout, K, K, s, p))
    out.append(v.lmkd_conv2d_fwd_row_tiles_seg(n, H, H, Cs, Cout, K, K, s, p, seg, t0))
    out.append(t0[0])
    out.append(v.lmkd_conv2d_bwd_data_bn_tiles(n, H, H, Cin, Cout, K, K, s, p))
    t0[0] = -1
    out.append(v.lmkd_conv2d_bwd_data_bn_tiles_seg(n, H, H, Cin, Cout, K, K, s, p, seg, t0))
    out.append(t0[0])
    out.append(v.lmkd_conv2d_bwd_weight_workspace(n, H, H, Cs, Cout, K, K, s, p))
    out.append(v.lmkd_conv2d_bwd_weight_workspace_seg(n, H, H, Cs, Cout, K, K, s, p, seg))
    return out


# names of the entries of record()'s list, for failure messages
FIELDS = (["plan%d[%d]" % (k, i) for k in range(3) for i in range(5)] +
          ["fwd_row_tiles", "fwd_row_tiles_cs", "fwd_row_tiles_seg", "fwd_row_tiles_seg.tiles0", "bwd_data_bn_tiles",
           "bwd_data_bn_tiles_seg", "bwd_data_bn_tiles_seg.tiles0", "bwd_weight_workspace", "bwd_weight_workspace_seg"])


def sweep(L):
    res = {}
    try:
        for st in settings():
            apply(L, *st)
            res[setting_key(*st)] = {shape_key(sh, n): record(L, sh, n) for sh in SHAPES for n in FRAMES}
    finally:
        restore(L)
    return res


def main():
    sys.path.insert(0, ROOT)
    import litemkd_amd
    res = sweep(litemkd_amd.lib())
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(path, "wb") as f:
        f.write(gzip.compress(json.dumps(res, separators=(",", ":")).encode(), 9, mtime=0))
    print(path, len(res), "settings")


if __name__ == "__main__":
    main()
