"""The 19 distinct convolutions of the ResNet-50 trunk at 224 x 224 (tools/gen_conv_plan_golden.RESNET50) at frame counts a test can
afford, and what keeps them on the kernels the 200-frame trunk call of the benchmark runs.  One table for the GPU test that launches
them (tests/test_gpu_resnet50.py) and the host test that guards it (tests/test_host_cpu.py).

Frames by OUTPUT map size: the fewest that still leave several row tiles of 128 and a ragged last one.  At these counts the automatic
tile choice of the forward / data gradient differs from the 200-frame one (pick_conv_cfg takes 128 x 128 only from 1024 tiles on), so
the tile is pinned (lmkd_conv_set_tile) to whatever lmkd_conv2d_plan reports for that kind at 200 frames; with the pin the plan's
(tile, XCD tile order, parity classes, kernel family) are those of the 200-frame launch.  The weight gradient needs no pin: its (tile,
XCD order, family) already agree - r50.l3.reduce excepted, whose XCD-grouped split appears from 32 pixel splits on: 26 frames."""
import ctypes
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_conv_plan_golden", os.path.join(ROOT, "tools", "gen_conv_plan_golden.py"))
_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gen)

RESNET50 = list(_gen.RESNET50)      # (name, H (= W), Cs, Cin, Cout, K, stride, pad)
FULL = 200                          # frames per trunk call of the benchmark
FRAMES_BY_OUTPUT_MAP = {56: 5, 28: 9, 14: 21, 7: 45}
FRAMES_EXCEPT = {"r50.l3.reduce": 26}
MODES = {"fp32x3": 2, "fp32h2": 4}  # lmkd_conv_set_compute_dtype numbering
# which of lmkd_conv2d_plan's five ints must agree with the 200-frame launch: tile id, XCD tile order, parity classes, kernel family
# (forward, data gradient); tile id, XCD order, family (weight gradient: [2] is the number of pixel splits, [3] the grid in all kinds)
FIELDS = {0: (0, 1, 2, 4), 1: (0, 1, 2, 4), 2: (0, 1, 4)}


def frames(shape):
    name, H, _, _, _, K, s, p = shape
    return FRAMES_EXCEPT.get(name, FRAMES_BY_OUTPUT_MAP[(H + 2 * p - K) // s + 1])


def plan(L, kind, N, shape):
    _, H, Cs, Cin, Cout, K, s, p = shape
    info = (ctypes.c_int * 5)()
    L.call("lmkd_conv2d_plan", kind, N, H, H, Cs, Cin, Cout, K, K, s, p, info)
    return tuple(info)


def pins(L, shape):
    """-> (forward tile id, data-gradient tile id) of the 200-frame launch in the current mode (no pin set)"""
    return plan(L, 0, FULL, shape)[0], plan(L, 1, FULL, shape)[0]


def assert_same_kernels(L, shape):
    """in the library's current arithmetic mode: the launches of `shape` at frames(shape), forward and data gradient with their tile
    pinned, report the plan fields of the 200-frame launches.  -> the pins.  Leaves the tile override at 0 (automatic)."""
    N = frames(shape)
    want = {kind: plan(L, kind, FULL, shape) for kind in (0, 1, 2)}
    tiles = (want[0][0], want[1][0])
    try:
        for kind in (0, 1, 2):
            L.call("lmkd_conv_set_tile", tiles[kind] if kind < 2 else 0)
            got = plan(L, kind, N, shape)
            a, b = [got[i] for i in FIELDS[kind]], [want[kind][i] for i in FIELDS[kind]]
            assert a == b, "%s kind %d: plan %s at %d frames (tile pinned to %s), %s at %d" % (shape[0], kind, got, N,
                                                                                               tiles[kind] if kind < 2 else "-", want[kind], FULL)
    finally:
        L.call("lmkd_conv_set_tile", 0)
    return tiles
