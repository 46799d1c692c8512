"""The weight plane buffer's layout, host side (no GPU): the numpy statement tests/_wplanes_ref.py is consistent with itself - both
fragment orders are bijections onto their regions, the regions tile the buffer, the truncation planes reconstruct the value - and its
total is the size the library reports for every arithmetic (csrc/wplanes.h through lmkd_conv2d_plane_elems)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wplanes_ref as R  # noqa: E402

# (ncols, Kp): the stem's padded K, a K with an odd number of 32-wide groups, three 32-column tiles
DIMS = [(64, 224), (32, 288), (32, 576), (96, 64), (64, 96)]


@pytest.mark.parametrize("frag", [R.frag32, R.frag16])
@pytest.mark.parametrize("npl", [1, 2, 3])
def test_fragment_orders_are_bijections_onto_their_regions(frag, npl):
    for ncols, Kp in DIMS:
        i = frag(ncols, Kp, npl)
        full = np.concatenate([(i + 512 * j).ravel() for j in range(npl)])
        assert np.array_equal(np.sort(full), np.arange(ncols * Kp * npl)), (ncols, Kp)


@pytest.mark.parametrize("arith", list(R.MODES))
def test_regions_tile_the_buffer(arith):
    n = 96 * 224
    reg = list(R.regions(n, arith).values())
    assert reg[0][0] == 0 and all(a[1] == b[0] for a, b in zip(reg, reg[1:])) and reg[-1][1] == R.total(n, arith)
    assert R.total(n, arith) == {"bf16": n, "fp32x3": 12 * n, "fp32x3_9": 12 * n, "fp32h2": 18 * n + 32}[arith]


def test_truncation_planes_reconstruct_the_value():
    rng = np.random.default_rng(0)
    x = np.concatenate([(rng.standard_normal(4096) * s).astype(np.float32) for s in (0.05, 3.0, 1e-4, 1e30, 1e-30)] +
                       [np.array([0.0, -0.0, 0.25, -0.25, 16777215.0, 1.0 / 3.0], np.float32)])
    p = R.trunc3(x)
    rec = sum((q.astype(np.uint32) << 16).view(np.float32).astype(np.float64) for q in p)
    assert np.array_equal(rec, x.astype(np.float64))      # the sum of the planes, formed in fp64 without rounding, is the value


def test_every_specified_element_is_written_once():
    """planes() leaves its sentinel only in the 30 unspecified halfwords behind the max |w| word"""
    w = np.full((64, 3, 7, 7), 0.125, np.float32)      # no plane of 0.125 (or of the padding's zeros) has the sentinel's bits
    for arith in R.MODES:
        out, reg = R.planes(w, 4, 0, arith)
        left = np.flatnonzero(out == R.SENTINEL)
        want = np.arange(reg["amax"][0] + 2, reg["amax"][1]) if arith == "fp32h2" else np.arange(0)
        assert np.array_equal(left, want), arith


def test_total_is_the_librarys_plane_elems():
    import litemkd_amd
    L = litemkd_amd.lib()
    try:
        for arith, mode in R.MODES.items():
            L.call("lmkd_conv_set_compute_dtype", mode)
            for ncols, Kp in DIMS:
                assert L.value("lmkd_conv2d_plane_elems", ncols, Kp) == R.total(ncols * Kp, arith), (arith, ncols, Kp)
    finally:
        L.call("lmkd_conv_set_compute_dtype", 2)
