"""Plain numpy statements of the attention-map arithmetic (include/lmkd.h lmkd_gradcam_fwd / lmkd_cam_overlay_u8, ops.jet_lut), written
from its definition:

    mode 0 (Grad-CAM)   w[f, c] = (sum_p dA[f, p, c]) / HW,  raw[f, p] = max(0, sum_c w[f, c] A[f, p, c])
    mode 1 (HiResCAM)   raw[f, p] = max(0, sum_c dA[f, p, c] A[f, p, c])          (w is still reported)
    both                cam[f, p] = (raw[f, p] - min_p raw) / (1e-7 + max_p raw - min_p raw)
    JET                 x2 = clip(765 - |8 i - centre|, 0, 510), centres 1530 / 1020 / 510 (R / G / B), byte = (x2 + 1) >> 1
    overlay             q = min(255, (int)(cam * 255 + 0.5)) -> PIL BILINEAR -> lut -> (lut * (256 - a) + frame * a + 128) >> 8

Every function computes in the dtype of its inputs (fp64 = the reference, fp32 = the yardstick of tests/_anchor.py)."""
import numpy as np


def gradcam(A, dA, mode):
    """A, dA [F, ..., C] -> (w [F, C], raw [F, ...], cam [F, ...])"""
    F, C = A.shape[0], A.shape[-1]
    a, d = A.reshape(F, -1, C), dA.reshape(F, -1, C)
    HW = a.shape[1]
    w = d.sum(1) / A.dtype.type(HW)
    s = (w[:, None, :] * a).sum(-1) if mode == 0 else (d * a).sum(-1)
    raw = np.maximum(s, 0)
    return w, raw.reshape(A.shape[:-1]), normalise(raw).reshape(A.shape[:-1])


def normalise(raw):
    """raw [F, HW] -> (raw - min) / (1e-7 + (max - min)) per frame: the range is formed first, so that a constant map gives 0 / 1e-7 in fp32
    too (added to max, 1e-7 is below half an ulp of any max > 1)"""
    mn, mx = raw.min(1, keepdims=True), raw.max(1, keepdims=True)
    return (raw - mn) / (raw.dtype.type(1e-7) + (mx - mn))


def gradcam_torch(A, dA, mode):
    """the same arithmetic with torch's CPU kernels, in the dtype of the inputs (fp32: the yardstick of tests/_anchor.py)"""
    import torch
    F, C = A.shape[0], A.shape[-1]
    a, d = A.reshape(F, -1, C), dA.reshape(F, -1, C)
    w = d.sum(1) / a.shape[1]
    raw = torch.relu((w[:, None, :] * a).sum(-1) if mode == 0 else (d * a).sum(-1))
    mn, mx = raw.min(1, keepdim=True).values, raw.max(1, keepdim=True).values
    cam = (raw - mn) / (1e-7 + (mx - mn))
    return w, raw.reshape(A.shape[:-1]), cam.reshape(A.shape[:-1])


def jet_lut():
    i = np.arange(256, dtype=np.int64)
    return np.stack([(np.clip(765 - np.abs(8 * i - c), 0, 510) + 1) >> 1 for c in (1530, 1020, 510)], 1).astype(np.uint8)


def quantise(cam):
    return np.minimum(255, (cam.astype(np.float32) * np.float32(255) + np.float32(0.5)).astype(np.int64)).astype(np.uint8)


def blend(colour, frames, alpha256):
    """uint8 [..., 3] x 2 -> (colour * (256 - a) + frame * a + 128) >> 8; frames None: the colour alone"""
    if frames is None:
        return colour
    return ((colour.astype(np.int64) * (256 - alpha256) + frames.astype(np.int64) * alpha256 + 128) >> 8).astype(np.uint8)


def overlay(cam, frames, out_hw, alpha256, lut=None):
    """cam [F, h, w] -> uint8 [F, Ho, Wo, 3] through PIL's own resampler"""
    from PIL import Image
    lut = jet_lut() if lut is None else lut
    Ho, Wo = out_hw
    q = quantise(cam)
    up = np.stack([np.asarray(Image.fromarray(q[f], "L").resize((Wo, Ho), Image.BILINEAR)) for f in range(q.shape[0])])
    return blend(lut[up], frames, alpha256)
