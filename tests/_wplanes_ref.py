"""The plane buffer of a convolution weight (DESIGN.md "Weight plane buffer"; csrc/wplanes.h), stated in numpy, independently of the
kernels: (OIHW weight, Cs, pack mode, arithmetic) -> the expected uint16 buffer and its region table.  bf16 rounding and the truncation
split are integer arithmetic on the fp32 bits, the fp16 planes are numpy's round-to-nearest conversion, the scale is integer arithmetic."""
import numpy as np

MODES = {"bf16": 1, "fp32x3": 2, "fp32x3_9": 3, "fp32h2": 4}      # lmkd_conv_set_compute_dtype
SENTINEL = 0xdead                                                  # what planes() leaves in the unspecified halfwords


def kw_padded(Cs, KW):
    return KW if Cs >= 32 else ((KW * Cs + 31) // 32) * 32 // Cs


def packed(w, Cs, mode):
    """K-major packed weight [ncols][Kp]: mode 0 Wp[co][(kh KWp + kw) Cs + ci] (zero padding), mode 1 Wd[ci][(kh KW + kw) Co + co]"""
    Co, Cin, KH, KW = w.shape
    if mode == 0:
        p = np.zeros((Co, KH, kw_padded(Cs, KW), Cs), np.float32)
        p[:, :, :KW, :Cin] = w.transpose(0, 2, 3, 1)
        return p.reshape(Co, -1)
    return np.ascontiguousarray(w.transpose(1, 2, 3, 0)).reshape(Cin, -1)


def regions(n, arith):
    """name -> (first, past-the-last) 16-bit element; in order, gapless, ending at the buffer's size"""
    if arith == "bf16":
        return {"bf16_32": (0, n)}
    r = {"x3_32_pos": (0, 3 * n), "x3_32_neg": (3 * n, 6 * n), "x3_16_pos": (6 * n, 9 * n), "x3_16_neg": (9 * n, 12 * n)}
    if arith == "fp32h2":
        r.update({"h2_16_pos": (12 * n, 14 * n), "h2_16_neg": (14 * n, 16 * n), "amax": (16 * n, 16 * n + 32), "h2_32_pos": (16 * n + 32, 18 * n + 32)})
    return r


def total(n, arith):
    return list(regions(n, arith).values())[-1][1]


def kslot(q):
    return ((q & 1) << 1) | (q >> 1)


def frag32(ncols, Kp, npl):
    """index of plane 0 of element (col, k) in a region in v_mfma 32x32x16 fragment order; plane p at + 512 p"""
    col, k = np.meshgrid(np.arange(ncols), np.arange(Kp), indexing="ij")
    return ((((col >> 5) * (Kp >> 4) + (k >> 4)) * npl) * 64 + (col & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)


def frag16(ncols, Kp, npl):
    """... in v_mfma 16x16x32 fragment order"""
    col, k = np.meshgrid(np.arange(ncols), np.arange(Kp), indexing="ij")
    return ((((col >> 4) * (Kp >> 5) + (k >> 5)) * npl) * 64 + (col & 15) + 16 * kslot((k >> 3) & 3)) * 8 + (k & 7)


def trunc3(x):
    """x = p0 + p1 + p2, each the truncation to bf16 of what the ones before left"""
    b0 = x.view(np.uint32)
    r1 = x - (b0 & 0xffff0000).view(np.float32)
    b1 = r1.view(np.uint32)
    r2 = r1 - (b1 & 0xffff0000).view(np.float32)
    return [(b >> 16).astype(np.uint16) for b in (b0, b1, r2.view(np.uint32))]


def bf16_rne(x):
    b = x.view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def h2_scale(amax_bits):
    """2^s with max |w| 2^s in (2^14, 2^15]"""
    e = ((amax_bits >> 23) & 0xff) - 127 + (1 if amax_bits & 0x7fffff else 0)
    s = 0 if amax_bits == 0 else min(max(15 - e, -126), 126)
    return np.array([(s + 127) << 23], np.uint32).view(np.float32)[0]


def h2(x):
    h0 = x.astype(np.float16)
    h1 = (x - h0.astype(np.float32)).astype(np.float16)
    return h0.view(np.uint16), h1.view(np.uint16)


def planes(w, Cs, mode, arith):
    """-> (uint16 buffer, region table); the 30 halfwords behind the max |w| word hold SENTINEL"""
    P = packed(np.ascontiguousarray(w, np.float32), Cs, mode)
    ncols, Kp = P.shape
    n = ncols * Kp
    reg = regions(n, arith)
    out = np.full(total(n, arith), SENTINEL, np.uint16)
    if arith == "bf16":
        out[frag32(ncols, Kp, 1)] = bf16_rne(P)
        return out, reg
    for order, idx in (("32", frag32(ncols, Kp, 3)), ("16", frag16(ncols, Kp, 3))):
        for j, p in enumerate(trunc3(P)):
            out[reg["x3_%s_pos" % order][0] + idx + 512 * j] = p
            out[reg["x3_%s_neg" % order][0] + idx + 512 * j] = p ^ 0x8000
    if arith == "fp32h2":
        bits = int(np.abs(P).max().view(np.uint32))
        i16, i32 = frag16(ncols, Kp, 2), frag32(ncols, Kp, 2)
        for j, p in enumerate(h2(P * h2_scale(bits))):
            out[reg["h2_16_pos"][0] + i16 + 512 * j] = p
            out[reg["h2_16_neg"][0] + i16 + 512 * j] = p ^ 0x8000
            out[reg["h2_32_pos"][0] + i32 + 512 * j] = p
        out[reg["amax"][0]:reg["amax"][0] + 2] = np.array([bits], np.uint32).view(np.uint16)
    return out, reg
