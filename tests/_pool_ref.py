"""The stem and head pooling stages of csrc/norm_pool.hip stated in numpy (vectorised, no per-element loops), for tests that ask for
EQUALITY with the HIP kernels.

The contract pinned here:
  * stem: y = maxpool3x3/s2/p1(relu(c * scale + shift)); the arg-max byte of a window is the tap number kh * 3 + kw of its FIRST maximum
    in scan order (kh, then kw) over the taps that lie inside the image - taps in the padding keep their numbers and never win; cmax is
    the raw c at that tap.  A window whose maximum is 0 therefore names its first valid tap.
  * frames [0, N0) read table 0, frames [N0, N) table 1 of a [2][5][C] table (one [5][C] table when N0 = N).
    stats rows: mean, invstd, scale, shift, unbiased variance (unused here).  coef rows: A = gamma * invstd, mean(g), mean(g * xhat) and,
    with two segments, sum g * xhat, sum g.
  * the BatchNorm backward sums run over the POOLED tensors (dy, cmax) with the mask cmax * scale + shift > 0; each mean is one fp64
    quotient rounded ONCE to fp32.
  * head: window i of an axis of length L is [floor(i * L / 4), ceil((i + 1) * L / 4)); the first maximum in scan order (h, then w) of a
    window takes its gradient dy / 16; windows overlap, so a position can collect up to four.

Every function computes in the dtype of its first tensor argument (float32 or float64).  On the inputs of grid_inputs /
head_grid_inputs every intermediate value is a small dyadic rational, so both dtypes - and any summation order or FMA contraction - give
the same numbers (tests/test_pool_ref_host.py proves it), which is what allows `torch.equal` against the kernels."""
import numpy as np


# the cases of tests/test_gpu_pool.py (convolution-output N, H, W, C, N0), checked for exactness and ties by tests/test_pool_ref_host.py.
# 1x1 ... 2x2: windows made of padding; 3x5, 5x7: odd, a last window cut on neither side; 4x4, 8x6: even - the last row / column of 2x2
# blocks has no window below / right of it; 17x35, 31x29: several workgroups; N0 = 3 | 1 | 2: one segment and both splits.
# 2x130x130x64: 8450 pooled rows = 67 virtual blocks of the reduce kernel, so the coefficient kernel adds more than one slice.
STEM_SEED, HEAD_SEED = 1, 2
STEM_HW = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (4, 4), (5, 7), (8, 6), (17, 35), (31, 29)]
STEM_BIG = (2, 130, 130, 64, 2)
STEM_CASES = [(3, h, w, C, n0) for (h, w) in STEM_HW for C in (8, 64) for n0 in (3, 1, 2)] + [STEM_BIG]


def pooled_size(L):
    """output length of a 3 / stride 2 / pad 1 window over L"""
    return (L + 2 - 3) // 2 + 1


def round_bf16(x):
    """fp32 values rounded to the nearest bf16 (ties to even), returned as fp32 - the rounding of the kernels' bf16 stores"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def _steps(rng, lo, hi, step, shape):
    """uniform multiples of `step` in [lo, hi]"""
    return rng.integers(round(lo / step), round(hi / step) + 1, size=shape).astype(np.float64) * step


def _choice(rng, values, shape):
    return np.asarray(values, dtype=np.float64)[rng.integers(0, len(values), size=shape)]


ZERO_CHANNEL = 5      # channels c % 8 == ZERO_CHANNEL: bn(c) > 0 only where |c| = 2, so most windows have maximum 0
FLIP_CHANNEL = 1      # channels c % 4 == FLIP_CHANNEL: the second segment's scale has the opposite sign


STEM_MIN_TIE_SHARE, STEM_MIN_ZERO_SHARE = 0.125, 0.04      # of the windows of a case with at least 100 windows per frame and channel


def grid_gamma(seed, C):
    """the BatchNorm weight that belongs to grid_inputs(seed, ..., C, ...): values in {+-1/2, +-1, 2}"""
    rng = np.random.default_rng([seed, 17])
    gamma = _choice(rng, [-0.5, 0.5, -1.0, 1.0, 2.0], (C,))
    gamma[ZERO_CHANNEL::8] = 1.0
    return gamma


def grid_inputs(seed, N, H, W, C, N0):
    """-> c [N, H, W, C], dy [N, OH, OW, C], stats ([5][C], or [2][5][C] when 0 < N0 < N), coef ([3][C] / [2][5][C]); all float64.

    c: multiples of 1/4 in [-2, 2]; mean: multiples of 1/4 in [-1, 1]; invstd in {1/2, 1, 2}; scale = gamma * invstd with gamma =
    grid_gamma(seed, C) (negative on some channels); shift: multiples of 1/4 in [-2, 1], chosen freely - the kernels only read the
    table; dy, mean(g), mean(g * xhat): multiples of 1/8 in [-1, 1]; the sums of a two-segment coef table: multiples of 1/8 in [-4, 4].
    Channels c % 8 == ZERO_CHANNEL have scale +-1 and shift -7/4: positive at one of the 17 values of c, (16/17)^9 = 0.58 of their windows
    are 0.  In the second table, channels c % 4 == FLIP_CHANNEL carry -scale (a table is free to: A = gamma * invstd stays what the
    coefficient kernel writes), so reading the wrong table changes arg-max bytes."""
    rng = np.random.default_rng([seed, N, H, W, C, N0])
    OH, OW = pooled_size(H), pooled_size(W)
    two = 0 < N0 < N
    c = _steps(rng, -2.0, 2.0, 0.25, (N, H, W, C))
    dy = _steps(rng, -1.0, 1.0, 0.125, (N, OH, OW, C))
    gamma = grid_gamma(seed, C)
    for _ in range(64):
        stats, coef = [], []
        for s in range(2 if two else 1):
            mean = _steps(rng, -1.0, 1.0, 0.25, (C,))
            invstd = _choice(rng, [0.5, 1.0, 2.0], (C,))
            shift = _steps(rng, -2.0, 1.0, 0.25, (C,))
            invstd[ZERO_CHANNEL::8] = 1.0
            shift[ZERO_CHANNEL::8] = -1.75
            scale = gamma * invstd
            if s == 1:
                scale[FLIP_CHANNEL::4] *= -1.0
            stats.append(np.stack([mean, invstd, scale, shift, 1.0 / (invstd * invstd)]))
            rows = [gamma * invstd, _steps(rng, -1.0, 1.0, 0.125, (C,)), _steps(rng, -1.0, 1.0, 0.125, (C,))]
            if two:
                rows += [_steps(rng, -4.0, 4.0, 0.125, (C,)), _steps(rng, -4.0, 4.0, 0.125, (C,))]
            coef.append(np.stack(rows))
        stats, coef = (np.stack(stats), np.stack(coef)) if two else (stats[0], coef[0])
        # eight channels' tables can by chance leave few positive maxima: the tables (not c) are drawn again - deterministically, from
        # the same generator - until the case holds the ties and zero windows it exists for
        pos_tie, zero = window_tie_shares(c, stats, N0)
        if OH * OW < 100 or (pos_tie >= STEM_MIN_TIE_SHARE and zero >= STEM_MIN_ZERO_SHARE):
            return c, dy, stats, coef
    raise AssertionError("grid_inputs: no draw with enough ties")


HEAD_MIN_TIE_SHARE = 0.125


def head_grid_inputs(seed, F, H, W, C):
    """-> x [F, H, W, C] (post-ReLU: multiples of 1/4 in [0, 2], about a third zeros), dy [F, C] (multiples of 1/8 in [-1, 1]); float64.
    A window of two such elements ties with probability 1/9 + 4/9 * 1/8 = 1/6, larger windows more often; a small tensor (C = 4: a few
    dozen windows) can fall short of that by chance, so x is drawn again - deterministically, from the same generator - until at least
    HEAD_MIN_TIE_SHARE of its windows that hold more than one element have a tied maximum."""
    rng = np.random.default_rng([seed, F, H, W, C])
    for _ in range(64):
        x = _steps(rng, 0.25, 2.0, 0.25, (F, H, W, C))
        x[rng.random((F, H, W, C)) < 1.0 / 3.0] = 0.0
        share = head_tie_share(x)
        if share is None or share >= HEAD_MIN_TIE_SHARE:
            return x, _steps(rng, -1.0, 1.0, 0.125, (F, C))
    raise AssertionError("head_grid_inputs: no draw with enough ties")


def _rows(table, N, N0, dt):
    """the five rows of a stats / coef table per frame: [rows][N, 1, 1, C] (frames from N0 on read the second table)"""
    t = np.asarray(table).astype(dt)
    if t.ndim == 2:
        return [np.broadcast_to(t[r], (N, 1, 1, t.shape[1])) for r in range(t.shape[0])]
    assert t.ndim == 3 and t.shape[0] == 2 and 0 < N0 < N, "a [2][..][C] table needs 0 < N0 < N"
    sel = (np.arange(N) >= N0).astype(np.int64)
    return [t[sel, r][:, None, None, :] for r in range(t.shape[1])]


def _taps(a, OH, OW, fill):
    """[9, N, OH, OW, C]: tap kh * 3 + kw of every window of a [N, H, W, C], `fill` where the tap lies in the padding"""
    N, H, W, C = a.shape
    p = np.full((N, H + 2, W + 2, C), fill, dtype=a.dtype)
    p[:, 1:H + 1, 1:W + 1] = a
    return np.stack([p[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] for kh in range(3) for kw in range(3)])


def bn_relu_maxpool(c, stats, N0):
    """-> y, idx (uint8), cmax, each [N, OH, OW, C]"""
    N, H, W, C = c.shape
    dt = c.dtype
    OH, OW = pooled_size(H), pooled_size(W)
    _, _, scale, shift, _ = _rows(stats, N, N0, dt)
    v = np.maximum(c * scale + shift, dt.type(0))
    taps = _taps(v, OH, OW, -np.inf)
    idx = np.argmax(taps, axis=0)      # numpy: the first occurrence of the maximum = the first tap in scan order; padding (-inf) never wins
    y = np.take_along_axis(taps, idx[None], 0)[0]
    cmax = np.take_along_axis(_taps(c, OH, OW, 0.0), idx[None], 0)[0]
    return y, idx.astype(np.uint8), cmax


def maxpool_bwd(dy, idx, H, W):
    """g [N, H, W, C]: every window hands its dy to the position its arg-max byte names"""
    N, OH, OW, C = dy.shape
    assert (OH, OW) == (pooled_size(H), pooled_size(W)) and idx.shape == dy.shape
    gp = np.zeros((N, H + 2, W + 2, C), dtype=dy.dtype)
    for kh in range(3):
        for kw in range(3):
            gp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] += np.where(idx == kh * 3 + kw, dy, dy.dtype.type(0))
    return np.ascontiguousarray(gp[:, 1:H + 1, 1:W + 1])


def pooled_bn_stats(dy, cmax, stats, gamma, count, rows0=0, count0=0, round_coef=True):
    """The BatchNorm backward sums from the pooled side.  dy, cmax: [..., C] (any leading shape; `rows0` counts flattened rows).
    -> sum g, sum g * xhat ([C], or [2][C] for two segments: 0 < rows0 < rows), coef ([3][C] / [2][5][C]).
    count (count0): pre-pooling elements per channel (of segment 0).  The quotients are formed in fp64 and - round_coef - rounded once to
    fp32, A = gamma * invstd is the fp32 product, as bn_bwd_coef_kernel forms them; round_coef=False keeps float64 throughout."""
    C = dy.shape[-1]
    dt = dy.dtype
    d, cm = dy.reshape(-1, C), cmax.reshape(-1, C)
    rows = d.shape[0]
    st = np.asarray(stats).astype(dt)
    two = 0 < rows0 < rows
    assert st.ndim == (3 if two else 2)
    segs = [(0, rows0, count0, st[0]), (rows0, rows, count - count0, st[1])] if two else [(0, rows, count, st)]
    ct = np.float32 if round_coef else np.float64
    sums_g, sums_gx, coef = [], [], []
    for r0, r1, cnt, t in segs:
        mean, invstd, scale, shift = t[0], t[1], t[2], t[3]
        x = cm[r0:r1]
        g = np.where(x * scale + shift > 0, d[r0:r1], dt.type(0))
        sg, sgx = g.sum(0), (g * ((x - mean) * invstd)).sum(0)
        rows_ = [np.asarray(gamma).astype(ct) * np.asarray(t[1]).astype(ct), (sg.astype(np.float64) / cnt).astype(ct),
                 (sgx.astype(np.float64) / cnt).astype(ct)]
        if two:
            rows_ += [sgx.astype(ct), sg.astype(ct)]
        sums_g.append(sg)
        sums_gx.append(sgx)
        coef.append(np.stack(rows_))
    if two:
        return np.stack(sums_g), np.stack(sums_gx), np.stack(coef)
    return sums_g[0], sums_gx[0], coef[0]


def stem_unpool_terms(dy, idx, c, stats, coef, N0):
    """-> A, m * g, mean(g), xhat * mean(g * xhat), each broadcastable to [N, H, W, C]: the partial terms of dc"""
    N, H, W, C = c.shape
    dt = c.dtype
    mean, invstd, scale, shift, _ = _rows(stats, N, N0, dt)
    cf = _rows(coef, N, N0, dt)
    g = np.where(c * scale + shift > 0, maxpool_bwd(dy.astype(dt), idx, H, W), dt.type(0))
    return cf[0], g, cf[1], (c - mean) * invstd * cf[2]


def stem_unpool_bn_bwd(dy, idx, c, stats, coef, N0):
    """dc = A * (m * g - mean(g) - xhat * mean(g * xhat)) with g = maxpool_bwd(dy, idx), m = (c * scale + shift > 0), xhat = (c - mean) * invstd"""
    A, g, mg, xm = stem_unpool_terms(dy, idx, c, stats, coef, N0)
    return A * (g - mg - xm)


def head_windows(L):
    """the four windows [lo, hi) of an axis of length L"""
    return [((i * L) // 4, -((-(i + 1) * L) // 4)) for i in range(4)]


def head_pool(x):
    """AdaptiveMaxPool2d((4, 4)) and the mean over its 16 outputs: x [F, H, W, C] -> y [F, C]"""
    F, H, W, C = x.shape
    s = np.zeros((F, C), dtype=x.dtype)
    for h0, h1 in head_windows(H):
        for w0, w1 in head_windows(W):
            s += x[:, h0:h1, w0:w1].reshape(F, -1, C).max(1)
    return s * x.dtype.type(1.0 / 16.0)


def head_argmax(x):
    """[16, F, C]: flat position h * W + w of the first maximum (scan order h, then w) of each of the 16 windows"""
    F, H, W, C = x.shape
    out = []
    for h0, h1 in head_windows(H):
        for w0, w1 in head_windows(W):
            ww = w1 - w0
            am = np.argmax(x[:, h0:h1, w0:w1].reshape(F, -1, C), axis=1)      # first occurrence, row-major = scan order
            out.append((h0 + am // ww) * W + (w0 + am % ww))
    return np.stack(out)


def head_pool_bwd(x, dy):
    """dx [F, H, W, C]: every window adds dy / 16 at its arg-max position"""
    F, H, W, C = x.shape
    dt = x.dtype
    gv = dy.astype(dt) * dt.type(1.0 / 16.0)
    pos = np.arange(H * W)[None, :, None]
    k = np.zeros((F, H * W, C), dtype=dt)
    for p in head_argmax(x):
        k += (pos == p[:, None, :])
    return (gv[:, None, :] * k).reshape(F, H, W, C)


def window_tie_shares(c, stats, N0):
    """-> (share of the stem's windows whose maximum is positive and attained by more than one valid tap, share whose maximum is 0)"""
    N, H, W, C = c.shape
    _, _, scale, shift, _ = _rows(stats, N, N0, c.dtype)
    taps = _taps(np.maximum(c * scale + shift, 0), pooled_size(H), pooled_size(W), -np.inf)
    m = taps.max(0)
    tied = (taps == m[None]).sum(0) > 1
    return float((tied & (m > 0)).mean()), float((m == 0).mean())


def head_tie_share(x):
    """of the head's windows that hold more than one element (only those can tie): the share whose maximum is attained more than once;
    None when every window is a single element (H, W in {1, 2, 4})"""
    F, H, W, C = x.shape
    n = []
    for h0, h1 in head_windows(H):
        for w0, w1 in head_windows(W):
            if (h1 - h0) * (w1 - w0) > 1:
                s = x[:, h0:h1, w0:w1].reshape(F, -1, C)
                n.append((s == s.max(1, keepdims=True)).sum(1) > 1)
    return float(np.mean(n)) if n else None
