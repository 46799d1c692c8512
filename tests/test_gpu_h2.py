"""GPU: the two-plane fp16 arithmetic of the 3x3 convolutions ('fp32h2', lmkd_conv_set_compute_dtype(4); csrc/conv_patch16.h) - what
bench.py's headline line runs.  fp32 = h0 + h1 with h0 = fp16(x 2^s), h1 = fp16(x 2^s - h0), 2^s a power of two from max |tensor|.

The accuracy claims (error against fp64 at the level of the three-plane bf16 mode and of native fp32) are tested where the other
arithmetic modes are: tests/test_gpu_fullsize.py (every convolution of the trunk at 200 frames), tests/test_gpu_episode.py (episodes
against the oracle, 64 px ... 400 frames of 224^2), tests/test_gpu_merged.py / test_gpu_schedule.py (merged call, benchmark schedule).
Here: what is specific to the mode - the maxima the producers record, the weight packs, and the corners of the scaling (zero tensors,
tiny / huge magnitudes, one outlier dominating the maximum, maxima that are exact powers of two)."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wplanes_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def h2_mode():
    from litemkd_amd import ops
    ops.set_conv_compute_dtype("fp32h2")
    yield
    ops.reset_compute_dtypes()


def _word(t, i=0):
    """the recorded maximum of frame segment i: the largest of the segment's slots (csrc/common.h amax_commit)"""
    return _seg_max(t._lmkd_amax, i)


def _seg_max(words, i=0):
    """word 0 of each of the 64 slots (16 words apart) of segment i; words 1-3 of a slot hold the range fence's counts"""
    return float(words.view(torch.float32).view(2, 64, 16)[i, :, 0].max())


def _launches():
    import litemkd_amd
    return litemkd_amd.lib().value("lmkd_conv_h2_launches")


def test_producers_record_the_maximum(dev):
    """BatchNorm apply (+ residual, ReLU), BatchNorm backward and the stem's BatchNorm + ReLU + max-pool fold max |output| into the word the
    tensor carries - exactly torch's abs().max(), per frame segment"""
    from litemkd_amd import ops
    g = torch.Generator(device=dev).manual_seed(0)
    N, H, C, F0 = 6, 14, 64, 2
    x0 = torch.randn(N, H, H, C, device=dev, generator=g) * 3
    x0[F0:] *= 0.01
    r = torch.randn(N, H, H, C, device=dev, generator=g)
    gam, bet = 1 + 0.1 * torch.randn(C, device=dev, generator=g), 0.1 * torch.randn(C, device=dev, generator=g)
    wp = ops._pack_weights(torch.randn(C, C, 3, 3, device=dev, generator=g) * 0.05, C, 0)
    for seg in (0, F0):
        if seg:
            c, part, T0 = ops.conv_fwd(x0, wp, C, 3, 3, 1, 1, True, seg=seg)
            st = ops.bn_stats_train(part, N * H * H, gam, bet, None, None, seg=(T0, seg * H * H))
        else:
            c, part = ops.conv_fwd(x0, wp, C, 3, 3, 1, 1, True)
            st = ops.bn_stats_train(part, N * H * H, gam, bet, torch.zeros(C, device=dev), torch.ones(C, device=dev))
        y = ops.bn_apply(c, st, True, res=r, seg=seg)
        parts = [y] if not seg else [y[:seg], y[seg:]]
        for i, p in enumerate(parts):
            assert _word(y, i) == float(p.abs().max()), (seg, i)
        dy = torch.randn(N, H, H, C, device=dev, generator=g) * 1e-3
        dx = ops.bn_backward(dy, c, None, st, gam, 2, seg=seg)[0]
        parts = [dx] if not seg else [dx[:seg], dx[seg:]]
        for i, p in enumerate(parts):
            assert _word(dx, i) == float(p.abs().max()), (seg, i)
    xa = torch.rand(3, 3, 64, 64, device=dev, generator=g)
    w = torch.nn.Parameter(torch.randn(64, 3, 7, 7, device=dev, generator=g) * 0.05)
    y = ops.StemFn.apply(xa, w, gam, bet, torch.zeros(C, device=dev), torch.ones(C, device=dev), True)
    assert _word(y) == float(y.detach().abs().max())


def test_weight_planes_repack_equals_split(dev):
    """lmkd_conv2d_repack_multi (after an optimizer step) writes what lmkd_conv2d_pack_weights + lmkd_conv2d_split_weights write: the bf16
    planes, the two fp16 planes of W and -W, and max |w| - bit for bit, for both pack modes"""
    import litemkd_amd
    from litemkd_amd import ops
    L = litemkd_amd.lib()
    g = torch.Generator(device=dev).manual_seed(1)
    ws = [torch.randn(64, 64, 3, 3, device=dev, generator=g) * 0.05, torch.randn(128, 64, 3, 3, device=dev, generator=g) * 3.0,
          torch.randn(128, 64, 1, 1, device=dev, generator=g) * 1e-4]
    ents = []
    for w in ws:
        for mode in (0, 1):
            ents.append((w, w.shape[1], mode, ops._pack_weights(w, w.shape[1], mode)))
    m = len(ents)
    outs = [torch.zeros_like(e[3]) for e in ents]
    wp = (ctypes.c_void_p * m)(*[e[0].data_ptr() for e in ents])
    wf = (ctypes.c_void_p * m)(*[o.data_ptr() for o in outs])
    dims = (ctypes.c_int * (6 * m))(*[v for e in ents for v in (e[0].shape[0], e[0].shape[1], e[1], e[0].shape[2], e[0].shape[3], e[2])])
    L.call("lmkd_conv2d_repack_multi", wp, wf, dims, m, None)
    torch.cuda.synchronize()
    for e, o in zip(ents, outs):
        word, end = R.regions(e[0].numel(), "fp32h2")["amax"]      # (every pack here is unpadded: as many elements as the weight)
        assert o.numel() == R.total(e[0].numel(), "fp32h2")
        assert torch.equal(o[:word + 2], e[3][:word + 2]) and torch.equal(o[end:], e[3][end:]), tuple(e[0].shape)
        assert float(o[word:word + 2].view(torch.float32)) == float(e[0].abs().max())


def _conv3(x, w, dy, seg=0):
    from litemkd_amd import ops
    C = w.shape[0]
    ops.amax_compute(x, seg)
    ops.amax_compute(dy, seg)
    n0 = _launches()
    y = ops.conv_fwd(x, ops._pack_weights(w, x.shape[-1], 0), C, 3, 3, 1, 1, True, seg=seg)[0]
    dx = ops.conv_bwd_data(dy, ops._pack_weights(w, x.shape[-1], 1), x.shape, C, 3, 3, 1, 1, seg=seg)
    dw = ops.conv_bwd_weight(x, dy, w.shape, 1, 1, seg=seg)
    torch.cuda.synchronize()
    assert _launches() - n0 == 3, "the two-plane kernels did not run"
    return y, dx, dw


def _ref3(x, w, dy):
    xd = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    yd = F.conv2d(xd, wd, padding=1)
    yd.backward(dy.permute(0, 3, 1, 2).double())
    return yd.detach().permute(0, 2, 3, 1), xd.grad.permute(0, 2, 3, 1), wd.grad


def _rel(a, r):
    return float((a.double() - r).norm() / r.norm().clamp_min(1e-300))


@pytest.mark.parametrize("sx,sw,sdy", [(1.0, 1.0, 1.0), (1e-30, 1.0, 1e10), (1e25, 1e-3, 1e8), (1.0, 1e-18, 1e-12), (2.0 ** -7, 2.0 ** 3, 2.0 ** -20)])
def test_magnitudes(dev, sx, sw, sdy):
    """operands from 1e-30 to 1e25 (results representable in fp32): the power-of-two scales centre every tensor on the fp16 range -
    relative-L2 error against fp64 below 1.5e-6 whatever the magnitudes"""
    g = torch.Generator(device=dev).manual_seed(2)
    N, H, C = 8, 14, 64
    x = torch.relu(torch.randn(N, H, H, C, device=dev, generator=g)) * sx
    w = torch.randn(C, C, 3, 3, device=dev, generator=g) * (2.0 / (9 * C)) ** 0.5 * sw
    dy = torch.randn(N, H, H, C, device=dev, generator=g) * sdy
    for got, ref in zip(_conv3(x, w, dy), _ref3(x, w, dy)):
        assert torch.isfinite(got).all()
        assert _rel(got, ref) < 1.5e-6, _rel(got, ref)


def test_maximum_that_is_a_power_of_two_and_zero_tensors(dev):
    """max |x| exactly 2^k scales to 2^15 (finite in fp16: 65504); an all-zero operand gives an all-zero result"""
    g = torch.Generator(device=dev).manual_seed(3)
    N, H, C = 4, 14, 64
    x = torch.rand(N, H, H, C, device=dev, generator=g)
    x[1, 3, 3, 5] = 4.0
    w = torch.randn(C, C, 3, 3, device=dev, generator=g) * 0.05
    w[3, 2, 1, 1] = -0.5
    dy = torch.randn(N, H, H, C, device=dev, generator=g).clamp(-2, 2)
    dy[0, 0, 0, 0] = 2.0
    for got, ref in zip(_conv3(x, w, dy), _ref3(x, w, dy)):
        assert torch.isfinite(got).all() and _rel(got, ref) < 1.5e-6
    z = torch.zeros_like(x)
    y, dx, dw = _conv3(z, w, dy)
    assert float(y.abs().max()) == 0.0 and float(dw.abs().max()) == 0.0 and torch.isfinite(dx).all()
    y, dx, dw = _conv3(x, w, torch.zeros_like(dy))
    assert float(dx.abs().max()) == 0.0 and float(dw.abs().max()) == 0.0


def test_one_outlier_dominating_the_maximum(dev):
    """one element 2^20 times the rest takes the scale with it: the rest falls below the range where the second plane is a normal fp16
    number.  What those elements lose is bounded ABSOLUTELY by 2^-25 of the scaled tensor - against the OUTPUT's scale (set by the outlier's
    products) the error stays at fp32 level; and on the outputs the outlier does not reach, the error relative to THEIR scale is bounded by
    2^-25 2^20 / ... - measured here, not assumed: below 2e-3 of those outputs' norm, i.e. the mode degrades gracefully to ~fp16 x 2 planes
    minus 20 bits where an fp32 kernel would keep 24; the trunk's tensors sit 2^4 .. 2^9 below their maxima (profiles/r04_h2_error.txt)"""
    g = torch.Generator(device=dev).manual_seed(4)
    N, H, C = 4, 14, 64
    x = torch.relu(torch.randn(N, H, H, C, device=dev, generator=g))
    x[0, 7, 7, 0] = 2.0 ** 20
    w = torch.randn(C, C, 3, 3, device=dev, generator=g) * 0.05
    dy = torch.randn(N, H, H, C, device=dev, generator=g)
    (y, dx, dw), (yr, dxr, dwr) = _conv3(x, w, dy), _ref3(x, w, dy)
    assert _rel(y, yr) < 1.5e-6 and _rel(dx, dxr) < 1.5e-6 and _rel(dw, dwr) < 1.5e-6
    assert _rel(y[1:], yr[1:]) < 2e-3      # frames the outlier does not touch


def test_two_segments_scale_independently(dev):
    """two frame segments with maxima 1e6 apart in one launch: each segment is scaled by its own power of two (a maximum holds the
    words of two segments), so the result equals two launches bit for bit"""
    g = torch.Generator(device=dev).manual_seed(5)
    N, F0, H, C = 7, 3, 14, 64
    x = torch.relu(torch.randn(N, H, H, C, device=dev, generator=g))
    x[F0:] *= 1e-6
    w = torch.randn(C, C, 3, 3, device=dev, generator=g) * 0.05
    dy = torch.randn(N, H, H, C, device=dev, generator=g)
    dy[:F0] *= 1e-5
    y, dx, dw = _conv3(x, w, dy, seg=F0)
    ya, dxa, dwa = _conv3(x[:F0].contiguous(), w, dy[:F0].contiguous())
    yb, dxb, dwb = _conv3(x[F0:].contiguous(), w, dy[F0:].contiguous())
    assert torch.equal(y, torch.cat([ya, yb])) and torch.equal(dx, torch.cat([dxa, dxb]))
    assert _rel(dw, (dwa.double() + dwb.double())) < 2e-6


def test_without_the_maxima_the_three_plane_kernels_run(dev):
    """a launch whose operands carry no maximum (a tensor from elsewhere) is not an error: it runs the three-plane form"""
    from litemkd_amd import ops
    g = torch.Generator(device=dev).manual_seed(6)
    x = torch.relu(torch.randn(4, 14, 14, 64, device=dev, generator=g))
    w = torch.randn(64, 64, 3, 3, device=dev, generator=g) * 0.05
    n0 = _launches()
    y = ops.conv_fwd(x, ops._pack_weights(w, 64, 0), 64, 3, 3, 1, 1, True)[0]
    assert _launches() == n0
    ops.set_conv_compute_dtype("fp32x3")
    y3 = ops.conv_fwd(x, ops._pack_weights(w, 64, 0), 64, 3, 3, 1, 1, True)[0]
    assert torch.equal(y, y3)


def test_subnormal_second_plane_reaches_the_matrix_pipe(dev):
    """x = 1 + 2^-20 beside one element 2^14: scaled by 2^1, the second plane of the small elements is 2^-19 - a SUBNORMAL fp16 number.
    v_mfma_f32_16x16x32_f16 must take it as it is (no flush to zero): with a weight that is 0.5 on the centre tap of the matching
    channel and 0 elsewhere, y = 0.5 x EXACTLY (one non-zero product per output: nothing for the fp32 accumulator to round)"""
    g = torch.Generator(device=dev).manual_seed(7)
    N, H, C = 2, 14, 64
    x = torch.full((N, H, H, C), 1.0 + 2.0 ** -20, device=dev)
    x[0, 0, 0, 0] = 2.0 ** 14
    w = torch.zeros(C, C, 3, 3, device=dev)
    w[torch.arange(C), torch.arange(C), 1, 1] = 0.5
    dy = torch.randn(N, H, H, C, device=dev, generator=g)
    y, dx, dw = _conv3(x, w, dy)
    assert torch.equal(y, 0.5 * x)
    # the data gradient is 0.5 dy through the two-plane representation of dy: exact where dy's residual fits the second plane, else within
    # one fp32 ulp (2^-23 relative) - or, for the elements below 2^-17 of the maximum, within 2^-25 of the scaled tensor
    import math
    s = 15 - math.ceil(math.log2(float(dy.abs().max())))
    assert bool(((dx - 0.5 * dy).abs() <= 0.5 * (2.0 ** -23 * dy.abs() + 2.0 ** (-25 - s))).all())
    assert float((dx == 0.5 * dy).float().mean()) > 0.45


def test_uint8_frames_carry_a_unit_maximum(dev):
    """frames from the uint8 transform (Resize / crop / flip / ToTensor, values in [0, 1]) carry the constant maximum 1.0 - an upper bound is
    a valid scale - so the stem runs its two-plane kernels on them too; result equal to the three-plane arithmetic to fp32 rounding"""
    import litemkd_amd
    from litemkd_amd import ops
    g = torch.Generator().manual_seed(8)
    F_, S = 8, 64
    u8 = torch.randint(0, 256, (F_, 72, 80, 3), dtype=torch.uint8, generator=g).to(dev)
    cy = torch.tensor([3], dtype=torch.int32, device=dev)
    cx = torch.tensor([5], dtype=torch.int32, device=dev)
    fl = torch.tensor([1], dtype=torch.int32, device=dev)
    w = torch.nn.Parameter((torch.randn(64, 3, 7, 7, generator=g) * 0.05).to(dev))
    gam, bet = (1 + 0.1 * torch.randn(64, generator=g)).to(dev), (0.1 * torch.randn(64, generator=g)).to(dev)
    outs = {}
    for mode in ("fp32h2", "fp32x3"):
        ops.set_conv_compute_dtype(mode)
        x4 = ops.frames_u8_to_nhwc4(u8, cy, cx, fl, S)
        n0 = _launches()
        outs[mode] = ops.StemFn.apply(x4, w, gam, bet, torch.zeros(64, device=dev), torch.ones(64, device=dev), True).detach()
        assert _launches() - n0 == (1 if mode == "fp32h2" else 0)
    assert float((outs["fp32h2"] - outs["fp32x3"]).abs().max()) <= 2e-6 * float(outs["fp32x3"].abs().max())


def test_training_across_optimizer_steps_tracks_the_three_plane_arithmetic(dev):
    """50 full-size episodes with three optimizer steps under bench.py's schedule in fp32h2 and in fp32x3, same seeds: every weight stays
    finite and the losses after the steps agree to 2 %.  (A regression test: the words that hold a tensor's maximum were once recycled
    by the allocator while the weight-gradient stream's last kernel - the stem's - had not started; it then read a maximum of zero,
    its fp16 planes overflowed and the stem's weights were NaN after the first optimizer step - with finite losses, ReLU(NaN) being 0.
    The race needs the pool of words to be recycled inside the weight-gradient stream's 2.5 ms tail: this loop hit it in about half of
    its runs; test_words_are_protected_on_every_stream_that_reads_them checks the protection itself.)"""
    from litemkd_amd import ops, trainloop as TL
    from litemkd_amd.options import default_args
    from litemkd_amd.schedule import Schedule
    import litemkd_amd
    L = litemkd_amd.lib()
    out = {}
    pool_tensors, ops._AMAX_POOL_TENSORS = ops._AMAX_POOL_TENSORS, 4      # a new pool of words every four tensors: the recycling happens many times per episode
    ops.amax_pool_reset()
    ops.h2_fence_reset()
    fb0 = L.value("lmkd_conv_h2_fallbacks")
    for mode in ("fp32h2", "fp32x3"):
        with Schedule.bench(conv_dtype=mode).applied():
            cfg = default_args(shot=5, device=dev, trans_dropout=0.1, training_iterations=10 ** 9, print_freq=10 ** 9)
            torch.manual_seed(1234)
            student, teacher, src, distiller, acc_fn, _, opt, sch = TL.make(cfg, base_seed=2024)
            pool = [src.episode(e) for e in range(2)]
            losses = []
            for i in range(50):
                loss, _, _ = TL.train_task(pool[i % 2], student, teacher, distiller, acc_fn, cfg)
                losses.append(loss.detach().clone())      # no host synchronisation, no reference to the episode's tensors: the next forward is
                del loss                                  # enqueued - and allocates - while the weight-gradient stream still runs
                if (i + 1) % 16 == 0:
                    opt.step()
                    opt.zero_grad()
                sch.step()
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(p).all()) for p in student.parameters()), mode
            out[mode] = torch.stack([l.float() for l in losses]).cpu()
            ops.join_all_streams()
            if mode == "fp32h2":      # the range fence judged every episode's tensors and flagged none: no launch fell back to three planes
                ops.h2_fence_step(wait=True)
                assert ops.h2_fence_flagged() == [] and L.value("lmkd_conv_h2_fallbacks") == fb0
    ops._AMAX_POOL_TENSORS = pool_tensors
    ops.amax_pool_reset()
    a, b = out["fp32h2"], out["fp32x3"]
    assert torch.isfinite(a).all() and float(((a - b).abs() / b.abs()).max()) < 0.02, (a[-4:], b[-4:])


def _parked_weight_grad(dev, protect):
    """ops.weight_grad queued on the weight-gradient stream BEHIND a one-second sleep kernel; then every reference to its operands (and
    to the words of their maxima) is dropped and same-sized tensors full of garbage are allocated and written on the caller's stream - the
    allocator hands the blocks out again unless the side stream was recorded on them.  -> (dW the side stream computed, reference dW)"""
    from litemkd_amd import ops
    g = torch.Generator(device=dev).manual_seed(12)
    C, N, H = 64, 8, 28
    st = _identity_table(C, dev)
    w = torch.nn.Parameter(torch.randn(C, C, 3, 3, device=dev, generator=g) * 0.05)
    x0 = torch.relu(torch.randn(N, H, H, C, device=dev, generator=g))
    dy0 = torch.randn(N, H, H, C, device=dev, generator=g) * 1e-3
    ref = ops.conv_bwd_weight(ops.amax_compute(x0.clone()), ops.amax_compute(dy0.clone()), tuple(w.shape), 1, 1).clone()
    w.grad = torch.zeros_like(w)
    pool_tensors, ops._AMAX_POOL_TENSORS = ops._AMAX_POOL_TENSORS, 1      # every maximum in a pool of its own: freed with its tensor
    ops.amax_pool_reset()
    box = {"x": ops.bn_apply(x0, st, False), "dy": ops.bn_apply(dy0, st, False)}      # producers: the words come from the pools
    nw = box["x"]._lmkd_amax.numel()
    orig = torch.Tensor.record_stream
    if not protect:      # the round-4 state: operands recorded on the side stream, their words not
        torch.Tensor.record_stream = lambda self, s: None if self.dtype is torch.int32 else orig(self, s)
    prev = ops.SIDE_WGRAD
    ops.SIDE_WGRAD = True
    junk = []

    class _InBackward(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return t * 1.0

        @staticmethod
        def backward(ctx, gr):
            sw = ops._wgrad_stream(dev)
            with torch.cuda.stream(sw):
                torch.cuda._sleep(2_000_000_000)      # parks the side stream: the weight gradient below has not started when the blocks are reused
            assert ops.weight_grad(w, box["x"], box["dy"], 1, 1) is None
            box.clear()                               # the operands and their words die here
            ops.amax_pool_reset()
            for _ in range(4):                        # ... and the caller's stream takes blocks of the same sizes and overwrites them
                junk.append(torch.full((nw,), 0x7f000000, dtype=torch.int32, device=dev))
                junk.append(torch.full((N, H, H, C), 3.0e30, device=dev))
            return gr
    try:
        _InBackward.apply(torch.ones(1, device=dev, requires_grad=True)).sum().backward()
        ops.wait_weight_grads()
        torch.cuda.synchronize()
    finally:
        ops.SIDE_WGRAD = prev
        torch.Tensor.record_stream = orig
        ops._AMAX_POOL_TENSORS = pool_tensors
        ops.amax_pool_reset()
    return w.grad.clone(), ref


def test_operands_and_words_survive_until_the_side_stream_has_read_them(dev):
    """the constructed, one-run form of the round-4 lifetime bug (before: a 50-episode loop that hit the race in about half
    of its runs).  With the protection - record_stream on the operands AND on the words of their maxima, ops.weight_grad - the parked
    kernel still finds its operands: its result equals the one computed in stream order, bit for bit.  With the words' protection switched
    off (the state of round 4's first version) the same construction corrupts the result: the test bites."""
    got, ref = _parked_weight_grad(dev, protect=True)
    assert torch.equal(got, ref)
    got, ref = _parked_weight_grad(dev, protect=False)
    assert not torch.equal(got, ref), "the construction no longer reproduces the hazard it guards against"


def test_words_are_protected_on_every_stream_that_reads_them(dev, monkeypatch):
    """the words of a maximum live in a pool tensor that is freed when its last word dies; every stream whose kernels touch them must be
    recorded on that tensor (torch.Tensor.record_stream), or the allocator recycles the block under a kernel that has not started:
    (1) the weight-gradient stream for the words of both operands of ops.weight_grad, (2) any stream that takes a word from a pool
    created on another stream"""
    from litemkd_amd import ops
    calls = []
    orig = torch.Tensor.record_stream

    def spy(self, s):
        calls.append((self.data_ptr(), self.dtype, s.cuda_stream))
        return orig(self, s)
    monkeypatch.setattr(torch.Tensor, "record_stream", spy)
    g = torch.Generator(device=dev).manual_seed(9)
    x = ops.amax_compute(torch.relu(torch.randn(4, 14, 14, 64, device=dev, generator=g)))
    dy = ops.amax_compute(torch.randn(4, 14, 14, 64, device=dev, generator=g))
    w = torch.nn.Parameter(torch.randn(64, 64, 3, 3, device=dev, generator=g) * 0.05)
    w.grad = torch.zeros_like(w)
    prev = ops.SIDE_WGRAD
    ops.SIDE_WGRAD = True

    class _InBackward(torch.autograd.Function):      # ops.weight_grad joins its stream at the end of the backward pass: it has to run inside one
        @staticmethod
        def forward(ctx, t):
            return t * 1.0

        @staticmethod
        def backward(ctx, gr):
            assert ops.weight_grad(w, x, dy, 1, 1) is None      # accumulated into w.grad on the weight-gradient stream
            return gr
    try:
        _InBackward.apply(torch.ones(1, device=dev, requires_grad=True)).sum().backward()
        ops.wait_weight_grads()
    finally:
        ops.SIDE_WGRAD = prev
    sw = ops._wgrad_stream(dev).cuda_stream
    for t in (x, dy):
        assert (t._lmkd_amax.data_ptr(), torch.int32, sw) in calls, "the words of an operand were not recorded on the weight-gradient stream"
    ops.amax_pool_reset()
    first = ops._amax_slot(dev)                              # a new pool, created on the current stream
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        second = ops._amax_slot(dev)                         # the same pool, from another stream
    pool_ptr = ops._AMAX_POOLS[dev.index]["buf"].data_ptr()
    assert second.data_ptr() == first.data_ptr() + 4 * first.numel()
    assert (pool_ptr, torch.int32, side.cuda_stream) in calls, "the pool was not recorded on the second stream"
    torch.cuda.synchronize()


@pytest.mark.parametrize("trained", [False, True], ids=["fresh", "trained-like"])
def test_bound_of_the_loader_side_batchnorm(dev, trained):
    """a consumer that applies relu(BatchNorm(c)) in its loader scales by a BOUND of the activation's maximum: the convolution records
    max |c| (lmkd_amax_desc::out_words: in its epilogue, or - a launch on another kernel - by a pass of its own), the statistics launch folds
    |scale| max |c| + |shift| over the channels (lmkd_amax_desc on lmkd_bn_finalize(_seg)).  The bound is never below the true maximum (an overflow of
    the fp16 planes otherwise) and, on unit-variance data, within 2^4 of it; the consumers then agree with the three-plane form to fp32
    rounding"""
    import litemkd_amd
    from litemkd_amd import ops
    g = torch.Generator(device=dev).manual_seed(10)
    for (N, seg, H, Cin, C, stride) in ((6, 0, 14, 64, 64, 1), (6, 2, 28, 64, 128, 2), (4, 0, 14, 96, 64, 1)):      # the last: 96 channels -> not the patch kernel's tiles
        x = ops.amax_compute(torch.relu(torch.randn(N, H, H, Cin, device=dev, generator=g)), seg)
        w1 = torch.randn(C, Cin, 3, 3, device=dev, generator=g) * (2.0 / (9 * Cin)) ** 0.5
        w2 = torch.randn(C, C, 3, 3, device=dev, generator=g) * (2.0 / (9 * C)) ** 0.5
        gam, bet = 1 + 0.3 * torch.randn(C, device=dev, generator=g), 0.3 * torch.randn(C, device=dev, generator=g)
        if trained:      # a trained network's tables and inputs: |gamma| ~ U(0.2, 3) of either sign, beta ~ N(0, 1), log-normal activations, weights with a 2^6 channel spread
            sg = torch.where(torch.randn(C, device=dev, generator=g) < 0, -1.0, 1.0)
            gam, bet = (0.2 + 2.8 * torch.rand(C, device=dev, generator=g)) * sg, torch.randn(C, device=dev, generator=g)
            x = ops.amax_compute(x * torch.exp(2.0 * torch.randn(N, H, H, Cin, device=dev, generator=g)), seg)
            w1 = w1 * torch.exp2(6.0 * torch.rand(C, 1, 1, 1, device=dev, generator=g) - 3.0)
        upd = []
        ops.set_defer(upd)
        try:
            c1, st1 = ops._conv_bn_train_or_eval(x, w1, Cin, stride, 1, gam, bet, torch.zeros(C, device=dev), torch.ones(C, device=dev), True, seg=seg, bound=True)
            a1 = ops.bn_apply(c1, st1, True, seg=seg)
            parts = [a1] if not seg else [a1[:seg], a1[seg:]]
            for i, p in enumerate(parts):
                bound, true = _seg_max(c1._lmkd_pre_amax, i), float(p.max())
                # the bound takes max |c1| over ALL channels for every channel: with a spread of |gamma| it is looser (each factor of two
                # costs one of the 17 binades of full precision); measured 2^0.5 .. 2^1.3 on fresh tables, recorded for the trained-like ones
                assert true <= bound <= (256 if trained else 16) * true, (N, seg, C, i, bound, true)
                import os
                if os.environ.get("LMKD_PARITY_LOG"):
                    with open(os.environ["LMKD_PARITY_LOG"], "a") as f:
                        f.write("bound / true maximum of relu(BatchNorm(c1)) [%s tables, %d frames, C %d, segment %d]: 2^%.2f\n" % (
                            "trained-like" if trained else "fresh", N, C, i, __import__("math").log2(bound / true)))
            # the consumer: conv2 with the BatchNorm in its loader, two-plane against three-plane
            n0 = _launches()
            y_h2 = ops.conv_fwd(c1, ops._pack_weights(w2, C, 0), C, 3, 3, 1, 1, True, pre_stats=st1, seg=seg)[0]
            assert _launches() - n0 == 1
            ops.set_conv_compute_dtype("fp32x3")
            y_x3 = ops.conv_fwd(c1, ops._pack_weights(w2, C, 0), C, 3, 3, 1, 1, True, pre_stats=st1, seg=seg)[0]
            ops.set_conv_compute_dtype("fp32h2")
            assert float((y_h2 - y_x3).norm() / y_x3.norm()) < 2e-6
            # ... and with an fp64 evaluation of the same convolution (the loader's BatchNorm + ReLU in fp32, as the kernels compute it)
            ref = F.conv2d(a1.permute(0, 3, 1, 2).double(), w2.double(), padding=1).permute(0, 2, 3, 1)
            assert _rel(y_h2, ref) < 1.5e-6, _rel(y_h2, ref)
        finally:
            ops.set_defer(None)


def _identity_table(C, dev):
    st = torch.zeros(5, C, device=dev)
    st[2] = 1.0      # scale 1, shift 0: lmkd_bn_apply_seg copies its input - a producer that touches every element
    return st


def test_range_fence_takes_the_three_plane_form(dev):
    """the run-time fence of the two-plane arithmetic.  A producer that is given its tensor's previous maximum counts the elements the two
    fp16 planes do not resolve fully against it (csrc/common.h amax_commit_stat); lmkd_h2_fence_eval judges the counts once per episode
    (ops.h2_fence_step) and a flagged site's maximum is withheld from the convolutions, which then run the three-plane form:
    (1) the tensor of test_one_outlier_dominating_the_maximum - one element 2^20 above the rest - is flagged in its second episode, its
        convolution falls back (lmkd_conv_h2_fallbacks counts it) and the frames the outlier misses come out at fp32 level, not 2e-3;
    (2) a log-normal tensor (sigma = 2: 18 % of its elements below 2^-17 of the maximum, but none of its mass) and a half-normal one (the
        benchmark's kind) are NOT flagged and keep the two-plane kernels."""
    import litemkd_amd
    from litemkd_amd import ops
    L = litemkd_amd.lib()
    ops.h2_fence_reset()
    g = torch.Generator(device=dev).manual_seed(11)
    N, H, C = 4, 14, 64
    w = torch.randn(C, C, 3, 3, device=dev, generator=g) * 0.05
    wp = ops._pack_weights(w, C, 0)
    st = _identity_table(C, dev)
    outlier = torch.relu(torch.randn(N, H, H, C, device=dev, generator=g))
    outlier[0, 7, 7, 0] = 2.0 ** 20
    lognormal = torch.exp(2.0 * torch.randn(N, H, H, C, device=dev, generator=g))
    halfnormal = torch.relu(torch.randn(N, H, H, C, device=dev, generator=g))
    tensors = {("y", 1): outlier, ("y", 2): lognormal, ("y", 3): halfnormal}
    for ep in range(3):
        for site, x in tensors.items():
            ops.bn_apply(x, st, False, site=site)
        ops.h2_fence_step(wait=True)
        assert ops.h2_fence_flagged() == ([] if ep == 0 else [("y", 1)]), ep      # judged from the second episode on (the first has no reference)
    for site, x in tensors.items():
        y = ops.bn_apply(x, st, False, site=site)
        assert torch.equal(y, x)
        n0, f0 = _launches(), L.value("lmkd_conv_h2_fallbacks")
        out = ops.conv_fwd(y, wp, C, 3, 3, 1, 1, True)[0]
        ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), padding=1).permute(0, 2, 3, 1)
        fell_back = site == ("y", 1)
        assert _launches() - n0 == (0 if fell_back else 1) and L.value("lmkd_conv_h2_fallbacks") - f0 == (1 if fell_back else 0), site
        assert _rel(out, ref) < 1.5e-6, (site, _rel(out, ref))
        if fell_back:
            assert _rel(out[1:], ref[1:]) < 1.5e-6, _rel(out[1:], ref[1:])      # the frames the outlier does not touch
    ops.h2_fence_step(wait=True)
    ops.h2_fence_reset()


def test_range_fence_judges_each_lane_on_its_own(dev, monkeypatch):
    """the range fence in the pipelined loop (trainloop.PipelinedEpisodes: the forward of episode i + 1, on the other lane, is queued before
    the backward of episode i).  A stand-in student writes the outlier tensor of test_range_fence_takes_the_three_plane_form at one site in
    every episode.  The h2_fence_step() of _backward(i) judges episode i's entries only - the other lane's stay pending, their producers
    need not have run - and, each lane comparing against its own previous episode, the outlier is flagged when episode 2 (the second of
    lane 0) is judged, on every run."""
    from types import SimpleNamespace
    from litemkd_amd import ops, trainloop as TL
    g = torch.Generator(device=dev).manual_seed(11)
    N, H, C = 4, 14, 64
    outlier = torch.relu(torch.randn(N, H, H, C, device=dev, generator=g))
    outlier[0, 7, 7, 0] = 2.0 ** 20
    st = _identity_table(C, dev)
    site = ("y", 1)

    class Student(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones((), device=dev))

        def forward(self, context_images, context_labels, target_images):
            ops.bn_apply(outlier, st, False, site=site)      # this episode's producer, on its lane's stream
            return {"logits": self.w * target_images.sum()}

    class Teacher(torch.nn.Module):
        def forward(self, context_features, context_labels, target_features):
            return {"logits": target_features.sum()}

    x, labels = torch.rand(1, 5, 8, device=dev), torch.arange(5, device=dev).float().unsqueeze(0)
    ep = {"support_set": x, "target_set": x, "support_set_feature_teacher": x, "target_set_feature_teacher": x,
          "support_labels": labels, "target_labels": labels}
    cfg = SimpleNamespace(device=dev, way=5, distill_name="plain")
    distiller = SimpleNamespace(plain=lambda logits, teacher_logits, target_labels: {"loss": logits})
    judged = []
    step = ops.h2_fence_step

    def spy(wait=False):
        before = sorted({e[1] for e in ops._FENCE_PENDING})
        step(wait=True)      # (this call's verdicts are taken in at once: a flag belongs to the episode judged here)
        judged.append((ops.LANE[0], before, sorted({e[1] for e in ops._FENCE_PENDING}), ops.h2_fence_flagged()))
    monkeypatch.setattr(ops, "h2_fence_step", spy)
    for run in range(3):
        ops.h2_fence_reset()
        del judged[:]
        pipe = TL.PipelinedEpisodes(Student(), Teacher(), distiller, lambda logits, target_labels: logits.detach(), cfg, depth=1)
        for _ in range(5):
            pipe.push(ep)
        pipe.flush()
        torch.cuda.synchronize()
        assert [j[:3] for j in judged] == [(0, [0, 1], [1]), (1, [0, 1], [0]), (0, [0, 1], [1]), (1, [0, 1], [0]), (0, [0], [])], (run, judged)
        assert [j[3] for j in judged] == [[], [], [site], [site], [site]], (run, judged)
    ops.h2_fence_reset()


@pytest.mark.parametrize("frames,H,seg", [(37, 56, 0), (64, 56, 23), (400, 14, 0), (5, 7, 2)])
def test_persistent_layer1_kernel_equals_one_workgroup_per_tile(dev, frames, H, seg):
    """round 5: the two-plane launches with Cout <= 64 run conv_patch_x3_kernel<.., 3, ..> (v_mfma_f32_32x32x16_f16) with PERSISTENT workgroups -
    each walks several tiles and requests its next tile's first patch chunk during the current tile's last.  Same tiles, same fragment and
    summation order: forward (with BatchNorm partial sums and the recorded maximum), data gradient plain, accumulating, and with the
    BatchNorm-backward sums in its epilogue are bit-identical to one workgroup per tile (lmkd_conv_set_persistent(0)); ragged last tiles and
    two frame segments included (the tile count at 37 x 56 x 56 is not a multiple of anything)."""
    import litemkd_amd
    from litemkd_amd import ops
    L = litemkd_amd.lib()
    g = torch.Generator(device=dev).manual_seed(5)
    C = 64
    x = torch.relu(torch.randn(frames, H, H, C, device=dev, generator=g))
    dy = torch.randn(frames, H, H, C, device=dev, generator=g) * 1e-2
    w = torch.randn(C, C, 3, 3, device=dev, generator=g) * (2.0 / (9 * C)) ** 0.5
    res = torch.randn(frames, H, H, C, device=dev, generator=g)
    ops.amax_compute(x, seg)
    ops.amax_compute(dy, seg)
    wp, wd = ops._pack_weights(w, C, 0), ops._pack_weights(w, C, 1)

    # the loader-side BatchNorm + ReLU instance (PRE): rows 2 / 3 of a [segments][5][C] table are scale / shift
    table = torch.zeros(2 if seg else 1, 5, C, device=dev)
    table[:, 2] = torch.rand(table.shape[0], C, device=dev, generator=g) * 0.5 + 0.5
    table[:, 3] = torch.rand(table.shape[0], C, device=dev, generator=g) * 0.2 - 0.1
    xr = torch.empty_like(x)      # max |relu(bn(x))| per segment: what lmkd_bn_finalize's bound stands for in the product (ops._amax_ptr(pre=True))
    for sgi, (f0, f1) in enumerate(((0, seg), (seg, frames)) if seg else ((0, frames),)):
        xr[f0:f1] = torch.relu(x[f0:f1] * table[sgi, 2] + table[sgi, 3])
    x._lmkd_pre_amax = ops.amax_compute(xr, seg)._lmkd_amax
    table = table if seg else table[0]

    def run():
        words = ops._amax_slot(dev)
        y, st = ops.conv_fwd(x, wp, C, 3, 3, 1, 1, True, seg=seg, amax_out=words)[:2]
        ypre = ops.conv_fwd(x, wp, C, 3, 3, 1, 1, True, pre_stats=table, seg=seg)[0]
        dx = ops.conv_bwd_data(dy, wd, x.shape, C, 3, 3, 1, 1, seg=seg)
        acc = res.clone()
        ops.conv_bwd_data(dy, wd, x.shape, C, 3, 3, 1, 1, out=acc, accumulate=True, seg=seg)
        torch.cuda.synchronize()
        return y, st, _seg_max(words, 0), _seg_max(words, 1), dx, acc, ypre
    try:
        n0 = _launches()
        a = run()
        assert _launches() - n0 == 4
        L.call("lmkd_conv_set_persistent", 0)
        b = run()
    finally:
        L.call("lmkd_conv_set_persistent", 1)
    for u, v in zip(a, b):
        if torch.is_tensor(u):
            assert torch.equal(u, v)
        else:
            assert u == v
    assert _rel(a[0], _ref3(x, w, dy)[0]) < 1.5e-6


def test_scatter_epilogue_of_the_32x32_two_plane_kernel(dev):
    """lmkd_conv_set_patch16(0) sends every two-plane patch launch to conv_patch_x3_kernel<.., 3, ..>, also the stride-2 data gradient whose
    four parity classes scatter their rows (the epilogue's table path; the plain launches compute their offsets) and the 128-column tiles:
    against fp64, and against the 16x16x32 kernel's result (same arithmetic, another summation order)."""
    import litemkd_amd
    from litemkd_amd import ops
    L = litemkd_amd.lib()
    g = torch.Generator(device=dev).manual_seed(6)
    N, H, Ci, Co = 12, 28, 64, 128
    dy = torch.randn(N, H // 2, H // 2, Co, device=dev, generator=g) * 1e-2
    w = torch.randn(Co, Ci, 3, 3, device=dev, generator=g) * (2.0 / (9 * Ci)) ** 0.5
    ops.amax_compute(dy, 0)
    wd = ops._pack_weights(w, Ci, 1)
    xd = torch.zeros(N, Ci, H, H, device=dev, dtype=torch.float64, requires_grad=True)
    F.conv2d(xd, w.double(), stride=2, padding=1).backward(dy.permute(0, 3, 1, 2).double())
    ref = xd.grad.permute(0, 2, 3, 1)
    out = {}
    try:
        for p16 in (1, 0):
            L.call("lmkd_conv_set_patch16", p16)
            n0 = _launches()
            out[p16] = ops.conv_bwd_data(dy, wd, (N, H, H, Ci), Co, 3, 3, 2, 1)
            torch.cuda.synchronize()
            assert _launches() - n0 == 1
    finally:
        L.call("lmkd_conv_set_patch16", 1)
    assert _rel(out[0], ref) < 1.5e-6 and _rel(out[1], ref) < 1.5e-6
    assert _rel(out[0], out[1].double()) < 1e-6

