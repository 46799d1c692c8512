"""Tensor-level wrappers over the C ABI (include/lmkd.h) and the autograd Functions that tie
the HIP kernels into torch.autograd.  torch is plumbing here (device memory, stream, autograd
graph); all arithmetic of the hot path happens in liblmkd_hip.so.

Activations are NHWC fp32.  Every wrapper checks device/dtype/contiguity and raises on misuse."""
import ctypes
import functools
import os
import itertools
import math

import torch

from ._lib import lib
from . import _audit


# ------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------
def _raw_stream(device_index=None):
    """the current HIP stream of the (current) device as an integer handle: torch.cuda.current_stream() builds a Stream object and
    resolves the device through four Python layers (7.6 us, 230 times per episode: 1.75 ms of the forward's host time); the raw
    binding costs 0.3 us"""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice() if device_index is None else device_index)


def _stream():
    return ctypes.c_void_p(_raw_stream())


def _p(t):
    if t is None:
        return None
    if _audit.ON:
        _audit.note(t)
    return ctypes.c_void_p(t.data_ptr())


def _pw(t):
    """address of a tensor as a plain integer (the members of AmaxDesc, pointer arrays), noted for the stream-lifetime audit like _p"""
    if t is None:
        return None
    if _audit.ON:
        _audit.note(t)
    return t.data_ptr()


def _chk(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("lite-mkd_amd ops need CUDA(HIP) tensors; got a %s tensor — the HIP hot path has no CPU fallback" % t.device)
        if t.dtype not in (torch.float32, torch.int64, torch.int32, torch.uint8, torch.int16, torch.bfloat16):
            raise RuntimeError("unsupported dtype %s" % t.dtype)
        if not t.is_contiguous():
            raise RuntimeError("non-contiguous tensor passed to a HIP op")


def _ints(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _f32(x):
    return ctypes.c_float(float(x))


def _empty(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


# Storage type of the trunk's activation / activation-gradient tensors in HBM (lmkd_set_activation_dtype): fp32, or bf16 for
# BASELINE configs[2] (the reference trains under autocast).  Statistics, weights, weight gradients and everything after the pooled
# head stay fp32.
_ACT_DTYPE = [torch.float32]


def set_activation_dtype(name):
    """'fp32' | 'bf16' (needs set_conv_compute_dtype('bf16'))"""
    modes = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16)}
    if name not in modes:
        raise ValueError(name)
    lib().call("lmkd_set_activation_dtype", modes[name][0])
    _ACT_DTYPE[0] = modes[name][1]


def get_activation_dtype():
    return "bf16" if _ACT_DTYPE[0] is torch.bfloat16 else "fp32"


def _empty_act(shape, like):
    return torch.empty(shape, dtype=_ACT_DTYPE[0], device=like.device)


# ------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------
def gemm(layA, layB, M, N, K, A, lda, B, ldb, C, ldc, alpha=1.0, beta=0.0, bias=None, relu=False,
         batch=1, sA=0, sB=0, sC=0, A_off=0, B_off=0, C_off=0, split_k=None, k_block=0):
    """C = alpha*op(A)*op(B) + beta*C + bias.  *_off are element offsets into the tensors' storage.
    split_k: True / False forces lmkd_gemm_f32_splitk / lmkd_gemm_f32 for this call (None: the module default GEMM_SPLIT_K).
    k_block (a multiple of 4, 0: off): sum K in blocks of that many terms, one launch per block, each adding its product of a fresh
    accumulator to C in the epilogue (beta = 1; bias and ReLU with the last).  A kernel's accumulator takes its K terms one after the
    other, so its rounding error grows like K; in blocks it grows like sqrt(K k_block), which is what a blocked CPU GEMM has."""
    if k_block and K > k_block:
        for k0 in range(0, K, k_block):
            kk, last = min(k_block, K - k0), k0 + k_block >= K
            gemm(layA, layB, M, N, kk, A, lda, B, ldb, C, ldc, alpha, beta if k0 == 0 else 1.0, bias if last else None, relu and last,
                 batch, sA, sB, sC, A_off + (k0 if layA == "K" else k0 * lda), B_off + (k0 if layB == "K" else k0 * ldb), C_off, split_k, 0)
        return C
    _chk(A, B, C, bias)
    es = 4
    if _audit.ON:
        for t in (A, B, C):
            _audit.note(t)
    if GEMM_SPLIT_K if split_k is None else split_k:
        ws, tk = _gemm_workspace(C)
        lib().call("lmkd_gemm_f32_splitk", layA.encode(), layB.encode(), M, N, K, _f32(alpha),
                   ctypes.c_void_p(A.data_ptr() + A_off * es), lda, sA,
                   ctypes.c_void_p(B.data_ptr() + B_off * es), ldb, sB, _f32(beta),
                   ctypes.c_void_p(C.data_ptr() + C_off * es), ldc, sC, _p(bias), int(relu), batch, _p(ws), ws.numel(), _p(tk), _stream())
        return C
    lib().call("lmkd_gemm_f32", layA.encode(), layB.encode(), M, N, K, _f32(alpha),
               ctypes.c_void_p(A.data_ptr() + A_off * es), lda, sA,
               ctypes.c_void_p(B.data_ptr() + B_off * es), ldb, sB, _f32(beta),
               ctypes.c_void_p(C.data_ptr() + C_off * es), ldc, sC, _p(bias), int(relu), batch, _stream())
    return C


def _gemm_in_blocks(k_block):
    """gemm with this k_block where the call passes none"""
    return functools.partial(gemm, k_block=k_block) if k_block else gemm


# split-K workspace (32 MB) + ticket words of lmkd_gemm_f32_splitk, one pair per (device, stream): GEMMs of two streams may run together.
# OFF by default: alone, the 32-tile fc GEMMs run twice as fast split (tools/gemm_splitk_bench.py), inside the episode the same-box A/B
# reads 34.24 / 34.21 / 34.18 episodes/s with it against 34.43 / 34.33 / 34.34 without (they overlap the other trunk call's kernels).
GEMM_SPLIT_K = False
_GEMM_WS = {}


def _gemm_workspace(like):
    key = (like.device.index, _raw_stream(like.device.index))
    e = _GEMM_WS.get(key)
    if e is None:
        e = _GEMM_WS[key] = (torch.empty(32 << 20, dtype=torch.uint8, device=like.device),
                             torch.zeros(lib().value("lmkd_gemm_ticket_words"), dtype=torch.int32, device=like.device))
    return e


def stack_rows(a, b):
    """[a; b] along dim 0 for 2-D row-major tensors.  When b starts exactly where a ends in the SAME storage (the two halves of one
    tensor: the support / query rows of the pooled features and of the fc outputs, which autograd hands back as two views) the result is
    a view of that storage - no cat launch, no copy; otherwise torch.cat."""
    if (a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[1] and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous()
            and a.numel() > 0 and b.numel() > 0 and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and a.storage_offset() + a.numel() == b.storage_offset()):
        return torch.as_strided(a, (a.shape[0] + b.shape[0], a.shape[1]), (a.shape[1], 1), a.storage_offset())
    return torch.cat([a, b], 0)


def linear_fwd(x, w, b, k_block=0):
    """y[M,N] = x[M,K] w[N,K]^T + b"""
    M, K = x.shape
    N = w.shape[0]
    y = _empty((M, N), x)
    return gemm("K", "K", M, N, K, x, K, w, K, y, N, bias=b, k_block=k_block)


# Ticket buffers of the single-launch column reductions (lmkd_ticket_words() zeroed int32 words, left zeroed by every launch): one
# per (device, stream), because launches of two streams may run at the same time.
_TICKETS = {}


def _tickets(like):
    key = (like.device.index, _raw_stream(like.device.index))
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS[key] = torch.zeros(lib().value("lmkd_ticket_words"), dtype=torch.int32, device=like.device)
    return t


COLSUM_MAX_COLS = 16384      # lmkd_colsum: cdiv(C, 32) ticket words of 512


def colsum(a, b=None, out=None, accumulate=False):
    """out[c] (+)= sum_r a[r, c] (* b[r, c]).  lmkd_colsum takes 16384 columns; a wider tensor (the 18432-wide in_proj bias gradient of the
    MFM teacher's three-modality fusion) goes through it in column blocks, each copied to a contiguous tensor first."""
    rows, C = a.shape
    if out is None:
        out = _empty((C,), a)
        accumulate = False
    if C > COLSUM_MAX_COLS:
        for c0 in range(0, C, COLSUM_MAX_COLS):
            c1 = min(C, c0 + COLSUM_MAX_COLS)
            colsum(a[:, c0:c1].contiguous(), None if b is None else b[:, c0:c1].contiguous(), out[c0:c1], accumulate)
        return out
    _chk(a, b, out)
    ws = torch.empty(lib().value("lmkd_colsum_workspace", C), dtype=torch.uint8, device=a.device)
    lib().call("lmkd_colsum", _p(a), _p(b), _p(out), rows, C, int(accumulate), _p(ws), _p(_tickets(a)), _stream())
    return out


# Direct gradient accumulation (DIRECT_PARAM_GRAD, switched on by the loops that own a FusedOptimizer, like SIDE_WGRAD): the fused
# Functions add the gradients of BatchNorm / Linear / TRX parameters INTO the parameters' .grad inside their own kernels (the
# BatchNorm coefficient kernel, the GEMM's beta = 1 epilogue, the column-sum kernel) and hand autograd None - ~100 ATen add launches
# per episode less on the critical stream.  The two trunk calls of an episode run on two streams and meet the same BatchNorm
# parameters: the call on the side stream accumulates into a SHADOW of the gradient buffer (FlatParams.shadow, registered here per
# parameter), which the optimizer adds to the real one before it steps - no two streams ever add to the same address.
DIRECT_PARAM_GRAD = False
_GRAD_SLOT = {}


def register_grad_slot(param, shadow_view):
    """param.grad (a view into the flat gradient buffer) may be accumulated into directly; shadow_view: the same view of the
    shadow buffer for kernels that run on the side stream"""
    _GRAD_SLOT[param.data_ptr()] = (weakref.ref(param), shadow_view)


def _grad_target(param):
    """-> tensor to accumulate this parameter's gradient into, or None (autograd path)"""
    if not DIRECT_PARAM_GRAD or param is None or not param.requires_grad:
        return None
    e = _GRAD_SLOT.get(param.data_ptr())
    if e is None or e[0]() is not param or param.grad is None or _has_hooks(param):
        return None
    # kernels of the side stream (query-frame trunk call: BatchNorm parameters) and of the auxiliary stream (second TRX head: TRX
    # parameters) add to the shadow buffer, everything on the caller's stream to .grad: no address is ever added to from two streams
    dev = param.device.index
    return e[1] if stream_role(_raw_stream(dev)) in ((dev, "side"), (dev, "aux")) else param.grad


# Inference Linear on the bf16-plane convolution kernels: y = relu?(x W^T + b) is a 1x1 convolution over M one-pixel "frames" whose
# BatchNorm-affine epilogue (lmkd_conv2d_fwd_bn: acc * scale + shift, ReLU) carries scale = 1, shift = b.  In the library's default
# arithmetic (fp32 as 3 x bf16) this runs the MFM teacher's 0.57 TFLOP of encoder GEMMs on the bf16 matrix pipe instead of the
# fp32 MFMA of gemm_kernel; the packed / split weights of the frozen modules are cached like the trunk's.
_AFFINE_CACHE = {}


def linear_infer(x, w, b=None, relu=False):
    M, K = x.shape
    N = w.shape[0]
    cd = lib().value("lmkd_conv_get_compute_dtype")
    if cd == 0 or K % 32 != 0 or N % 32 != 0 or _ACT_DTYPE[0] is not torch.float32 or torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
        y = _empty((M, N), x)
        return gemm("K", "K", M, N, K, x, K, w, K, y, N, bias=b, relu=relu)
    _chk(x, w, b)
    mark_cacheable(w)
    wp = _pack_linear(w, w.view(N, K, 1, 1), K)
    # [5][N] epilogue table (scale = 1, shift = bias), cached per bias TENSOR (identity checked through a weak reference: a recycled
    # device address must never return another module's bias) and in-place version
    key = (b.data_ptr() if b is not None else 0, N, str(x.device))
    hit = _AFFINE_CACHE.get(key)
    if hit is not None and (hit[0] is None) == (b is None) and (b is None or (hit[0]() is b and hit[1] == b._version)):
        st = hit[2]
    else:
        st = torch.zeros((5, N), dtype=torch.float32, device=x.device)
        st[2].fill_(1.0)
        if b is not None:
            st[3].copy_(b)
        if len(_AFFINE_CACHE) > 256:
            _AFFINE_CACHE.clear()
        _AFFINE_CACHE[key] = (weakref.ref(b) if b is not None else None, b._version if b is not None else 0, st)
    y = _empty((M, N), x)
    lib().call("lmkd_conv2d_fwd_bn", _p(x), _p(wp), _p(y), _p(st), None, int(relu), M, 1, 1, K, N, 1, 1, 1, 0, _stream(), None)
    return y


def _pack_linear(w, w4, K):
    """pack cache entry of a 2-D Linear weight, packed as the [N, K, 1, 1] convolution weight it is"""
    e = _pack_cache[w.data_ptr()]
    tag = (w._version, WEIGHT_EPOCH[0])
    key = (K, 0, lib().value("lmkd_conv_get_compute_dtype"))
    cur = torch.cuda.current_stream()
    hit = e["packs"].get(key)
    if hit is not None and hit[0] == tag:
        if hit[3] is not None and hit[3] != cur.cuda_stream:
            cur.wait_event(hit[2])
        return hit[1]
    wp = _pack_weights(w4, K, 0, out=hit[1] if hit is not None else None)
    _audit.audit_ok(wp, "cached pack: lives with its parameter (re-packed in place); readers on other streams wait for the pack's event")
    ev = torch.cuda.Event()
    ev.record(cur)
    e["packs"][key] = (tag, wp, ev, cur.cuda_stream)
    return wp


class LinearFn(torch.autograd.Function):
    """nn.Linear (resnet18_2fc.py:56-64 fc1/fc2).  fwd/dgrad/wgrad on the MFMA GEMM, bias grad = column sum.
    k_block: gemm's, for the forward and the input gradient (the weight gradient sums over the rows)."""

    @staticmethod
    def forward(ctx, x, w, b, k_block=0):
        x = x.contiguous()
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        ctx.bias = b
        ctx.k_block = k_block
        return linear_fwd(x, w.contiguous(), b, k_block)

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        M, K = x.shape
        N = w.shape[0]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _empty((M, K), x)
            gemm("K", "N", M, K, N, dy, N, w, K, dx, K, k_block=ctx.k_block)          # dx = dy @ W
        if ctx.needs_input_grad[1]:          # dW = dy^T @ x
            dw = deliver_wgrad(w, lambda t, beta: gemm("M", "N", N, K, M, dy, N, x, K, t, K, beta=beta), (N, K), dy, x)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = deliver_colsum(ctx.bias, dy)
        return dx, dw, db, None


# fc1 / fc2 over the support-frame and the query-frame features (resnet18_2fc.py:56-64: four nn.Linear calls on 200-row inputs) as ONE
# autograd node: the rows of the two trunk calls are stacked, so each weight sees one 400-row GEMM forward and one for the weight
# gradient, and the input gradient of BOTH heads is one GEMM over the concatenated K = 2 x 2048 (split-K: 56 output tiles) instead of
# four 32-workgroup launches of 56 us each in the idle stretch between the heads' and the trunk's backward.
FUSE_TWO_HEAD_LINEAR = True


class TwoHeadLinearFn(torch.autograd.Function):
    """X = the pooled features of the support frames (rows [0, Nc)) followed by those of the query frames.
    k_block: gemm's, for the forward and the input gradient, as LinearFn's"""

    @staticmethod
    def forward(ctx, X, Nc, w1, b1, w2, b2, k_block=0):
        X = X.contiguous()
        M, K = X.shape
        N = w1.shape[0]
        Y1, Y2 = _empty((M, N), X), _empty((M, N), X)
        gemm("K", "K", M, N, K, X, K, w1, K, Y1, N, bias=b1, k_block=k_block)
        gemm("K", "K", M, N, K, X, K, w2, K, Y2, N, bias=b2, k_block=k_block)
        ctx.save_for_backward(X, w1, w2)
        ctx.Nc = Nc
        ctx.k_block = k_block
        ctx.params = (w1, b1, w2, b2)
        return Y1[:Nc], Y1[Nc:], Y2[:Nc], Y2[Nc:]

    @staticmethod
    def backward(ctx, g1c, g1t, g2c, g2t):
        _audit.engine_owned(g1c, g1t, g2c, g2t)
        X, w1, w2 = ctx.saved_tensors
        pw1, pb1, pw2, pb2 = ctx.params
        M, K = X.shape
        N = w1.shape[0]
        Nc = ctx.Nc

        def full(gc, gt):
            if gc is None and gt is None:
                return None
            gc = gc if gc is not None else torch.zeros((Nc, N), dtype=X.dtype, device=X.device)
            gt = gt if gt is not None else torch.zeros((M - Nc, N), dtype=X.dtype, device=X.device)
            return stack_rows(gc.contiguous(), gt.contiguous())      # the TRX head returns the two halves of ONE gradient tensor: a view
        G = [full(g1c, g1t), full(g2c, g2t)]
        dX = None
        if ctx.needs_input_grad[0]:
            live = [(g, w) for g, w in zip(G, (w1, w2)) if g is not None]
            dX = _empty((M, K), X)
            if live:                # dX = G1 @ W1 (+ G2 @ W2 accumulated in the second GEMM's epilogue: no cat of the gradients / weights)
                for i, (g, w) in enumerate(live):
                    gemm("K", "N", M, K, N, g, N, w, K, dX, K, beta=0.0 if i == 0 else 1.0, k_block=ctx.k_block)
            else:
                dX.zero_()
        outs = [dX if ctx.needs_input_grad[0] else None, None]
        for g, pw, pb in zip(G, (pw1, pw2), (pb1, pb2)):
            dw = db = None
            if g is not None:
                if pw.requires_grad:
                    dw = deliver_wgrad(pw, lambda t, beta, g=g: gemm("M", "N", N, K, M, g, N, X, K, t, K, beta=beta), (N, K), g, X)
                if pb is not None and pb.requires_grad:
                    db = deliver_colsum(pb, g)
            outs += [dw, db]
        return tuple(outs) + (None,)


def two_head_linear_x(X, Nc, fc1, fc2):
    """X [Nc + Nt, K] = support-frame rows followed by query-frame rows -> fc1(X[:Nc]), fc1(X[Nc:]), fc2(X[:Nc]), fc2(X[Nc:]).
    The modules' `gemm_k_block` attribute, where set (module_k_block), is the GEMMs' k_block"""
    if FUSE_TWO_HEAD_LINEAR and X.is_cuda and X.dim() == 2 and fc1.weight.shape == fc2.weight.shape and fc1.bias is not None and fc2.bias is not None:
        return TwoHeadLinearFn.apply(X, Nc, fc1.weight, fc1.bias, fc2.weight, fc2.bias, fc1.__dict__.get("gemm_k_block", 0))
    cf, tf = X[:Nc], X[Nc:]
    return fc1(cf), fc1(tf), fc2(cf), fc2(tf)


def two_head_linear(cf, tf, fc1, fc2):
    """-> fc1(cf), fc1(tf), fc2(cf), fc2(tf)"""
    return two_head_linear_x(torch.cat([cf, tf], 0), cf.shape[0], fc1, fc2)


# ------------------------------------------------------------------------------------------
# convolution pieces
# ------------------------------------------------------------------------------------------
# Packed weights of module parameters are cached: the two trunk calls of an episode and all episodes between two optimizer
# steps reuse them.  Only parameters that a module has registered with mark_cacheable() are cached (identity is checked
# through a weak reference, so a recycled device address can never return another tensor's pack); the cache entry is
# validated by the parameter's in-place `_version` (torch optimizers, load_state_dict) and by WEIGHT_EPOCH, which the
# fused HIP optimizer bumps because it updates the flat buffer through raw pointers.
import weakref

WEIGHT_EPOCH = [0]
_pack_cache = {}


def mark_cacheable(param):
    ptr = param.data_ptr()
    e = _pack_cache.get(ptr)
    if e is None or e["ref"]() is not param:
        _pack_cache[ptr] = {"ref": weakref.ref(param), "packs": {}}


def pack_weights(w, Cs, mode):
    e = _pack_cache.get(w.data_ptr())
    owner = e["ref"]() if e is not None else None
    if owner is None or owner.data_ptr() != w.data_ptr() or owner.shape != w.shape:
        return _pack_weights(w, Cs, mode)
    tag = (owner._version, WEIGHT_EPOCH[0])
    key = (Cs, mode, lib().value("lmkd_conv_get_compute_dtype"))      # one persistent buffer per arithmetic mode
    hit = e["packs"].get(key)
    if hit is not None and hit[0] == tag:
        if hit[3] is not None and hit[3] != _raw_stream():
            torch.cuda.current_stream().wait_event(hit[2])            # packed on the other stream: order this stream behind the pack kernel
        return hit[1]
    cur = torch.cuda.current_stream()
    # stale or missing: (re)pack - into the SAME buffer when there is one, so that its address stays valid for a captured hipGraph
    # (trainloop.GraphedEpisode) and the allocator is left alone
    wp = _pack_weights(w, Cs, mode, out=hit[1] if hit is not None else None)
    _audit.audit_ok(wp, "cached pack: lives with its parameter (re-packed in place); readers on other streams wait for the pack's event")
    ev = torch.cuda.Event()
    ev.record(cur)
    e["packs"][key] = (tag, wp, ev, cur.cuda_stream)
    return wp


_REPACK_KEEP = [None]


def refresh_packs(streams=()):
    """Re-pack, on the current stream and IN PLACE, every cached pack of the current arithmetic mode whose weights have changed since
    (optimizer step, in-place update), make `streams` wait for it and mark the packs as visible everywhere.  A captured episode
    calls pack_weights() during capture and must find every pack valid (no pack kernel inside the graph): GraphedEpisode calls this
    before capture and before every replay."""
    cur = torch.cuda.current_stream()
    cd = lib().value("lmkd_conv_get_compute_dtype")
    n = 0
    stale = []      # (weight, planes, (Cout, Cin, Cs, KH, KW, mode)): re-packed by ONE launch in the bf16-plane modes
    for e in _pack_cache.values():
        owner = e["ref"]()
        if owner is None:
            continue
        tag = (owner._version, WEIGHT_EPOCH[0])
        for key, hit in e["packs"].items():
            if key[2] != cd:
                continue
            if hit[0] != tag:
                if cd == 0 or owner.dim() != 4 or not owner.is_contiguous() or owner.dtype != torch.float32:
                    _pack_weights(owner.view(owner.shape[0], -1, 1, 1) if owner.dim() == 2 else owner, key[0], key[1], out=hit[1])
                else:
                    stale.append((owner, hit[1], tuple(owner.shape[:2]) + (key[0],) + tuple(owner.shape[2:]) + (key[1],)))
                n += 1
            if hit[0] != tag or hit[3] is not None:
                e["packs"][key] = (tag, hit[1], hit[2], None)
    if stale:
        m = len(stale)
        ws = (ctypes.c_void_p * m)(*[t[0].data_ptr() for t in stale])
        wfs = (ctypes.c_void_p * m)(*[t[1].data_ptr() for t in stale])
        dims = (ctypes.c_int * (6 * m))(*[v for t in stale for v in t[2]])
        lib().call("lmkd_conv2d_repack_multi", ws, wfs, dims, m, _stream())
        _REPACK_KEEP[0] = stale      # the weights / planes stay referenced until the next refresh (the launch reads them asynchronously)
    with (_x3_scope() if _WCAT else contextlib.nullcontext()):      # concatenated TRX projection weights (_trx_wcat_packs; opt-in): three-plane packs also in the one-plane mode
        cdx = lib().value("lmkd_conv_get_compute_dtype")
        for key, e in _WCAT.items():
            wk, wv = e["rk"](), e["rv"]()
            if wk is None or wv is None or key[2] != cdx:
                continue
            if e["tag"] != (wk._version, wv._version, WEIGHT_EPOCH[0]):
                _wcat_build(e, wk, wv)
                n += 1
            e["stream"] = None
    for s in streams:
        s.wait_stream(cur)
    return n


# ---- fp32 as two fp16 planes ('fp32h2', lmkd_conv_set_compute_dtype(4); csrc/conv_patch16.h) ----
# The kernels scale an operand by a power of two taken from max |operand|.  The maximum of a trunk tensor is folded into a device word
# by the kernel that WRITES the tensor (BatchNorm apply, BatchNorm backward apply, the stem's pooling: lmkd_amax_desc::out_words) and travels
# with the tensor as the attribute `_lmkd_amax`; a convolution whose operands carry it runs the two-plane form (lmkd_amax_desc::x_words /
# dy_words), any other launch - a tensor from elsewhere, a view - the three-plane form: both fp32-class, so a lost word costs time, never
# correctness.
_AMAX_POOLS = {}
_AMAX_WORDS = [0]
_AMAX_POOL_TENSORS = 256      # maxima per pool (8 KB each: 2 frame segments x 64 slots x 64 bytes, csrc/common.h amax_commit)


def _h2_mode():
    return lib().value("lmkd_conv_get_compute_dtype") == 4


def _amax_slot(dev):
    """the zeroed words of one maximum (lmkd_amax_words(): per frame segment, 64 slots that the producer's waves fold their maxima into)
    as an int32 view of a pool; the pool is zeroed once, on the stream that first needs it (every other stream waits for that), and
    inside a hipGraph capture it is a pool of the capture, so a replay zeroes it again"""
    if not _AMAX_WORDS[0]:
        _AMAX_WORDS[0] = lib().value("lmkd_amax_words")
    nw = _AMAX_WORDS[0]
    cap = torch.cuda.is_current_stream_capturing()
    cur = torch.cuda.current_stream(dev)
    p = _AMAX_POOLS.get(dev.index)
    if p is None or p["next"] + nw > p["buf"].numel() or p["cap"] != cap:
        buf = torch.zeros(_AMAX_POOL_TENSORS * nw, dtype=torch.int32, device=dev)
        ev = torch.cuda.Event()
        ev.record(cur)
        p = _AMAX_POOLS[dev.index] = {"buf": buf, "next": 0, "cap": cap, "event": ev, "seen": {cur.cuda_stream}}
    if cur.cuda_stream not in p["seen"]:
        cur.wait_event(p["event"])
        p["buf"].record_stream(cur)      # the pool's block must not be recycled under kernels of this stream (it is freed when its last word dies)
        p["seen"].add(cur.cuda_stream)
    i = p["next"]
    p["next"] = i + nw
    return p["buf"][i:i + nw]


_AMAX_UNIT = {}


def _amax_unit_words(dev):
    """the words of a maximum equal to 1.0 in both frame segments (constant; one tensor per device)"""
    w = _AMAX_UNIT.get(dev.index)
    if w is None:
        nw = lib().value("lmkd_amax_words")
        w = torch.zeros(nw, dtype=torch.int32, device=dev)
        w[0] = 0x3f800000
        w[nw // 2] = 0x3f800000
        _AMAX_UNIT[dev.index] = w
    return w


def amax_pool_reset():
    """the next word comes from a new pool (a hipGraph capture: each graph zeroes the pool its own words live in)"""
    _AMAX_POOLS.clear()


class AmaxDesc(ctypes.Structure):
    """include/lmkd.h lmkd_amax_desc: the range bookkeeping of one launch (explicit argument of the *_seg entry points)"""
    _fields_ = [("x_words", ctypes.c_void_p), ("dy_words", ctypes.c_void_p), ("out_words", ctypes.c_void_p), ("ref_words", ctypes.c_void_p),
                ("flags", ctypes.c_int)]


AMAX_FENCED = 1


def _desc_arg(d):
    return ctypes.byref(d) if d is not None else None


# The range fence of the two-plane arithmetic.  Every tensor a producer writes belongs to a SITE - ("y" | "a" | "d" | "p", data_ptr of the
# BatchNorm weight whose output / gradient / loader-side bound it is).  A site owns persistent reference words (the maximum its tensor had
# in the previous episode); the producer counts, against that reference, how much of the tensor the two fp16 planes do not resolve fully
# (csrc/common.h amax_commit_stat) and h2_fence_step() - once per episode, no host synchronisation: the verdict is read an episode or two
# later - lets lmkd_h2_fence_eval judge the counts.  A flagged site stays flagged (h2_fence_reset() clears): its tensor's maximum is
# withheld from the convolutions, which then run the three-plane form, and lmkd_conv_h2_fallbacks() counts those launches.
# Per lane (LANE): a pending entry carries the lane it was written on and only that lane's h2_fence_step() judges it - on the lane's
# stream, which is ordered behind that episode's producers and no other's - and a site keeps reference words per lane, so no evaluation
# writes words that another lane's producers read.  The sequential loop runs on lane 0 alone; in the pipelined loop each lane compares
# against its own previous episode.
H2_FENCE = os.environ.get("LMKD_H2_FENCE", "1") != "0"      # (bench.py A/B: LMKD_H2_FENCE=0 runs the two-plane arithmetic unfenced)
_FENCE_SITES = {}        # site -> {"ref": {lane: persistent words}, "bad": bool}
_FENCE_PENDING = []      # (site, lane, words) written since that lane's last h2_fence_step()
_FENCE_INFLIGHT = []     # (event, pinned host flags, [sites], keep-alive)


def _fence_watch(site, words, dev):
    """a launch is about to write the words of a tensor of `site` (None: not fenced): in training, outside a capture, they wait for this
    lane's next h2_fence_step() -> address of the lane's reference words of the site, for the launch to count against (else None)"""
    if site is None or not (H2_FENCE and torch.is_grad_enabled()) or torch.cuda.is_current_stream_capturing():
        return None
    if len(_FENCE_PENDING) > 4096:      # nobody calls h2_fence_step(): keep the newest
        del _FENCE_PENDING[:2048]
    refs = _FENCE_SITES.setdefault(site, {"ref": {}, "bad": False})["ref"]
    if LANE[0] not in refs:
        refs[LANE[0]] = torch.zeros(lib().value("lmkd_amax_words"), dtype=torch.int32, device=dev)
        _audit.audit_ok(refs[LANE[0]], "persistent: a site's reference words are never freed")
    _FENCE_PENDING.append((site, LANE[0], words))
    return refs[LANE[0]].data_ptr()


def h2_fence_reset():
    """forget every verdict and reference (a new model, another data distribution)"""
    _FENCE_SITES.clear()
    del _FENCE_PENDING[:]
    del _FENCE_INFLIGHT[:]


def h2_fence_flagged():
    """the sites the fence has flagged so far"""
    return sorted(k for k, e in _FENCE_SITES.items() if e["bad"])


def _fence_poll(wait=False):
    keep = []
    for ev, host, sites, alive in _FENCE_INFLIGHT:
        if wait:
            ev.synchronize()
        if not ev.query():
            keep.append((ev, host, sites, alive))
            continue
        for site, f in zip(sites, host.tolist()):
            if f:
                _FENCE_SITES[site]["bad"] = True
    _FENCE_INFLIGHT[:] = keep


def h2_fence_step(wait=False):
    """judge the tensors this lane (LANE) has written since its last call (one small launch + one 4-bytes-per-tensor copy to pinned memory,
    both asynchronous) and take in the verdicts that have arrived.  Call once per episode, under the episode's lane, on a stream that is
    ordered behind the episode's producers (after backward()).  wait=True (tests, bench.py): also wait for every verdict in flight."""
    if not _FENCE_PENDING and not _FENCE_INFLIGHT:
        return
    if torch.cuda.is_current_stream_capturing():
        return
    _fence_poll()
    lane = LANE[0]
    pend = [e for e in _FENCE_PENDING if e[1] == lane]
    if pend:
        _FENCE_PENDING[:] = [e for e in _FENCE_PENDING if e[1] != lane]
        n = len(pend)
        dev = pend[0][2].device
        P = ctypes.c_void_p * n
        words = P(*[w.data_ptr() for _, _, w in pend])
        refs = P(*[_FENCE_SITES[site]["ref"][lane].data_ptr() for site, _, _ in pend])
        flags = torch.empty(n, dtype=torch.int32, device=dev)
        lib().call("lmkd_h2_fence_eval", words, refs, n, _p(flags), _stream())
        host = torch.empty(n, dtype=torch.int32).pin_memory()
        host.copy_(flags, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        _FENCE_INFLIGHT.append((ev, host, [site for site, _, _ in pend], (pend, flags)))
    if wait:
        _fence_poll(wait=True)


def _amax_out(t, site=None):
    """call for the launch that writes t: -> AmaxDesc whose out_words are fresh zeroed words that the launch folds max |t| into (and, with a
    site, ref_words = the site's reference: the launch also leaves the range statistics); the words travel with t.  None outside fp32h2."""
    if t.dtype is not torch.float32 or not _h2_mode():
        return None
    w = _amax_slot(t.device)
    t._lmkd_amax = w
    if site is not None:
        t._lmkd_site = site
    return AmaxDesc(None, None, _pw(w), _fence_watch(site, w, t.device), 0)


_AMAX_ATTRS = ("_lmkd_amax", "_lmkd_site", "_lmkd_pre_amax", "_lmkd_pre_site")


def _amax_tag(t):
    """what travels with a tensor in fp32h2 (its maximum's words, its fence site; the same for the loader-side bound) - to carry across
    save_for_backward, which may hand back a new tensor object"""
    return None if t is None else tuple(getattr(t, a, None) for a in _AMAX_ATTRS)


def _amax_retag(t, tag):
    if t is not None and tag is not None:
        for a, v in zip(_AMAX_ATTRS, tag):
            if v is not None:
                setattr(t, a, v)


def _amax_ptr(t, pre=False):
    """-> (words pointer | None, fenced): pre: t is a raw convolution output that the consumer normalises + rectifies in its loader: the
    words are the BOUND of max |relu(BatchNorm(t))| that lmkd_bn_finalize(_seg) wrote (_conv_bn_train_or_eval(bound=True)).  A tensor whose
    site the range fence has flagged yields no words: the launch runs the three-plane form."""
    if t is None:
        return None, False
    w = getattr(t, "_lmkd_pre_amax" if pre else "_lmkd_amax", None)
    if w is None:
        return None, False
    site = getattr(t, "_lmkd_pre_site" if pre else "_lmkd_site", None)
    if site is not None and H2_FENCE:
        e = _FENCE_SITES.get(site)
        if e is not None and e["bad"]:
            return None, True
    return _pw(w), False


def _amax_operands(x, dy, pre=False):
    """-> AmaxDesc naming the maxima of a convolution's operands where they are known (None outside fp32h2)"""
    if not _h2_mode():
        return None
    px, fx = _amax_ptr(x, pre)
    pd, fd = _amax_ptr(dy)
    if px is None and pd is None and not (fx or fd):
        return None
    return AmaxDesc(px, pd, None, None, AMAX_FENCED if (fx or fd) else 0)


def amax_compute(t, seg=0):
    """max |t| by a reduction pass of its own (tensors that no kernel of this library wrote: tests, tools); seg = F0: per frame segment"""
    nw = lib().value("lmkd_amax_words")
    w = torch.zeros(nw, dtype=torch.int32, device=t.device)
    seg = _seg_frames(seg, t.shape[0])
    n0 = (t.numel() // t.shape[0]) * seg if seg else t.numel()
    lib().call("lmkd_amax", _p(t), n0, w.data_ptr(), _stream())
    if seg:
        lib().call("lmkd_amax", t.data_ptr() + 4 * n0, t.numel() - n0, w.data_ptr() + 2 * nw, _stream())
    t._lmkd_amax = w
    return t


def _pack_weights(w, Cs, mode, out=None):
    Cout, Cin, KH, KW = w.shape
    n = lib().value("lmkd_conv2d_packed_weight_elems", Cout, Cin, Cs, KH, KW, mode)
    cd = lib().value("lmkd_conv_get_compute_dtype")
    _chk(w)
    if cd == 0:
        wp = out if out is not None else _empty((n,), w)
        lib().call("lmkd_conv2d_pack_weights", _p(w), _p(wp), Cout, Cin, Cs, KH, KW, mode, _stream())
        return wp
    # every other arithmetic: the weight's plane buffer - 16-bit planes in MFMA fragment order, fetched into registers (layout: DESIGN.md 3.1)
    wp = _empty((n,), w)
    lib().call("lmkd_conv2d_pack_weights", _p(w), _p(wp), Cout, Cin, Cs, KH, KW, mode, _stream())
    ncols = Cout if mode == 0 else Cin
    planes = out if out is not None else torch.empty((lib().value("lmkd_conv2d_plane_elems", ncols, n // ncols),), dtype=torch.int16, device=w.device)
    lib().call("lmkd_conv2d_split_weights", _p(wp), planes.data_ptr(), ncols, n // ncols, _stream())
    return planes


# Library default (also the default of liblmkd_hip.so itself): exact 3-way bf16 split, six products - a caller of the C ABI needs no
# protocol for it.  bench.py and the training CLI run "fp32h2" (the trunk's convolutions on two fp16 planes, three products, scales from
# the tensors' maxima: csrc/conv_patch16.h), which this module's functions support by carrying the maxima with the tensors (_amax_*).
DEFAULT_CONV_DTYPE = "fp32x3"


def set_conv_compute_dtype(dtype):
    """Process-wide arithmetic of the convolutions (lmkd_conv_set_compute_dtype; one process per GPU, set before launching):
    'fp32x3' (DEFAULT): fp32 tensors and accumulation, each fp32 product formed on the bf16 matrix pipe from an exact 3-way
    bf16 split of both operands (6 of the 9 cross products; 'fp32x3_9': all nine) - fp32-class error (tests/test_gpu_fullsize.py).
    'fp32h2': 'fp32x3' with the 3x3 convolutions' forward / data gradient / window weight gradient on TWO fp16 planes and three products
    (power-of-two scales from the tensors' maxima; csrc/conv_patch16.h) - the same error class at half the MFMA work.
    'fp32': native fp32 MFMA (v_mfma_f32_32x32x2_f32).  'bf16' (BASELINE configs[2]): operands rounded to bf16, fp32 accumulation;
    with set_activation_dtype('bf16') the trunk's tensors in HBM are bf16 as well."""
    modes = {"fp32": 0, "bf16": 1, "fp32x3": 2, "fp32x3_9": 3, "fp32h2": 4}
    if dtype not in modes:
        raise ValueError(dtype)
    lib().call("lmkd_conv_set_compute_dtype", modes[dtype])   # (the packed-weight cache keeps one buffer per mode)
    if dtype != "bf16" and _ACT_DTYPE[0] is not torch.float32:
        set_activation_dtype("fp32")                         # bf16 tensors exist in the one-plane mode only


def get_conv_compute_dtype():
    return ("fp32", "bf16", "fp32x3", "fp32x3_9", "fp32h2")[lib().value("lmkd_conv_get_compute_dtype")]


def reset_compute_dtypes():
    """back to the library defaults: fp32x3 convolutions, fp32 tensors"""
    set_conv_compute_dtype(DEFAULT_CONV_DTYPE)
    set_activation_dtype("fp32")


import contextlib


@contextlib.contextmanager
def compute_dtypes(conv, act="fp32"):
    """with ops.compute_dtypes('bf16', 'bf16'): ...  - switch the process-wide arithmetic for a block and restore it afterwards"""
    prev = (get_conv_compute_dtype(), get_activation_dtype())
    set_conv_compute_dtype(conv)
    set_activation_dtype(act)
    try:
        yield
    finally:
        set_conv_compute_dtype(prev[0])
        set_activation_dtype(prev[1])


def conv_out_size(H, K, s, p):
    return (H + 2 * p - K) // s + 1


# Optional per-launch timing of the conv kernels with HIP events on the launch stream (bench.py roofline):
# set ops.CONV_TIMING = [] to collect (kernel family, algorithmic FLOPs, start event, end event).
CONV_TIMING = None


class _timed:
    def __init__(self, family, flops, nbytes=0):
        self.on = CONV_TIMING is not None
        if self.on:
            self.rec = (family, flops, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), nbytes)

    def __enter__(self):
        if self.on:
            self.rec[2].record()

    def __exit__(self, *a):
        if self.on:
            self.rec[3].record()
            CONV_TIMING.append(self.rec)


def _conv_family(kind, N, H, W, Cs, Cin, Cout, KH, KW, stride, pad):
    """name under which a forward (kind 0) / data-gradient (1) launch is timed: the LDS-patch kernel (conv_patch_x3_kernel: same-size
    convolutions of the bf16-plane modes) or the im2col-gather kernels (conv_gemm_kernel / conv_gemm_x3_kernel)"""
    if CONV_TIMING is None:
        return "conv_gemm_kernel"
    import ctypes
    info = (ctypes.c_int * 5)()
    lib().call("lmkd_conv2d_plan", kind, N, H, W, Cs, Cin, Cout, KH, KW, stride, pad, info)
    return "conv_patch_kernel" if info[4] == 1 else "conv_gemm_kernel"


def _seg_frames(seg, N):
    """frame split of a two-segment tensor (both trunk calls of an episode as one [F0 + F1, ...] tensor), 0 = one segment"""
    seg = int(seg or 0)
    return seg if 0 < seg < N else 0


def conv_fwd(x, wp, Cout, KH, KW, stride, pad, want_stats, pre_stats=None, seg=0, amax_out=None):
    """x NHWC [N,H,W,Cs] -> (y [N,Ho,Wo,Cout], stat partial [T,Cout,2] | None).  pre_stats: x is the RAW output of the previous
    convolution and the loader applies relu(BatchNorm(x)) with that layer's [5][Cs] table (lmkd_conv2d_fwd_pre).
    seg = F0 > 0: frames [0, F0) and [F0, N) are two BatchNorm batches (lmkd_conv2d_fwd_seg): pre_stats is [2, 5, Cs] and the result is
    (y, part, T0) - the first T0 rows of part belong to segment 0.
    amax_out (fp32h2): zeroed words that the launch folds max |y| into (lmkd_amax_desc::out_words)"""
    _chk(x, wp, pre_stats)
    N, H, W, Cs = x.shape
    seg = _seg_frames(seg, N)
    Ho, Wo = conv_out_size(H, KH, stride, pad), conv_out_size(W, KW, stride, pad)
    y = _empty_act((N, Ho, Wo, Cout), x)
    part = None
    t0 = (ctypes.c_int * 1)()
    if want_stats:
        T = lib().value("lmkd_conv2d_fwd_row_tiles_seg", N, H, W, Cs, Cout, KH, KW, stride, pad, seg, t0)
        part = _empty((T, Cout, 2), x)
    cin = 3 if Cs == 4 else Cs
    with _timed(_conv_family(0, N, H, W, Cs, cin, Cout, KH, KW, stride, pad), 2.0 * N * Ho * Wo * Cout * cin * KH * KW,
                x.element_size() * x.numel() + y.element_size() * y.numel() + 4 * wp.numel()):
        d = _amax_operands(x, None, pre=pre_stats is not None)
        if amax_out is not None and _h2_mode():
            d = d if d is not None else AmaxDesc(None, None, None, None, 0)
            d.out_words = _pw(amax_out)
        if seg or d is not None:
            lib().call("lmkd_conv2d_fwd_seg", _p(x), _p(pre_stats), _p(wp), _p(y), _p(part), N, H, W, Cs, Cout, KH, KW, stride, pad, seg, _stream(),
                       _desc_arg(d))
        elif pre_stats is not None:
            lib().call("lmkd_conv2d_fwd_pre", _p(x), _p(pre_stats), _p(wp), _p(y), _p(part), N, H, W, Cs, Cout, KH, KW, stride, pad, _stream())
        else:
            lib().call("lmkd_conv2d_fwd", _p(x), _p(wp), _p(y), _p(part), N, H, W, Cs, Cout, KH, KW, stride, pad, _stream())
    return (y, part, int(t0[0])) if seg else (y, part)


# The data gradient that feeds relu + BatchNorm backward leaves that backward's reduction in its epilogue (lmkd_conv2d_bwd_data_bn) where
# the launch has the form: one pass over (dx, bn input) and one launch per such BatchNorm less (16 launches, 0.44 ms of
# bn_bwd_reduce_kernel per episode; BatchNorm family 3.8 -> 3.4 ms, 453 -> 437 launches).  Neutral in episodes/s (same-box: first 33.73 /
# 33.74 / 33.85 with against 33.91 / 33.87 / 33.90 without, on the final kernels 36.11 / 36.06 / 36.01 / 36.06 against 36.11 / 36.04 /
# 36.03 / 36.00): the reduction kernels it removes ran beside the weight-gradient stream's MFMA kernels.  On: fewer passes over HBM.
DGRAD_BN_STATS = True


def conv_bwd_data(dy, wd, x_shape, Cout, KH, KW, stride, pad, out=None, accumulate=False, bn=None, seg=0):
    """bn = (x_bn, stats): the gradient feeds relu(BatchNorm(x_bn)) backward -> (dx, part | None), part = the [T, Cin, 2] partial sums
    bn_backward(part=...) takes in place of its reduction pass (None: this launch has no fused form).
    seg = F0 > 0: two frame segments (lmkd_conv2d_bwd_data_seg); stats is [2, 5, Cin] and part becomes (part, T0)."""
    N, H, W, Cin = x_shape
    seg = _seg_frames(seg, N)
    _chk(dy, wd, out)
    if accumulate and out is None:
        raise ValueError("accumulate needs an output buffer")
    dx = out if out is not None else _empty_act((N, H, W, Cin), dy)
    part = None
    t0 = (ctypes.c_int * 1)()
    if bn is not None and DGRAD_BN_STATS and not accumulate:
        T = lib().value("lmkd_conv2d_bwd_data_bn_tiles_seg", N, H, W, Cin, Cout, KH, KW, stride, pad, seg, t0)
        if T > 0:
            _chk(bn[0], bn[1])
            part = _empty((T, Cin, 2), dy)
    with _timed(_conv_family(1, N, H, W, Cin, Cin, Cout, KH, KW, stride, pad), 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * Cout * Cin * KH * KW,
                dy.element_size() * dy.numel() + dx.element_size() * dx.numel() * (2 if accumulate else 1) + 4 * wd.numel()
                + (bn[0].element_size() * bn[0].numel() if part is not None else 0)):      # the fused form also reads the BatchNorm input
        d = _amax_operands(None, dy)
        if seg or d is not None:
            lib().call("lmkd_conv2d_bwd_data_seg", _p(dy), _p(wd), _p(dx), _p(bn[0]) if part is not None else None,
                       _p(bn[1]) if part is not None else None, _p(part), N, H, W, Cin, Cout, KH, KW, stride, pad, int(accumulate), seg, _stream(),
                       _desc_arg(d))
            if part is not None and seg:
                part = (part, int(t0[0]))
        elif part is not None:
            lib().call("lmkd_conv2d_bwd_data_bn", _p(dy), _p(wd), _p(dx), _p(bn[0]), _p(bn[1]), _p(part), N, H, W, Cin, Cout, KH, KW, stride,
                       pad, _stream())
        else:
            lib().call("lmkd_conv2d_bwd_data", _p(dy), _p(wd), _p(dx), N, H, W, Cin, Cout, KH, KW, stride, pad, int(accumulate), _stream())
    return (dx, part) if bn is not None else dx


def conv_bwd_weight(x, dy, w_shape, stride, pad, pre_stats=None, acc_into=None, seg=0):
    """pre_stats: x is a raw conv output, relu(BatchNorm(x)) is recomputed in the loader (lmkd_conv2d_bwd_weight_pre).
    acc_into: a contiguous OIHW tensor (the weight's .grad) that receives `+= dW` in the slab-reduce kernel itself.
    seg = F0 > 0: two frame segments, pre_stats [2, 5, Cs] (lmkd_conv2d_bwd_weight_seg: one launch over all frames)."""
    Cout, Cin, KH, KW = w_shape
    N, H, W, Cs = x.shape
    seg = _seg_frames(seg, N)
    _chk(x, dy, pre_stats, acc_into)
    nbytes = lib().value("lmkd_conv2d_bwd_weight_workspace_seg", N, H, W, Cs, Cout, KH, KW, stride, pad, seg)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    dw = acc_into if acc_into is not None else _empty(w_shape, x)
    with _timed("conv_wgrad_kernel", 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * Cout * Cin * KH * KW,
                x.element_size() * x.numel() + dy.element_size() * dy.numel() + 4 * dw.numel()):
        d = _amax_operands(x, dy, pre=pre_stats is not None)
        if seg or d is not None:
            lib().call("lmkd_conv2d_bwd_weight_seg", _p(x), _p(pre_stats), _p(dy), _p(dw), _p(ws), nbytes, N, H, W, Cs, Cin, Cout, KH, KW,
                       stride, pad, int(acc_into is not None), seg, _stream(), _desc_arg(d))
        elif acc_into is not None:
            lib().call("lmkd_conv2d_bwd_weight_acc", _p(x), _p(pre_stats), _p(dy), _p(dw), _p(ws), nbytes, N, H, W, Cs, Cin, Cout, KH, KW,
                       stride, pad, _stream())
        elif pre_stats is not None:
            lib().call("lmkd_conv2d_bwd_weight_pre", _p(x), _p(pre_stats), _p(dy), _p(dw), _p(ws), nbytes, N, H, W, Cs, Cin, Cout, KH, KW,
                       stride, pad, _stream())
        else:
            lib().call("lmkd_conv2d_bwd_weight", _p(x), _p(dy), _p(dw), _p(ws), nbytes, N, H, W, Cs, Cin, Cout, KH, KW, stride, pad, _stream())
    return dw


# The weight gradient of a layer feeds nothing in the backward chain (only the optimizer), so it need not sit on the stream that
# carries the data-gradient / BatchNorm chain: with SIDE_WGRAD the Functions' backward launches it on ONE extra stream and
# accumulates it into `weight.grad` there (returning None to autograd, which would otherwise add it on the chain's stream).
# All weight-gradient accumulations are ordered on that single stream; an end-of-backward engine callback makes the caller's
# stream wait for it, and the optimizer / all-reduce / zero_grad entry points wait again.  +2.8 % episodes/s (same-box A/B).
# OFF by default: with it on, torch.autograd.grad() returns None for conv weights and tensor / post-accumulate hooks on them
# never fire (the gradient does not pass through autograd).  trainloop.train and bench.py, which own the optimizer, switch it
# on; a weight that carries hooks always takes the autograd path.
SIDE_WGRAD = False
# False: no wait at the end of backward(); the caller promises to call wait_weight_grads() before it reads or modifies any
# weight.grad (trainloop.FusedOptimizer does, so the next episode's forward can overlap the last weight gradients)
SYNC_WGRAD_AT_BACKWARD_END = True
_WG_CB = [None]      # id of the autograd graph task whose end-of-backward callback is queued (a backward that raised leaves a
                     # stale id behind, which the next backward — a new graph task — does not match)


def wait_weight_grads():
    """make the current (and the default) stream wait for every weight gradient launched on the side stream"""
    for sw in forked_streams(roles=("wgrad",)):
        torch.cuda.current_stream(sw.device).wait_stream(sw)
        if not torch.cuda.is_current_stream_capturing():      # a wait on a capturing stream's event would pull the default stream into the capture
            torch.cuda.default_stream(sw.device).wait_stream(sw)


def join_all_streams():
    """make the current stream wait for EVERY stream this module has created on its device - the weight-gradient stream, the side /
    auxiliary / lane-main streams of every lane.  The optimizer calls it before it reads or zeroes the gradient buffers (and their
    shadow): kernels on the side and auxiliary streams add parameter gradients directly (DIRECT_PARAM_GRAD), hand autograd None, and are
    therefore NOT joined to the caller's stream by the autograd engine; that the stem's weight gradient happens to order the side stream
    before the weight-gradient stream is not something to rely on (a frozen or hooked stem weight breaks it)."""
    if not _STREAMS:
        return      # nothing was ever forked (this includes every CPU-side caller)
    cur = torch.cuda.current_stream()
    dev = cur.device.index if hasattr(cur, "device") and cur.device is not None else torch.cuda.current_device()
    wait_weight_grads()
    for s in forked_streams(torch.device("cuda", dev), roles=("side", "aux", "main")):
        if s.cuda_stream != cur.cuda_stream:
            cur.wait_stream(s)


def _end_of_backward():
    _WG_CB[0] = None
    wait_weight_grads()


def _has_hooks(w):
    return bool(getattr(w, "_backward_hooks", None)) or bool(getattr(w, "_post_accumulate_grad_hooks", None))


def _on_wgrad_stream(device, work, reads):
    """work() on the weight-gradient stream, after everything queued so far on the current stream; reads: the tensors (or None) it reads"""
    sw = _wgrad_stream(device)
    sw.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(sw):
        work()
    for t in reads:
        if t is not None:
            t.record_stream(sw)
    _join_at_backward_end()


def _join_at_backward_end():
    if SYNC_WGRAD_AT_BACKWARD_END:
        task = torch._C._current_graph_task_id()
        if _WG_CB[0] != task:
            _WG_CB[0] = task
            torch.autograd.Variable._execution_engine.queue_callback(_end_of_backward)


# Linear / TRX projection weights: their gradient GEMMs (dW = dy^T x: 53 - 71 us each, 0.3 ms per episode) feed nothing in the backward
# chain either; with SIDE_WGRAD and DIRECT_PARAM_GRAD they run on the weight-gradient stream and add straight into .grad there (both TRX
# heads: the stream orders them, no shadow buffer involved), and the head's stream goes on with the input gradient.
SIDE_LINEAR_WGRAD = True


def side_accumulate(param, fn, *reads):
    """fn(param.grad) on the weight-gradient stream, after everything queued so far on the current stream; reads: the tensors fn reads.
    -> False (nothing done) unless the gradient may be accumulated directly (see DIRECT_PARAM_GRAD, SIDE_WGRAD)"""
    if not (SIDE_LINEAR_WGRAD and SIDE_WGRAD and DIRECT_PARAM_GRAD and param.is_leaf and param.requires_grad) or _has_hooks(param):
        return False
    e = _GRAD_SLOT.get(param.data_ptr())
    if e is None or e[0]() is not param or param.grad is None:
        return False
    _on_wgrad_stream(param.device, lambda: fn(param.grad), reads)
    return True


# A parameter gradient reaches its parameter one of three ways, tried in this order: added into .grad on the weight-gradient stream
# (side_accumulate), added into .grad or its shadow on the caller's stream (_grad_target), or returned to autograd as a fresh tensor.
def deliver_wgrad(param, launch, shape, *reads):
    """the weight gradient launch(target, beta) computes with a gemm (beta = 1 adds to the target); shape: the gradient's; reads: the tensors
    the launch reads.  -> None after accumulating it directly, else the fresh gradient tensor"""
    if side_accumulate(param, lambda t: launch(t, 1.0), *reads):
        return None
    t = _grad_target(param)
    if t is not None:
        launch(t, 1.0)
        return None
    dw = _empty(shape, reads[0])
    launch(dw, 0.0)
    return dw


def deliver_colsum(param, a, b=None):
    """the column-sum gradient sum_r a[r, :] (* b[r, :]) of a bias / LayerNorm parameter: -> None after accumulating it directly, else the
    fresh gradient tensor.  (It feeds nothing and is small: never on the weight-gradient stream.)"""
    t = _grad_target(param)
    if t is None:
        return colsum(a, b)
    colsum(a, b, out=t, accumulate=True)
    return None


def weight_grad(w, x, dy, stride, pad, pre_stats=None, seg=0):
    """dW of a convolution for autograd — or None after accumulating it into w.grad on the weight-gradient stream."""
    if not (SIDE_WGRAD and w.is_leaf and w.requires_grad) or _has_hooks(w):
        return conv_bwd_weight(x, dy, tuple(w.shape), stride, pad, pre_stats, seg=seg)

    def work():
        if w.grad is not None and w.grad.is_contiguous() and w.grad.dtype == torch.float32:
            conv_bwd_weight(x, dy, tuple(w.shape), stride, pad, pre_stats, acc_into=w.grad, seg=seg)      # += in the slab reduce
        else:
            dw = conv_bwd_weight(x, dy, tuple(w.shape), stride, pad, pre_stats, seg=seg)
            if w.grad is None:
                w.grad = dw
            else:
                w.grad.add_(dw)
    # read by the side-stream kernel: x, dy, the words holding their maxima (fp32h2: it reads them when it starts) and pre_stats - no
    # block of theirs may be recycled under it
    words = [getattr(t, attr, None) for t in (x, dy) for attr in ("_lmkd_amax", "_lmkd_pre_amax")]
    _on_wgrad_stream(x.device, work, [x, dy] + words + [pre_stats])
    return None


BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def bn_stats_train(part, count, gamma, beta, running_mean, running_var, seg=None, bound=None):
    """seg = (T0, count0): two frame segments - partial rows [0, T0) / [T0, T), count0 / count - count0 elements per channel ->
    stats [2, 5, C]; the running statistics are not touched (the caller defers both updates: apply_deferred).
    bound = (words of max |x|, zeroed words for the bound, site | None) (fp32h2): the launch also writes a bound of max |relu(BatchNorm(x))|"""
    T, C, _ = part.shape
    d = None
    if bound is not None:
        d = AmaxDesc(_pw(bound[0]), None, _pw(bound[1]), _fence_watch(bound[2], bound[1], part.device), 0)
    if seg is not None:
        T0, count0 = seg
        if running_mean is not None or running_var is not None:
            raise ValueError("two frame segments: the running-statistics updates are deferred (ops.set_defer)")
        stats = _empty((2, 5, C), part)
        scratch = torch.empty(2 * 64 * 2 * C, dtype=torch.float64, device=part.device)
        lib().call("lmkd_bn_finalize_seg", _p(part), T, T0, C, count0, count - count0, _p(gamma), _p(beta), _f32(BN_EPS), _p(stats), _p(scratch),
                   _p(_tickets(part)), _stream(), _desc_arg(d))
        return stats
    stats = _empty((5, C), part)
    scratch = torch.empty(64 * 2 * C, dtype=torch.float64, device=part.device)
    lib().call("lmkd_bn_finalize", _p(part), T, C, count, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
               _f32(BN_MOMENTUM), _f32(BN_EPS), _p(stats), _p(scratch), _p(_tickets(part)), _stream(), _desc_arg(d))
    return stats


def bn_stats_eval(gamma, beta, running_mean, running_var):
    C = gamma.shape[0]
    stats = _empty((5, C), gamma)
    lib().call("lmkd_bn_eval_stats", C, _p(gamma), _p(beta), _p(running_mean), _p(running_var), _f32(BN_EPS), _p(stats), _stream())
    return stats


def _rows0(t, seg):
    """rows (pixels) of frame segment 0 of the NHWC tensor t; its row count when there is one segment"""
    rows = t.numel() // t.shape[-1]
    seg = _seg_frames(seg, t.shape[0])
    return seg * (rows // t.shape[0]) if seg else rows


def bn_apply(x, stats, relu, res=None, rstats=None, want_bits=False, seg=0, site=None):
    """-> y, or (y, bits) with want_bits: the packed ReLU mask (y > 0), one bit per element, for bn_backward(mask_mode 3).
    seg = F0 > 0: stats (and rstats) are [2, 5, C], one table per frame segment.  site: the range fence's name for y (h2_fence_step)"""
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty_like(x)
    mode = 0 if res is None else (2 if rstats is not None else 1)
    _chk(x, stats, res, rstats)
    bits = torch.empty(x.numel() // 32, dtype=torch.int32, device=x.device) if want_bits else None
    lib().call("lmkd_bn_apply_seg", _p(x), _p(stats), _p(res), _p(rstats), _p(y), rows, _rows0(x, seg), C, int(relu), mode, _p(bits), _stream(),
               _desc_arg(_amax_out(y, site)))
    return (y, bits) if want_bits else y


def bn_backward(dy, x, yact, stats, gamma, mask_mode, want_g=False, dx_out=None, beta=None, part=None, seg=0):
    """-> dx, g (masked dy) | None, dgamma, dbeta.  mask_mode 1: yact = the activation output; 3: yact = its packed bit mask.
    beta (the BatchNorm bias parameter) given and DIRECT_PARAM_GRAD on: dgamma / dbeta are added into gamma.grad / beta.grad (or
    their side-stream shadows) by the coefficient kernel and None is returned for both.
    part: the reduction already happened in the data gradient that produced dy (conv_bwd_data(bn=...); mask_mode 2, no g)"""
    C = x.shape[-1]
    rows = x.numel() // C
    seg = _seg_frames(seg, x.shape[0])      # two frame segments: stats [2, 5, C]; part = (tensor, T0)
    rows0 = _rows0(x, seg)
    _chk(dy, x, yact, stats, gamma)
    dx = dx_out if dx_out is not None else torch.empty_like(x)
    g = torch.empty_like(x) if want_g else None
    tg = _grad_target(gamma) if beta is not None else None
    tb = _grad_target(beta) if tg is not None else None
    direct = tg is not None and tb is not None
    dgamma, dbeta = (tg, tb) if direct else (_empty((C,), x), _empty((C,), x))
    coef = _empty((2, 5, C) if seg else (3, C), x)
    ws = torch.empty(lib().value("lmkd_bn_bwd_workspace", C) * (2 if seg else 1), dtype=torch.uint8, device=x.device)
    if part is not None:
        if mask_mode != 2 or want_g:
            raise ValueError("partial sums of the data gradient: mask_mode 2 without g")
        part, T0 = part if isinstance(part, tuple) else (part, part.shape[0])
        _chk(part)
        lib().call("lmkd_bn_backward_part_seg", _p(part), part.shape[0], T0, _p(dy), _p(x), _p(stats), _p(gamma), _p(dx), _p(dgamma), _p(dbeta),
                   _p(coef), _p(ws), _p(_tickets(x)), rows, rows0, C, int(direct), _stream(), _desc_arg(_amax_out(dx, ("d", gamma.data_ptr()))))
    else:
        lib().call("lmkd_bn_backward_seg", _p(dy), _p(x), _p(yact), _p(stats), _p(gamma), _p(dx), _p(g), _p(dgamma), _p(dbeta),
                   _p(coef), _p(ws), _p(_tickets(x)), rows, rows0, C, mask_mode, int(direct), _stream(), _desc_arg(_amax_out(dx, ("d", gamma.data_ptr()))))
    return (dx, g, None, None) if direct else (dx, g, dgamma, dbeta)


# When the two trunk calls of an episode run on two HIP streams (backbone: overlap_trunk_calls), the running-statistics
# updates are deferred and applied afterwards in program order (support call first, then query call), so the result is
# identical to the serial reference order.  _DEFER is the list collecting (running_mean, running_var, stats).
_DEFER = None


def set_defer(lst):
    global _DEFER
    _DEFER = lst


def deferring():
    return _DEFER is not None


def apply_deferred(entries, counters=None):
    """entries: [(running_mean, running_var, stats)] in program order; updates of the same BatchNorm (the two trunk calls of an
    episode) are applied in that order.  One launch for all layers (lmkd_bn_running_update_multi_nbt).
    counters: {running_mean.data_ptr(): num_batches_tracked tensor} - bumped by the same launch, once per update applied."""
    if not entries:
        return
    layers, order = {}, []
    for rm, rv, stats in entries:
        k = rm.data_ptr()
        if k not in layers:
            layers[k] = [rm, rv, []]
            order.append(k)
        layers[k][2].append(stats)
    rounds = max(len(layers[k][2]) for k in order)
    for r0 in range(0, rounds, 2):      # two updates per layer and launch
        ks = [k for k in order if len(layers[k][2]) > r0]
        n = len(ks)
        P = ctypes.c_void_p * n
        rm = P(*[layers[k][0].data_ptr() for k in ks])
        rv = P(*[layers[k][1].data_ptr() for k in ks])
        s0 = P(*[layers[k][2][r0].data_ptr() for k in ks])
        s1 = P(*[(layers[k][2][r0 + 1].data_ptr() if len(layers[k][2]) > r0 + 1 else None) for k in ks])
        C = (ctypes.c_int * n)(*[layers[k][0].shape[0] for k in ks])
        nbt = P(*[(counters[k].data_ptr() if counters and k in counters else None) for k in ks])
        lib().call("lmkd_bn_running_update_multi_nbt", rm, rv, s0, s1, nbt, C, n, _f32(BN_MOMENTUM), _stream())


# Stream sets ("lanes").  An episode uses up to three forward streams: the caller's (support-frame trunk call, heads, loss), a side
# stream (query-frame trunk call) and an auxiliary one (frozen teacher head, second TRX head).  trainloop.PipelinedEpisodes runs
# the forward of episode i + 1 beside the backward of episode i: the two episodes in flight use different lanes (LANE 0 / 1), each
# with a main stream of its own (lane_main) in place of the caller's.
LANE = [0]
# Every stream this module forks, in order of creation: (device index, lane, "main" | "side" | "aux") -> stream, and the device's
# weight-gradient stream under (device index, None, "wgrad").  Nothing outside this section reads a key: the four getters
# below create on first request (under the current lane), lane_streams / forked_streams / stream_role only look.
_STREAMS = {}
_STREAM_ROLE = {}      # raw handle -> (device index, role)
# HIP stream priorities (torch: -1 = high, 0 = default) of the streams this module creates, by lane and for the weight-gradient stream;
# set before the first stream is created (bench.py LMKD_PRIO)
STREAM_PRIORITY = {0: 0, 1: 0, "wgrad": 0}
HEADS_ON_TWO_STREAMS = True      # TRX_2fcsup: the 'ce' head on the auxiliary stream beside the 'kl' head


def _new_stream(device, key):
    return torch.cuda.Stream(device=device, priority=int(STREAM_PRIORITY.get(key, 0)))


def device_index(device):
    """the index the stream table is keyed with: torch.device('cuda') (index None - the training CLI's default before init_distributed
    fills it in) means the current device"""
    device = torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


@contextlib.contextmanager
def lane(k):
    """run the body under stream set k; the previous lane is restored afterwards, also when the body raises"""
    prev, LANE[0] = LANE[0], int(k)
    try:
        yield
    finally:
        LANE[0] = prev


def _forked(device, lane, role):
    """the one creating getter; lane None: the device's weight-gradient stream (role "wgrad", its STREAM_PRIORITY key)"""
    dev = device_index(device)
    if (dev, lane, role) not in _STREAMS:
        s = _STREAMS[(dev, lane, role)] = _new_stream(device, role if lane is None else lane)
        _STREAM_ROLE[s.cuda_stream] = (dev, role)
    return _STREAMS[(dev, lane, role)]


def lane_main(device):
    return _forked(device, LANE[0], "main")


def side_stream(device):
    return _forked(device, LANE[0], "side")


def aux_stream(device):
    """a third forward stream: the frozen teacher head of an episode runs there beside the student's trunk (trainloop.train_task)"""
    return _forked(device, LANE[0], "aux")


def _wgrad_stream(device):
    return _forked(device, None, "wgrad")


def lane_streams(device, roles=("side", "aux", "main")):
    """the streams of these roles that exist for the CURRENT lane on `device`, in the order of `roles`"""
    keys = [(device_index(device), LANE[0], role) for role in roles]
    return [_STREAMS[key] for key in keys if key in _STREAMS]


def forked_streams(device=None, roles=("wgrad", "side", "aux", "main")):
    """every stream of these roles created so far (on `device`; None: on any), role by role in the order of `roles`"""
    dev = None if device is None else device_index(device)
    return [s for role in roles for (d, _, r), s in _STREAMS.items() if r == role and (dev is None or d == dev)]


def stream_role(raw):
    """-> (device index, role) of the forked stream with this raw handle, None for any other stream"""
    return _STREAM_ROLE.get(raw)


FUSE_EVAL_BN = True      # eval mode: BatchNorm (+ residual, ReLU) in the convolution epilogue (lmkd_conv2d_fwd_bn)


def _eval_fused():
    """every arithmetic mode has the epilogue (conv_gemm_kernel STATS == 2, x3_epilogue EP); with bf16 tensors in HBM the eval
    forward stays two-pass (the stored convolution output is rounded before the BatchNorm there)"""
    return FUSE_EVAL_BN and not torch.is_grad_enabled() and _ACT_DTYPE[0] is torch.float32


def conv_bn_eval(x, w, Cs, stride, pad, gamma, beta, rm, rv, relu, res=None, feeds_conv=True):
    """inference: relu?(BN_eval(conv(x)) (+ res)) in one kernel; bit-identical to conv_fwd + bn_stats_eval + bn_apply.
    fp32h2: x's maximum (recorded by the launch that wrote x) puts the launch on two planes, and - feeds_conv: y is a convolution's
    operand - the epilogue records max |y| for the next one (the BatchNorm + ReLU are applied there: no bound is needed)"""
    Cout, _, KH, KW = w.shape
    wp = pack_weights(w, Cs, 0)
    stats = bn_stats_eval(gamma, beta, rm, rv)
    _chk(x, wp, res)
    N, H, W, _ = x.shape
    Ho, Wo = conv_out_size(H, KH, stride, pad), conv_out_size(W, KW, stride, pad)
    y = _empty((N, Ho, Wo, Cout), x)
    cin = 3 if Cs == 4 else Cs
    with _timed(_conv_family(0, N, H, W, Cs, cin, Cout, KH, KW, stride, pad), 2.0 * N * Ho * Wo * Cout * cin * KH * KW,
                x.element_size() * x.numel() + y.element_size() * y.numel() + 4 * wp.numel()):
        d = _amax_operands(x, None)
        if feeds_conv and _h2_mode():
            d = d if d is not None else AmaxDesc(None, None, None, None, 0)
            wds = _amax_slot(x.device)
            d.out_words = _pw(wds)
            y._lmkd_amax = wds
        lib().call("lmkd_conv2d_fwd_bn", _p(x), _p(wp), _p(y), _p(stats), _p(res), int(relu), N, H, W, Cs, Cout, KH, KW, stride, pad,
                   _stream(), _desc_arg(d))
    return y


# Training: the BatchNorm + ReLU between two convolutions of a block runs in the CONSUMER's loader (forward conv and weight
# gradient), so the normalised activation is never written to HBM; the block output is written once, together with its ReLU
# mask as bits for the backward.  The loaders exist in all arithmetic modes (conv_gemm_kernel / conv_gemm_x3_kernel, conv_wgrad_kernel /
# conv_wgrad_x3_kernel, bit-identical to the materialising path in each); the POLICY uses them in the native fp32 mode only: measured
# at 200 frames, the bf16-plane forward pays 14-112 us (3xbf16) / 32-81 us (bf16) for the store-side arithmetic and the weight
# gradient up to 30 us, against 12-56 us for the bn_apply launch they save (tools/pre_bench.py).  FUSE_PRE_ALL_MODES forces them on.
FUSE_TRAIN_BN = True
FUSE_PRE_ALL_MODES = False
PRE_IN_PLANE_MODES = True      # the three-plane modes' share of that policy (bench.py LMKD_PRE_X3=0 switches it off for an A/B)


def _train_fused():
    """block-output ReLU mask as bits (every mode)"""
    return FUSE_TRAIN_BN


def _train_pre():
    """inner BatchNorm + ReLU in the consumers' loaders (the loaders exist for fp32 tensors only).  Policy: the native fp32 mode and,
    since round 3, the three-plane modes - with the patch / window kernels the loader arithmetic runs once per patch / window row
    and the headline benchmark is indifferent (31.8 vs 31.6 episodes/s, same box) while 16 launches per episode and a quarter of
    the activation memory go away; the one-plane bf16 mode keeps the materialised activation (56.0 vs 59.7)."""
    cd = lib().value("lmkd_conv_get_compute_dtype")
    return (FUSE_TRAIN_BN and _ACT_DTYPE[0] is torch.float32
            and (FUSE_PRE_ALL_MODES or cd == 0 or (cd in (2, 3, 4) and PRE_IN_PLANE_MODES)))


def _conv_bn_train_or_eval(x, w, Cs, stride, pad, gamma, beta, rm, rv, training, pre_stats=None, seg=0, bound=False):
    """bound (fp32h2, training): the output y feeds a consumer that applies relu(BatchNorm(y)) in its loader - the convolution records
    max |y| (lmkd_amax_desc::out_words) and the statistics launch turns it into a bound of max |relu(BatchNorm(y))| per frame segment,
    which travels with y as `_lmkd_pre_amax` (its site for the range fence: ("p", gamma))"""
    Cout, _, KH, KW = w.shape
    wp = pack_weights(w, Cs, 0)
    seg = _seg_frames(seg, x.shape[0]) if training else 0      # eval: one table (the running statistics) for every frame
    bw = cw = bnd = None
    if bound and training and x.dtype is torch.float32 and _h2_mode():
        cw, bw = _amax_slot(x.device), _amax_slot(x.device)
        bnd = (cw, bw, ("p", gamma.data_ptr()))
    if seg:
        # both trunk calls of the episode in this launch: per-segment batch statistics -> [2, 5, C]; the two running-statistics updates are
        # deferred and applied in the reference's order (support call, then query call) by apply_deferred
        if _DEFER is None:
            raise RuntimeError("two frame segments need deferred running-statistics updates (ops.set_defer)")
        y, part, T0 = conv_fwd(x, wp, Cout, KH, KW, stride, pad, True, pre_stats, seg=seg, amax_out=cw)
        count = y.numel() // Cout
        stats = bn_stats_train(part, count, gamma, beta, None, None, seg=(T0, seg * (count // y.shape[0])), bound=bnd)
        _DEFER.append((rm, rv, stats[0]))
        _DEFER.append((rm, rv, stats[1]))
        if bw is not None:
            y._lmkd_pre_amax, y._lmkd_pre_site = bw, bnd[2]
        return y, stats
    y, part = conv_fwd(x, wp, Cout, KH, KW, stride, pad, training, pre_stats, amax_out=cw)
    if bw is not None:
        y._lmkd_pre_amax, y._lmkd_pre_site = bw, bnd[2]
    if training:
        if _DEFER is not None:
            stats = bn_stats_train(part, y.numel() // Cout, gamma, beta, None, None, bound=bnd)
            _DEFER.append((rm, rv, stats))
        else:
            stats = bn_stats_train(part, y.numel() // Cout, gamma, beta, rm, rv, bound=bnd)
    else:
        stats = bn_stats_eval(gamma, beta, rm, rv)
    return y, stats


STEM_POOLED_BWD = True      # the stem's BatchNorm backward from the pooled side (lmkd_bn_backward_stats + lmkd_stem_unpool_bn_bwd); False: round-2 path


class StemFn(torch.autograd.Function):
    """conv7x7/2 + BN + ReLU + maxpool3x3/2 (torchvision resnet children 0-3, resnet18_2fc.py:33).
    Input NCHW [F,3,H,W] (the reference's frame layout), output NHWC [F,H/4,W/4,64]."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, rm, rv, training, seg=0):
        """seg = F0 > 0: frames [0, F0) and [F0, F) of x are the two trunk calls of an episode (two BatchNorm batches, one launch per kernel)"""
        _chk(x, w, gamma, beta, rm, rv)
        if x.dim() == 4 and x.shape[-1] == 4 and x.shape[1] != 3:
            x4 = x.contiguous()                      # already NHWC4 (frames_u8_to_nhwc4)
            F_, H, W, _ = x4.shape
        else:
            F_, Cin, H, W = x.shape
            if Cin != 3:
                raise RuntimeError("stem expects 3-channel frames")
            x4 = _empty((F_, H, W, 4), x)
            xd = _amax_out(x4)      # (frames: no site - ToTensor output lies in [0, 1])
            lib().call("lmkd_nchw3_to_nhwc4", _p(x.contiguous()), _p(x4), F_, H, W, _stream(), xd.out_words if xd is not None else None)
        seg = _seg_frames(seg, F_) if training else 0
        c, stats = _conv_bn_train_or_eval(x4, w, 4, 2, 3, gamma, beta, rm, rv, training, seg=seg)
        N, Hc, Wc, C = c.shape
        Ho, Wo = conv_out_size(Hc, 3, 2, 1), conv_out_size(Wc, 3, 2, 1)
        y = _empty_act((N, Ho, Wo, C), x)
        idx = torch.empty((N, Ho, Wo, C), dtype=torch.uint8, device=x.device)
        # training: also the raw convolution output at each window's arg-max - the BatchNorm backward then takes its sums from the
        # pooled tensors (lmkd_bn_backward_stats) instead of the 4x larger pre-pooling ones
        cmax = torch.empty_like(y) if (training and (STEM_POOLED_BWD or seg)) else None
        lib().call("lmkd_bn_relu_maxpool_fwd_seg", _p(c), _p(stats), _p(y), _p(idx), _p(cmax), N, seg if seg else N, Hc, Wc, C, _stream(),
                   _desc_arg(_amax_out(y, ("y", gamma.data_ptr()))))
        if BLOCK_TAPS is not None:
            BLOCK_TAPS.append({"stem_c": c, "stem_st": stats, "stem_idx": idx, "seg": seg})
        if training:
            ctx.save_for_backward(x4, c, stats, idx, gamma, w, cmax)
            ctx.beta = beta
            ctx.amax = _amax_tag(x4)
        ctx.training = training
        ctx.seg = seg
        return y

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        if not ctx.training:
            raise NotImplementedError("backward through eval-mode BatchNorm is not part of the hot path")
        x4, c, stats, idx, gamma, w, cmax = ctx.saved_tensors
        _amax_retag(x4, ctx.amax)      # the maximum recorded in the forward (a saved tensor may come back as a new object)
        dy = dy.contiguous()
        N, Hc, Wc, C = c.shape
        seg = ctx.seg
        if seg:
            # both trunk calls: sums per segment in one reduce + one coefficient launch, then one fused un-pool + BatchNorm-backward pass
            # that also adds (segment 0 + segment 1) into the BatchNorm parameter gradients
            tg = _grad_target(gamma)
            tb = _grad_target(ctx.beta) if tg is not None else None
            direct = tg is not None and tb is not None
            dgamma, dbeta = (tg, tb) if direct else (_empty((C,), c), _empty((C,), c))
            coef = _empty((2, 5, C), c)
            ws = torch.empty(2 * lib().value("lmkd_bn_bwd_workspace", C), dtype=torch.uint8, device=c.device)
            prow, crow = dy.numel() // C // N, c.numel() // C // N
            lib().call("lmkd_bn_backward_stats_seg", _p(dy), _p(cmax), _p(stats), _p(gamma), _p(coef), _p(ws), _p(_tickets(c)),
                       N * prow, seg * prow, N * crow, seg * crow, C, _stream())
            dc = torch.empty_like(c)
            lib().call("lmkd_stem_unpool_bn_bwd_seg", _p(dy), _p(idx), _p(c), _p(stats), _p(coef), _p(dc), _p(dgamma), _p(dbeta), int(direct),
                       N, seg, Hc, Wc, C, _stream(), _desc_arg(_amax_out(dc, ("d", gamma.data_ptr()))))
            if direct:
                dgamma = dbeta = None
        elif cmax is not None:
            # sums of the BatchNorm backward over the pooled tensors, then max-pool backward + BatchNorm backward apply in one pass:
            # the 642 MB pre-pooling gradient is never written
            tg = _grad_target(gamma)
            tb = _grad_target(ctx.beta) if tg is not None else None
            direct = tg is not None and tb is not None
            dgamma, dbeta = (tg, tb) if direct else (_empty((C,), c), _empty((C,), c))
            coef = _empty((3, C), c)
            ws = torch.empty(lib().value("lmkd_bn_bwd_workspace", C), dtype=torch.uint8, device=c.device)
            lib().call("lmkd_bn_backward_stats", _p(dy), _p(cmax), _p(stats), _p(gamma), _p(dgamma), _p(dbeta), _p(coef), _p(ws),
                       _p(_tickets(c)), dy.numel() // C, c.numel() // C, C, int(direct), _stream())
            dc = torch.empty_like(c)
            lib().call("lmkd_stem_unpool_bn_bwd", _p(dy), _p(idx), _p(c), _p(stats), _p(coef), _p(dc), N, Hc, Wc, C, _stream(),
                       _desc_arg(_amax_out(dc, ("d", gamma.data_ptr()))))
            if direct:
                dgamma = dbeta = None
        else:
            g = torch.empty_like(c)
            lib().call("lmkd_maxpool_bwd", _p(dy), _p(idx), _p(g), N, Hc, Wc, C, _stream())
            dc, _, dgamma, dbeta = bn_backward(g, c, None, stats, gamma, 2, dx_out=g, beta=ctx.beta)
        dw = weight_grad(w, x4, dc, 2, 3)
        return None, dw, dgamma, dbeta, None, None, None, None


def frames_pair_to_nhwc4(a, b):
    """the support frames followed by the query frames as ONE NHWC4 tensor [Fa + Fb, H, W, 4] (the stem's input layout; merged trunk call).
    Either input may be NCHW [F, 3, H, W] float frames (the reference's layout) or already NHWC4."""
    _chk(a, b)

    def geom(t):
        if t.dim() == 4 and t.shape[-1] == 4 and t.shape[1] != 3:
            return t.shape[0], t.shape[1], t.shape[2], True
        if t.dim() != 4 or t.shape[1] != 3:
            raise RuntimeError("stem expects 3-channel frames")
        return t.shape[0], t.shape[2], t.shape[3], False
    Fa, H, W, a4 = geom(a)
    Fb, Hb, Wb, b4 = geom(b)
    if (H, W) != (Hb, Wb):
        raise RuntimeError("support and query frames differ in size")
    out = _empty((Fa + Fb, H, W, 4), a)
    words = _amax_slot(out.device) if (_h2_mode() and not (a4 or b4)) else None      # fp32h2: the stem's kernels scale by max |frames|, per segment
    for seg, (t, is4, dst, F_) in enumerate(((a, a4, out[:Fa], Fa), (b, b4, out[Fa:], Fb))):
        if is4:
            dst.copy_(t)
        else:
            lib().call("lmkd_nchw3_to_nhwc4", _p(t.contiguous()), _p(dst), F_, H, W, _stream(),
                       words.data_ptr() + 2 * words.numel() * seg if words is not None else None)      # (bytes: half the words per segment)
    if words is not None:
        out._lmkd_amax = words
    return out


def frames_u8_to_nhwc4(frames_u8, crop_y, crop_x, flip, size, frames_per_video=8, out=None):
    """uint8 frames [F,Hs,Ws,3] (after the host Resize) -> float NHWC4 [F,size,size,4] in [0,1]: per-video crop offsets and
    horizontal-flip flags (int32 device tensors, one entry per video), ToTensor scaling.  The result can be passed to the
    backbones in place of the float NCHW frames (the stem recognises the layout)."""
    _chk(frames_u8, crop_y, crop_x, flip)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise RuntimeError("frames_u8_to_nhwc4 expects uint8 [F,H,W,3] frames")
    F_, Hs, Ws, _ = frames_u8.shape
    nv = F_ // frames_per_video
    if nv * frames_per_video != F_ or crop_y.numel() != nv or crop_x.numel() != nv or flip.numel() != nv:
        raise RuntimeError("one crop/flip entry per video of %d frames expected" % frames_per_video)
    if out is None:
        out = torch.empty((F_, size, size, 4), dtype=torch.float32, device=frames_u8.device)
    elif tuple(out.shape) != (F_, size, size, 4) or out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError("frames_u8_to_nhwc4: `out` must be a contiguous float32 [%d, %d, %d, 4] tensor" % (F_, size, size))
    lib().call("lmkd_frames_u8_to_nhwc4", _p(frames_u8), _p(out), _p(crop_y), _p(crop_x), _p(flip), F_, Hs, Ws, size, size,
               frames_per_video, _stream())
    if _h2_mode():      # ToTensor output lies in [0, 1]: 1.0 is a valid maximum (an upper bound costs range, not correctness) for both frame segments
        out._lmkd_amax = _amax_unit_words(out.device)
    return out


_RESIZE_PLANS = {}


def _resize_plan(n_in, n_out, device):
    key = (n_in, n_out, str(device))
    if key not in _RESIZE_PLANS:
        ks = lib().value("lmkd_resize_plan", n_in, n_out, None, None)
        if ks <= 0:
            raise RuntimeError("lmkd_resize_plan(%d, %d) failed" % (n_in, n_out))
        b = torch.empty((n_out, 2), dtype=torch.int32)
        k = torch.empty((n_out, ks), dtype=torch.int32)
        lib().value("lmkd_resize_plan", n_in, n_out, ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(k.data_ptr()))
        _RESIZE_PLANS[key] = (b.to(device), k.to(device), ks)
    return _RESIZE_PLANS[key]


def resized_shape(H, W, size):
    """output (height, width) of Resize(size) on H x W frames (functional.py:44-59): short side -> `size` (int; unchanged if it
    already matches) or an (h, w) tuple"""
    if isinstance(size, int):
        if (W <= H and W == size) or (H <= W and H == size):
            return H, W
        return (int(size * H / W), size) if W < H else (size, int(size * W / H))
    return tuple(size)


def resize_frames_u8(frames_u8, size):
    """Resize(size) of the reference's frame transform (video_reader.py:96-101; functional.resize_clip -> PIL BILINEAR) on uint8
    frames [F,H,W,C]: short side -> `size` (int; unchanged if it already matches, functional.py:46-50) or (h, w) tuple.
    Bit-identical to Pillow (tests/golden/resize.npz)."""
    _chk(frames_u8)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4:
        raise RuntimeError("resize_frames_u8 expects uint8 [F,H,W,C] frames")
    F_, H, W, C = frames_u8.shape
    oh, ow = resized_shape(H, W, size)
    x = frames_u8                                 # (returned as it is when the size already matches)
    if ow != W:
        b, k, ks = _resize_plan(W, ow, x.device)
        t = torch.empty((F_, H, ow, C), dtype=torch.uint8, device=x.device)
        lib().call("lmkd_resize_pass_u8", _p(x), _p(t), _p(b), _p(k), ks, F_ * H, W, ow, C, _stream())
        x = t
    if oh != H:
        b, k, ks = _resize_plan(H, oh, x.device)
        t = torch.empty((F_, oh, ow, C), dtype=torch.uint8, device=x.device)
        lib().call("lmkd_resize_pass_u8", _p(x), _p(t), _p(b), _p(k), ks, F_, H, oh, ow * C, _stream())
        x = t
    return x


def frames_resize_crop_nhwc4(frames_u8, resize, crop_y, crop_x, flip, size, frames_per_video=8, out=None):
    """Resize(resize) -> crop (size x size at crop_y / crop_x of the resized frame) -> flip -> ToTensor of uint8 frames [F,H,W,3] that share
    one resolution, in ONE launch (lmkd_frames_resize_crop_nhwc4): bit-identical to resize_frames_u8 + frames_u8_to_nhwc4, without the
    two intermediate images and without the part of the resized frame the crop discards (video_reader.py:92-112,377-385)."""
    _chk(frames_u8, crop_y, crop_x, flip)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise RuntimeError("frames_resize_crop_nhwc4 expects uint8 [F,H,W,3] frames")
    F_, Hs, Ws, _ = frames_u8.shape
    oh, ow = resized_shape(Hs, Ws, resize)
    nv = F_ // frames_per_video
    if nv * frames_per_video != F_ or crop_y.numel() != nv or crop_x.numel() != nv or flip.numel() != nv:
        raise RuntimeError("one crop/flip entry per video of %d frames expected" % frames_per_video)
    if size > oh or size > ow:
        raise RuntimeError("crop %d exceeds the resized frame %d x %d" % (size, oh, ow))
    if out is None:
        out = torch.empty((F_, size, size, 4), dtype=torch.float32, device=frames_u8.device)
    elif tuple(out.shape) != (F_, size, size, 4) or out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError("frames_resize_crop_nhwc4: `out` must be a contiguous float32 [%d, %d, %d, 4] tensor" % (F_, size, size))
    bh, kh, ksh = _resize_plan(Ws, ow, frames_u8.device)
    bv, kv, ksv = _resize_plan(Hs, oh, frames_u8.device)
    for f0 in range(0, F_, 65528 // frames_per_video * frames_per_video):      # (the frame index travels in gridDim.y)
        f1 = min(F_, f0 + 65528 // frames_per_video * frames_per_video)
        v0, v1 = f0 // frames_per_video, f1 // frames_per_video
        lib().call("lmkd_frames_resize_crop_nhwc4", _p(frames_u8[f0:f1]), _p(out[f0:f1]), _p(bh), _p(kh), int(ksh), _p(bv), _p(kv), int(ksv),
                   _p(crop_y[v0:v1]), _p(crop_x[v0:v1]), _p(flip[v0:v1]), f1 - f0, Hs, Ws, oh, ow, size, size, frames_per_video, _stream())
    if _h2_mode():      # ToTensor output lies in [0, 1] (frames_u8_to_nhwc4)
        out._lmkd_amax = _amax_unit_words(out.device)
    return out


# parallel.EarlyAllReduce: while set, the trunk's forward registers this tensor hook on the input of its last stage - it fires when the
# backward pass has left that stage (the gradients of the last stage, the heads and the matcher are final)
GRAD_READY_HOOK = None


# Test aid: with BLOCK_TAPS set to a list, every ResBlockFn / StemFn training forward appends its BatchNorm inputs and
# statistics, so a test can reproduce the exact ReLU masks the HIP backward uses (mask flips at pre-activations within fp32
# rounding of zero are the one legitimate source of percent-level gradient differences between two fp32 implementations).
BLOCK_TAPS = None


def split_block_taps(taps):
    """taps of a merged trunk call (entries over both frame segments, "seg" = frames of the first) -> the list two separate calls would
    have left: every entry of the support-frame call, then every entry of the query-frame call (tensors sliced, [2, 5, C] tables split)"""
    if not any(t.get("seg") for t in taps):
        return [{k: v for k, v in t.items() if k != "seg"} for t in taps]
    calls = ([], [])
    for t in taps:
        s = t["seg"]
        for k in (0, 1):
            d = {}
            for key, v in t.items():
                if key == "seg":
                    continue
                d[key] = v[k] if key in ("stem_st", "st1", "st2") else (v[:s] if k == 0 else v[s:])
            calls[k].append(d)
    return calls[0] + calls[1]


def _amax_carriers(x, chain):
    """the saved tensors of a block that carry fp32h2 maxima into its backward: x, the stored activations, the raw outputs (inner stages)"""
    return [x] + [s[4] for s in chain[:-1]] + [s[2] for s in chain[:-1]]


class ResBlockFn(torch.autograd.Function):
    """torchvision residual block as a chain of conv-BN(-ReLU) stages: BasicBlock (conv3x3/s - conv3x3) or Bottleneck (ResNet-50, v1.5:
    conv1x1 - conv3x3/s - conv1x1), (+ conv1x1/s-BN downsample) + add + ReLU.  One autograd node per block; backward is hand-scheduled so
    that the masked gradient buffer of the residual branch is reused as the block-input gradient accumulator."""

    @staticmethod
    def forward(ctx, x, stride, training, seg, *params):
        """params: (w, gamma, beta, running_mean, running_var) of each of the 2 or 3 chain stages, then of the downsample (None x 5 when
        absent); kernel size and padding come from the weights, the stride sits on the first 3x3 stage and on the downsample.
        seg = F0 > 0: frames [0, F0) | [F0, F) of x are the two trunk calls of an episode - one launch per kernel for both, per-segment
        BatchNorm statistics ([2, 5, C] tables), bit-identical activations and activation gradients to two calls"""
        n = len(params) // 5 - 1
        stages = [params[5 * i:5 * i + 5] for i in range(n)]
        wd, gd, bd, rmd, rvd = params[5 * n:]
        strides = [stride if i == n - 2 else 1 for i in range(n)]
        _chk(x, *[s[0] for s in stages], wd)
        if not training and _eval_fused():
            ctx.training = False
            h = x
            for (w, g, b, rm, rv), s in zip(stages[:-1], strides):
                h = conv_bn_eval(h, w, h.shape[-1], s, w.shape[2] // 2, g, b, rm, rv, True)
            r = x if wd is None else conv_bn_eval(x, wd, x.shape[-1], stride, 0, gd, bd, rmd, rvd, False, feeds_conv=False)
            w, g, b, rm, rv = stages[-1]
            return conv_bn_eval(h, w, h.shape[-1], strides[-1], w.shape[2] // 2, g, b, rm, rv, True, r)
        fused = training and _train_fused()
        pre = training and _train_pre()
        if n == 3:
            # fp32h2: the 3x3 convolution's raw input c1 comes from a 1x1 convolution (a gather kernel: no maximum in its epilogue, a reduction
            # pass instead); materialising relu(bn1(c1)) - whose BatchNorm-apply records the maximum for free - is faster here (ResNet-50 + MFM:
            # 12.4 against 11.9 episodes/s), so the Bottleneck keeps the loader-side BatchNorm for the other arithmetics only
            pre = pre and not (os.environ.get("LMKD_R50_PRE_H2", "0") != "1" and _h2_mode())
        seg = _seg_frames(seg, x.shape[0]) if training else 0
        h, hst, chain = x, None, []      # chain: (w, gamma, c, st, a) per stage, what the backward needs
        for i, ((w, g, b, rm, rv), s) in enumerate(zip(stages, strides)):
            # (only the first stage's output asks for the fp32h2 bound of its loader-side BatchNorm)
            c, st = _conv_bn_train_or_eval(h, w, h.shape[-1], s, w.shape[2] // 2, g, b, rm, rv, training, pre_stats=hst, seg=seg, bound=pre and i == 0)
            a = None
            if i < n - 1 and pre:         # the next convolution normalises + rectifies c in its loader: a = relu(bn(c)) is never stored
                h, hst = c, st
            elif i < n - 1:
                h = a = bn_apply(c, st, True, seg=seg, site=("a", g.data_ptr()))
            chain.append((w, g, c, st, a))
        if wd is not None:
            cd, std = _conv_bn_train_or_eval(x, wd, x.shape[-1], stride, 0, gd, bd, rmd, rvd, training, seg=seg)
            res, rst = cd, std
        else:
            cd = std = None
            res, rst = x, None
        if fused:
            y, ybits = bn_apply(c, st, True, res, rst, want_bits=True, seg=seg, site=("y", g.data_ptr()))
        else:
            y, ybits = bn_apply(c, st, True, res, rst, seg=seg, site=("y", g.data_ptr())), None
        ctx.training, ctx.seg, ctx.stride, ctx.strides, ctx.has_ds, ctx.fused = training, seg, stride, strides, wd is not None, fused
        ctx.betas = tuple(s[2] for s in stages) + (bd,)      # BatchNorm biases: the backward may add their gradients straight into .grad (DIRECT_PARAM_GRAD)
        if training:
            if BLOCK_TAPS is not None:      # c{i} / st{i}: the raw convolution outputs of the inner stages in both forms (pre and materialised)
                tap = {}
                for i, s in enumerate(chain[:-1], 1):
                    tap["c%d" % i], tap["st%d" % i] = s[2], s[3]
                BLOCK_TAPS.append({**tap, "y": y, "seg": seg})
            # fused: the backward needs neither a (recomputed from c in the weight-gradient loader) nor y (its mask travels as bits)
            ctx.save_for_backward(x, ybits if fused else y, *[t for s in chain for t in s], wd, gd, cd, std)
            ctx.amax = tuple(_amax_tag(t) for t in _amax_carriers(x, chain))
        return y

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        if not ctx.training:
            raise NotImplementedError("backward through eval-mode BatchNorm is not part of the hot path")
        x, y, *saved = ctx.saved_tensors
        wd, gd, cd, std = saved[-4:]
        chain = [saved[i:i + 5] for i in range(0, len(saved) - 4, 5)]      # (w, gamma, c, st, a) per stage
        n = len(chain)
        for t, tag in zip(_amax_carriers(x, chain), ctx.amax):      # the maxima recorded in the forward (saved tensors may come back as new objects)
            _amax_retag(t, tag)
        dy = dy.contiguous()
        stride, strides, seg = ctx.stride, ctx.strides, ctx.seg
        grads = [None] * n      # (dw, dgamma, dbeta) per stage
        # the last BatchNorm (+ReLU mask from y, or from its bits); g = masked dy = gradient of both residual branches
        w, gam, c, st, _ = chain[-1]
        dc, g, dg, db = bn_backward(dy, c, y, st, gam, 3 if ctx.fused else 1, want_g=True, beta=ctx.betas[n - 1], seg=seg)
        for i in range(n - 1, 0, -1):      # dc: the gradient of stage i's raw output; (c, st, a, gam): its input, the output of stage i - 1
            k = w.shape[2]
            _, gam, c, st, a = chain[i - 1]
            # weight gradient first: its stream then waits for the BatchNorm backward only, not for the data gradient
            dw = weight_grad(w, c, dc, strides[i], k // 2, st, seg=seg) if a is None else weight_grad(w, a, dc, strides[i], k // 2, seg=seg)
            grads[i] = (dw, dg, db)
            da, part = conv_bwd_data(dc, pack_weights(w, w.shape[1], 1), c.shape, w.shape[0], k, k, strides[i], k // 2, bn=(c, st), seg=seg)      # + the BatchNorm's backward sums where the launch has the form
            del dc
            dc, _, dg, db = bn_backward(da, c, None, st, gam, 2, dx_out=da, beta=ctx.betas[i - 1], part=part, seg=seg)    # mask from c*scale+shift > 0
            w = chain[i - 1][0]
        k = w.shape[2]
        grads[0] = (weight_grad(w, x, dc, strides[0], k // 2, seg=seg), dg, db)
        dwd = dgd = dbd = None
        need_dx = ctx.needs_input_grad[0]
        dx = None
        if ctx.has_ds:
            dcd, _, dgd, dbd = bn_backward(g, cd, None, std, gd, 0, dx_out=g, beta=ctx.betas[n], seg=seg)
            dwd = weight_grad(wd, x, dcd, stride, 0, seg=seg)
            if need_dx:
                # the first stage's gradient writes every input pixel; the strided 1x1 one then accumulates onto the quarter of the
                # pixels it reaches (parity classes without a tap launch nothing) instead of writing three quarters of zeros
                dx = conv_bwd_data(dc, pack_weights(w, w.shape[1], 1), x.shape, w.shape[0], k, k, strides[0], k // 2, seg=seg)
                conv_bwd_data(dcd, pack_weights(wd, wd.shape[1], 1), x.shape, wd.shape[0], 1, 1, stride, 0, out=dx, accumulate=True, seg=seg)
        else:
            dx = g                                    # identity branch
            if need_dx:
                conv_bwd_data(dc, pack_weights(w, w.shape[1], 1), x.shape, w.shape[0], k, k, strides[0], k // 2, out=dx, accumulate=True, seg=seg)   # dx += dgrad(first stage)
        return (dx if need_dx else None, None, None, None, *[v for dw, dg, db in grads for v in (dw, dg, db, None, None)],
                dwd, dgd, dbd, None, None)


class PoolHeadFn(torch.autograd.Function):
    """AdaptiveMaxPool2d((4,4)) -> mean over the 16 patches (resnet18_2fc.py:44-54). NHWC in, [F,C] out."""

    @staticmethod
    def forward(ctx, x):
        _chk(x)
        F_, H, W, C = x.shape
        y = _empty((F_, C), x)
        lib().call("lmkd_adaptive_maxpool_mean_fwd", _p(x), _p(y), F_, H, W, C, _stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        (x,) = ctx.saved_tensors
        F_, H, W, C = x.shape
        dx = torch.empty_like(x)
        lib().call("lmkd_adaptive_maxpool_mean_bwd", _p(x), _p(dy.contiguous()), _p(dx), F_, H, W, C, _stream())
        return dx


# ------------------------------------------------------------------------------------------
# attention maps (csrc/cam.hip; heatmap_vis.py:20-48, teacher/code/heatmap_vis.py:16-27)
# ------------------------------------------------------------------------------------------
# The six non-STRM backbones hand their trunk's NHWC map to the pooled head through pool_head().  While a tap is active (cam.grad_cam)
# the map is cut out of the graph there and becomes a leaf: a backward from the logits ends at it and never enters the trunk.  With no
# tap active pool_head IS PoolHeadFn.apply.
_CAM_TAP = [None]
CAM_MAX_C, CAM_MAX_HW = 4096, 2048      # lmkd_gradcam_fwd's limits (csrc/cam.hip)
CAM_GRADCAM, CAM_HIRESCAM = 0, 1


class CamTap:
    """the maps that entered the pooled head during one forward, as autograd leaves.  The two-call schedules (two streams, MobileNet)
    deliver the support frames' map and then the query frames'; the merged trunk call delivers one map of both, support frames first."""

    def __init__(self, n_support):
        self.n_support = int(n_support)
        self.leaves = []

    def record(self, x):
        if len(self.leaves) == 2:
            raise RuntimeError("a third map reached the pooled head in one forward")
        x = x.detach().requires_grad_()
        self.leaves.append(x)
        return x

    def split(self, tensors=None):
        """-> (support, query) of the recorded maps, or of `tensors` (one per recorded map: their gradients)"""
        ts = list(self.leaves if tensors is None else tensors)
        if len(ts) == 2:
            s, q = ts
        elif len(ts) == 1 and ts[0].shape[0] > self.n_support:
            s, q = ts[0][:self.n_support], ts[0][self.n_support:]
        elif len(ts) == 1:
            raise RuntimeError("the one recorded map holds %d frames, the support set alone %d: no query frames reached the pooled head" % (
                ts[0].shape[0], self.n_support))
        else:
            raise RuntimeError("%d maps reached the pooled head: this backbone does not pool through ops.pool_head" % len(ts))
        if s.shape[0] != self.n_support:
            raise RuntimeError("the first recorded map holds %d frames, the support set %d" % (s.shape[0], self.n_support))
        return s, q


@contextlib.contextmanager
def cam_tap(n_support):
    """record the maps entering the pooled head in the body's forward; the tap is cleared afterwards, also when the body raises"""
    if _CAM_TAP[0] is not None:
        raise RuntimeError("a Grad-CAM tap is already active")
    tap = _CAM_TAP[0] = CamTap(n_support)
    try:
        yield tap
    finally:
        _CAM_TAP[0] = None


@contextlib.contextmanager
def module_k_block(root, k_block):
    """the Linear heads and TRX matchers under `root` sum their GEMMs in blocks of k_block terms (gemm's k_block) in the body: the
    `gemm_k_block` attribute that backbone.resnet.Linear, two_head_linear_x and TemporalCrossTransformer hand to their autograd
    Functions (the MFM teacher sets it on its own head for good).  Every module gets it and gets its previous state back afterwards;
    other models, threads and streams of the process are not touched"""
    mods = [(m, m.__dict__.get("gemm_k_block")) for m in root.modules()]
    try:
        for m, _ in mods:
            m.gemm_k_block = int(k_block)
        yield
    finally:
        for m, prev in mods:
            if prev is None:
                m.__dict__.pop("gemm_k_block", None)
            else:
                m.gemm_k_block = prev


def pool_head(x):
    """AdaptiveMaxPool2d((4, 4)) + mean over the patches of the trunk's map (PoolHeadFn), through the tap when one is active"""
    tap = _CAM_TAP[0]
    if tap is not None:
        x = tap.record(x)
    return PoolHeadFn.apply(x)


def gradcam(A, dA, mode=CAM_GRADCAM):
    """A, dA [F, h, w, C] (or [F, HW, C]) fp32: the map entering the pooled head and the score's gradient with respect to it ->
    (weights [F, C], raw [F, h, w], cam [F, h, w]) - mode 0 Grad-CAM, mode 1 HiResCAM (include/lmkd.h lmkd_gradcam_fwd)"""
    _mnv3_chk(A, dA)
    if A.dtype != torch.float32 or dA.dtype != torch.float32 or A.shape != dA.shape or A.dim() not in (3, 4):
        raise RuntimeError("gradcam expects two fp32 tensors of one shape [F, h, w, C] or [F, HW, C]")
    F_, C = A.shape[0], A.shape[-1]
    HW = A.numel() // max(F_ * C, 1)
    weights = _empty((F_, C), A)
    raw = _empty(tuple(A.shape[:-1]), A)
    cam = _empty(tuple(A.shape[:-1]), A)
    lib().call("lmkd_gradcam_fwd", _p(A), _p(dA), _p(weights), _p(raw), _p(cam), F_, HW, C, int(mode), _stream())
    return weights, raw, cam


def jet_lut(device=None):
    """the JET colour table [256, 3] uint8 (RGB) in integers: channel value x2 = clip(765 - |8 i - centre|, 0, 510) with centres 1530
    (red), 1020 (green), 510 (blue), byte = (x2 + 1) >> 1"""
    i = torch.arange(256, dtype=torch.int64)
    lut = torch.stack([((765 - (8 * i - c).abs()).clamp(0, 510) + 1) >> 1 for c in (1530, 1020, 510)], 1).to(torch.uint8)
    return lut if device is None else lut.to(device)


_JET = {}


def cam_overlay(cam, frames_u8, out_hw, image_weight=0.5, lut=None):
    """cam [F, h, w] fp32 in [0, 1] -> uint8 [F, Ho, Wo, 3]: quantised to 8 bit, upsampled to out_hw = (Ho, Wo) as Pillow's BILINEAR does,
    coloured through `lut` (uint8 [256, 3]; default jet_lut) and blended with frames_u8 (uint8 RGB [F, Ho, Wo, 3]; None: the coloured map
    alone) as (colour * (256 - a) + frame * a + 128) >> 8, a = round(256 * image_weight)"""
    _mnv3_chk(cam, frames_u8, lut)
    Ho, Wo = (int(v) for v in out_hw)
    if cam.dtype != torch.float32 or cam.dim() != 3:
        raise RuntimeError("cam_overlay expects an fp32 [F, h, w] map")
    F_, h, w = cam.shape
    if frames_u8 is not None and (frames_u8.dtype != torch.uint8 or tuple(frames_u8.shape) != (F_, Ho, Wo, 3)):
        raise RuntimeError("cam_overlay: frames must be uint8 [%d, %d, %d, 3]" % (F_, Ho, Wo))
    if not 0.0 <= image_weight <= 1.0:
        raise ValueError("image_weight %r outside [0, 1]" % (image_weight,))
    if lut is None:
        key = str(cam.device)
        if key not in _JET:
            _JET[key] = jet_lut(cam.device)
        lut = _JET[key]
    elif lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
        raise RuntimeError("cam_overlay: lut must be uint8 [256, 3]")
    bh, kh, ksh = _resize_plan(w, Wo, cam.device)
    bv, kv, ksv = _resize_plan(h, Ho, cam.device)
    out = torch.empty((F_, Ho, Wo, 3), dtype=torch.uint8, device=cam.device)
    for f0 in range(0, F_, 65535):      # (the frame index travels in gridDim.y)
        f1 = min(F_, f0 + 65535)
        lib().call("lmkd_cam_overlay_u8", _p(cam[f0:f1]), _p(frames_u8[f0:f1]) if frames_u8 is not None else None, _p(out[f0:f1]),
                   _p(bh), _p(kh), int(ksh), _p(bv), _p(kv), int(ksv), _p(lut), f1 - f0, h, w, Ho, Wo, int(round(256 * image_weight)), _stream())
    return out


# ------------------------------------------------------------------------------------------
# matchers
# ------------------------------------------------------------------------------------------
def h2d_async(t, device, dtype=None):
    """host tensor -> device without stalling the stream: through pinned memory, non-blocking.  (A `.to(device)` of a PAGEABLE host
    tensor makes the host wait until the stream has drained: five such copies per episode - labels, class plan - left the GPU idle for
    0.2 - 0.5 ms at every episode start, 1.6 ms per episode in the kernel trace of round 3.)"""
    if t.is_cuda:
        return t.to(dtype) if dtype is not None and t.dtype != dtype else t
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous().pin_memory().to(device, non_blocking=True)


class ClassPlan:
    """Host-side description of the support set's class structure (built from the CPU copy of the labels; ONE small pinned,
    non-blocking upload per episode).  Mirrors torch.unique + _extract_class_indices of the reference (TRX_2fcsup.py:108,118-119)."""

    def __init__(self, support_labels, way, cpu_copy=None, nq_hint=None):
        lab = cpu_copy if cpu_copy is not None else support_labels.detach().to("cpu")
        vals = [int(v) for v in lab.long().tolist()]
        self.way = way
        self.classes = sorted(set(vals))
        for c in self.classes:
            if c < 0 or c >= way:
                raise IndexError("support label %d outside [0,%d)" % (c, way))
        order, self.counts = [], []
        for c in self.classes:
            idx = [i for i, v in enumerate(vals) if v == c]
            order += idx
            self.counts.append(len(idx))
        self.ns = len(vals)
        self.labels = vals                        # class of every support video, host side (OtamFn hands them to the library's checks)
        pos = [0] * self.ns                       # pos[n] = class-sorted position of support video n
        for p_, n in enumerate(order):
            pos[n] = p_
        dev = support_labels.device if support_labels.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        # one upload: [cls | rowmap | identity tail]: rowmap followed by the tail IS full_rowmap() for any query count up to `tail`
        tail = max(64, 2 * self.ns) if nq_hint is None else int(nq_hint)
        # (the class-sorted order rides at the end of the same upload: order[p] = support video at class-sorted position p, for PatchDistFn)
        packed = torch.tensor(vals + pos + list(range(self.ns, self.ns + tail)) + order, dtype=torch.int32)
        self._packed = h2d_async(packed, dev)
        self.cls = self._packed[:self.ns]
        self.rowmap = self._packed[self.ns:2 * self.ns]
        self.order = self._packed[2 * self.ns + tail:]
        self._tail = tail
        self.uniform = len(set(self.counts)) == 1
        self._full = {}
        self._pos = pos

    def full_rowmap(self, nv):
        """support rows class-sorted, query rows in place: [Ns + Nq] int32 - a view of the plan's single upload (no launch) while
        the query count fits its identity tail"""
        if nv not in self._full:
            nq = nv - self.ns
            if 0 <= nq <= self._tail:
                self._full[nv] = self._packed[self.ns:self.ns + nv]
            else:
                self._full[nv] = torch.cat([self.rowmap, torch.arange(self.ns, nv, dtype=torch.int32, device=self.rowmap.device)])
        return self._full[nv]

    def padded_rowmap(self, nv, slots):
        """full_rowmap with class s given slots[s] >= counts[s] video positions (the unused ones stay empty): [Ns + Nq] int32, queries
        after sum(slots).  One small upload per (nv, slots), made on the current stream."""
        key = (nv, tuple(slots))
        if key not in self._full:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the padded class layout of this episode must exist before a hipGraph capture: run the episode eagerly first")
            to_pad, start, p_ = {}, 0, 0
            for c, sl in zip(self.counts, slots):
                for j in range(c):
                    to_pad[p_ + j] = start + j
                p_, start = p_ + c, start + sl
            pos = [to_pad[p] for p in self._pos] + list(range(start, start + nv - self.ns))
            self._full[key] = h2d_async(torch.tensor(pos, dtype=torch.int32), self.device)
        return self._full[key]


# The 2 * card projections of a TRX head (card = 2 frame pairs, 3 frame triples: 6912 columns), for pairs
# P = Xp @ [Wk[:, :Din] | Wk[:, Din:] | Wv[:, :Din] | Wv[:, Din:]]^T (400 x 4608 x 2048), and their
# input gradient dXp = dP @ Wcat are 1x1 convolutions over 400 one-pixel frames: in the three-plane arithmetic (the library default)
# they run the bf16-plane patch kernel - ONE launch of 288 (forward) / 128 (input gradient) workgroups at the convolutions' rate
# instead of 2 + 4 launches of the fp32-MFMA GEMM at 50 - 64 TFLOP/s.  Wcat's fragment-order planes are cached per (Wk, Wv) and rebuilt
# in place when either changes (optimizer step).  The weight gradient stays on the GEMM (weight-gradient stream).
# OFF by default: measured (rocprofv3, in the episode) the forward launch takes 116 us against 2 x 55 for the GEMMs and the input
# gradient (128 workgroups, K = 4608) 226 - 263 us against 4 x 35; same-box episodes/s 35.74 / 35.73 vs 35.60 / 35.58 (f32) and 72.9 vs
# 72.3 (bf16 tensors) - inside the noise.  The heads keep their native fp32 MFMA products.
TRX_PROJ_ON_CONV = False
_WCAT = {}


def _wcat_build(e, wk, wv):
    card = e.get("card", 2)
    D, Din = wk.shape[0], wk.shape[1] // card
    torch.cat([w.detach()[:, s * Din:(s + 1) * Din] for w in (wk, wv) for s in range(card)], 0, out=e["cat"])
    w4 = e["cat"].view(2 * card * D, Din, 1, 1)
    e["p0"] = _pack_weights(w4, Din, 0, out=e.get("p0"))
    e["p1"] = _pack_weights(w4, Din, 1, out=e.get("p1"))
    e["tag"] = (wk._version, wv._version, WEIGHT_EPOCH[0])
    cur = torch.cuda.current_stream()
    ev = torch.cuda.Event()
    ev.record(cur)
    e["event"], e["stream"] = ev, cur.cuda_stream


@contextlib.contextmanager
def _x3_scope():
    """the head's fp32 GEMMs on the convolution kernels: in the one-plane bf16 mode (BASELINE configs[2]: bf16 trunk, heads fp32) the
    process-wide arithmetic is switched to fp32-as-3xbf16 / fp32 tensors for the enclosed launches and restored afterwards (one host
    thread launches at a time: the forward's, then the autograd engine's)"""
    cd = lib().value("lmkd_conv_get_compute_dtype")
    if cd != 1:
        yield
        return
    act = get_activation_dtype()
    lib().call("lmkd_conv_set_compute_dtype", 2)
    set_activation_dtype("fp32")
    try:
        yield
    finally:
        lib().call("lmkd_conv_set_compute_dtype", 1)
        set_activation_dtype(act)


def _trx_wcat_packs(wk, wv, card=2):
    """-> (forward planes, data-gradient planes) of the concatenated projection weight as a [2*card*D, Din, 1, 1] convolution weight, or
    None when the projections stay on the GEMM (native fp32 mode, odd sizes).  Call inside _x3_scope()."""
    cd = lib().value("lmkd_conv_get_compute_dtype")
    D, K2 = wk.shape
    if (not TRX_PROJ_ON_CONV or cd not in (2, 3) or _ACT_DTYPE[0] is not torch.float32 or K2 % (32 * card) != 0 or D % 32 != 0
            or wv.shape != wk.shape):
        return None
    key = (wk.data_ptr(), wv.data_ptr(), cd)
    e = _WCAT.get(key)
    if e is None or e["rk"]() is not wk or e["rv"]() is not wv:
        if len(_WCAT) > 16:
            _WCAT.clear()
        e = _WCAT[key] = {"rk": weakref.ref(wk), "rv": weakref.ref(wv), "card": card,
                          "cat": torch.empty((2 * card * D, K2 // card), dtype=torch.float32, device=wk.device)}
        _wcat_build(e, wk, wv)
    elif e["tag"] != (wk._version, wv._version, WEIGHT_EPOCH[0]):
        _wcat_build(e, wk, wv)
    elif e["stream"] is not None and e["stream"] != torch.cuda.current_stream().cuda_stream:
        torch.cuda.current_stream().wait_event(e["event"])
    return e["p0"], e["p1"]


_TUPLE_TABLES = {}


def trx_tuple_table(L, card, device):
    """device int32 [C(L, card), card]: the frame tuples in itertools.combinations order (TRX.py:70-72).  One tensor per (L, card,
    device) for the life of the process - never freed, a captured hipGraph holds its address.  The upload is synchronous (made by the
    first eager episode, before any capture), so every stream may read the table afterwards."""
    device = torch.device(device)
    key = (L, card, device.index if device.index is not None else torch.cuda.current_device())
    t = _TUPLE_TABLES.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the frame-tuple table for (%d frames, cardinality %d) must exist before a hipGraph capture: run one eager episode first" % (L, card))
        t = _TUPLE_TABLES[key] = torch.tensor(list(itertools.combinations(range(L), card)), dtype=torch.int32).reshape(-1, card).to(device)
    return t


def _trx_card(wk, wv, Din, L):
    """cardinality of the frame tuples, from the width of the tuple Linear (TRX.py:61-62): 2 or 3"""
    card, rest = divmod(wk.shape[1], Din)
    if rest or card not in (2, 3) or wv.shape != wk.shape:
        raise RuntimeError("TRX: k_linear %s / v_linear %s do not take 2 or 3 frames of %d features" % (tuple(wk.shape), tuple(wv.shape), Din))
    if L < card:
        raise RuntimeError("TRX: %d frames per video, tuples of %d" % (L, card))
    return card


def _trx_class_slots(counts, T):
    """video positions per class in the class-sorted tuple rows: the class's own count, raised until count * T is a multiple of 4 (the
    GEMMs over one class's rows read float4 along them).  8 frames: T = 28 or 56, nothing is ever added; 4 frames, pairs (T = 6): an odd
    shot count takes one empty position, whose key / value rows are zero and lie outside the class's softmax segment - they add nothing
    to any product."""
    out = []
    for c in counts:
        while (c * T) % 4:
            c += 1
        out.append(c)
    return out


def _trx_forward(sup, qry, plan, wk, bk, wv, bv, gamma, beta, pe, mask, want_grad, k_block=0):
    """Shared by the student heads (with grad) and the frozen teacher head.
    sup [Ns,L,2048], qry [Nq,L,2048] -> logits [Nq,way] (+ saved tensors).  k_block: gemm's, for every GEMM of the head (the MFM teacher's)"""
    gemm = _gemm_in_blocks(k_block)
    Ns, L, Din = sup.shape
    Nq = qry.shape[0]
    D = wk.shape[0]
    card = _trx_card(wk, wv, Din, L)
    T = math.comb(L, card)
    NV = Ns + Nq
    X = stack_rows(sup.reshape(Ns * L, Din), qry.reshape(Nq * L, Din))      # (the fc head's output halves: a view, no copy)
    Xp = torch.empty_like(X)
    lib().call("lmkd_add_pe", _p(X), _p(pe), _p(mask), _p(Xp), NV * L, Din, L, _stream())
    # per-frame projections: P = Xp @ [Wk[:, slot 0] | .. | Wk[:, slot card-1] | Wv[:, slot 0] | .. | Wv[:, slot card-1]]^T
    PW = 2 * card * D
    P = _empty((NV * L, PW), X)
    packs = None
    if TRX_PROJ_ON_CONV:
        with _x3_scope():
            packs = _trx_wcat_packs(wk, wv, card)
            if packs is not None:
                lib().call("lmkd_conv2d_fwd", _p(Xp), _p(packs[0]), _p(P), None, NV * L, 1, 1, Din, PW, 1, 1, 1, 0, _stream())
    if packs is None:
        gemm("K", "K", NV * L, D, Din, Xp, Din, wk, card * Din, P, PW, batch=card, sB=Din, sC=D)
        gemm("K", "K", NV * L, D, Din, Xp, Din, wv, card * Din, P, PW, batch=card, sB=Din, sC=D, C_off=card * D)
    slots = _trx_class_slots(plan.counts, T)
    padded = slots != plan.counts
    NsP = sum(slots)
    rowmap = plan.padded_rowmap(NV, slots) if padded else plan.full_rowmap(NV)
    alloc = (lambda shape, like: torch.zeros(shape, dtype=torch.float32, device=like.device)) if padded else _empty
    Kn = alloc(((NsP + Nq) * T, D), X)
    V = alloc(((NsP + Nq) * T, D), X)
    Khat = alloc(((NsP + Nq) * T, D), X) if want_grad else None
    rstd = alloc(((NsP + Nq) * T,), X) if want_grad else None
    if card == 2:
        lib().call("lmkd_trx_tuple_ln_fwd", _p(P), _p(bk), _p(bv), _p(gamma), _p(beta), _p(rowmap), _p(Kn), _p(Khat), _p(V),
                   _p(rstd), NV, L, D, _f32(1e-5), _stream())
    else:
        lib().call("lmkd_trx_tuples_ln_fwd", _p(P), _p(bk), _p(bv), _p(gamma), _p(beta), _p(rowmap), _p(trx_tuple_table(L, card, X.device)),
                   _p(Kn), _p(Khat), _p(V), _p(rstd), NV, L, card, T, D, _f32(1e-5), _stream())
    Rs, Rq = NsP * T, Nq * T
    Sk, Sv = Kn[:Rs], V[:Rs]
    Qk, Qv = Kn[Rs:], V[Rs:]
    S = _empty((Rq, Rs), X)
    gemm("K", "K", Rq, Rs, D, Qk, D, Sk, D, S, Rs, alpha=1.0 / math.sqrt(D))
    nseg = len(plan.classes)
    seg_cnt = [c * T for c in plan.counts]      # the class's own tuple rows: its softmax segment
    seg_k = [c * T for c in slots]              # rows the class occupies (== seg_cnt unless padded)
    seg_off = [sum(seg_k[:i]) for i in range(nseg)]
    lib().call("lmkd_segment_softmax_fwd", _p(S), Rq, Rs, nseg, _ints(seg_off), _ints(seg_cnt), _stream())
    proto = _empty((nseg, Rq, D), X)
    if plan.uniform:
        gemm("K", "N", Rq, D, seg_k[0], S, Rs, Sv, D, proto, D, batch=nseg, sA=seg_k[0], sB=seg_k[0] * D, sC=Rq * D)
    else:
        for s in range(nseg):
            gemm("K", "N", Rq, D, seg_k[s], S, Rs, Sv, D, proto, D, A_off=seg_off[s], B_off=seg_off[s] * D, C_off=s * Rq * D)
    logits = torch.zeros((Nq, plan.way), dtype=torch.float32, device=X.device)
    lib().call("lmkd_trx_dist_fwd", _p(Qv), _p(proto), _p(logits), Nq, plan.way, T, D, nseg, _ints(plan.classes), _stream())
    saved = (Xp, Kn, V, Khat, rstd, S, proto, rowmap, seg_off, seg_cnt)
    return logits, saved


def _trx_keep(ctx, saved, sup, qry, wk, bk, wv, bv, gamma, beta, mask, plan, *more):
    """what _trx_backward reads, kept on ctx (saved: _trx_forward's; more: further tensors to save behind the twelve)"""
    Xp, Kn, V, Khat, rstd, S, proto, rowmap, seg_off, seg_cnt = saved
    ctx.save_for_backward(Xp, Kn, V, Khat, rstd, S, proto, rowmap, wk, wv, gamma, mask, *more)
    ctx.plan, ctx.seg_off, ctx.seg_cnt = plan, seg_off, seg_cnt
    ctx.shapes = (sup.shape, qry.shape)
    ctx.biases = (bk, bv, beta)
    ctx.wkv = (wk, wv)      # the parameter OBJECTS (saved tensors come back as other Python objects): identity keys of the caches


class TRXLogitsFn(torch.autograd.Function):
    """TemporalCrossTransformer.forward (TRX_2fcsup.py:74-148) for one head."""

    @staticmethod
    def forward(ctx, sup, qry, wk, bk, wv, bv, gamma, beta, pe, mask, plan, k_block=0):
        _chk(sup, qry, wk, bk, wv, bv, gamma, beta, pe, mask)
        logits, saved = _trx_forward(sup.contiguous(), qry.contiguous(), plan, wk, bk, wv, bv, gamma, beta, pe, mask, True, k_block)
        _trx_keep(ctx, saved, sup, qry, wk, bk, wv, bv, gamma, beta, mask, plan)
        ctx.k_block = k_block
        return logits

    @staticmethod
    def backward(ctx, g):
        _audit.engine_owned(g)
        return _trx_backward(ctx, g) + (None,)


def _kv_norm_backward(dKn, dV, Khat, rstd, gamma, bk, bv, beta):
    """the middle of both K/V heads' backward (TRX, CTX): the key LayerNorm's parameter gradients, dKn -> dKraw in place, the two projection
    bias gradients.  -> dgamma, dbeta, dbk, dbv, each None where deliver_colsum accumulated it directly"""
    rows, D = dKn.shape
    dgamma = deliver_colsum(gamma, dKn, Khat)
    dbeta = deliver_colsum(beta, dKn)
    lib().call("lmkd_layernorm_bwd_rows", _p(dKn), _p(Khat), _p(rstd), _p(gamma), rows, D, _stream())
    return dgamma, dbeta, deliver_colsum(bk, dKn), deliver_colsum(bv, dV)


def _trx_backward(ctx, g, gsim=None, gram=None):
        """backward of TRXLogitsFn (g: d logits) and TRXSupFn (+ gsim: d of the prototype cosine similarities)"""
        gemm = _gemm_in_blocks(getattr(ctx, "k_block", 0))
        Xp, Kn, V, Khat, rstd, S, proto, rowmap, wk, wv, gamma, mask = ctx.saved_tensors[:12]
        plan, seg_off, seg_cnt = ctx.plan, ctx.seg_off, ctx.seg_cnt
        (Ns, L, Din), (Nq, _, _) = ctx.shapes
        D = wk.shape[0]
        card = wk.shape[1] // Din
        T = math.comb(L, card)
        PW = 2 * card * D
        slots = _trx_class_slots(plan.counts, T)      # (see _trx_forward: empty video positions, all-zero rows)
        seg_k = [c * T for c in slots]
        NV, Rs, Rq = Ns + Nq, sum(slots) * T, Nq * T
        rows = Rs + Rq
        nseg = len(plan.classes)
        g = g.contiguous()
        Sk, Sv, Qk, Qv = Kn[:Rs], V[:Rs], Kn[Rs:], V[Rs:]
        dKn = _empty((rows, D), Xp)
        dV = _empty((rows, D), Xp)
        dSk, dSv, dQk, dQv = dKn[:Rs], dV[:Rs], dKn[Rs:], dV[Rs:]
        dp_sim = None
        if gsim is not None:      # needs the prototypes themselves: before they are overwritten below
            dp_sim = torch.empty_like(proto)
            lib().call("lmkd_trx_sup_sim_bwd", _p(proto), _ints(plan.classes), _p(gram), _p(gsim.contiguous()), _p(dp_sim), Nq, plan.way,
                       nseg, T, D, _stream())
        # proto <- dproto ; dQv = -sum_c dproto_c
        lib().call("lmkd_trx_dist_bwd", _p(Qv), _p(proto), _p(g), _p(dQv), Nq, plan.way, T, D, nseg, _ints(plan.classes), _stream())
        if dp_sim is not None:
            lib().call("lmkd_axpby", _p(dp_sim), _p(proto), _f32(1.0), _f32(1.0), proto.numel(), _stream())
        dS = _empty((Rq, Rs), Xp)
        if plan.uniform:
            c = seg_k[0]
            gemm("K", "K", Rq, c, D, proto, D, Sv, D, dS, Rs, batch=nseg, sA=Rq * D, sB=c * D, sC=c)        # dP = dproto @ Vc^T
            gemm("M", "N", c, D, Rq, S, Rs, proto, D, dSv, D, batch=nseg, sA=c, sB=Rq * D, sC=c * D)       # dVc = P^T @ dproto
        else:
            for s in range(nseg):
                c, o = seg_k[s], seg_off[s]
                gemm("K", "K", Rq, c, D, proto, D, Sv, D, dS, Rs, A_off=s * Rq * D, B_off=o * D, C_off=o)
                gemm("M", "N", c, D, Rq, S, Rs, proto, D, dSv, D, A_off=o, B_off=s * Rq * D, C_off=o * D)
        lib().call("lmkd_segment_softmax_bwd", _p(S), _p(dS), Rq, Rs, nseg, _ints(seg_off), _ints(seg_cnt), _stream())
        sc = 1.0 / math.sqrt(D)
        gemm("K", "N", Rq, D, Rs, dS, Rs, Sk, D, dQk, D, alpha=sc)                                        # dQk = sc * dS @ Sk
        gemm("M", "N", Rs, D, Rq, dS, Rs, Qk, D, dSk, D, alpha=sc)                                        # dSk = sc * dS^T @ Qk
        dgamma, dbeta, dbk, dbv = _kv_norm_backward(dKn, dV, Khat, rstd, gamma, *getattr(ctx, "biases", (None, None, None)))
        dP = _empty((NV * L, PW), Xp)
        if card == 2:
            lib().call("lmkd_trx_tuple_bwd_gather", _p(dKn), _p(dV), _p(rowmap), _p(dP), NV, L, D, _stream())
        else:
            lib().call("lmkd_trx_tuples_bwd_gather", _p(dKn), _p(dV), _p(rowmap), _p(trx_tuple_table(L, card, Xp.device)), _p(dP), NV, L,
                       card, T, D, _stream())
        # weight grads: dW[:, slot] = dP[:, blk]^T @ Xp
        dwk, dwv = (deliver_wgrad(w, lambda t, beta, off=off: gemm("M", "N", D, Din, NV * L, dP, PW, Xp, Din, t, card * Din, batch=card, sA=D, sC=Din,
                                                                    A_off=off, beta=beta), (D, card * Din), dP, Xp)
                    for w, off in ((wk, 0), (wv, card * D)))
        # input grads: dXp = sum_blk dP[:, blk] @ W[:, slot]
        dX = _empty((NV * L, Din), Xp)
        packs = None
        if TRX_PROJ_ON_CONV:
            with _x3_scope():
                packs = _trx_wcat_packs(*getattr(ctx, "wkv", (wk, wv)), card)
                if packs is not None:      # dXp = dP @ Wcat: the data gradient of the 1x1 convolution of _trx_forward
                    lib().call("lmkd_conv2d_bwd_data", _p(dP), _p(packs[1]), _p(dX), NV * L, 1, 1, Din, PW, 1, 1, 1, 0, 0, _stream())
        if packs is None:
            for i, w in enumerate((wk, wv)):
                for s_ in range(card):
                    gemm("K", "N", NV * L, Din, D, dP, PW, w, card * Din, dX, Din, beta=0.0 if i + s_ == 0 else 1.0, A_off=(i * card + s_) * D,
                         B_off=s_ * Din)
        if mask is not None:
            lib().call("lmkd_mul", _p(dX), _p(mask), _p(dX), dX.numel(), _stream())
        dsup = dX[:Ns * L].reshape(Ns, L, Din)
        dqry = dX[Ns * L:].reshape(Nq, L, Din)
        return dsup, dqry, dwk, dbk, dwv, dbv, dgamma, dbeta, None, None, None


def _trx_sup_sim(proto, plan, Nq, T, D):
    nseg = len(plan.classes)
    sim = _empty((Nq, plan.way, plan.way), proto)
    gram = _empty((Nq, nseg, nseg), proto)
    lib().call("lmkd_trx_sup_sim_fwd", _p(proto), _ints(plan.classes), _p(sim), _p(gram), Nq, plan.way, nseg, T, D, _stream())
    return sim, gram


class TRXSupFn(torch.autograd.Function):
    """TemporalCrossTransformer.forward of TRX_sup.py:74-178: the TRX logits ('query') plus, per query, the cosine similarity
    between its class prototypes ('support_set' [Nq, way, way])."""

    @staticmethod
    def forward(ctx, sup, qry, wk, bk, wv, bv, gamma, beta, pe, mask, plan):
        _chk(sup, qry, wk, bk, wv, bv, gamma, beta, pe, mask)
        logits, saved = _trx_forward(sup.contiguous(), qry.contiguous(), plan, wk, bk, wv, bv, gamma, beta, pe, mask, True)
        Xp, Kn, V, Khat, rstd, S, proto, rowmap, seg_off, seg_cnt = saved
        L, D = sup.shape[1], wk.shape[0]
        sim, gram = _trx_sup_sim(proto, plan, qry.shape[0], math.comb(L, wk.shape[1] // sup.shape[2]), D)
        _trx_keep(ctx, saved, sup, qry, wk, bk, wv, bv, gamma, beta, mask, plan, gram)
        return logits, sim

    @staticmethod
    def backward(ctx, g, gsim):
        _audit.engine_owned(g, gsim)
        return _trx_backward(ctx, g, gsim, ctx.saved_tensors[12])


def trx_sup_nograd(sup, qry, plan, wk, bk, wv, bv, gamma, beta, pe, mask=None):
    _chk(sup, qry, wk, bk, wv, bv, gamma, beta, pe, mask)
    logits, saved = _trx_forward(sup.contiguous(), qry.contiguous(), plan, wk, bk, wv, bv, gamma, beta, pe, mask, False)
    L, D = sup.shape[1], wk.shape[0]
    return logits, _trx_sup_sim(saved[6], plan, qry.shape[0], math.comb(L, wk.shape[1] // sup.shape[2]), D)[0]


def trx_logits_nograd(sup, qry, plan, wk, bk, wv, bv, gamma, beta, pe, mask=None):
    _chk(sup, qry, wk, bk, wv, bv, gamma, beta, pe, mask)
    return _trx_forward(sup.contiguous(), qry.contiguous(), plan, wk, bk, wv, bv, gamma, beta, pe, mask, False)[0]


# While SEED_SLOTS is a SeedSlots object (a hipGraph is being captured), every dropout mask takes its seed from the next slot of a
# device buffer instead of a kernel argument; the replay loop writes fresh seeds into the slots before each replay.
SEED_SLOTS = None


class SeedSlots:
    def __init__(self, device, n=16):
        self.dev = torch.zeros(n, dtype=torch.int64, device=device)
        self.used = 0

    def next_ptr(self):
        if self.used >= self.dev.numel():
            raise RuntimeError("more than %d dropout calls in one captured episode" % self.dev.numel())
        self.used += 1
        return self.dev.data_ptr() + 8 * (self.used - 1)

    def stage(self, seeds):
        """seeds of the next replay (one per slot used during capture, in call order) -> device, on the current stream.  A fresh
        pinned block per call (torch's pinned allocator does not recycle it before the copy has run): the host may be many replays
        ahead of the device"""
        if not seeds:
            return
        h = torch.zeros(self.dev.numel(), dtype=torch.int64)
        h[:len(seeds)] = torch.tensor(seeds, dtype=torch.int64)
        self.dev.copy_(h.pin_memory(), non_blocking=True)


def dropout_mask(shape, p, seed, device):
    m = torch.empty(shape, dtype=torch.float32, device=device)
    if SEED_SLOTS is not None:      # capture: `seed` is ignored, the slot is filled before every replay
        lib().call("lmkd_dropout_mask_dev", _p(m), m.numel(), _f32(p), ctypes.c_void_p(SEED_SLOTS.next_ptr()), _stream())
    else:
        lib().call("lmkd_dropout_mask", _p(m), m.numel(), _f32(p), ctypes.c_ulonglong(seed), _stream())
    return m


class SupportDKFn(torch.autograd.Function):
    """SupportDK.forward (TRX_2fcsup.py:162-189): labels ignored, class-sorted support assumed."""

    @staticmethod
    def forward(ctx, sup, way, shot):
        sup = sup.contiguous()
        _chk(sup)
        Ns, L, D = sup.shape
        if Ns != way * shot:
            raise RuntimeError("shape '[%d, %d, %d, %d]' is invalid for input of size %d" % (way, shot, L, D, sup.numel()))
        out = _empty((way, way - 1), sup)
        ws = torch.empty(lib().value("lmkd_supportdk_workspace", way), dtype=torch.uint8, device=sup.device)
        lib().call("lmkd_supportdk_fwd", _p(sup), _p(out), way, shot, L, D, _p(ws), _stream())
        ctx.save_for_backward(sup)
        ctx.ws = (way, shot)
        return out

    @staticmethod
    def backward(ctx, g):
        _audit.engine_owned(g)
        (sup,) = ctx.saved_tensors
        way, shot = ctx.ws
        Ns, L, D = sup.shape
        d = torch.empty_like(sup)
        lib().call("lmkd_supportdk_bwd", _p(sup), _p(g.contiguous()), _p(d), way, shot, L, D, _stream())
        return d, None, None


class EDistFn(torch.autograd.Function):
    """e_dist.forward (e_dist_fc2.py:52-91)."""

    @staticmethod
    def forward(ctx, sup, qry, plan):
        sup, qry = sup.contiguous(), qry.contiguous()
        _chk(sup, qry)
        Ns, L, D = sup.shape
        Nq = qry.shape[0]
        sm, qm = _empty((Ns, D), sup), _empty((Nq, D), sup)
        lib().call("lmkd_mean_frames", _p(sup), _p(sm), Ns, L, D, _stream())
        lib().call("lmkd_mean_frames", _p(qry), _p(qm), Nq, L, D, _stream())
        dist = _empty((Nq, Ns), sup)
        logits = _empty((Nq, plan.way), sup)
        lib().call("lmkd_edist_fwd", _p(qm), _p(sm), _p(plan.cls), _p(dist), _p(logits), Nq, Ns, plan.way, D, _stream())
        ctx.save_for_backward(sm, qm, dist)
        ctx.plan, ctx.L = plan, L
        return logits

    @staticmethod
    def backward(ctx, g):
        _audit.engine_owned(g)
        sm, qm, dist = ctx.saved_tensors
        plan, L = ctx.plan, ctx.L
        Ns, D = sm.shape
        Nq = qm.shape[0]
        dqm, dsm = torch.empty_like(qm), torch.empty_like(sm)
        lib().call("lmkd_edist_bwd", _p(qm), _p(sm), _p(plan.cls), _p(dist), _p(g.contiguous()), _p(dqm), _p(dsm), Nq, Ns, plan.way, D, _stream())
        dsup, dqry = _empty((Ns, L, D), sm), _empty((Nq, L, D), sm)
        lib().call("lmkd_mean_frames_bwd", _p(dsm), _p(dsup), Ns, L, D, _stream())
        lib().call("lmkd_mean_frames_bwd", _p(dqm), _p(dqry), Nq, L, D, _stream())
        return dsup, dqry, None


def otam_plan_check(plan):
    """the OTAM head's softmax runs over every class 0 .. way-1: a class without a support video (the reference returns a narrower
    tensor there) is a ValueError, raised from the host-side plan before anything is launched"""
    missing = [c for c in range(plan.way) if c not in plan.classes]
    if missing:
        raise ValueError("the OTAM head needs a support video of every class 0 .. %d: class %d has none (support classes %s)"
                         % (plan.way - 1, missing[0], plan.classes))
    if getattr(plan, "_labels_c", None) is None:
        plan._labels_c = _ints(plan.labels)
    return plan._labels_c


def otam_pitch(Ns, L):
    """row pitch of the [Nq * L, .] matrices over the support frames, and the row count of the support-frame matrices (include/lmkd.h)"""
    return (Ns * L + 3) & ~3


class OtamFn(torch.autograd.Function):
    """CNN_OTAM.forward (teacher/code/model.py:3319-3343): frame cosine distances, the ordered alignment in both directions, class means,
    softmax -> [Nq, way] probabilities.  No parameters.  2 library calls forward (4 launches), 2 backward (4 launches); csrc/otam.hip."""

    @staticmethod
    def forward(ctx, sup, qry, plan):
        labels_c = otam_plan_check(plan)
        sup, qry = sup.contiguous(), qry.contiguous()
        _chk(sup, qry)
        if sup.dtype != torch.float32 or qry.dtype != torch.float32 or sup.dim() != 3 or qry.shape[1:] != sup.shape[1:]:
            raise RuntimeError("OtamFn expects fp32 [N, L, D] features; got %s %s and %s %s" % (sup.dtype, tuple(sup.shape), qry.dtype, tuple(qry.shape)))
        Ns, L, D = sup.shape
        Nq = qry.shape[0]
        if plan.ns != Ns:
            raise RuntimeError("OtamFn: %d support videos, %d support labels" % (Ns, plan.ns))
        ldd = otam_pitch(Ns, L)
        X, Y = qry.view(Nq * L, D), sup.view(Ns * L, D)
        if ldd != Ns * L:      # zero pad rows: the backward's product over the support frames runs over the pitch
            Y = torch.cat([Y, Y.new_zeros(ldd - Ns * L, D)])
        n, dist = _empty((Nq * L, ldd), sup), _empty((Nq * L, ldd), sup)
        rq, rs = _empty((Nq * L,), sup), _empty((Ns * L,), sup)
        lib().call("lmkd_otam_frame_dist_fwd", _p(X), _p(Y), _p(n), _p(rq), _p(rs), _p(dist), Nq, Ns, L, D, _stream())
        cum, logits = _empty((Nq, Ns), sup), _empty((Nq, plan.way), sup)
        lib().call("lmkd_otam_align_fwd", _p(dist), _p(plan.cls), labels_c, _p(cum), _p(logits), Nq, Ns, plan.way, L, _stream())
        ctx.save_for_backward(X, Y, n, rq, rs, dist, cum, logits)
        ctx.plan, ctx.dims = plan, (Ns, Nq, L, D)
        ctx.mark_non_differentiable(cum)
        return logits, cum

    @staticmethod
    def backward(ctx, g, _gcum):
        _audit.engine_owned(g)
        X, Y, n, rq, rs, dist, cum, logits = ctx.saved_tensors
        plan = ctx.plan
        Ns, Nq, L, D = ctx.dims
        ldd = otam_pitch(Ns, L)
        dD = _empty((Nq * L, ldd), X)
        lib().call("lmkd_otam_align_bwd", _p(g.contiguous()), _p(logits), _p(dist), _p(plan.cls), plan._labels_c, _p(dD), Nq, Ns, plan.way, L,
                   _stream())
        Gd, dQ, dS = _empty((Nq * L, ldd), X), _empty((Nq * L, D), X), _empty((ldd, D), X)
        lib().call("lmkd_otam_frame_dist_bwd", _p(dD), _p(X), _p(Y), _p(n), _p(rq), _p(rs), _p(Gd), _p(dQ), _p(dS), Nq, Ns, L, D, _stream())
        return dS[:Ns * L].view(Ns, L, D), dQ.view(Nq, L, D), None


CTX_MAX_FRAMES = 256      # support frames of one class the CTX kernels take (include/lmkd.h)


def _ctx_layout(plan, Ns, L):
    """the class layout lmkd_ctx_attend_* take, cached on the plan: (nseg, seg_off, seg_cnt, seg_col) over the class-sorted support
    positions (plan.order names the video at each position)"""
    if plan.ns != Ns:
        raise RuntimeError("CtxLogitsFn: %d support videos, %d support labels" % (Ns, plan.ns))
    if max(plan.counts) * L > CTX_MAX_FRAMES:
        raise RuntimeError("CtxLogitsFn: a class with %d support videos of %d frames: the CTX kernels take %d frames per class"
                           % (max(plan.counts), L, CTX_MAX_FRAMES))
    lay = getattr(plan, "_ctx_layout", None)
    if lay is None:
        off = [sum(plan.counts[:i]) for i in range(len(plan.counts))]
        lay = plan._ctx_layout = (len(plan.counts), _ints(off), _ints(plan.counts), _ints(plan.classes))
    return lay


def _ctx_forward(sup, qry, plan, wk, bk, wv, bv, gamma, beta, pe, mask, want_grad):
    """CrossTransformer.forward (teacher/code/model.py:2859-2924) in 5 launches whatever the episode's classes look like: position
    encoding (+ dropout), the two projections, LayerNorm of the keys, one attend launch.  -> logits [Nq, way], saved tensors"""
    if sup.dtype != torch.float32 or sup.dim() != 3 or qry.dim() != 3 or qry.shape[1:] != sup.shape[1:]:
        raise RuntimeError("CtxLogitsFn expects fp32 [N, L, Din] features; got %s %s and %s" % (sup.dtype, tuple(sup.shape), tuple(qry.shape)))
    Ns, L, Din = sup.shape
    Nq = qry.shape[0]
    D = wk.shape[0]
    if wk.shape != (D, Din) or wv.shape != (D, Din) or pe.shape != (L, Din):
        raise RuntimeError("CtxLogitsFn: k_linear %s / v_linear %s / pe %s do not take frames of %d features"
                           % (tuple(wk.shape), tuple(wv.shape), tuple(pe.shape), Din))
    nseg, seg_off, seg_cnt, seg_col = _ctx_layout(plan, Ns, L)
    rows = (Ns + Nq) * L
    X = stack_rows(sup.reshape(Ns * L, Din), qry.reshape(Nq * L, Din))
    Xp = torch.empty_like(X)
    lib().call("lmkd_add_pe", _p(X), _p(pe), _p(mask), _p(Xp), rows, Din, L, _stream())
    Kn, V = _empty((rows, D), X), _empty((rows, D), X)
    gemm("K", "K", rows, D, Din, Xp, Din, wk, Din, Kn, D, bias=bk)
    gemm("K", "K", rows, D, Din, Xp, Din, wv, Din, V, D, bias=bv)
    Khat = _empty((rows, D), X) if want_grad else None
    rstd = _empty((rows,), X) if want_grad else None
    lib().call("lmkd_ctx_ln_fwd", _p(Kn), _p(gamma), _p(beta), _p(Kn), _p(Khat), _p(rstd), rows, D, _f32(1e-5), _stream())
    A = _empty((Nq * L, Ns * L), X) if want_grad else None
    logits = _empty((Nq, plan.way), X)
    lib().call("lmkd_ctx_attend_fwd", _p(Kn), _p(V), _p(plan.order), _p(A), _p(logits), Ns, Nq, plan.way, L, D, nseg, seg_off, seg_cnt, seg_col,
               _stream())
    return logits, (Xp, Kn, V, Khat, rstd, A)


class CtxLogitsFn(torch.autograd.Function):
    """CrossTransformer.forward (teacher/code/model.py:2859-2924): the frame-level cross-transformer head, csrc/ctx.hip, DESIGN.md 18.
    Parameter gradients go the way of TRXLogitsFn's, through deliver_wgrad / deliver_colsum."""

    @staticmethod
    def forward(ctx, sup, qry, wk, bk, wv, bv, gamma, beta, pe, mask, plan):
        _chk(sup, qry, wk, bk, wv, bv, gamma, beta, pe, mask)
        logits, (Xp, Kn, V, Khat, rstd, A) = _ctx_forward(sup.contiguous(), qry.contiguous(), plan, wk, bk, wv, bv, gamma, beta, pe, mask, True)
        ctx.save_for_backward(Xp, Kn, V, Khat, rstd, A, wk, wv, gamma, mask)
        ctx.plan = plan
        ctx.shapes = (sup.shape, qry.shape)
        ctx.biases = (bk, bv, beta)
        return logits

    @staticmethod
    def backward(ctx, g):
        _audit.engine_owned(g)
        Xp, Kn, V, Khat, rstd, A, wk, wv, gamma, mask = ctx.saved_tensors
        plan = ctx.plan
        (Ns, L, Din), (Nq, _, _) = ctx.shapes
        D = wk.shape[0]
        rows = (Ns + Nq) * L
        nseg, seg_off, seg_cnt, seg_col = _ctx_layout(plan, Ns, L)
        dS, E = torch.empty_like(A), _empty((nseg * Nq * L, D), Xp)
        dKn, dV = _empty((rows, D), Xp), _empty((rows, D), Xp)
        lib().call("lmkd_ctx_attend_bwd", _p(g.contiguous()), _p(Kn), _p(V), _p(plan.order), _p(A), _p(dS), _p(E), _p(dKn), _p(dV), Ns, Nq, plan.way,
                   L, D, nseg, seg_off, seg_cnt, seg_col, _stream())
        dgamma, dbeta, dbk, dbv = _kv_norm_backward(dKn, dV, Khat, rstd, gamma, *ctx.biases)
        grads = [deliver_wgrad(w, lambda t, beta, dy=dy: gemm("M", "N", D, Din, rows, dy, D, Xp, Din, t, Din, beta=beta), (D, Din), dy, Xp)
                 for w, dy in ((wk, dKn), (wv, dV))]      # dW = dy^T Xp
        dX = _empty((rows, Din), Xp)
        gemm("K", "N", rows, Din, D, dKn, D, wk, Din, dX, Din)
        gemm("K", "N", rows, Din, D, dV, D, wv, Din, dX, Din, beta=1.0)
        if mask is not None:
            lib().call("lmkd_mul", _p(dX), _p(mask), _p(dX), dX.numel(), _stream())
        return (dX[:Ns * L].reshape(Ns, L, Din), dX[Ns * L:].reshape(Nq, L, Din), grads[0], dbk, grads[1], dbv, dgamma, dbeta, None, None,
                None)


def ctx_logits_nograd(sup, qry, plan, wk, bk, wv, bv, gamma, beta, pe, mask=None):
    """the frozen teacher's head: the same five launches, nothing kept"""
    _chk(sup, qry, wk, bk, wv, bv, gamma, beta, pe, mask)
    return _ctx_forward(sup.contiguous(), qry.contiguous(), plan, wk, bk, wv, bv, gamma, beta, pe, mask, False)[0]


# ------------------------------------------------------------------------------------------
# loss / accuracy
# ------------------------------------------------------------------------------------------
class D2MLossFn(torch.autograd.Function):
    """w_kl*kd_loss + w_sup*inter_class_relation + w_ce*cross_entropy (distillers.py:7-30,295-337),
    values and logits gradients in one launch.  Returns a [4] tensor: total, kl, sup, ce."""

    @staticmethod
    def forward(ctx, s_kl, t_kl, s_ce, labels, s_sup, t_sup, T, w_kl, w_sup, w_ce):
        ts = [t.contiguous() if t is not None else None for t in (s_kl, t_kl, s_ce, labels, s_sup, t_sup)]
        s_kl, t_kl, s_ce, labels, s_sup, t_sup = ts
        _chk(*ts)
        ref = s_kl if s_kl is not None else (s_ce if s_ce is not None else s_sup)
        if labels is not None and labels.dtype != torch.int64:
            raise RuntimeError("labels must be int64 (the reference casts with .type(torch.LongTensor), trainwandb.py:441)")
        out = _empty((4,), ref)
        # the three logits gradients live in ONE buffer: the backward scales them with one launch
        sizes = [t.numel() if t is not None else 0 for t in (s_kl, s_ce, s_sup)]
        gbuf = _empty((sum(sizes),), ref)
        g_kl = gbuf[:sizes[0]].view_as(s_kl) if s_kl is not None else None
        g_ce = gbuf[sizes[0]:sizes[0] + sizes[1]].view_as(s_ce) if s_ce is not None else None
        g_sup = gbuf[sizes[0] + sizes[1]:].view_as(s_sup) if s_sup is not None else None
        q = s_kl if s_kl is not None else s_ce
        Rq, C = (q.shape if q is not None else (0, 0))
        Rs, Cs = (s_sup.shape if s_sup is not None else (0, 0))
        lib().call("lmkd_d2m_loss", _p(s_kl), _p(t_kl), _p(s_ce), _p(labels), _p(s_sup), _p(t_sup), Rq, C, Rs, Cs, _f32(T),
                   _f32(w_kl), _f32(w_sup), _f32(w_ce), _p(out), _p(g_kl), _p(g_ce), _p(g_sup), _stream())
        ctx.grads = (gbuf, sizes, tuple(t.shape if t is not None else None for t in (s_kl, s_ce, s_sup)))
        return out

    @staticmethod
    def backward(ctx, gout):
        _audit.engine_owned(gout)
        gbuf, sizes, shapes = ctx.grads
        g = gbuf * gout[0]                         # only the total carries gradient; one launch for the three tensors
        o0, o1 = sizes[0], sizes[0] + sizes[1]
        parts = (g[:o0], g[o0:o1], g[o1:])

        def sc(i):
            return None if shapes[i] is None else parts[i].view(shapes[i])
        return sc(0), None, sc(1), None, sc(2), None, None, None, None, None


class MSELossFn(torch.autograd.Function):
    """F.mse_loss(student, teacher) (mean reduction; distillers.py:138): value + student gradient in one pass."""

    @staticmethod
    def forward(ctx, s, t):
        s, t = s.contiguous(), t.contiguous()
        _chk(s, t)
        if s.shape != t.shape:
            raise RuntimeError("The size of tensor a %s must match the size of tensor b %s" % (tuple(s.shape), tuple(t.shape)))
        out = _empty((1,), s)
        g = torch.empty_like(s)
        ws = torch.empty(lib().value("lmkd_mse_loss_workspace"), dtype=torch.uint8, device=s.device)
        lib().call("lmkd_mse_loss", _p(s), _p(t), s.numel(), _p(out), _p(g), _p(ws), _stream())
        ctx.g = g
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        _audit.engine_owned(gout)
        return ctx.g * gout, None


def accuracy(l1, l2, labels):
    """aggregate_accuracy (utils.py:116-121) on l1 (+ l2): -> (acc 0-dim tensor, predictions int64)"""
    l1 = l1.contiguous()
    l2 = l2.contiguous() if l2 is not None else None
    labels = labels.contiguous()
    _chk(l1, l2, labels)
    R, C = l1.shape
    pred = torch.empty((R,), dtype=torch.int64, device=l1.device)
    acc = _empty((1,), l1)
    lib().call("lmkd_accuracy", _p(l1), _p(l2), _p(labels), _p(pred), _p(acc), R, C, _stream())
    return acc[0], pred


class GlobalAvgPoolFn(torch.autograd.Function):
    """AdaptiveAvgPool2d(1) of the torchvision ResNet-50 the teacher's per-modality model is built on, and the mean over `group`
    consecutive frames with it (Action_Recognition_Resnet50.forward: the mean over a clip's frames of the per-frame means).
    NHWC [F, H, W, C] in the trunk's storage type -> [F / group, C] fp32."""

    @staticmethod
    def forward(ctx, x, group=1):
        _chk(x)
        F_, H, W, C = x.shape
        group = int(group)
        if x.dtype is not _ACT_DTYPE[0]:      # the kernel instance follows the process-wide storage type, not the tensor
            raise RuntimeError("GlobalAvgPoolFn: %s input while the activation storage type is %s" % (x.dtype, get_activation_dtype()))
        if group < 1 or F_ % group:
            raise RuntimeError("GlobalAvgPoolFn: %d frames are no multiple of the group of %d" % (F_, group))
        y = _empty((F_ // group, C), x)
        lib().call("lmkd_global_avgpool_fwd", _p(x), _p(y), F_, H, W, C, group, _stream())
        ctx.shape, ctx.group, ctx.act = (F_, H, W, C), group, (x.dtype, x.device)
        return y

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        F_, H, W, C = ctx.shape
        dy = dy.contiguous()
        _chk(dy)
        dx = torch.empty(ctx.shape, dtype=ctx.act[0], device=ctx.act[1])
        lib().call("lmkd_global_avgpool_bwd", _p(dy), _p(dx), F_, H, W, C, ctx.group, _stream())
        return dx, None


class SoftmaxCEFn(torch.autograd.Function):
    """nn.CrossEntropyLoss (mean) with the accuracy and the predictions of the same pass -> ([2] tensor: loss, accuracy; predictions).
    The logits gradient is written by the forward launch; the backward scales it (D2MLossFn's arrangement)."""

    @staticmethod
    def forward(ctx, logits, labels, labels_host):
        R, C = logits.shape
        out = _empty((2,), logits)
        pred = torch.empty((R,), dtype=torch.int64, device=logits.device)
        g = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        rows = _empty((2 * R,), logits)
        host = ctypes.c_void_p(labels_host.data_ptr()) if labels_host is not None else None
        lib().call("lmkd_softmax_ce", _p(logits), _p(labels), host, _p(out), _p(pred), _p(g), _p(rows), R, C, _stream())
        ctx.g = g
        ctx.mark_non_differentiable(pred)
        return out, pred

    @staticmethod
    def backward(ctx, gout, _gpred):
        _audit.engine_owned(gout)
        return ctx.g * gout[0], None, None      # only the loss carries gradient


def softmax_ce(logits, labels, with_pred=False):
    """criterion(output, label) of pretrain.py (nn.CrossEntropyLoss) for any number of classes -> (loss, accuracy) as 0-dim tensors, the
    loss with its autograd graph; with_pred: (loss, accuracy, predictions).  labels: int64 [R].  Labels on the host are range-checked
    there (a label outside [0, C) raises before anything is launched) and go up through pinned memory; labels already on the device are
    not read back - the kernel indexes with none outside the range and that row's loss is NaN."""
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise RuntimeError("softmax_ce: logits [R, C] and labels [R] expected, got %s and %s" % (tuple(logits.shape), tuple(labels.shape)))
    if labels.dtype != torch.int64:
        raise RuntimeError("labels must be int64")
    if logits.dtype != torch.float32:
        raise RuntimeError("softmax_ce: fp32 logits expected, got %s" % logits.dtype)
    logits = logits.contiguous()
    _chk(logits)
    host = None
    if not labels.is_cuda:
        host = labels.contiguous()
        labels = h2d_async(host, logits.device)
    labels = labels.contiguous()
    _chk(labels)
    out, pred = SoftmaxCEFn.apply(logits, labels, host)
    return (out[0], out[1].detach(), pred) if with_pred else (out[0], out[1].detach())


_plan_cache = [None, None, None]
_cpu_labels = [None, None]
_PLANS_BY_CPU = {}      # (id of the CPU label tensor, its _version, way) -> (weakref, plan): a resident episode pool re-uses its plans


def note_cpu_labels(device_labels, cpu_labels):
    """prepare_task moves the (CPU) support labels to the device; remembering the CPU copy lets get_plan build the class
    plan without a device->host copy, i.e. without draining the stream between episodes."""
    _cpu_labels[0], _cpu_labels[1] = device_labels, cpu_labels


def get_plan(support_labels, way):
    """ClassPlan for this label tensor; cached on tensor identity so Student.forward can build it BEFORE the backbone
    kernels are queued and the classifier reuses it.  Plans are also remembered per CPU label tensor (identity + in-place version):
    an episode that comes round again (a resident pool) costs no upload at all."""
    if _plan_cache[0] is support_labels and _plan_cache[1] == way:
        return _plan_cache[2]
    src = _cpu_labels[1] if _cpu_labels[0] is support_labels else (support_labels if not support_labels.is_cuda else None)
    plan = None
    if src is not None:
        key = (id(src), src._version, way)
        hit = _PLANS_BY_CPU.get(key)
        if hit is not None and hit[0]() is src:
            plan = hit[1]
    if plan is None:
        plan = ClassPlan(support_labels, way, src)
        if src is not None:
            if len(_PLANS_BY_CPU) > 64:
                _PLANS_BY_CPU.clear()
            _PLANS_BY_CPU[(id(src), src._version, way)] = (weakref.ref(src), plan)
    _plan_cache[0], _plan_cache[1], _plan_cache[2] = support_labels, way, plan
    return plan


# ------------------------------------------------------------------------------------------
# MobileNetV3-Large student trunk (model/backbone/moblienetv3.py: torchvision mobilenet_v3_large().features; csrc/mobile.hip)
# ------------------------------------------------------------------------------------------
MNV3_BN_EPS = 1e-3          # torchvision mobilenet_v3_large: BatchNorm2d(eps=0.001, momentum=0.01) everywhere
MNV3_BN_MOMENTUM = 0.01
ACT_NONE, ACT_RELU, ACT_HARDSWISH = 0, 1, 2


def _mnv3_chk(*tensors):
    if _ACT_DTYPE[0] is not torch.float32:
        raise RuntimeError("the MobileNetV3 backbone runs fp32 activations only; set_activation_dtype('%s') is not supported for it"
                           % get_activation_dtype())
    _chk(*tensors)      # (C % 8 == 0 and the shapes: checked by the entry points themselves)


def _mnv3_bn_stats(part, count, bn, training, updates):
    """[5][C] BatchNorm table: train mode from the partial sums `part` ([T][C][2]) of `count` elements per channel, the running-statistics
    update (rm, rv, num_batches_tracked, stats) appended to `updates` (mnv3_running_update applies it); eval mode from the running
    statistics"""
    gamma, beta, rm, rv, nbt = bn
    C = gamma.shape[0]
    stats = _empty((5, C), gamma)
    if training:
        scratch = torch.empty(64 * 2 * C, dtype=torch.float64, device=gamma.device)
        lib().call("lmkd_bn_finalize", _p(part), part.shape[0], C, count, _p(gamma), _p(beta), None, None, _f32(0.0), _f32(MNV3_BN_EPS),
                   _p(stats), _p(scratch), _p(_tickets(part)), _stream(), None)
        if updates is not None:
            updates.append((rm, rv, nbt, stats))
    else:
        lib().call("lmkd_bn_eval_stats", C, _p(gamma), _p(beta), _p(rm), _p(rv), _f32(MNV3_BN_EPS), _p(stats), _stream())
    return stats


def mnv3_running_update(first, second):
    """running mean / var (momentum 0.01) and num_batches_tracked of every BatchNorm of the trunk in ONE launch: first = the updates of the
    support-frame call, second = the query-frame call's (same layers, same order; may be empty), applied in the reference's order"""
    if not first:
        return
    if second and len(second) != len(first):
        raise ValueError("the two trunk calls saw different BatchNorm layers")
    n = len(first)
    P = ctypes.c_void_p * n
    rm = P(*[_pw(e[0]) for e in first])
    rv = P(*[_pw(e[1]) for e in first])
    s0 = P(*[_pw(e[3]) for e in first])
    s1 = P(*[(_pw(second[i][3]) if second else None) for i in range(n)])
    nbt = P(*[_pw(e[2]) for e in first])
    C = (ctypes.c_int * n)(*[e[0].shape[0] for e in first])
    lib().call("lmkd_bn_running_update_multi_nbt", rm, rv, s0, s1, nbt, C, n, _f32(MNV3_BN_MOMENTUM), _stream())


def mnv3_bn_act(x, stats, act, res=None):
    C = x.shape[-1]
    y = torch.empty_like(x)
    _mnv3_chk(x, stats, res)
    lib().call("lmkd_bn_act_fwd", _p(x), _p(stats), _p(res), _p(y), x.numel() // C, C, int(act), _stream())
    return y


def mnv3_bn_act_bwd(dy, x, stats, gamma, act):
    """train-mode backward of mnv3_bn_act -> dx, dgamma, dbeta"""
    C = x.shape[-1]
    rows = x.numel() // C
    _mnv3_chk(dy, x, stats, gamma)
    dx = torch.empty_like(x)
    dparams = _empty((2, C), x)
    ws = torch.empty(lib().value("lmkd_bn_act_bwd_workspace", rows, C), dtype=torch.uint8, device=x.device)
    lib().call("lmkd_bn_act_bwd", _p(dy), _p(x), _p(stats), _p(gamma), _p(dx), _p(dparams), _p(ws), ws.numel(), rows, C, int(act), _stream())
    return dx, dparams[1], dparams[0]


def _stat_part(rows, C, like, training):
    return _empty((lib().value("lmkd_mnv3_stat_tiles", rows), C, 2), like) if training else None


_ONES = {}


def _mnv3_pw_wgrad(dc, x, rows, Cout, Cin, shape):
    """dW = dc^T @ x of a 1x1 convolution: K = rows runs to 400 x 112^2, and the GEMM's workgroups tile only the small Cout x Cin output.
    The rows are split into S slices as a strided batch (S partial products [S][Cout][Cin]), then the slices are added by a second GEMM
    ones[1, S] @ partials[S, Cout Cin] (ones are exact in every arithmetic mode): fixed order, deterministic."""
    S = next((s for s in (64, 32, 16, 8, 4) if rows % s == 0 and rows // s >= 256), 1)
    dw = _empty(shape, x)
    if S == 1:
        return gemm("M", "N", Cout, Cin, rows, dc, Cout, x, Cin, dw, Cin)
    R = rows // S
    part = _empty((S, Cout, Cin), x)
    gemm("M", "N", Cout, Cin, R, dc, Cout, x, Cin, part, Cin, batch=S, sA=R * Cout, sB=R * Cin, sC=Cout * Cin)
    key = (x.device.index, S)
    ones = _ONES.get(key)
    if ones is None:
        ones = _ONES[key] = torch.ones(S, dtype=torch.float32, device=x.device)
    gemm("K", "N", 1, Cout * Cin, S, ones, S, part, Cout * Cin, dw, Cout * Cin)
    return dw


class MnvStemFn(torch.autograd.Function):
    """features.0: Conv2d(3, 16, 3, stride 2, pad 1, no bias) + BatchNorm + Hardswish.  Input NCHW [F, 3, H, W] (the reference's frame
    layout, moved to NHWC4 here) or NHWC4; output NHWC [F, Ho, Wo, 16]"""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, rm, rv, nbt, training, updates):
        _mnv3_chk(x, w)
        if x.dim() == 4 and x.shape[-1] == 4 and x.shape[1] != 3:
            x4 = x.contiguous()                      # already NHWC4 (frames_u8_to_nhwc4)
        else:
            if x.dim() != 4 or x.shape[1] != 3:
                raise RuntimeError("MobileNetV3 stem expects 3-channel frames, NCHW or NHWC4")
            F_, _, H, W = x.shape
            x4 = _empty((F_, H, W, 4), x)
            lib().call("lmkd_nchw3_to_nhwc4", _p(x.contiguous()), _p(x4), F_, H, W, _stream(), None)
        N, H, W, Cs = x4.shape
        if tuple(w.shape) != (16, 3, 3, 3):
            raise RuntimeError("MnvStemFn: a [16, 3, 3, 3] weight expected")
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        c = _empty((N, Ho, Wo, 16), x4)
        part = _stat_part(N * Ho * Wo, 16, x4, training)
        lib().call("lmkd_stem3x3_fwd", _p(x4), _p(w.contiguous()), _p(c), _p(part), N, H, W, _stream())
        stats = _mnv3_bn_stats(part, N * Ho * Wo, (gamma, beta, rm, rv, nbt), training, updates)
        ctx.training = training
        ctx.save_for_backward(x4, c, stats, gamma)
        return mnv3_bn_act(c, stats, ACT_HARDSWISH)

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        if not ctx.training:
            raise RuntimeError("MobileNetV3 backbone: backward through eval-mode BatchNorm is not supported")
        x4, c, stats, gamma = ctx.saved_tensors
        dc, dgamma, dbeta = mnv3_bn_act_bwd(dy.contiguous(), c, stats, gamma, ACT_HARDSWISH)
        N, H, W, _ = x4.shape
        dw = _empty((16, 3, 3, 3), x4)
        ws = torch.empty(lib().value("lmkd_stem3x3_bwd_weight_workspace", N, H, W), dtype=torch.uint8, device=x4.device)
        lib().call("lmkd_stem3x3_bwd_weight", _p(x4), _p(dc), _p(dw), _p(ws), ws.numel(), N, H, W, 0, _stream())
        return None, dw, dgamma, dbeta, None, None, None, None, None


class MnvConvBNActFn(torch.autograd.Function):
    """Conv2dNormActivation of an InvertedResidual / features.16: y = act(BatchNorm(conv(x))) (+ res).
    spec = (kind, K, stride, act): kind 'pw' = 1x1 convolution as a GEMM [N H W, Cin] x [Cout, Cin]^T on lmkd_gemm_f32 (+ lmkd_col_stats for
    the BatchNorm's partial sums); kind 'dw' = depthwise K x K convolution (lmkd_dw_conv_*, statistics in its epilogue).
    res (nullable): the block's shortcut, added after the project BatchNorm (act must be none)."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, rm, rv, nbt, res, spec, training, updates):
        kind, K, stride, act = spec
        x = x.contiguous()
        _mnv3_chk(x, w, res)
        N, H, W, Cin = x.shape
        Cout = w.shape[0]
        w = w.contiguous()
        if kind == "pw":
            rows = N * H * W
            c = _empty((N, H, W, Cout), x)
            gemm("K", "K", rows, Cout, Cin, x, Cin, w, Cin, c, Cout)
            part = _stat_part(rows, Cout, x, training)
            if training:
                lib().call("lmkd_col_stats", _p(c), _p(part), rows, Cout, _stream())
        elif kind == "dw":
            if Cout != Cin or tuple(w.shape[1:]) != (1, K, K):
                raise RuntimeError("MnvConvBNActFn: depthwise weight [C, 1, K, K] expected, got %s" % (tuple(w.shape),))
            pad = (K - 1) // 2
            Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
            rows = N * Ho * Wo
            c = _empty((N, Ho, Wo, Cout), x)
            part = _stat_part(rows, Cout, x, training)
            lib().call("lmkd_dw_conv_fwd", _p(x), _p(w), _p(c), _p(part), N, H, W, Cin, K, stride, _stream())
        else:
            raise ValueError(kind)
        if res is not None and (act != ACT_NONE or res.shape != c.shape):
            raise RuntimeError("MnvConvBNActFn: the residual add follows a BatchNorm without activation, same shape")
        stats = _mnv3_bn_stats(part, rows, (gamma, beta, rm, rv, nbt), training, updates)
        ctx.spec, ctx.training, ctx.has_res = spec, training, res is not None
        ctx.save_for_backward(x, w, c, stats, gamma)
        return mnv3_bn_act(c, stats, act, res)

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        if not ctx.training:
            raise RuntimeError("MobileNetV3 backbone: backward through eval-mode BatchNorm is not supported")
        kind, K, stride, act = ctx.spec
        x, w, c, stats, gamma = ctx.saved_tensors
        dy = dy.contiguous()
        dc, dgamma, dbeta = mnv3_bn_act_bwd(dy, c, stats, gamma, act)
        N, H, W, Cin = x.shape
        Cout = w.shape[0]
        dx = dw = None
        if kind == "pw":
            rows = N * H * W
            if ctx.needs_input_grad[0]:
                dx = _empty((N, H, W, Cin), x)
                gemm("K", "N", rows, Cin, Cout, dc, Cout, w, Cin, dx, Cin)          # dx = dc @ W
            if ctx.needs_input_grad[1]:
                dw = _mnv3_pw_wgrad(dc, x, rows, Cout, Cin, tuple(w.shape))
        else:
            if ctx.needs_input_grad[0]:
                dx = _empty((N, H, W, Cin), x)
                lib().call("lmkd_dw_conv_bwd_data", _p(dc), _p(w), _p(dx), N, H, W, Cin, K, stride, _stream())
            if ctx.needs_input_grad[1]:
                dw = _empty(tuple(w.shape), x)
                ws = torch.empty(lib().value("lmkd_dw_conv_bwd_weight_workspace", N, H, W, Cin, K, stride), dtype=torch.uint8, device=x.device)
                lib().call("lmkd_dw_conv_bwd_weight", _p(x), _p(dc), _p(dw), _p(ws), ws.numel(), N, H, W, Cin, K, stride, 0, _stream())
        dres = dy if ctx.has_res else None
        return dx, dw, dgamma, dbeta, None, None, None, dres, None, None, None


class MnvSEFn(torch.autograd.Function):
    """torchvision SqueezeExcitation: y = a * hardsigmoid(fc2(relu(fc1(mean_hw(a))))), fc1 / fc2 = 1x1 convolutions with bias on [frames, C]
    rows (GEMMs on lmkd_gemm_f32, bias and ReLU in the epilogue)"""

    @staticmethod
    def forward(ctx, a, w1, b1, w2, b2):
        a = a.contiguous()
        _mnv3_chk(a, w1, b1, w2, b2)
        N, H, W, C = a.shape
        Q = w1.shape[0]
        HW = H * W
        m = _empty((N, C), a)
        lib().call("lmkd_se_mean", _p(a), _p(m), N, HW, C, _stream())
        z1 = _empty((N, Q), a)
        gemm("K", "K", N, Q, C, m, C, w1.contiguous(), C, z1, Q, bias=b1, relu=True)
        z2 = _empty((N, C), a)
        gemm("K", "K", N, C, Q, z1, Q, w2.contiguous(), Q, z2, C, bias=b2)
        s = _empty((N, C), a)
        lib().call("lmkd_hardsigmoid_fwd", _p(z2), _p(s), N * C, _stream())
        y = torch.empty_like(a)
        lib().call("lmkd_se_scale_fwd", _p(a), _p(s), _p(y), N, HW, C, _stream())
        ctx.save_for_backward(a, m, z1, z2, s, w1, w2)
        return y

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        a, m, z1, z2, s, w1, w2 = ctx.saved_tensors
        dy = dy.contiguous()
        N, H, W, C = a.shape
        Q = w1.shape[0]
        HW = H * W
        ds = _empty((N, C), a)
        lib().call("lmkd_se_scale_bwd", _p(dy), _p(a), _p(s), None, None, _p(ds), N, HW, C, _stream())
        dz2 = _empty((N, C), a)
        lib().call("lmkd_hardsigmoid_bwd", _p(ds), _p(z2), _p(dz2), N * C, _stream())
        w1c, w2c = w1.contiguous(), w2.contiguous()
        dw2 = _empty(tuple(w2.shape), a)
        gemm("M", "N", C, Q, N, dz2, C, z1, Q, dw2, Q)                 # dW2 = dz2^T @ z1
        db2 = colsum(dz2)
        dz1 = _empty((N, Q), a)
        gemm("K", "N", N, Q, C, dz2, C, w2c, Q, dz1, Q)                # dz1 = dz2 @ W2
        g1 = _empty((N, Q), a)
        lib().call("lmkd_relu_backward", _p(dz1), _p(z1), _p(g1), N * Q, _stream())
        dw1 = _empty(tuple(w1.shape), a)
        gemm("M", "N", Q, C, N, g1, Q, m, C, dw1, C)                   # dW1 = g1^T @ m
        db1 = colsum(g1)
        dm = _empty((N, C), a)
        gemm("K", "N", N, C, Q, g1, Q, w1c, C, dm, C)                  # dm = g1 @ W1
        da = torch.empty_like(a)
        lib().call("lmkd_se_scale_bwd", _p(dy), _p(a), _p(s), _p(dm), _p(da), None, N, HW, C, _stream())
        return da, dw1, db1, dw2, db2


# ------------------------------------------------------------------------------------------
# STRM student family (model/backbone/strm18_student.py, strmbackbone.py, model/classifiers/strm_res18_sup.py; csrc/strm.hip)
# ------------------------------------------------------------------------------------------
STRM_PATCHES = 16
# tests: a dict here collects the selections an episode made - "pool": the arg-max bytes of every PatchPoolFn call in call order,
# "dist": the arg-min rows of every PatchDistFn call, "relu": the ReLU masks of the head in call order (bottleneck MLPs, token MLP
# [V,8,D], pair embedding), "dropout": the three dropout masks (attn_pat.pe, fr_enrich.pe, DistanceLoss) - so that a reference evaluation can run
# on the same selections and masks (as BLOCK_TAPS for the trunk)
STRM_TAPS = None


def _strm_chk(*tensors):
    if _ACT_DTYPE[0] is not torch.float32:
        raise RuntimeError("the STRM backbones run fp32 activations only; set_activation_dtype('%s') is not supported for them"
                           % get_activation_dtype())
    _chk(*tensors)


def strm_patchpool_fwd(x, pe, mask=None):
    """x [F,H,W,C] NHWC -> (y [F,16,C] = (AdaptiveMaxPool2d((4,4))(x) + pe) * mask, idx uint8 [F,16,C] = h * W + w of the maximum)"""
    _strm_chk(x, pe, mask)
    F_, H, W, C = x.shape
    y = _empty((F_, STRM_PATCHES, C), x)
    idx = torch.empty((F_, STRM_PATCHES, C), dtype=torch.uint8, device=x.device)
    lib().call("lmkd_strm_patchpool_fwd", _p(x), _p(pe), _p(mask), _p(y), _p(idx), F_, H, W, C, _stream())
    return y, idx


def strm_patchpool_bwd(dy, mask, idx, H, W):
    """gradient of strm_patchpool_fwd's input from dy [F,16,C] and the stored selections"""
    _strm_chk(dy, mask, idx)
    F_, _, C = dy.shape
    dx = _empty((F_, H, W, C), dy)
    lib().call("lmkd_strm_patchpool_bwd", _p(dy), _p(mask), _p(idx), _p(dx), F_, H, W, C, _stream())
    return dx


class PatchPoolFn(torch.autograd.Function):
    """strm18_student.py:236-246 + the table add and dropout of Self_Attn_Bot.pe (:131-132): NHWC trunk output -> [F,16,C] patches"""

    @staticmethod
    def forward(ctx, x, pe, mask):
        x = x.contiguous()
        y, idx = strm_patchpool_fwd(x, pe, mask)
        if STRM_TAPS is not None:
            STRM_TAPS.setdefault("pool", []).append(idx)
        ctx.save_for_backward(idx, mask)
        ctx.hw = (x.shape[1], x.shape[2])
        return y

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        idx, mask = ctx.saved_tensors
        return strm_patchpool_bwd(dy.contiguous(), mask, idx, *ctx.hw), None, None


def strm_attn_fwd(x, qkv, gamma):
    """x [F,16,C], qkv [F,16,3C] -> (y = gamma * softmax(Q K^T) V + x, probs [F,16,16])"""
    _strm_chk(x, qkv, gamma)
    F_, NP, C = x.shape
    if NP != STRM_PATCHES or tuple(qkv.shape) != (F_, NP, 3 * C):
        raise RuntimeError("strm_attn_fwd expects x [F,16,C] and qkv [F,16,3C]")
    y = torch.empty_like(x)
    probs = _empty((F_, NP, NP), x)
    lib().call("lmkd_strm_attn_fwd", _p(x), _p(qkv), _p(gamma), _p(y), _p(probs), F_, C, _stream())
    return y, probs


def strm_attn_bwd(dy, qkv, probs, gamma):
    """-> (dqkv [F,16,3C], dgamma [1]); the residual's input gradient is dy"""
    _strm_chk(dy, qkv, probs, gamma)
    F_, NP, C = dy.shape
    dqkv = torch.empty_like(qkv)
    part = _empty((F_,), dy)
    dgamma = _empty((1,), dy)
    lib().call("lmkd_strm_attn_bwd", _p(dy), _p(qkv), _p(probs), _p(gamma), _p(dqkv), _p(part), _p(dgamma), F_, C, _stream())
    return dqkv, dgamma


class PatchAttnFn(torch.autograd.Function):
    """Self_Attn_Bot.forward (strm18_student.py:134-163) on the table-added patches: the three projections as ONE GEMM over the
    concatenated weights, then energy / softmax / attn V / gamma * out + x per frame in one launch"""

    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, wv, bv, gamma):
        x = x.contiguous()
        F_, NP, C = x.shape
        wcat = torch.cat([wq, wk, wv], 0)
        bcat = torch.cat([bq, bk, bv], 0)
        _strm_chk(x, wcat, bcat, gamma)
        qkv = _empty((F_, NP, 3 * C), x)
        gemm("K", "K", F_ * NP, 3 * C, C, x, C, wcat, C, qkv, 3 * C, bias=bcat)
        y, probs = strm_attn_fwd(x, qkv, gamma)
        ctx.save_for_backward(x, wcat, qkv, probs, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        x, wcat, qkv, probs, gamma = ctx.saved_tensors
        dy = dy.contiguous()
        F_, NP, C = x.shape
        M = F_ * NP
        dqkv, dgamma = strm_attn_bwd(dy, qkv, probs, gamma)
        dw = _empty((3 * C, C), x)
        gemm("M", "N", 3 * C, C, M, dqkv, 3 * C, x, C, dw, C)            # d[Wq; Wk; Wv] = dqkv^T @ x
        db = colsum(dqkv.view(M, 3 * C))
        dx = dy.clone()
        gemm("K", "N", M, C, 3 * C, dqkv, 3 * C, wcat, C, dx, C, beta=1.0)      # dx = dy + dqkv @ [Wq; Wk; Wv]
        return dx, dw[:C], db[:C], dw[C:2 * C], db[C:2 * C], dw[2 * C:], db[2 * C:], dgamma


GEMM_ROW_TILE = 64      # lmkd_gemm_f32 rounds a row's dot product according to the row's position inside its 64-row tile


def _row_segments(M, seg):
    """row ranges to launch a row-wise GEMM over: the whole range when the second trunk call's rows start on a tile boundary, else one
    launch per call - then every row sits where it would in the reference's two separate calls and the result is bit-identical to them
    (measured: 1 ulp differences in res18_2048's output otherwise, tests/test_gpu_strm.py::test_one_call_head_equals_two_calls)"""
    if not seg or seg >= M or seg % GEMM_ROW_TILE == 0:
        return [(0, M)]
    return [(0, seg), (seg, M - seg)]


class LinearXFn(torch.autograd.Function):
    """y = relu?(x W^T + b) (+ res): nn.Linear with the ReLU in the GEMM's epilogue or the residual in its beta = 1 accumulate
    (Bottleneck_Perceptron_3_layer_res / Bottleneck_Perceptron_2_layer, res18_2048, fc1 / fc2: strm18_student.py:65-99,258-276).
    seg: rows [0, seg) come from the support frames, the rest from the query frames (_row_segments)."""

    @staticmethod
    def forward(ctx, x, w, b, relu, res, seg=0, k_block=0):
        x = x.contiguous()
        w = w.contiguous()
        _strm_chk(x, w, b, res)
        if relu and res is not None:
            raise RuntimeError("LinearXFn: ReLU and residual together are not used by any STRM layer")
        M, K = x.shape
        N = w.shape[0]
        y = res.contiguous().clone() if res is not None else _empty((M, N), x)
        for r0, rows in _row_segments(M, seg):
            gemm("K", "K", rows, N, K, x, K, w, K, y, N, beta=1.0 if res is not None else 0.0, bias=b, relu=relu, A_off=r0 * K, C_off=r0 * N,
                 k_block=k_block)
        if relu and STRM_TAPS is not None:
            STRM_TAPS.setdefault("relu", []).append(y > 0)
        ctx.save_for_backward(x, w, y if relu else None)
        ctx.has_res, ctx.seg, ctx.k_block = res is not None, seg, k_block
        return y

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        x, w, y = ctx.saved_tensors
        dy = dy.contiguous()
        M, K = x.shape
        N = w.shape[0]
        g = dy
        if y is not None:
            g = _empty((M, N), x)
            lib().call("lmkd_relu_backward", _p(dy), _p(y), _p(g), M * N, _stream())
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _empty((M, K), x)
            for r0, rows in _row_segments(M, ctx.seg):
                gemm("K", "N", rows, K, N, g, N, w, K, dx, K, A_off=r0 * N, C_off=r0 * K, k_block=ctx.k_block)
        if ctx.needs_input_grad[1]:
            dw = _empty((N, K), x)
            gemm("M", "N", N, K, M, g, N, x, K, dw, K)
        if ctx.needs_input_grad[2]:
            db = colsum(g)
        return dx, dw, db, None, (dy if ctx.has_res else None), None, None


class PatchMeanFn(torch.autograd.Function):
    """torch.mean over the 16 patches (strm18_student.py:254-255): [F,16,C] -> [F,C]"""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        _strm_chk(x)
        F_, NP, C = x.shape
        y = _empty((F_, C), x)
        lib().call("lmkd_mean_frames", _p(x), _p(y), F_, NP, C, _stream())
        ctx.shape = (F_, NP, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        F_, NP, C = ctx.shape
        dx = _empty((F_, NP, C), dy)
        lib().call("lmkd_mean_frames_bwd", _p(dy.contiguous()), _p(dx), F_, NP, C, _stream())
        return dx


def strm_tokmlp_fwd(x, pe, mask, w1, b1, w2, b2):
    """x [V,L,D], 2 <= L <= 16 -> (xp = (x + pe) * mask, y = W2 relu(W1 xp + b1) + b2 + xp along the frame axis)"""
    _strm_chk(x, pe, mask, w1, b1, w2, b2)
    V, L, D = x.shape
    xp, y = torch.empty_like(x), torch.empty_like(x)
    hmask = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if STRM_TAPS is not None else None
    lib().call("lmkd_strm_tokmlp_fwd", _p(x), _p(pe), _p(mask), _p(w1), _p(b1), _p(w2), _p(b2), _p(xp), _p(y), _p(hmask), V, L, D, _stream())
    if hmask is not None:
        STRM_TAPS.setdefault("relu", []).append(hmask)
    return xp, y


def strm_tokmlp_bwd(dy, xp, mask, w1, b1, w2):
    """-> (dx, dW1 [L,L], db1 [L], dW2 [L,L], db2 [L]): the library's dparams row is dW1 | db1 | dW2 | db2, 2 L^2 + 2 L floats"""
    _strm_chk(dy, xp, mask, w1, b1, w2)
    V, L, D = dy.shape
    dx = torch.empty_like(dy)
    part = _empty((lib().value("lmkd_strm_tokmlp_parts", V, D), 2 * L * L + 2 * L), dy)
    dp = _empty((2 * L * L + 2 * L,), dy)
    lib().call("lmkd_strm_tokmlp_bwd", _p(dy), _p(xp), _p(mask), _p(w1), _p(b1), _p(w2), _p(dx), _p(part), _p(dp), V, L, D, _stream())
    n = L * L
    return dx, dp[:n].view(L, L), dp[n:n + L], dp[n + L:2 * n + L].view(L, L), dp[2 * n + L:]


class TokenMLPFn(torch.autograd.Function):
    """MLP_Mix_Enrich.forward up to residual2 (strm18_student.py:185-196): table add + dropout, Token_Perceptron over the frames, residual"""

    @staticmethod
    def forward(ctx, x, pe, mask, w1, b1, w2, b2):
        x = x.contiguous()
        w1, w2 = w1.contiguous(), w2.contiguous()
        xp, y = strm_tokmlp_fwd(x, pe, mask, w1, b1, w2, b2)
        ctx.save_for_backward(xp, mask, w1, b1, w2)
        return y

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        xp, mask, w1, b1, w2 = ctx.saved_tensors
        dx, dw1, db1, dw2, db2 = strm_tokmlp_bwd(dy.contiguous(), xp, mask, w1, b1, w2)
        return dx, None, None, dw1, db1, dw2, db2


def _strm_plan_check(plan, Ns):
    if not plan.uniform or len(plan.classes) != plan.way or plan.ns != Ns:
        raise NotImplementedError("the patch-distance head needs every one of the %d classes with the same number of support videos "
                                  "(got %s)" % (plan.way, plan.counts))
    return plan.counts[0]


def strm_patchdist_embed(X, w, b, L):
    """X [NV*L, Din] frame features, clsW weight [Hd, 2 Din] -> (P [NV*L, 2 Hd] per-frame projections through both halves of clsW,
    E [NV*T, Hd] = relu(P_a[i] + P_b[j] + b) per frame pair)"""
    _strm_chk(X, w, b)
    M, Din = X.shape
    Hd = w.shape[0]
    P = _empty((M, 2 * Hd), X)
    gemm("K", "K", M, Hd, Din, X, Din, w, 2 * Din, P, 2 * Hd)
    gemm("K", "K", M, Hd, Din, X, Din, w, 2 * Din, P, 2 * Hd, B_off=Din, C_off=Hd)
    NV = M // L
    E = _empty((NV * (L * (L - 1) // 2), Hd), X)
    lib().call("lmkd_strm_pair_embed", _p(P), _p(b), _p(E), NV, L, Hd, _stream())
    if STRM_TAPS is not None:
        STRM_TAPS.setdefault("relu", []).append(E > 0)
    return P, E


def set_patchdist_tiled(mode):
    """which minimum-distance kernel strm_patchdist_fwd launches, process-wide (lmkd_patchdist_set_tiled): -1 = the measured dispatch
    (the LDS-tiled kernel for L > 8), 0 = never tiled, 1 = always tiled, also at L <= 8.  Both kernels give the same bits."""
    lib().call("lmkd_patchdist_set_tiled", int(mode))


def strm_patchdist_fwd(E, plan, Ns, Nq, L):
    """-> (logits [Nq, way], dist [Nq*T, way], idx int32 [Nq*T, way]: row member * T + t of the nearest support pair row per class)"""
    shot = _strm_plan_check(plan, Ns)
    T = L * (L - 1) // 2
    dist = _empty((Nq * T, plan.way), E)
    idx = torch.empty((Nq * T, plan.way), dtype=torch.int32, device=E.device)
    logits = _empty((Nq, plan.way), E)
    lib().call("lmkd_strm_patchdist_fwd", _p(E), _p(plan.order), _p(dist), _p(idx), _p(logits), Ns, Nq, plan.way, shot, L, E.shape[1], _stream())
    return logits, dist, idx


def strm_patchdist_bwd(E, plan, dist, idx, g, Ns, Nq, L):
    """g [Nq, way], explicit selections idx -> (dpre [NV*T, Hd] gradient before the ReLU, dP [NV*L, 2 Hd])"""
    shot = _strm_plan_check(plan, Ns)
    _strm_chk(E, dist, idx, g)
    Hd = E.shape[1]
    dpre = torch.empty_like(E)
    dP = _empty(((Ns + Nq) * L, 2 * Hd), E)
    lib().call("lmkd_strm_patchdist_bwd", _p(E), _p(plan.order), _p(plan.rowmap), _p(dist), _p(idx), _p(g), _p(dpre), _p(dP), Ns, Nq, plan.way,
               shot, L, Hd, _stream())
    return dpre, dP


class PatchDistFn(torch.autograd.Function):
    """DistanceLoss.forward (strm_res18_sup.py:188-243): dropout, clsW over frame pairs as two per-frame half projections, ReLU, per class
    the minimum Euclidean distance over the class's support pair rows, mean over the pairs, negated -> [Nq, way]"""

    @staticmethod
    def forward(ctx, sup, qry, w, b, mask, plan):
        Ns, L, Din = sup.shape
        Nq = qry.shape[0]
        X = stack_rows(sup.reshape(Ns * L, Din), qry.reshape(Nq * L, Din))
        w = w.contiguous()
        _strm_chk(X, w, b, mask)
        if mask is not None:
            Xd = torch.empty_like(X)
            lib().call("lmkd_mul", _p(X), _p(mask), _p(Xd), X.numel(), _stream())
        else:
            Xd = X
        P, E = strm_patchdist_embed(Xd, w, b, L)
        logits, dist, idx = strm_patchdist_fwd(E, plan, Ns, Nq, L)
        if STRM_TAPS is not None:
            STRM_TAPS.setdefault("dist", []).append(idx)
        ctx.save_for_backward(Xd, w, E, dist, idx, mask)
        ctx.plan, ctx.dims = plan, (Ns, Nq, L)
        return logits

    @staticmethod
    def backward(ctx, g):
        _audit.engine_owned(g)
        Xd, w, E, dist, idx, mask = ctx.saved_tensors
        Ns, Nq, L = ctx.dims
        dX, dw, db = strm_patchdist_grads(Xd, w, E, ctx.plan, dist, idx, g.contiguous(), mask, Ns, Nq, L)
        Din = Xd.shape[1]
        return dX[:Ns * L].view(Ns, L, Din), dX[Ns * L:].view(Nq, L, Din), dw, db, None, None


def strm_patchdist_grads(Xd, w, E, plan, dist, idx, g, mask, Ns, Nq, L):
    """the whole backward of PatchDistFn from explicit selections: Xd [NV*L, Din] (dropout applied), E = strm_patchdist_embed(Xd, ...)[1],
    dist / idx [Nq*T, way] as strm_patchdist_fwd returns them, g [Nq, way] -> (dX [NV*L, Din], dclsW [Hd, 2 Din], dbias [Hd])"""
    M, Din = Xd.shape
    Hd = w.shape[0]
    dpre, dP = strm_patchdist_bwd(E, plan, dist, idx, g, Ns, Nq, L)
    db = colsum(dpre)
    dw = _empty((Hd, 2 * Din), Xd)
    gemm("M", "N", Hd, Din, M, dP, 2 * Hd, Xd, Din, dw, 2 * Din)                           # dclsW[:, :Din] = dP_a^T @ X
    gemm("M", "N", Hd, Din, M, dP, 2 * Hd, Xd, Din, dw, 2 * Din, A_off=Hd, C_off=Din)      # dclsW[:, Din:] = dP_b^T @ X
    dX = _empty((M, Din), Xd)
    gemm("K", "N", M, Din, Hd, dP, 2 * Hd, w, 2 * Din, dX, Din)
    gemm("K", "N", M, Din, Hd, dP, 2 * Hd, w, 2 * Din, dX, Din, beta=1.0, A_off=Hd, B_off=Din)
    if mask is not None:
        lib().call("lmkd_mul", _p(dX), _p(mask), _p(dX), dX.numel(), _stream())
    return dX, dw, db


# ------------------------------------------------------------------------------------------
# MFM teacher fusion, training (teacher/mfm.py; csrc/mfm.hip): the parts of nn.TransformerEncoderLayer that are not GEMMs,
# as autograd Functions on the current stream.  Parameter gradients go back through autograd: the direct-accumulation paths above
# belong to the student's pipelined episode, and the teacher trainer owns a plain optimizer step.
# ------------------------------------------------------------------------------------------
MFM_LN_EPS = 1e-5


class MaskMulFn(torch.autograd.Function):
    """x o mask: a feature dropout (nn.Dropout) whose mask (0 or 1/(1-p), lmkd_dropout_mask) the caller made"""

    @staticmethod
    def forward(ctx, x, mask):
        x = x.contiguous()
        _chk(x, mask)
        if mask.shape != x.shape:
            raise RuntimeError("dropout mask %s for a %s tensor" % (tuple(mask.shape), tuple(x.shape)))
        ctx.save_for_backward(mask)
        y = torch.empty_like(x)
        lib().call("lmkd_mul", _p(x), _p(mask), _p(y), x.numel(), _stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        mask, = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        lib().call("lmkd_mul", _p(dy), _p(mask), _p(dx), dy.numel(), _stream())
        return dx, None


def feature_dropout(x, mask):
    return x if mask is None else MaskMulFn.apply(x, mask)


class SumFn(torch.autograd.Function):
    """x_0 + x_1 + ... in that order on lmkd_axpby (the three fused features, model.py:1632-1633)"""

    @staticmethod
    def forward(ctx, *xs):
        xs = [x.contiguous() for x in xs]
        _chk(*xs)
        if any(x.shape != xs[0].shape for x in xs):
            raise RuntimeError("SumFn: shapes %s" % [tuple(x.shape) for x in xs])
        out = torch.empty_like(xs[0])
        for i, x in enumerate(xs):
            lib().call("lmkd_axpby", _p(x), _p(out), _f32(1.0), _f32(1.0 if i else 0.0), out.numel(), _stream())
        return out

    @staticmethod
    def backward(ctx, g):
        _audit.engine_owned(g)
        return tuple(g if need else None for need in ctx.needs_input_grad)


class MfmLayerNormFn(torch.autograd.Function):
    """LayerNorm(x + res) * gamma + beta, the post-norm of nn.TransformerEncoderLayer (norm1 / norm2): x, res [rows, D].
    Saved for the backward: xhat [rows, D], rstd [rows]."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta):
        x, res = x.contiguous(), res.contiguous()
        _chk(x, res, gamma, beta)
        rows, D = x.shape
        y, xhat, rstd = _empty((rows, D), x), _empty((rows, D), x), _empty((rows,), x)
        lib().call("lmkd_layernorm_train_fwd", _p(x), _p(res), rows, _p(gamma), _p(beta), None, _p(y), D, _p(xhat), _p(rstd), rows, D,
                   _f32(MFM_LN_EPS), _stream())
        ctx.save_for_backward(xhat, rstd, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        _audit.engine_owned(dy)
        xhat, rstd, gamma = ctx.saved_tensors
        dy = dy.contiguous()
        rows, D = xhat.shape
        dpre = _empty((rows, D), dy)
        lib().call("lmkd_layernorm_train_bwd", _p(dy), D, None, _p(xhat), _p(rstd), _p(gamma), _p(dpre), None, rows, D, _stream())
        dgamma = colsum(dy, xhat) if ctx.needs_input_grad[2] else None
        dbeta = colsum(dy) if ctx.needs_input_grad[3] else None
        return dpre, dpre, dgamma, dbeta      # d(x + res) reaches both summands


class MfmPosCatFn(torch.autograd.Function):
    """cat_i( dropout_i( LayerNorm_i(x_i + emb_i[r mod L]) ) ) -> [rows, n * d]  (TrainablePositionalEncoding.forward, model.py:1143-1151,
    and the torch.cat of the fusions' forward, :1321 / :1381).  Arguments after L: per modality x [rows, d], emb [L, d], gamma, beta,
    mask ([rows, d] or None).  Each LayerNorm writes its column slice of the result; in the backward each reads its slice of the
    gradient at the result's row stride.  The embedding gradient is the sum of dpre over the videos per position."""

    @staticmethod
    def forward(ctx, L, *a):
        n = len(a) // 5
        if len(a) != 5 * n or n == 0:
            raise RuntimeError("MfmPosCatFn: five arguments per modality")
        xs = [a[5 * i].contiguous() for i in range(n)]
        embs = [a[5 * i + 1].contiguous() for i in range(n)]
        rows, d = xs[0].shape
        D = n * d
        for i in range(n):
            _chk(xs[i], embs[i], a[5 * i + 2], a[5 * i + 3], a[5 * i + 4])
            if xs[i].shape != (rows, d) or embs[i].shape != (L, d) or rows % L:
                raise RuntimeError("MfmPosCatFn: modality %d is %s with embeddings %s, expected (%d, %d) and (%d, %d)"
                                   % (i, tuple(xs[i].shape), tuple(embs[i].shape), rows, d, L, d))
            if a[5 * i + 4] is not None and a[5 * i + 4].shape != (rows, d):
                raise RuntimeError("MfmPosCatFn: dropout mask %s for rows of %s" % (tuple(a[5 * i + 4].shape), (rows, d)))
        cat = _empty((rows, D), xs[0])
        saved = []
        for i in range(n):
            gamma, beta, mask = a[5 * i + 2], a[5 * i + 3], a[5 * i + 4]
            xhat, rstd = _empty((rows, d), cat), _empty((rows,), cat)
            if _audit.ON:
                _audit.note(cat)
            lib().call("lmkd_layernorm_train_fwd", _p(xs[i]), _p(embs[i]), L, _p(gamma), _p(beta), _p(mask),
                       ctypes.c_void_p(cat.data_ptr() + 4 * i * d), D, _p(xhat), _p(rstd), rows, d, _f32(MFM_LN_EPS), _stream())
            saved += [xhat, rstd, gamma, mask]
        ctx.save_for_backward(*saved)
        ctx.n, ctx.L = n, L
        return cat

    @staticmethod
    def backward(ctx, dcat):
        _audit.engine_owned(dcat)
        dcat = dcat.contiguous()
        n, L = ctx.n, ctx.L
        rows, D = dcat.shape
        d = D // n
        out = [None]
        for i in range(n):
            xhat, rstd, gamma, mask = ctx.saved_tensors[4 * i:4 * i + 4]
            need = ctx.needs_input_grad[1 + 5 * i:1 + 5 * i + 4]
            dpre = _empty((rows, d), dcat)
            dyc = _empty((rows, d), dcat) if need[2] or need[3] else None
            if _audit.ON:
                _audit.note(dcat)
            lib().call("lmkd_layernorm_train_bwd", ctypes.c_void_p(dcat.data_ptr() + 4 * i * d), D, _p(mask), _p(xhat), _p(rstd), _p(gamma),
                       _p(dpre), _p(dyc), rows, d, _stream())
            demb = colsum(dpre.view(rows // L, L * d)).view(L, d) if need[1] else None
            out += [dpre if need[0] else None, demb, colsum(dyc, xhat) if need[2] else None, colsum(dyc) if need[3] else None, None]
        return tuple(out)


MFM_MAX_L = 16      # tokens per sequence of the fusions' attention (include/lmkd.h LMKD_MHA_SEQ_MAX_L)


def mfm_attn_family(L):
    """-> (infix of the lmkd_mha_<infix>* entry points, padded token count of their P) for sequences of L tokens: up to 8 tokens the
    kernels that hold the score block in registers, from 9 to MFM_MAX_L the 16-token family"""
    if L > MFM_MAX_L:
        raise RuntimeError("the MFM attention takes sequences of at most MFM_MAX_L = %d tokens, not %d" % (MFM_MAX_L, L))
    return ("small", 8) if L <= 8 else ("seq", 16)


class MfmAttnFn(torch.autograd.Function):
    """self-attention over L <= MFM_MAX_L tokens per (sequence, head): qkv [B*L, 3D] -> [B*L, D]; mask [B*H, L, L] (or None) is the
    dropout on the probabilities.  Saved for the backward: qkv, the probabilities before dropout ([B*H, 8, 8] up to 8 tokens,
    [B*H, 16, 16] beyond), the mask."""

    @staticmethod
    def forward(ctx, qkv, mask, L, H):
        qkv = qkv.contiguous()
        _chk(qkv, mask)
        M, D3 = qkv.shape
        D = D3 // 3
        if D3 != 3 * D or M % L:
            raise RuntimeError("MfmAttnFn: qkv %s for sequences of %d tokens" % (tuple(qkv.shape), L))
        B = M // L
        if mask is not None and mask.shape != (B * H, L, L):
            raise RuntimeError("MfmAttnFn: mask %s, expected %s" % (tuple(mask.shape), (B * H, L, L)))
        family, pad = mfm_attn_family(L)
        out, P = _empty((M, D), qkv), _empty((B * H, pad, pad), qkv)
        lib().call("lmkd_mha_%s_train_fwd" % family, _p(qkv), _p(mask), _p(out), _p(P), B, L, D, H, _stream())
        ctx.save_for_backward(qkv, P, mask)
        ctx.dims = (B, L, D, H)
        ctx.family = family
        return out

    @staticmethod
    def backward(ctx, dO):
        _audit.engine_owned(dO)
        qkv, P, mask = ctx.saved_tensors
        dO = dO.contiguous()
        B, L, D, H = ctx.dims
        dqkv = torch.empty_like(qkv)
        lib().call("lmkd_mha_%s_bwd" % ctx.family, _p(qkv), _p(P), _p(mask), _p(dO), _p(dqkv), B, L, D, H, _stream())
        return dqkv, None, None, None


MFM_LAYER_SITES = ("attn", "dropout1", "dropout", "dropout2")
# The fusions' Linear layers sum 2048 - 18432 terms per output; they are summed in blocks of this many (gemm's k_block), which keeps the
# rounding of the whole teacher's gradients at the level of a blocked CPU GEMM.  At widths up to it nothing changes.
MFM_K_BLOCK = 128


def mfm_encoder_layer_train(x, layer, L, nhead, masks=None):
    """one nn.TransformerEncoderLayer (defaults: post-norm, ReLU, eps 1e-5, batch_first) with autograd.  x [B*L, D]; masks: None (no
    dropout) or a dict over MFM_LAYER_SITES - "attn" [B*H, L, L] on the attention probabilities, "dropout1" [B*L, D] on the out_proj
    output, "dropout" [B*L, dim_feedforward] after the ReLU, "dropout2" [B*L, D] on the linear2 output; a missing site has none."""
    m = masks or {}
    at = layer.self_attn
    kb = MFM_K_BLOCK
    qkv = LinearFn.apply(x, at.in_proj_weight, at.in_proj_bias, kb)
    a = MfmAttnFn.apply(qkv, m.get("attn"), L, nhead)
    o = feature_dropout(LinearFn.apply(a, at.out_proj.weight, at.out_proj.bias, kb), m.get("dropout1"))
    x = MfmLayerNormFn.apply(x, o, layer.norm1.weight, layer.norm1.bias)
    h = feature_dropout(LinearXFn.apply(x, layer.linear1.weight, layer.linear1.bias, True, None, 0, kb), m.get("dropout"))
    f = feature_dropout(LinearFn.apply(h, layer.linear2.weight, layer.linear2.bias, kb), m.get("dropout2"))
    return MfmLayerNormFn.apply(x, f, layer.norm2.weight, layer.norm2.bias)
