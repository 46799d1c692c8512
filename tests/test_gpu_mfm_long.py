"""GPU: the MFM fusion for clips of 9 - 16 frames.  Kernel level: the 16-token attention family of csrc/mfm.hip
(lmkd_mha_seq, lmkd_mha_seq_train_fwd, lmkd_mha_seq_bwd), forward and backward, against fp64 torch by the project's anchored criterion
(HIP vs fp64 at most 3 x torch-CPU-fp32 vs fp64 + 2e-6), on NaN-filled outputs and twice for bit-identity; ops.MfmAttnFn's choice between
the two families; `_Fusion.forward` with every gradient, and `extract_feature`, against the module's own nn containers on the CPU and
against the restatement tests/_mfm_train_ref.py with explicit masks; the fused feature of ThreeTRXShiftLoopTime at 12 frames; and the chain
train_teacher -> extract --stage fusion at --seq_len 12 on the 2048-wide teacher."""
import argparse
import copy
import functools
import math
import os

import numpy as np
import pytest
import torch

import _anchor
import _mfm_train_ref as R
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
CPU_FP32_LIMIT = 1e-5      # the regime in which the anchored criterion discriminates: torch-CPU fp32's own deviation from fp64
PAD = 16                   # the family's P is [B*H, 16, 16]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    return torch.device("cuda", 0)


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _record(tag, pairs):
    for k, (eh, ec) in pairs.items():
        print("%s %-40s HIP vs fp64 %.3e | CPU fp32 vs fp64 %.3e" % (tag, k, eh, ec))
    _anchor.record(tag, pairs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the attention kernels
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, L, D, H): the first token beyond the 8-token family, an odd length with three heads and a head dimension that is no multiple of the
# 256 lanes, a last wave without rows (L = 12) at head dimension 320, the full block, the real width (head dimension 2048: 8 steps of a
# wave, 2 of a workgroup), and a head dimension of 50 - no multiple of 4, which takes the instances without 16-byte accesses, their last group of 4 cut
# short; then the lengths the other family serves too, down to the one-token softmax
LONG_SHAPES = [(3, 9, 128, 2), (3, 13, 192, 3), (2, 12, 960, 3), (2, 16, 128, 2), (2, 16, 6144, 3), (2, 11, 150, 3)]
SHORT_SHAPES = [(2, 8, 128, 2), (2, 5, 960, 3), (2, 1, 128, 2)]


@functools.lru_cache(maxsize=None)
def _attn_case(B, L, D, H, masked):
    g = torch.Generator().manual_seed(1000 + B + 10 * L + D + 7 * H)
    qkv, dO = torch.randn(B * L, 3 * D, generator=g), torch.randn(B * L, D, generator=g)
    mask = (torch.rand(B * H, L, L, generator=g) >= R.P_DROP).float() / (1 - R.P_DROP) if masked else None
    refs = []
    for dt in (torch.float32, torch.float64):
        x = qkv.detach().to(dt).clone().requires_grad_()
        hd = D // H
        q, k, v = (t.reshape(B, L, H, hd).transpose(1, 2) for t in x.chunk(3, dim=-1))
        P = torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(hd), dim=-1)
        PM = P if mask is None else P * mask.reshape(B, H, L, L).to(dt)
        out = (PM @ v).transpose(1, 2).reshape(B * L, D)
        out.backward(dO.to(dt))
        Pp = torch.zeros(B * H, PAD, PAD, dtype=dt)
        Pp[:, :L, :L] = P.detach().reshape(B * H, L, L)
        refs.append({"out": out.detach(), "P": Pp, "dqkv": x.grad})
    return qkv, dO, mask, refs[0], refs[1]


def _attn_hip(dev, qkv, dO, mask, B, L, D, H, family="seq"):
    import litemkd_amd
    from litemkd_amd import ops
    lib, p, st = litemkd_amd.lib(), ops._p, ops._stream()
    pad = PAD if family == "seq" else 8
    q, g = qkv.to(dev), dO.to(dev)
    m = None if mask is None else mask.to(dev)
    out, P, dqkv = _nan(dev, B * L, D), _nan(dev, B * H, pad, pad), _nan(dev, B * L, 3 * D)
    lib.call("lmkd_mha_%s_train_fwd" % family, p(q), p(m), p(out), p(P), B, L, D, H, st)
    lib.call("lmkd_mha_%s_bwd" % family, p(q), p(P), p(m), p(g), p(dqkv), B, L, D, H, st)
    torch.cuda.synchronize()
    return {"out": out.cpu(), "P": P.cpu(), "dqkv": dqkv.cpu()}


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", LONG_SHAPES + SHORT_SHAPES, ids=lambda s: "B%dL%dD%dH%d" % s)
def test_attention_kernels_are_anchored_to_fp64(dev, shape, masked):
    B, L, D, H = shape
    qkv, dO, mask, r32, r64 = _attn_case(B, L, D, H, masked)
    a = _attn_hip(dev, qkv, dO, mask, B, L, D, H)
    b = _attn_hip(dev, qkv, dO, mask, B, L, D, H)
    for k in a:
        assert bool(torch.isfinite(a[k]).all()), "%s: an element was not written" % k
        assert torch.equal(a[k], b[k]), "%s differs between two calls" % k
    beyond = torch.ones(PAD, PAD, dtype=torch.bool)
    beyond[:L, :L] = False
    assert int(beyond.sum()) == PAD * PAD - L * L and float(a["P"][:, beyond].abs().sum()) == 0.0, "P is not zero beyond L"
    pairs = {}
    split = lambda t: dict(zip(("dq", "dk", "dv"), t.chunk(3, dim=-1)))      # noqa: E731
    got, c32, c64 = ({"out": r["out"], "P": r["P"], **split(r["dqkv"])} for r in (a, r32, r64))
    for k in got:
        if L == 1 and k in ("dq", "dk"):      # a one-token softmax is the constant 1: dS = 0 exactly
            assert float(c64[k].abs().max()) == 0.0 and float(got[k].abs().max()) == 0.0, k
            continue
        assert float(c64[k].norm()) > 0.0, k
        pairs[k] = (_anchor.rel_l2(got[k], c64[k]), _anchor.rel_l2(c32[k], c64[k]))
    _record("mfm seq attn B%d L%d D%d H%d %s" % (B, L, D, H, "mask" if masked else "nomask"), pairs)
    for k in pairs:
        _anchor.anchored(k, got[k], c32[k], c64[k])
    if not masked:      # the inference entry point computes the same forward, to the bit
        import litemkd_amd
        from litemkd_amd import ops
        o = _nan(dev, B * L, D)
        litemkd_amd.lib().call("lmkd_mha_seq", ops._p(qkv.to(dev)), ops._p(o), B, L, D, H, ops._stream())
        assert torch.equal(o.cpu(), a["out"])


def test_buffers_off_a_16_byte_boundary_give_the_same_bits(dev):
    """the entry points take their 16-byte instances only where every buffer is aligned; 4 bytes off they take the scalar ones, which
    state the same sums in the same order"""
    import litemkd_amd
    from litemkd_amd import ops
    lib, p, st = litemkd_amd.lib(), ops._p, ops._stream()
    B, L, D, H = 2, 12, 960, 3
    qkv, dO, mask, _, _ = _attn_case(B, L, D, H, True)
    want = _attn_hip(dev, qkv, dO, mask, B, L, D, H)

    def off(t):      # the same values, 4 bytes past a 16-byte boundary
        buf = torch.full((t.numel() + 1,), float("nan"), device=dev)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    q, g, m = off(qkv), off(dO), mask.to(dev)
    out, P, dqkv, o2 = off(torch.zeros(B * L, D)), _nan(dev, B * H, PAD, PAD), off(torch.zeros(B * L, 3 * D)), off(torch.zeros(B * L, D))
    lib.call("lmkd_mha_seq_train_fwd", p(q), p(m), p(out), p(P), B, L, D, H, st)
    lib.call("lmkd_mha_seq_bwd", p(q), p(P), p(m), p(g), p(dqkv), B, L, D, H, st)
    lib.call("lmkd_mha_seq", p(q), p(o2), B, L, D, H, st)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want["out"]) and torch.equal(P.cpu(), want["P"]) and torch.equal(dqkv.cpu(), want["dqkv"])
    assert bool(torch.isfinite(o2).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the dispatch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(8, "small"), (12, "seq")], ids=lambda c: "L%d_%s" % c)
def test_autograd_function_calls_the_family_of_its_length(dev, case):
    from litemkd_amd import ops
    L, family = case
    B, D, H = 3, 192, 3
    qkv, dO, mask, _, _ = _attn_case(B, L, D, H, True)
    direct = _attn_hip(dev, qkv, dO, mask, B, L, D, H, family)
    x = qkv.to(dev).requires_grad_()
    out = ops.MfmAttnFn.apply(x, mask.to(dev), L, H)
    out.backward(dO.to(dev))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(direct["dqkv"]).all())
    assert torch.equal(out.detach().cpu(), direct["out"]) and torch.equal(x.grad.cpu(), direct["dqkv"])


def test_autograd_function_refuses_17_tokens(dev):
    from litemkd_amd import ops
    with pytest.raises(RuntimeError, match="16"):
        ops.MfmAttnFn.apply(torch.zeros(2 * 17, 3 * 128, device=dev), None, 17, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. the fusions
# ---------------------------------------------------------------------------------------------------------------------------------
FUSION_CONFIGS = [(2, 64, 12), (3, 64, 16), (3, 320, 9), (2, 320, 16)]      # (modalities, in_channels, seq_len); trans_num 2, 3 videos
MASKED_CONFIGS = [(3, 64, 13), (2, 320, 16)]
EXTRACT_CONFIGS = [(3, 64, 12), (2, 320, 16)]
N_VID, N_LAYERS = 3, 2


@functools.lru_cache(maxsize=None)
def _fusion_case(n_mod, d, L):
    seed = 300 + 10 * n_mod + d + L
    return R.make_fusion(n_mod, d, L, N_LAYERS, seed), tuple(R.fusion_inputs(seed + 1, n_mod, N_VID, L, d)), R.weights(seed + 2, (N_VID, L, d))


@functools.lru_cache(maxsize=None)
def _fusion_ref(n_mod, d, L, mask_seed=None):
    """(fp32, fp64) on the CPU, computed once: torch's nn containers with dropout off, the restatement with explicit masks"""
    mod, xs, w = _fusion_case(n_mod, d, L)
    fn = R.nn_fusion if mask_seed is None else R.restated(R.make_masks(mod, N_VID, L, mask_seed))
    return R.fusion_grads(fn, mod, xs, w, torch.float32), R.fusion_grads(fn, mod, xs, w, torch.float64)


def _fusion_hip(dev, mod, xs, w, masks=None, train=False):
    m = copy.deepcopy(mod).to(dev).train(train)
    xd = [x.to(dev).requires_grad_() for x in xs]
    y = m(*xd, masks=None if masks is None else {k: v.to(dev) for k, v in masks.items()})
    (y * w.to(dev)).sum().backward()
    torch.cuda.synchronize()
    out = {"out": y.detach().cpu()}
    out.update({"g_in%d" % i: x.grad.cpu() for i, x in enumerate(xd)})
    out.update({"g_" + k: v.grad.cpu() for k, v in m.named_parameters()})
    return out


def _check_fusion(tag, got, r32, r64):
    """tests/test_gpu_mfm_train.py's check: the output by _anchor.anchored, every gradient by _anchor.anchored_dict's rule (factor 3, floor
    2e-6, near-zero gradients on 1e-7 of the largest), in the regime where torch's CPU fp32 is within CPU_FP32_LIMIT of fp64.

    That regime depends on the host whose CPU computes the fp32 reference, not on the input alone: on (2, 320, 16) with masks one host's
    fp32 GEMM leaves every gradient 4e-7 - 6e-7 from fp64, another's flips one ReLU of layer 1's linear1 (a pre-activation within
    rounding of zero) and is 3e-4 - 1.3e-3 away on most of the 35 tensors, while the HIP result is the same 2e-7 - 4e-7 on both.  A
    reference that far off anchors nothing, so where it is beyond the limit the limit itself stands in for it: the HIP error must stay
    within 3 x CPU_FP32_LIMIT + 2e-6, the most the criterion allows anywhere inside its regime."""
    assert set(got) == set(r64)
    pairs = {k: (_anchor.rel_l2(got[k], r64[k]), _anchor.rel_l2(r32[k], r64[k])) for k in r64}
    _record(tag, pairs)
    grads = [k for k in r64 if k != "out"]
    for k in r64:
        assert bool(torch.isfinite(got[k]).all()) and got[k].shape == r64[k].shape, k
        assert float(r64[k].norm()) > 0.0, "%s: the fp64 reference is zero" % k
    beyond = sorted(k for k in r64 if not pairs[k][1] < CPU_FP32_LIMIT)
    if beyond:
        print("%s: torch-CPU fp32 is beyond %.0e of fp64 on this host for %d tensors (worst %.2e): held to the limit instead"
              % (tag, CPU_FP32_LIMIT, len(beyond), max(pairs[k][1] for k in beyond)))
    gmax = max(float(r64[k].abs().max()) for k in grads)
    worst = (0.0, "", 0.0, 0.0)
    for k in r64:
        zero = 0.0 if k == "out" else 1e-7 * gmax      # anchored_dict's zero_scale
        if k in beyond:
            e_hip, e_cpu = _anchor.anchored(k, got[k], r32[k], r64[k], factor=0.0, floor=3.0 * CPU_FP32_LIMIT + 2e-6, abs_floor=zero)
        else:
            e_hip, e_cpu = _anchor.anchored(k, got[k], r32[k], r64[k], abs_floor=zero)
        ratio = e_hip / (min(e_cpu, CPU_FP32_LIMIT) + 2e-6 / 3.0)
        if k != "out" and ratio > worst[0]:
            worst = (ratio, k, e_hip, e_cpu)
    print("%s worst ratio %.2f at %s (hip %.3e cpu %.3e)" % ((tag,) + worst))


@pytest.mark.parametrize("cfg", FUSION_CONFIGS, ids=lambda c: "mod%d_d%d_L%d" % c)
def test_fusion_without_dropout_matches_the_nn_containers(dev, cfg):
    mod, xs, w = _fusion_case(*cfg)
    r32, r64 = _fusion_ref(*cfg)
    _check_fusion("mfm long fusion mod %d d %d L %d eval" % cfg, _fusion_hip(dev, mod, xs, w), r32, r64)


@pytest.mark.parametrize("cfg", MASKED_CONFIGS, ids=lambda c: "mod%d_d%d_L%d" % c)
def test_fusion_with_explicit_masks_matches_the_restatement(dev, cfg):
    mod, xs, w = _fusion_case(*cfg)
    masks = R.make_masks(mod, N_VID, cfg[2], 17)
    r32, r64 = _fusion_ref(*cfg, mask_seed=17)
    assert float((r64["out"] - _fusion_ref(*cfg)[1]["out"]).abs().max()) > 1e-2      # the masks do something
    _check_fusion("mfm long fusion mod %d d %d L %d masks" % cfg, _fusion_hip(dev, mod, xs, w, masks, train=True), r32, r64)


@pytest.mark.parametrize("cfg", EXTRACT_CONFIGS, ids=lambda c: "mod%d_d%d_L%d" % c)
def test_inference_path_matches_the_training_path_and_fp64(dev, cfg):
    """extract_feature (the inference Linear arithmetic, lmkd_mha_seq) against the eval-mode forward (1e-5 relative L2: the existing
    criterion for the two Linear arithmetics) and anchored to the fp64 containers"""
    mod, xs, w = _fusion_case(*cfg)
    r32, r64 = _fusion_ref(*cfg)
    m = copy.deepcopy(mod).to(dev)
    got = m.extract_feature(*[x.to(dev) for x in xs]).cpu()
    ev = _fusion_hip(dev, mod, xs, w)["out"]
    assert bool(torch.isfinite(got).all()) and got.shape == r64["out"].shape
    near = _anchor.rel_l2(got, ev.double())
    pair = (_anchor.rel_l2(got, r64["out"]), _anchor.rel_l2(r32["out"], r64["out"]))
    print("extract_feature mod %d d %d L %d: %.3e from the eval-mode forward" % (cfg + (near,)))
    _record("mfm long extract_feature mod %d d %d L %d" % cfg, {"out": pair})
    assert near < 1e-5
    _anchor.anchored("out", got, r32["out"], r64["out"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the fused feature
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shirt", [1, 5])
def test_fused_feature_at_12_frames(dev, shirt):
    """ThreeTRXShiftLoopTime at seq_len 12, width 64, against the restatement in fp32 and fp64.  The training forward's fused feature
    (R.fused_feature: the second modality rolled by shirt_num for its fusion with the first, the third not) is compared with the three
    fusion calls ThreeTRXShiftLoopTime.forward makes; extract_feature rolls depth AND flow (model.py:1648-1664), so it is compared with
    the same three R.fusion terms under that roll."""
    from litemkd_amd.teacher.mfm import ThreeTRXShiftLoopTime
    L, d, n, layers = 12, 64, 3, 2
    args = argparse.Namespace(seq_len=L, trans_num=layers, shirt_num=shirt, m1="rgb", m2="depth", m3="flow")
    model = ThreeTRXShiftLoopTime(args, in_channels=d, head=False)
    p32 = O.make_mfm_params(500 + shirt, d=d, seq_len=L, num_layers=layers)
    model.load_state_dict(p32, strict=True)
    model = model.to(dev).eval()
    rgb, depth, flow = O.make_mfm_inputs(600 + shirt, n, d=d, seq_len=L)
    roll = lambda t: torch.cat((t[:, shirt:], t[:, :shirt]), dim=1)      # noqa: E731

    def refs(fn):
        out = []
        with torch.no_grad():
            for dt in (torch.float32, torch.float64):
                out.append(fn(*(t.to(dt) for t in (rgb, depth, flow)), {k: v.to(dt) for k, v in p32.items()}))
        return out

    def extract_ref(r, dp, fl, p):
        return (R.fusion((r, dp, fl), p, "three_fusion", layers) + R.fusion((r, roll(dp)), p, "fusion", layers)
                + R.fusion((r, roll(fl)), p, "fusion", layers))
    t32, t64 = refs(lambda r, dp, fl, p: R.fused_feature(r, dp, fl, p, shirt, layers))
    e32, e64 = refs(extract_ref)
    assert float((t64 - e64).abs().max()) > 1e-2      # the two rolls differ, so each comparison can tell them apart
    x = [t.to(dev) for t in (rgb, depth, flow)]
    with torch.no_grad():
        train_path = (model.three_fusion(*x) + model.fusion(x[0], roll(x[1]).contiguous()) + model.fusion(x[0], x[2])).cpu()
    got = model.extract_feature({"rgb": x[0], "depth": x[1], "flow": x[2]}).cpu()
    assert tuple(got.shape) == (n, L, d) and bool(torch.isfinite(got).all())
    pairs = {"forward": (_anchor.rel_l2(train_path, t64), _anchor.rel_l2(t32, t64)), "extract": (_anchor.rel_l2(got, e64), _anchor.rel_l2(e32, e64))}
    _record("mfm long fused feature L 12 shirt %d" % shirt, pairs)
    assert all(v[1] < CPU_FP32_LIMIT for v in pairs.values())
    _anchor.anchored("forward", train_path, t32, t64)
    _anchor.anchored("extract", got, e32, e64)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the chain at --seq_len 12
# ---------------------------------------------------------------------------------------------------------------------------------
TRAIN_FLAGS = ("--way 3 --shot 1 --query_per_class 1 --trans_num 1 --training_iterations 4 --tasks_per_batch 2 --trans_dropout 0.0 --opt adam "
               "-lr 0.0001 --print_freq 1 --save_freq 2 --seed 11").split()      # tests/test_gpu_mfm_train.py's


@pytest.fixture(scope="module")
def chain(dev, tmp_path_factory):
    """a tree of 4 classes x 2 videos of 12-frame features -> train_teacher.main (the 2048-wide teacher, trans_num 1, 4 iterations, optimizer
    steps after iterations 1 and 3, checkpoint 2 after iteration 1) -> extract --stage fusion from checkpoint_final.pt"""
    from litemkd_amd import extract as E
    from litemkd_amd import train_teacher as TT
    root = tmp_path_factory.mktemp("mfm_long_chain")
    feats, ck, fused = str(root / "feats"), str(root / "ck"), str(root / "fused")
    R.write_feature_tree(feats, classes=4, videos=2, seq_len=12, proto_scale=0.0)
    losses, accs, model, opt = TT.main(TRAIN_FLAGS + ["--seq_len", "12", "--feature_save_path", feats, "--checkpoint_dir", ck])
    torch.cuda.synchronize()
    steps = opt.steps
    del opt
    rec = E.main(["--stage", "fusion", "--seq_len", "12", "--feature_save_path", feats, "--out", fused,
                  "--checkpoint_dir", os.path.join(ck, "checkpoint_final.pt")])
    yield dict(feats=feats, ck=ck, fused=fused, losses=losses, steps=steps, model=model.eval(), rec=rec)
    del model
    torch.cuda.empty_cache()


def test_chain_trains_at_12_frames(dev, chain):
    print("losses", chain["losses"])
    assert len(chain["losses"]) == 4 and all(math.isfinite(v) for v in chain["losses"]) and chain["steps"] == 2
    first = torch.load(os.path.join(chain["ck"], "checkpoint2.pt"), map_location="cpu")      # after the first optimizer step
    final = torch.load(os.path.join(chain["ck"], "checkpoint_final.pt"), map_location="cpu")      # after the second
    assert first["iteration"] == 2 and sorted(final) == sorted(first["model_state_dict"])
    moved = [k for k in final if not torch.equal(final[k], first["model_state_dict"][k])]
    assert any(k.startswith("three_fusion.") for k in moved) and any(k.startswith("fusion.") for k in moved), moved
    assert tuple(final["three_fusion.positionEncoding1.position_embeddings.weight"].shape) == (12, 2048)
    assert all(bool(torch.isfinite(v).all()) for v in final.values())
    # the checkpoint loads into a default-constructed module of that length
    from litemkd_amd.teacher.mfm import ThreeTRXShiftLoopTime
    with torch.device(dev):
        plain = ThreeTRXShiftLoopTime(argparse.Namespace(seq_len=12, trans_num=1, shirt_num=1))
    plain.load_state_dict({k: v for k, v in final.items() if not k.startswith("bracnch.")}, strict=True)


def test_chain_writes_the_models_fused_features(dev, chain):
    assert (chain["rec"]["written"], chain["rec"]["skipped"]) == (8, 0)
    model = chain["model"]
    seen = 0
    for c in range(4):
        for v in range(2):
            rel = os.path.join("c%d" % c, "v%d_%d" % (c, v), "feature.npy")
            f = np.load(os.path.join(chain["fused"], rel))
            assert f.dtype == np.float32 and f.shape == (12, 2048) and np.isfinite(f).all()
            x = {m: torch.from_numpy(np.load(os.path.join(chain["feats"], m, rel))).unsqueeze(0).to(dev) for m in ("rgb", "depth", "flow")}
            want = model.extract_feature(x).reshape(12, 2048).cpu().numpy()
            assert np.array_equal(f, want), rel
            seen += 1
    assert seen == 8
