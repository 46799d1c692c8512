"""CPU oracle for the Lite-MKD per-episode hot path.  TEST INFRASTRUCTURE ONLY.

This file is a plain PyTorch-CPU fp32 restatement of the reference algorithm.  It
is the *checker*: only ``tests/``, ``__graft_entry__.smoke()`` and the
``cpu_baseline`` leg of ``bench.py`` may import it.  The product path
(``lite-mkd_amd/``) never imports anything from ``oracle/`` and fails loudly when
the HIP extension is missing.

Parity pins (see oracle/gen_golden.py, tests/golden/):
  * distillers / e_dist / SupportDK / TRX_2fcsup(+_fixed) / aggregate_accuracy are
    pinned against outputs of the reference's own modules imported in the build
    container (fixtures committed under tests/golden/).
  * The ResNet-18 trunk arithmetic lives in torchvision==0.14.0 (pinned in the
    reference's envirment.yml:128), which is absent from /root/reference and from
    this image: the trunk restatement below follows the published ResNet-18
    definition and is anchored on the reference call sites
    (model/backbone/resnet18_2fc.py:30-33,41-42), the parameter count 11 176 512 and
    the state-dict key names.  The reference holds no tests or golden vectors for it:
    TRUNK PARITY UNPINNED BY THE REFERENCE.
  * The MFM fusion (teacher/code/model.py:1135-1151,1300-1331,1361-1392,1648-1664) is
    pinned against the reference's own ThreeTRXShiftLoopTime.extract_feature at its
    fixed width 2048 (imported in the build container with test-only stubs for the
    dead imports `turtle`, `timm`, `torchvision.models`; weights from
    make_mfm_params(seed); outputs in tests/golden/mfm.npz).

All citations are file:line under /root/reference.
"""
import math
from itertools import combinations

import torch
import torch.nn.functional as F

# ----------------------------------------------------------------------------
# A2  ResNet-18 trunk  (torchvision resnet18().children()[:-2],
#     model/backbone/resnet18_2fc.py:30-33, called at :41-42)
# ----------------------------------------------------------------------------
# (stage index in nn.Sequential, in_ch, out_ch, first-block stride)
RESNET18_STAGES = [(4, 64, 64, 1), (5, 64, 128, 2), (6, 128, 256, 2), (7, 256, 512, 2)]
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def resnet18_trunk_param_shapes():
    """state_dict-style key -> shape for nn.Sequential(*children()[:-2])."""
    shapes = {"0.weight": (64, 3, 7, 7)}

    def bn(prefix, c):
        shapes[prefix + ".weight"] = (c,)
        shapes[prefix + ".bias"] = (c,)
        shapes[prefix + ".running_mean"] = (c,)
        shapes[prefix + ".running_var"] = (c,)
        shapes[prefix + ".num_batches_tracked"] = ()

    bn("1", 64)
    for idx, cin, cout, stride in RESNET18_STAGES:
        for b in range(2):
            p = "%d.%d" % (idx, b)
            shapes[p + ".conv1.weight"] = (cout, cin if b == 0 else cout, 3, 3)
            bn(p + ".bn1", cout)
            shapes[p + ".conv2.weight"] = (cout, cout, 3, 3)
            bn(p + ".bn2", cout)
            if b == 0 and (stride != 1 or cin != cout):
                shapes[p + ".downsample.0.weight"] = (cout, cin, 1, 1)
                bn(p + ".downsample.1", cout)
    return shapes


def init_resnet18_trunk(gen):
    """Seeded random init (no pretrained weights offline): Kaiming-normal fan_out
    convs, BN gamma=1 beta=0 — torchvision's ResNet.__init__ scheme."""
    sd = {}
    for k, shp in resnet18_trunk_param_shapes().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.long)
        elif k.endswith("running_mean"):
            sd[k] = torch.zeros(shp)
        elif k.endswith("running_var"):
            sd[k] = torch.ones(shp)
        elif len(shp) == 4:
            fan_out = shp[0] * shp[2] * shp[3]
            sd[k] = torch.randn(shp, generator=gen) * math.sqrt(2.0 / fan_out)
        elif k.endswith(".weight"):
            sd[k] = torch.ones(shp)
        else:
            sd[k] = torch.zeros(shp)
    return sd


def _bn(x, sd, prefix, training, update_running=True):
    rm, rv = sd[prefix + ".running_mean"], sd[prefix + ".running_var"]
    if training and not update_running:
        rm, rv = rm.clone(), rv.clone()
    return F.batch_norm(x, rm, rv, sd[prefix + ".weight"], sd[prefix + ".bias"],
                        training, BN_MOMENTUM, BN_EPS)


# Test hook: when set, every ReLU of the trunks calls RELU_HOOK(pre_activation) instead of F.relu, in execution order (stem,
# then relu1 / relu2 of each BasicBlock, relu1 / relu2 / relu3 of each Bottleneck; support call first, then query call).  The parity tests use it to impose the ReLU masks of
# the implementation under test on the fp32 and fp64 oracle runs: two fp32 evaluations of a ReLU network legitimately differ
# where a pre-activation lies within rounding of zero, and with the masks fixed the backward is a linear map that must agree to
# fp32 rounding.
RELU_HOOK = None


def _relu(t):
    return F.relu(t) if RELU_HOOK is None else RELU_HOOK(t)


# The same for the two arg-max selections of the path: POOL_HOOK(site, t) with site "stem" (the 3x3 / 2 max pool after the stem,
# t = its input) or "head" (AdaptiveMaxPool2d((4, 4)), t = the trunk's output map) replaces the pooling call, in execution order
# (support call first, then query).  ONE arg-max resolved differently - two candidates within rounding of each other - moves a
# gradient value to another pixel and with it every upstream parameter gradient by ~1e-3 of its norm, in either fp32 evaluation;
# with the selections of the implementation under test imposed (and checked to differ from fp64's only at such near-ties) the whole
# backward is a linear map.
POOL_HOOK = None


def _maxpool_stem(t):
    return F.max_pool2d(t, 3, 2, 1) if POOL_HOOK is None else POOL_HOOK("stem", t)


# BASELINE configs[2] ("bf16, MFMA conv path"): the reference runs its convolutions under autocast; the build's bf16 mode rounds
# the operands of EVERY convolution GEMM to bf16 (round to nearest even) and accumulates in fp32 - forward: conv(r(x), r(w));
# data gradient: from r(dy) and r(w); weight gradient: from r(x) and r(dy) - while activations, BatchNorm and the loss stay
# fp32.  CONV_BF16 = True makes the trunks below compute exactly that arithmetic on the CPU (in the dtype of the inputs: run it
# in fp64 for an accumulation-exact reference of the bf16 mode).
CONV_BF16 = False


def _r16(t):
    return t.detach().to(torch.bfloat16).to(t.dtype)


class _ConvBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, pad):
        ctx.save_for_backward(x, w)
        ctx.sp = (stride, pad)
        return F.conv2d(_r16(x), _r16(w), None, stride, pad)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pad = ctx.sp
        dyr = _r16(dy)
        dx = torch.nn.grad.conv2d_input(x.shape, _r16(w), dyr, stride=stride, padding=pad) if ctx.needs_input_grad[0] else None
        dw = torch.nn.grad.conv2d_weight(_r16(x), w.shape, dyr, stride=stride, padding=pad) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None


def _conv(x, w, stride=1, pad=0):
    if CONV_BF16:
        return _ConvBF16.apply(x, w, stride, pad)
    return F.conv2d(x, w, None, stride, pad)


# configs[2] with bf16 TENSORS in HBM (lmkd_set_activation_dtype(1); the reference's autocast keeps its activations in reduced
# precision too): every activation the trunk stores - convolution outputs, BatchNorm+ReLU outputs, block outputs, the pooled stem
# output - and the gradient that flows back through the same place is rounded to bf16 (RNE); BatchNorm statistics are those of the
# stored (rounded) convolution output; arithmetic between two stored tensors is fp32.  ACT_BF16 = True inserts exactly these
# rounding points (forward and backward) into the trunk below; use together with CONV_BF16.
ACT_BF16 = False


class _RoundSTE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return _r16(t)

    @staticmethod
    def backward(ctx, g):
        return _r16(g)


def _act(t):
    return _RoundSTE.apply(t) if ACT_BF16 else t


def resnet18_trunk(x, sd, training=True, update_running=True, taps=None):
    """[F,3,H,W] -> [F,512,H/32,W/32].  BN in train mode uses the batch statistics of
    THIS call (reference: Student.__init__ calls self.train(), model_select.py:21)."""
    def tap(name, t):
        if taps is not None:
            taps[name] = t
    x = _act(_conv(x, sd["0.weight"], 2, 3))
    tap("conv1", x)
    x = _relu(_bn(x, sd, "1", training, update_running))
    x = _act(_maxpool_stem(x))
    tap("pool", x)
    for idx, cin, cout, stride in RESNET18_STAGES:
        for b in range(2):
            p = "%d.%d" % (idx, b)
            s = stride if b == 0 else 1
            idn = x
            out = _act(_conv(x, sd[p + ".conv1.weight"], s, 1))
            out = _act(_relu(_bn(out, sd, p + ".bn1", training, update_running)))
            out = _act(_conv(out, sd[p + ".conv2.weight"], 1, 1))
            out = _bn(out, sd, p + ".bn2", training, update_running)
            if (p + ".downsample.0.weight") in sd:
                idn = _act(_conv(x, sd[p + ".downsample.0.weight"], s, 0))
                idn = _bn(idn, sd, p + ".downsample.1", training, update_running)
            x = _act(_relu(out + idn))
            tap(p, x)
    return x


# ResNet-50 trunk (torchvision resnet50().children()[:-2], resnet50_2fc.py:29-32; v1.5: stride on conv2)
RESNET50_STAGES = [(4, 64, 3, 1), (5, 128, 4, 2), (6, 256, 6, 2), (7, 512, 3, 2)]


def resnet50_trunk_param_shapes():
    shapes = {"0.weight": (64, 3, 7, 7)}

    def bn(prefix, c):
        shapes[prefix + ".weight"] = (c,)
        shapes[prefix + ".bias"] = (c,)
        shapes[prefix + ".running_mean"] = (c,)
        shapes[prefix + ".running_var"] = (c,)
        shapes[prefix + ".num_batches_tracked"] = ()

    bn("1", 64)
    cin = 64
    for idx, width, n, stride in RESNET50_STAGES:
        for b in range(n):
            p = "%d.%d" % (idx, b)
            shapes[p + ".conv1.weight"] = (width, cin, 1, 1)
            bn(p + ".bn1", width)
            shapes[p + ".conv2.weight"] = (width, width, 3, 3)
            bn(p + ".bn2", width)
            shapes[p + ".conv3.weight"] = (width * 4, width, 1, 1)
            bn(p + ".bn3", width * 4)
            if b == 0:
                shapes[p + ".downsample.0.weight"] = (width * 4, cin, 1, 1)
                bn(p + ".downsample.1", width * 4)
            cin = width * 4
    return shapes


def init_trunk_from_shapes(shapes, gen):
    sd = {}
    for k, shp in shapes.items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.long)
        elif k.endswith("running_mean"):
            sd[k] = torch.zeros(shp)
        elif k.endswith("running_var"):
            sd[k] = torch.ones(shp)
        elif len(shp) == 4:
            sd[k] = torch.randn(shp, generator=gen) * math.sqrt(2.0 / (shp[0] * shp[2] * shp[3]))
        elif k.endswith(".weight"):
            sd[k] = torch.ones(shp)
        else:
            sd[k] = torch.zeros(shp)
    return sd


def resnet50_trunk(x, sd, training=True, update_running=True):
    x = F.conv2d(x, sd["0.weight"], None, 2, 3)
    x = _relu(_bn(x, sd, "1", training, update_running))
    x = _maxpool_stem(x)
    for idx, width, n, stride in RESNET50_STAGES:
        for b in range(n):
            p = "%d.%d" % (idx, b)
            s = stride if b == 0 else 1
            idn = x
            out = _relu(_bn(F.conv2d(x, sd[p + ".conv1.weight"]), sd, p + ".bn1", training, update_running))
            out = _relu(_bn(F.conv2d(out, sd[p + ".conv2.weight"], None, s, 1), sd, p + ".bn2", training, update_running))
            out = _bn(F.conv2d(out, sd[p + ".conv3.weight"]), sd, p + ".bn3", training, update_running)
            if (p + ".downsample.0.weight") in sd:
                idn = _bn(F.conv2d(x, sd[p + ".downsample.0.weight"], None, s, 0), sd, p + ".downsample.1", training, update_running)
            x = _relu(out + idn)
    return x


# ----------------------------------------------------------------------------
# A3  pooled head (model/backbone/resnet18_2fc.py:44-77, resnet18_student.py:41-60)
# ----------------------------------------------------------------------------
def pooled_frame_features(fmap):
    """AdaptiveMaxPool2d((4,4)) -> reshape [F,C,16] -> permute -> mean over the 16
    patches (resnet18_2fc.py:44-54)."""
    p = F.adaptive_max_pool2d(fmap, (4, 4)) if POOL_HOOK is None else POOL_HOOK("head", fmap)
    p = p.reshape(p.shape[0], p.shape[1], 16).permute(0, 2, 1)
    return p.mean(dim=1)


def backbone_resnet18_2fc(ctx_imgs, tgt_imgs, params, seq_len=8, training=True, update_running=True):
    """resnet18_2fc.forward (resnet18_2fc.py:37-77). params: 'resnet.<k>', 'fc1.*', 'fc2.*'."""
    sd = {k[len("resnet."):]: v for k, v in params.items() if k.startswith("resnet.")}
    return head_2fc(resnet18_trunk(ctx_imgs, sd, training, update_running), resnet18_trunk(tgt_imgs, sd, training, update_running),
                    params, seq_len)


def head_2fc(fm_ctx, fm_tgt, params, seq_len=8):
    """everything of resnet18_2fc.forward after the two trunk calls (resnet18_2fc.py:44-77): pooled frame features, fc1 / fc2,
    reshape to [videos, seq_len, 2048], the two dicts.  Pinned by tests/golden/head.npz, which the reference's own forward produced
    from trunk output maps (oracle/gen_golden.py gen_head)."""
    cf, tf = pooled_frame_features(fm_ctx), pooled_frame_features(fm_tgt)
    out_c, out_t = {}, {}
    for h in (1, 2):
        w, b = params["fc%d.weight" % h], params["fc%d.bias" % h]
        out_c["context_features_%d" % h] = F.linear(cf, w, b).reshape(-1, seq_len, 2048)
        out_t["target_features_%d" % h] = F.linear(tf, w, b).reshape(-1, seq_len, 2048)
    return out_c, out_t


def backbone_resnet50_2fc(ctx_imgs, tgt_imgs, params, seq_len=8, training=True, update_running=True):
    """resnet50_2fc.forward (resnet50_2fc.py:38-78): ResNet-50 trunk, pooled 2048-d frame features, two 2048->2048 heads."""
    sd = {k[len("resnet."):]: v for k, v in params.items() if k.startswith("resnet.")}
    cf = pooled_frame_features(resnet50_trunk(ctx_imgs, sd, training, update_running))
    tf = pooled_frame_features(resnet50_trunk(tgt_imgs, sd, training, update_running))
    out_c, out_t = {}, {}
    for h in (1, 2):
        w, b = params["fc%d.weight" % h], params["fc%d.bias" % h]
        out_c["context_features_%d" % h] = F.linear(cf, w, b).reshape(-1, seq_len, 2048)
        out_t["target_features_%d" % h] = F.linear(tf, w, b).reshape(-1, seq_len, 2048)
    return out_c, out_t


def backbone_resnet18_student(ctx_imgs, tgt_imgs, params, seq_len=8, training=True, update_running=True):
    """resnet18_student.forward (resnet18_student.py:36-60): single 512->2048 head."""
    sd = {k[len("resnet."):]: v for k, v in params.items() if k.startswith("resnet.")}
    cf = pooled_frame_features(resnet18_trunk(ctx_imgs, sd, training, update_running))
    tf = pooled_frame_features(resnet18_trunk(tgt_imgs, sd, training, update_running))
    w, b = params["res18_2048.weight"], params["res18_2048.bias"]
    return (F.linear(cf, w, b).reshape(-1, seq_len, 2048),
            F.linear(tf, w, b).reshape(-1, seq_len, 2048))


# ----------------------------------------------------------------------------
# A4  PositionalEncoding (model/classifiers/TRX_2fcsup.py:24-48)
# ----------------------------------------------------------------------------
def positional_encoding_table(d_model=2048, max_len=12, scale=0.1):
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2) * -(math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term) * scale
    pe[:, 1::2] = torch.cos(position * div_term) * scale
    return pe.unsqueeze(0)


# ----------------------------------------------------------------------------
# A5  TemporalCrossTransformer.forward (TRX_2fcsup.py:74-148); dropout off (p=0)
# ----------------------------------------------------------------------------
def frame_tuples(seq_len=8, card=2):
    return [list(c) for c in combinations(range(seq_len), card)]


def trx_logits(support, labels, queries, p, way=5, seq_len=8, out_dim=1152):
    """p: dict with k_linear.{weight,bias}, v_linear.{weight,bias}, norm_k.{weight,bias}, pe.pe"""
    n_q, n_s = queries.shape[0], support.shape[0]
    pe = p["pe.pe"][:, :seq_len]
    support = support + pe
    queries = queries + pe
    tuples = frame_tuples(seq_len, 2)
    s = torch.stack([support[:, t, :].reshape(n_s, -1) for t in tuples], dim=-2)
    q = torch.stack([queries[:, t, :].reshape(n_q, -1) for t in tuples], dim=-2)
    T = len(tuples)
    s_k = F.linear(s, p["k_linear.weight"], p["k_linear.bias"])
    q_k = F.linear(q, p["k_linear.weight"], p["k_linear.bias"])
    s_v = F.linear(s, p["v_linear.weight"], p["v_linear.bias"])
    q_v = F.linear(q, p["v_linear.weight"], p["v_linear.bias"])
    s_k = F.layer_norm(s_k, (out_dim,), p["norm_k.weight"], p["norm_k.bias"], 1e-5)
    q_k = F.layer_norm(q_k, (out_dim,), p["norm_k.weight"], p["norm_k.bias"], 1e-5)
    cols = []
    for c in torch.unique(labels):
        idx = torch.nonzero(labels == c).reshape(-1)
        ck, cv = s_k[idx], s_v[idx]
        sc = torch.matmul(q_k.unsqueeze(1), ck.transpose(-2, -1)) / math.sqrt(out_dim)
        sc = sc.permute(0, 2, 1, 3).reshape(n_q, T, -1)
        sc = torch.softmax(sc, dim=-1)          # Softmax(dim=1) of each per-query 2-D slice (:66,127)
        sc = sc.reshape(n_q, T, -1, T).permute(0, 2, 1, 3)
        proto = torch.matmul(sc, cv).sum(dim=1)
        diff = q_v - proto
        dist = -(diff.pow(2).sum(dim=(-2, -1))) / T   # norm(dim=[-2,-1])**2 / tuples_len (:139-143)
        cols.append((int(c.long()), dist))
    out = torch.stack([dict(cols).get(j, torch.zeros(n_q)) for j in range(way)], dim=1)
    return out


def trx_sup_logits(support, labels, queries, p, way=5, seq_len=8, out_dim=1152):
    """TemporalCrossTransformer.forward of TRX_sup.py:74-178 -> ('query' [Nq,way] logits, 'support_set' [Nq,way,way]):
    the TRX logits plus the cosine similarity (dim = 28*1152 prototype entries) between each query's class prototypes;
    classes without support keep a zero prototype."""
    n_q, n_s = queries.shape[0], support.shape[0]
    pe = p["pe.pe"][:, :seq_len]
    support = support + pe
    queries = queries + pe
    tuples = frame_tuples(seq_len, 2)
    s = torch.stack([support[:, t, :].reshape(n_s, -1) for t in tuples], dim=-2)
    q = torch.stack([queries[:, t, :].reshape(n_q, -1) for t in tuples], dim=-2)
    T = len(tuples)
    s_k = F.layer_norm(F.linear(s, p["k_linear.weight"], p["k_linear.bias"]), (out_dim,), p["norm_k.weight"], p["norm_k.bias"], 1e-5)
    q_k = F.layer_norm(F.linear(q, p["k_linear.weight"], p["k_linear.bias"]), (out_dim,), p["norm_k.weight"], p["norm_k.bias"], 1e-5)
    s_v = F.linear(s, p["v_linear.weight"], p["v_linear.bias"])
    q_v = F.linear(q, p["v_linear.weight"], p["v_linear.bias"])
    protos = [torch.zeros(n_q, T, out_dim) for _ in range(way)]
    logits = [torch.zeros(n_q) for _ in range(way)]
    for c in torch.unique(labels):
        idx = torch.nonzero(labels == c).reshape(-1)
        ck, cv = s_k[idx], s_v[idx]
        sc = torch.matmul(q_k.unsqueeze(1), ck.transpose(-2, -1)) / math.sqrt(out_dim)
        sc = torch.softmax(sc.permute(0, 2, 1, 3).reshape(n_q, T, -1), dim=-1)
        sc = sc.reshape(n_q, T, -1, T).permute(0, 2, 1, 3)
        proto = torch.matmul(sc, cv).sum(dim=1)
        protos[int(c.long())] = proto
        logits[int(c.long())] = -((q_v - proto).pow(2).sum(dim=(-2, -1))) / T
    allp = torch.stack(protos, dim=-1).reshape(n_q, -1, way)                       # :171
    sim = F.cosine_similarity(allp.unsqueeze(2), allp.unsqueeze(3), dim=1)         # :173
    return torch.stack(logits, dim=1), sim


# ----------------------------------------------------------------------------
# A6  SupportDK.forward (TRX_2fcsup.py:162-189 == e_dist_fc2.py:17-44)
# ----------------------------------------------------------------------------
def support_dk(support, way=5, shot=5, seq_len=8):
    proto = support.reshape(way, shot, seq_len, 2048).mean(dim=1)
    rows = []
    for i in range(way):
        rows.append(torch.stack([-(proto[i] - proto[n]).pow(2).sum() / seq_len
                                 for n in range(way) if n != i]))
    return torch.stack(rows)


# ----------------------------------------------------------------------------
# A9  e_dist.forward (e_dist_fc2.py:52-91)
# ----------------------------------------------------------------------------
def e_dist_logits(support, labels, queries, way=5):
    sup = support.reshape(-1, 8, 2048)
    q = queries.reshape(-1, 8, 2048).mean(dim=1)
    cols = {}
    for c in torch.unique(labels):
        idx = torch.nonzero(labels == c).reshape(-1)
        sc = sup[idx].mean(dim=1)
        cols[int(c.long())] = -torch.cdist(q, sc, p=2).mean(dim=1)
    return torch.stack([cols.get(j, torch.zeros(q.shape[0])) for j in range(way)], dim=1)


# A7/A8 + wrappers -----------------------------------------------------------
def clf_TRX_2fcsup(ctx, labels, tgt, p, way=5, shot=5):
    """TRX_2fcsup.forward (TRX_2fcsup.py:205-224)."""
    return {"kl": trx_logits(ctx["context_features_1"], labels, tgt["target_features_1"], p, way),
            "ce": trx_logits(ctx["context_features_2"], labels, tgt["target_features_2"], p, way),
            "sup": support_dk(ctx["context_features_2"], way, shot)}


def clf_TRX_2fcsup_fixed(ctx, labels, tgt, p, way=5, shot=5):
    """TRX_2fcsup_fixed.forward (TRX_2fcsup.py:241-256), no_grad."""
    with torch.no_grad():
        return {"kl": trx_logits(ctx, labels, tgt, p, way), "sup": support_dk(ctx, way, shot)}


def clf_e_dist_fc2_sup(ctx, labels, tgt, way=5, shot=5):
    """e_dist_fc2_sup.forward (e_dist_fc2.py:139-172)."""
    return {"kl": e_dist_logits(ctx["context_features_1"], labels, tgt["target_features_1"], way),
            "ce": e_dist_logits(ctx["context_features_2"], labels, tgt["target_features_2"], way),
            "sup": support_dk(ctx["context_features_2"], way, shot)}


def clf_e_dist_1fc_sup(ctx, labels, tgt, way=5, shot=5):
    """e_dist_1fc_sup / e_dist_fc2_sup_fixed .forward (e_dist_fc2.py:175-231)."""
    return {"kl": e_dist_logits(ctx, labels, tgt, way), "sup": support_dk(ctx, way, shot)}


# ----------------------------------------------------------------------------
# A11-A13  distillers.py:7-30, 42-74, 286-337
# ----------------------------------------------------------------------------
def kd_loss(s, t, T):
    lp = F.log_softmax(s / T, dim=1)
    pt = F.softmax(t / T, dim=1)
    return F.kl_div(lp, pt, reduction="none").sum(1).mean() * T ** 2


def cosine_similarity(x, y, eps=1e-8):
    return (x * y).sum(1) / (x.norm(dim=1) * y.norm(dim=1) + eps)


def pearson_correlation(x, y, eps=1e-8):
    return cosine_similarity(x - x.mean(1).unsqueeze(1), y - y.mean(1).unsqueeze(1), eps)


def inter_class_relation(y_s, y_t):
    return 1 - pearson_correlation(y_s.softmax(dim=1), y_t.softmax(dim=1)).mean()


DEFAULT_CFG = {"soft_loss_weight_support": 1, "soft_loss_weight_query": 1, "hard_loss_weight": 1,
               "soft_loss_weight": 2, "feature_loss_weight": 1, "temperature": 4,
               "fcwsl_aerfa": 0.5, "fcwsl_beta": 1}       # options.py:51-60


def distill_fc_2_sup_dist(s, t, labels, cfg=DEFAULT_CFG):
    """Distiller.fc_2_sup_dist (distillers.py:295-337)."""
    kl = kd_loss(s["kl"], t["kl"], cfg["temperature"])
    sup = inter_class_relation(s["sup"], t["sup"])
    ce = F.cross_entropy(s["ce"], labels) / 16
    return {"soft_loss": kl, "hard_loss": 0.5 * sup + ce, "loss": kl + 0.5 * sup + ce}


def distill_KD(s, t, labels, cfg=DEFAULT_CFG):
    """Distiller.KD (distillers.py:42-74)."""
    ce = cfg["hard_loss_weight"] * F.cross_entropy(s, labels) / 16
    kl = cfg["soft_loss_weight"] * kd_loss(s, t, cfg["temperature"])
    return {"hard_loss": ce, "soft_loss": kl, "loss": ce + kl}


def distill_Dist_KD(s, t, labels, cfg=DEFAULT_CFG):
    """Distiller.Dist_KD (distillers.py:286-293)."""
    ce = cfg["hard_loss_weight"] * F.cross_entropy(s, labels) / 16
    d = cfg["soft_loss_weight"] * inter_class_relation(s, t)
    return {"soft_loss": d, "hard_loss": ce, "loss": ce + d}


def _focal(ce_s, ce_t):
    """1 - exp(-max(ce_s/(ce_t+1e-8), 0)) on detached values (distillers.py:84-88 and siblings)"""
    fw = ce_s.detach() / (ce_t.detach() + 1e-8)
    return 1 - torch.exp(-torch.clamp(fw, min=0))


def _ce16(s, labels):
    return F.cross_entropy(s, labels) / 16


# the remaining Distiller methods (distillers.py:76-733) that are compositions of kd_loss / inter_class_relation / CE
def distill_method(name, s, t, labels, cfg=DEFAULT_CFG):
    T = cfg["temperature"]
    hw, sw = cfg["hard_loss_weight"], cfg["soft_loss_weight"]
    if name == "KD":
        return distill_KD(s, t, labels, cfg)["loss"]
    if name == "Dist_KD":
        return distill_Dist_KD(s, t, labels, cfg)["loss"]
    if name == "fc_2_sup_dist":
        return distill_fc_2_sup_dist(s, t, labels, cfg)["loss"]
    if name == "ce":                                                    # :100-108
        return _ce16(s, labels)
    if name == "support_sim":                                           # :110-124 (20 queries hard-coded)
        return (cfg["soft_loss_weight_support"] * kd_loss(s["support_set"].reshape(20, 25), t["support_set"].reshape(20, 25), T)
                + cfg["soft_loss_weight_query"] * kd_loss(s["query"], t["query"], T) + hw * _ce16(s["query"], labels))
    if name == "wsl":                                                   # :76-98
        fw = _focal(F.cross_entropy(s, labels), F.cross_entropy(t, labels))
        return sw * fw * kd_loss(s, t, T) + hw * _ce16(s, labels)
    if name == "fc_2":                                                  # :152-161
        return hw * _ce16(s["fc_1"], labels) + sw * kd_loss(s["fc_2"], t, T)
    if name == "fc_2_wsl":                                              # :163-201
        fw = _focal(F.cross_entropy(s["fc_1"], labels), F.cross_entropy(s["fc_2"], labels))
        return (1 + fw) * kd_loss(s["fc_2"], t, T) + (2 - fw) * _ce16(s["fc_1"], labels)
    if name == "strm":                                                  # :203-213
        return 0.1 * _ce16(s["pat"], labels) + _ce16(s["fr"], labels)
    if name == "strm_KD":                                               # :215-227
        return 0.1 * _ce16(s["pat"], labels) + _ce16(s["fr"], labels) + sw * kd_loss(s["fr"], t, T)
    if name == "fc_2_sup":                                              # :229-284
        fw = _focal(F.cross_entropy(s["ce"], labels), F.cross_entropy(s["kl"], labels))
        return (1 + fw) * kd_loss(s["kl"], t["kl"], T) + (2 - fw) * (0.1 * kd_loss(s["sup"], t["sup"], T) / 16 + _ce16(s["ce"], labels))
    if name == "fc_2_sup_kl":                                           # :339-383
        return kd_loss(s["kl"], t["kl"], T) + 0.5 * kd_loss(s["sup"], t["sup"], T) + _ce16(s["ce"], labels)
    if name == "fc_2_sup_dist_cece":                                    # :385-429
        return kd_loss(s["kl"], t["kl"], T) + _ce16(s["kl"], labels) + 0.5 * inter_class_relation(s["sup"], t["sup"]) + _ce16(s["ce"], labels)
    if name == "fc_2_sup_klklcece":                                     # :431-475
        return kd_loss(s["kl"], t["kl"], T) + _ce16(s["kl"], labels) + 0.5 * kd_loss(s["sup"], t["sup"], T) + _ce16(s["ce"], labels)
    if name == "fc_2_sup_distdistcece":                                 # :477-499
        return inter_class_relation(s["kl"], t["kl"]) + _ce16(s["kl"], labels) + 0.5 * inter_class_relation(s["sup"], t["sup"]) + _ce16(s["ce"], labels)
    if name == "fc_2_sup_2":                                            # :501-547
        return (kd_loss(s["kl"], t["kl"], T) + inter_class_relation(s["sup_kl"], t["sup"])) + _ce16(s["ce"], labels) + inter_class_relation(s["sup_ce"], t["sup"])
    if name == "fc_2_sup_disver":                                       # :549-572
        return 0.5 * kd_loss(s["sup"], t["sup"], T) + inter_class_relation(s["kl"], t["kl"]) + _ce16(s["ce"], labels) + _ce16(s["kl"], labels)
    if name == "fc_2_sup_dist_wsl":                                     # :574-624
        fw = _focal(F.cross_entropy(s["ce"], labels), F.cross_entropy(s["kl"], labels))
        return (0.5 + fw) * kd_loss(s["kl"], t["kl"], T) + (1.5 - fw) * (0.5 * inter_class_relation(s["sup"], t["sup"]) + _ce16(s["ce"], labels))
    if name == "strm_fc_2_sup_dist":                                    # :626-653
        return (kd_loss(s["fr1"], t["kl"], T) + 0.5 * inter_class_relation(s["sup"], t["sup"]) + _ce16(s["fr2"], labels)
                + 0.1 * (kd_loss(s["pat"], t["kl"], T) + _ce16(s["pat"], labels)))
    if name == "strm_1fc_sup":                                          # :655-681
        return (kd_loss(s["fr"], t["kl"], T) + 0.5 * inter_class_relation(s["sup"], t["sup"]) + _ce16(s["fr"], labels)
                + 0.1 * (kd_loss(s["pat"], t["kl"], T) + _ce16(s["pat"], labels)))
    if name == "fc_1_sup" or name == "e_dist_1fc_sup":                  # :683-696, :713-733
        return _ce16(s["kl"], labels) + kd_loss(s["kl"], t["kl"], T) + 0.5 * inter_class_relation(s["sup"], t["sup"])
    if name == "fc_sup":                                                # :698-711
        return _ce16(s["kl"], labels) + 0.5 * inter_class_relation(s["sup"], t["sup"])
    raise KeyError(name)


# name -> (student keys or None for a plain tensor, teacher keys or None)
DISTILL_SIGNATURES = {
    "KD": (None, None), "Dist_KD": (None, None), "ce": (None, None), "wsl": (None, None),
    "fc_2": (("fc_1", "fc_2"), None), "fc_2_wsl": (("fc_1", "fc_2"), None),
    "strm": (("pat", "fr"), None), "strm_KD": (("pat", "fr"), None),
    "fc_2_sup_dist": (("kl", "ce", "sup"), ("kl", "sup")), "fc_2_sup": (("kl", "ce", "sup"), ("kl", "sup")),
    "fc_2_sup_kl": (("kl", "ce", "sup"), ("kl", "sup")), "fc_2_sup_dist_cece": (("kl", "ce", "sup"), ("kl", "sup")),
    "fc_2_sup_klklcece": (("kl", "ce", "sup"), ("kl", "sup")), "fc_2_sup_distdistcece": (("kl", "ce", "sup"), ("kl", "sup")),
    "fc_2_sup_2": (("kl", "ce", "sup_ce", "sup_kl"), ("kl", "sup")), "fc_2_sup_disver": (("kl", "ce", "sup"), ("kl", "sup")),
    "fc_2_sup_dist_wsl": (("kl", "ce", "sup"), ("kl", "sup")),
    "strm_fc_2_sup_dist": (("fr1", "fr2", "pat", "sup"), ("kl", "sup")), "strm_1fc_sup": (("fr", "pat", "sup"), ("kl", "sup")),
    "fc_1_sup": (("kl", "sup"), ("kl", "sup")), "fc_sup": (("kl", "sup"), ("kl", "sup")), "e_dist_1fc_sup": (("kl", "sup"), ("kl", "sup")),
}


def distill_inputs(name, seed, nq=25):
    """seeded logits for a method: -> (student, teacher, labels); 'sup*' keys are [5,4], the rest [nq,5]"""
    g = torch.Generator().manual_seed(seed)
    sk, tk = DISTILL_SIGNATURES[name]

    def mk(k):
        if k.startswith("sup"):
            return torch.randn(5, 4, generator=g) * 20 - 100
        return torch.randn(nq, 5, generator=g) * 30 - 300
    s = mk("x") if sk is None else {k: mk(k) for k in sk}
    t = mk("x") if tk is None else {k: mk(k) for k in tk}
    labels = torch.randint(0, 5, (nq,), generator=g)
    return s, t, labels


def distill_KL_feature(student, teacher, labels, cfg=DEFAULT_CFG):
    """Distiller.KL_feature (distillers.py:126-150): CE/16 + T^2 KL + MSE(student feature, teacher feature)"""
    ce = cfg["hard_loss_weight"] * F.cross_entropy(student["logits"], labels) / 16
    kl = cfg["soft_loss_weight"] * kd_loss(student["logits"], teacher["logits"], cfg["temperature"])
    feat = cfg["feature_loss_weight"] * F.mse_loss(student["feature"], teacher["feature"])
    return {"hard_loss": ce, "soft_loss": kl, "feature_loss": feat, "loss": ce + kl + feat}


# A14 ------------------------------------------------------------------------
def aggregate_accuracy(logits, labels):
    """utils.py:116-121."""
    return torch.mean(torch.eq(labels, torch.argmax(logits, dim=-1)).float())


# ----------------------------------------------------------------------------
# A10  MFM fusion  (teacher/code/model.py:1135-1151, 1300-1331, 1361-1392, 1648-1664)
#      eval mode (dropout off); nn.TransformerEncoderLayer defaults: post-norm, ReLU,
#      dim_feedforward 2048, LayerNorm eps 1e-5, batch_first.
# ----------------------------------------------------------------------------
def _trainable_pe(x, p, prefix):
    L = x.shape[1]
    emb = p[prefix + ".position_embeddings.weight"][:L].unsqueeze(0)
    return F.layer_norm(x + emb, (x.shape[-1],), p[prefix + ".LayerNorm.weight"],
                        p[prefix + ".LayerNorm.bias"], 1e-5)


def _encoder_layer(x, p, prefix, nhead):
    B, L, D = x.shape
    hd = D // nhead
    qkv = F.linear(x, p[prefix + ".self_attn.in_proj_weight"], p[prefix + ".self_attn.in_proj_bias"])
    q, k, v = qkv.chunk(3, dim=-1)
    q = q.reshape(B, L, nhead, hd).transpose(1, 2)
    k = k.reshape(B, L, nhead, hd).transpose(1, 2)
    v = v.reshape(B, L, nhead, hd).transpose(1, 2)
    att = torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(hd), dim=-1)
    o = (att @ v).transpose(1, 2).reshape(B, L, D)
    o = F.linear(o, p[prefix + ".self_attn.out_proj.weight"], p[prefix + ".self_attn.out_proj.bias"])
    x = F.layer_norm(x + o, (D,), p[prefix + ".norm1.weight"], p[prefix + ".norm1.bias"], 1e-5)
    ff = F.linear(F.relu(F.linear(x, p[prefix + ".linear1.weight"], p[prefix + ".linear1.bias"])),
                  p[prefix + ".linear2.weight"], p[prefix + ".linear2.bias"])
    return F.layer_norm(x + ff, (D,), p[prefix + ".norm2.weight"], p[prefix + ".norm2.bias"], 1e-5)


def mfm_three_fusion(x, y, z, p, prefix="three_fusion", num_layers=2):
    h = torch.cat((_trainable_pe(x, p, prefix + ".positionEncoding1"),
                   _trainable_pe(y, p, prefix + ".positionEncoding2"),
                   _trainable_pe(z, p, prefix + ".positionEncoding3")), dim=-1)
    for l in range(num_layers):
        h = _encoder_layer(h, p, "%s.transformer_encoder.layers.%d" % (prefix, l), 3)
    return F.linear(h, p[prefix + ".f1.weight"], p[prefix + ".f1.bias"])


def mfm_two_fusion(x, y, p, prefix="fusion", num_layers=2):
    h = torch.cat((_trainable_pe(x, p, prefix + ".positionEncoding1"),
                   _trainable_pe(y, p, prefix + ".positionEncoding2")), dim=-1)
    for l in range(num_layers):
        h = _encoder_layer(h, p, "%s.transformer_encoder.layers.%d" % (prefix, l), 2)
    return F.linear(h, p[prefix + ".f1.weight"], p[prefix + ".f1.bias"])


def mfm_extract_feature(rgb, depth, flow, p, shirt_num=1, num_layers=2):
    """ThreeTRXShiftLoopTime.extract_feature (teacher/code/model.py:1648-1664)."""
    f1 = mfm_three_fusion(rgb, depth, flow, p, num_layers=num_layers)
    d2 = torch.cat((depth[:, shirt_num:], depth[:, :shirt_num]), dim=1)
    f2 = mfm_two_fusion(rgb, d2, p, num_layers=num_layers)
    fl = torch.cat((flow[:, shirt_num:], flow[:, :shirt_num]), dim=1)
    f3 = mfm_two_fusion(rgb, fl, p, num_layers=num_layers)
    return f1 + f2 + f3


def mfm_param_shapes(d=2048, seq_len=8, num_layers=2, dff=2048):
    shp = {}

    def pe(prefix):
        shp[prefix + ".position_embeddings.weight"] = (seq_len, d)
        shp[prefix + ".LayerNorm.weight"] = (d,)
        shp[prefix + ".LayerNorm.bias"] = (d,)

    def enc(prefix, D):
        for l in range(num_layers):
            q = "%s.transformer_encoder.layers.%d" % (prefix, l)
            shp[q + ".self_attn.in_proj_weight"] = (3 * D, D)
            shp[q + ".self_attn.in_proj_bias"] = (3 * D,)
            shp[q + ".self_attn.out_proj.weight"] = (D, D)
            shp[q + ".self_attn.out_proj.bias"] = (D,)
            shp[q + ".linear1.weight"] = (dff, D)
            shp[q + ".linear1.bias"] = (dff,)
            shp[q + ".linear2.weight"] = (D, dff)
            shp[q + ".linear2.bias"] = (D,)
            for n in ("norm1", "norm2"):
                shp[q + "." + n + ".weight"] = (D,)
                shp[q + "." + n + ".bias"] = (D,)
        shp[prefix + ".f1.weight"] = (d, D)
        shp[prefix + ".f1.bias"] = (d,)

    for i in (1, 2, 3):
        pe("three_fusion.positionEncoding%d" % i)
    enc("three_fusion", 3 * d)
    for i in (1, 2):
        pe("fusion.positionEncoding%d" % i)
    enc("fusion", 2 * d)
    return shp


def make_mfm_params(seed, d=2048, seq_len=8, num_layers=2, dff=2048):
    """Seeded weights for the MFM fusion, keyed like the reference's state_dict (`fusion.*`, `three_fusion.*`).
    Each tensor is drawn from its own generator (seed mixed with a CRC of the key), so the values do not depend on the
    order in which a module happens to construct its parameters: gen_golden.py loads them into the reference's
    ThreeTRXShiftLoopTime, the tests into the oracle and into the HIP module.  Scales follow the torch defaults in
    magnitude (Linear U(+-1/sqrt(fan_in)), in_proj xavier-like) with non-trivial LayerNorm affines and biases."""
    import zlib
    out = {}
    for k, shp in mfm_param_shapes(d, seq_len, num_layers, dff).items():
        g = torch.Generator().manual_seed((int(seed) * 1000003 + zlib.crc32(k.encode())) & 0x7FFFFFFFFFFFFFFF)
        if k.endswith("position_embeddings.weight"):
            t = torch.randn(shp, generator=g)
        elif "LayerNorm.weight" in k or ".norm1.weight" in k or ".norm2.weight" in k:
            t = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif len(shp) == 1:                       # biases (incl. self_attn.in_proj_bias)
            t = 0.05 * torch.randn(shp, generator=g)
        else:                                     # matrices [out, in]
            bound = 1.0 / math.sqrt(shp[1])
            t = (torch.rand(shp, generator=g) * 2 - 1) * bound
        out[k] = t
    return out


def make_mfm_inputs(seed, n, d=2048, seq_len=8):
    """rgb / depth / flow per-modality features ~ |N(0,1)| (post-ReLU-like)"""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(n, seq_len, d, generator=g).abs() for _ in range(3))


# ----------------------------------------------------------------------------
# synthetic episodes + seeded weights — shared by tests and bench
# ----------------------------------------------------------------------------
def make_student_params(seed, backbone="resnet18_2fc", out_dim=1152, seq_len=8):
    g = torch.Generator().manual_seed(seed)
    params = {"backbone.resnet." + k: v for k, v in init_resnet18_trunk(g).items()}

    def linear(prefix, fout, fin):
        bound = 1.0 / math.sqrt(fin)
        params[prefix + ".weight"] = (torch.rand(fout, fin, generator=g) * 2 - 1) * bound
        params[prefix + ".bias"] = (torch.rand(fout, generator=g) * 2 - 1) * bound

    if backbone == "resnet18_2fc":
        linear("backbone.fc1", 2048, 512)
        linear("backbone.fc2", 2048, 512)
    else:
        linear("backbone.res18_2048", 2048, 512)
    params.update({"classifier.transformers." + k: v
                   for k, v in make_trx_params(g, out_dim, seq_len).items()})
    return params


def make_trx_params(g, out_dim=1152, seq_len=8):
    p = {}
    bound = 1.0 / math.sqrt(4096)
    for n in ("k_linear", "v_linear"):
        p[n + ".weight"] = (torch.rand(out_dim, 4096, generator=g) * 2 - 1) * bound
        p[n + ".bias"] = (torch.rand(out_dim, generator=g) * 2 - 1) * bound
    for n in ("norm_k", "norm_v"):
        p[n + ".weight"] = torch.ones(out_dim)
        p[n + ".bias"] = torch.zeros(out_dim)
    p["pe.pe"] = positional_encoding_table(2048, int(seq_len * 1.5))
    return p


def make_episode(seed, way=5, shot=5, query=5, seq_len=8, img=224, frames=True):
    """support_set/target_set ~ U[0,1) (ToTensor range, video_reader.py:384), teacher
    features ~ N(0,1), labels = seeded permutation of repeat_interleave(arange(way))."""
    g = torch.Generator().manual_seed(seed)
    ns, nq = way * shot, way * query
    ep = {}
    if frames:
        ep["support_set"] = torch.rand(ns * seq_len, 3, img, img, generator=g)
        ep["target_set"] = torch.rand(nq * seq_len, 3, img, img, generator=g)
    ep["support_set_feature_teacher"] = torch.randn(ns, seq_len, 2048, generator=g)
    ep["target_set_feature_teacher"] = torch.randn(nq, seq_len, 2048, generator=g)
    sl = torch.arange(way).repeat_interleave(shot)[torch.randperm(ns, generator=g)]
    tl = torch.arange(way).repeat_interleave(query)[torch.randperm(nq, generator=g)]
    ep["support_labels"] = sl.float()
    ep["target_labels"] = tl.float()
    return ep


def student_forward(ep, params, way=5, shot=5, classifier="TRX_2fcsup", backbone="resnet18_2fc",
                    training=True, update_running=True):
    """Student.forward (model_select.py:26-36) for the default plugins."""
    bp = {k[len("backbone."):]: v for k, v in params.items() if k.startswith("backbone.")}
    cp = {k[len("classifier.transformers."):]: v for k, v in params.items()
          if k.startswith("classifier.transformers.")}
    if backbone == "resnet18_2fc":
        ctx, tgt = backbone_resnet18_2fc(ep["support_set"], ep["target_set"], bp, 8, training, update_running)
    elif backbone == "resnet50_2fc":
        ctx, tgt = backbone_resnet50_2fc(ep["support_set"], ep["target_set"], bp, 8, training, update_running)
    else:
        ctx, tgt = backbone_resnet18_student(ep["support_set"], ep["target_set"], bp, 8, training, update_running)
    if classifier == "TRX_2fcsup":
        logits = clf_TRX_2fcsup(ctx, ep["support_labels"], tgt, cp, way, shot)
    elif classifier == "e_dist_fc2_sup":
        logits = clf_e_dist_fc2_sup(ctx, ep["support_labels"], tgt, way, shot)
    elif classifier == "e_dist_1fc_sup":
        logits = clf_e_dist_1fc_sup(ctx, ep["support_labels"], tgt, way, shot)
    elif classifier == "TRX":                      # model/classifiers/TRX.py:167-183: one head, bare [Nq, way] logits
        logits = trx_logits(ctx, ep["support_labels"], tgt, cp)
    else:
        raise KeyError(classifier)
    return {"logits": logits, "context_features": ctx, "target_features": tgt}


def train_episode(ep, params, teacher_params, way=5, shot=5, cfg=DEFAULT_CFG):
    """train_task (trainwandb.py:190-287): student fwd, teacher fwd, fc_2_sup_dist,
    accuracy on kl+ce, backward.  `params` tensors with requires_grad accumulate .grad."""
    out = student_forward(ep, params, way, shot)
    t_logits = clf_TRX_2fcsup_fixed(ep["support_set_feature_teacher"], ep["support_labels"],
                                    ep["target_set_feature_teacher"], teacher_params, way, shot)
    labels = ep["target_labels"].long()
    loss = distill_fc_2_sup_dist(out["logits"], t_logits, labels, cfg)
    acc = aggregate_accuracy(out["logits"]["kl"] + out["logits"]["ce"], labels)
    loss["loss"].backward()
    return loss["loss"].detach(), acc, out, t_logits


def train_loop(episodes, params, teacher_params, way=5, shot=5, opt="sgd", lr=1e-4, tasks_per_batch=16, milestones=(20000, 40000),
               total_iterations=None, cfg=DEFAULT_CFG):
    """A15: make() + train() of the reference (trainwandb.py:101-105 optimizer / MultiStepLR, :111-145 loop) over a list of
    episodes with torch's own optimizers: torch.optim.SGD(lr) (no momentum) or torch.optim.Adam(lr) on the trainable `params`,
    MultiStepLR(milestones, gamma=0.1); `iteration` is incremented before use, the step fires when (iteration+1) %
    tasks_per_batch == 0 or iteration == total_iterations-1, scheduler.step() runs every episode.
    -> (losses, accuracies); `params` are updated in place."""
    leaves = [v for k, v in params.items() if v.is_floating_point() and v.requires_grad]
    if opt == "adam":
        optimizer = torch.optim.Adam(leaves, lr=lr)
    elif opt == "sgd":
        optimizer = torch.optim.SGD(leaves, lr=lr)
    else:
        raise KeyError(opt)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=list(milestones), gamma=0.1)
    optimizer.zero_grad()
    total = len(episodes) if total_iterations is None else total_iterations
    losses, accs = [], []
    iteration = 0
    for ep in episodes:
        if iteration >= total:
            break
        iteration += 1
        loss, acc, _, _ = train_episode(ep, params, teacher_params, way, shot, cfg)
        losses.append(float(loss))
        accs.append(float(acc))
        if ((iteration + 1) % tasks_per_batch == 0) or (iteration == (total - 1)):
            optimizer.step()
            optimizer.zero_grad()
        scheduler.step()
    return losses, accs


# ----------------------------------------------------------------------------
# A0 (input side)  Resize(256) of the frame transform: video_reader.py:92-112 -> videotransforms/video_transforms.py:91-110
# -> functional.resize_clip (functional.py:24-63), which - its `interpolation` test being inverted (:55-58) - calls
# PIL.Image.resize(size, PIL.Image.BILINEAR) for the default Resize(interpolation='nearest').  The arithmetic is Pillow's
# (third-party, pinned pillow==9.3.0 in envirment.yml:93; the 8-bit resampler is unchanged through the 12.2.0 installed here):
# ImagingResample with the triangle filter, support 1.0 * max(scale, 1), coefficients normalised in double and rounded to
# 22-bit fixed point, a horizontal pass to uint8 and then a vertical pass, each  clip8((2^21 + sum(pixel * k)) >> 22).
# Restated below in numpy integers and pinned bit-exactly against PIL itself by oracle/gen_golden.py (tests/golden/resize.npz).
# ----------------------------------------------------------------------------
PIL_PRECISION_BITS = 32 - 8 - 2


def pil_bilinear_coeffs(in_size, out_size):
    """-> bounds [out,2] (first input index, count), coefficients [out, ksize] int32, ksize"""
    import numpy as np
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [0.0] * ksize
        ww = 0.0
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            w[x] = 1.0 - a if a < 1.0 else 0.0
            ww += w[x]
        for x in range(xmax):
            if ww != 0.0:
                w[x] /= ww
        for x in range(ksize):
            kk[xx, x] = int(-0.5 + w[x] * (1 << PIL_PRECISION_BITS)) if w[x] < 0 else int(0.5 + w[x] * (1 << PIL_PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def _pil_resample_axis(img, out_size, axis):
    import numpy as np
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    b, kk, _ = pil_bilinear_coeffs(img.shape[0], out_size)
    out = np.zeros((out_size,) + img.shape[1:], np.int64)
    for xx in range(out_size):
        s = np.full(img.shape[1:], 1 << (PIL_PRECISION_BITS - 1), np.int64)
        for x in range(int(b[xx, 1])):
            s += img[b[xx, 0] + x] * int(kk[xx, x])
        out[xx] = np.clip(s >> PIL_PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def pil_resize_bilinear_u8(img, out_w, out_h):
    """img uint8 [..., H, W, C] (numpy) -> [..., out_h, out_w, C]: PIL.Image.resize((out_w, out_h), BILINEAR)"""
    t = img
    if out_w != img.shape[-2]:
        t = _pil_resample_axis(t, out_w, t.ndim - 2)          # horizontal pass first
    if out_h != img.shape[-3]:
        t = _pil_resample_axis(t, out_h, t.ndim - 3)
    return t


def resize_short_side(im_h, im_w, size):
    """functional.py:45-52,66-73: output (h, w) of Resize(size) for an int size; unchanged if the short side already matches"""
    if (im_w <= im_h and im_w == size) or (im_h <= im_w and im_h == size):
        return im_h, im_w
    if im_w < im_h:
        return int(size * im_h / im_w), size
    return size, int(size * im_w / im_h)
