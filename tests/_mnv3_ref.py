"""torch-CPU restatement of torchvision's MobileNetV3-Large `features` and of the reference's mobile_large_2fc / mobile_large heads
(model/backbone/moblienetv3.py), for the MobileNetV3 tests only: NCHW, torch's own conv2d(groups=C), batch_norm, hardswish and
hardsigmoid, in whatever dtype the parameters have (fp32 or fp64).  Parameters are a {key: tensor} dict with the student's keys
(`backbone.mobile.0.<i>.…`)."""
import torch
import torch.nn.functional as F

# (in, kernel, expanded, out, SE, activation, stride) of features.1 .. 15, restated independently of the product's table
BLOCKS = [
    (16, 3, 16, 16, 0, "RE", 1), (16, 3, 64, 24, 0, "RE", 2), (24, 3, 72, 24, 0, "RE", 1),
    (24, 5, 72, 40, 1, "RE", 2), (40, 5, 120, 40, 1, "RE", 1), (40, 5, 120, 40, 1, "RE", 1),
    (40, 3, 240, 80, 0, "HS", 2), (80, 3, 200, 80, 0, "HS", 1), (80, 3, 184, 80, 0, "HS", 1),
    (80, 3, 184, 80, 0, "HS", 1), (80, 3, 480, 112, 1, "HS", 1), (112, 3, 672, 112, 1, "HS", 1),
    (112, 5, 672, 160, 1, "HS", 2), (160, 5, 960, 160, 1, "HS", 1), (160, 5, 960, 160, 1, "HS", 1),
]
SQUEEZE = {72: 24, 120: 32, 480: 120, 672: 168, 960: 240}
EPS, MOMENTUM = 1e-3, 0.01


def feature_shapes():
    """{key under features.: shape} of torchvision mobilenet_v3_large().features, in module order"""
    out = {}

    def cba(pre, cin, cout, k, groups=1):
        out[pre + "0.weight"] = (cout, cin // groups, k, k)
        for n in ("weight", "bias", "running_mean", "running_var"):
            out[pre + "1." + n] = (cout,)
        out[pre + "1.num_batches_tracked"] = ()
    cba("0.", 3, 16, 3)
    for i, (cin, k, exp, cout, se, _, _) in enumerate(BLOCKS):
        pre, j = "%d.block." % (i + 1), 0
        if exp != cin:
            cba(pre + "0.", cin, exp, 1)
            j = 1
        cba(pre + "%d." % j, exp, exp, k, groups=exp)
        j += 1
        if se:
            q = SQUEEZE[exp]
            out[pre + "%d.fc1.weight" % j] = (q, exp, 1, 1)
            out[pre + "%d.fc1.bias" % j] = (q,)
            out[pre + "%d.fc2.weight" % j] = (exp, q, 1, 1)
            out[pre + "%d.fc2.bias" % j] = (exp,)
            j += 1
        cba(pre + "%d." % j, exp, cout, 1)
    cba("16.", 160, 960, 1)
    return out


def _act(x, a):
    return F.relu(x) if a == "RE" else (F.hardswish(x) if a == "HS" else x)


def _cba(x, p, pre, stride, groups, act, training, update):
    w = p[pre + "0.weight"]
    k = w.shape[-1]
    y = F.conv2d(x, w, None, stride, (k - 1) // 2, 1, groups)
    rm, rv = p[pre + "1.running_mean"], p[pre + "1.running_var"]
    if training and update:
        # F.batch_norm updates the running buffers in place; keep the caller's tensors as they are and hand back new ones
        rm2, rv2 = rm.detach().clone(), rv.detach().clone()
        y = F.batch_norm(y, rm2, rv2, p[pre + "1.weight"], p[pre + "1.bias"], True, MOMENTUM, EPS)
        p[pre + "1.running_mean"], p[pre + "1.running_var"] = rm2, rv2
        p[pre + "1.num_batches_tracked"] = p[pre + "1.num_batches_tracked"] + 1
    else:
        y = F.batch_norm(y, None if training else rm, None if training else rv, p[pre + "1.weight"], p[pre + "1.bias"], training, MOMENTUM, EPS)
    return _act(y, act)


def features(x, params, prefix="backbone.mobile.0.", training=True, update=True):
    """x NCHW [F, 3, H, W] -> [F, 960, H/32, W/32].  With training and update, params' running buffers are replaced by updated copies."""
    p = {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix)}
    x = _cba(x, p, "0.", 2, 1, "HS", training, update)
    for i, (cin, k, exp, cout, se, act, stride) in enumerate(BLOCKS):
        pre, j, y = "%d.block." % (i + 1), 0, x
        if exp != cin:
            y = _cba(y, p, pre + "0.", 1, 1, act, training, update)
            j = 1
        y = _cba(y, p, pre + "%d." % j, stride, exp, act, training, update)
        j += 1
        if se:
            s = y.mean((2, 3), keepdim=True)
            s = F.relu(F.conv2d(s, p[pre + "%d.fc1.weight" % j], p[pre + "%d.fc1.bias" % j]))
            s = F.hardsigmoid(F.conv2d(s, p[pre + "%d.fc2.weight" % j], p[pre + "%d.fc2.bias" % j]))
            y = y * s
            j += 1
        y = _cba(y, p, pre + "%d." % j, 1, 1, None, training, update)
        x = y + x if (stride == 1 and cin == cout) else y
    x = _cba(x, p, "16.", 1, 1, "HS", training, update)
    for k, v in p.items():
        params[prefix + k] = v
    return x


def pooled(fmap):
    """AdaptiveMaxPool2d((4, 4)), reshape [F, 960, 16], mean over the 16 patches (moblienetv3.py:41-52)"""
    q = F.adaptive_max_pool2d(fmap, (4, 4))
    return q.reshape(q.shape[0], q.shape[1], 16).permute(0, 2, 1).mean(dim=1)


def backbone_2fc(ctx, tgt, params, seq_len=8, training=True, update=True):
    """mobile_large_2fc.forward: two trunk calls, then fc1 / fc2 -> the two dicts"""
    cf = pooled(features(ctx, params, training=training, update=update))
    tf = pooled(features(tgt, params, training=training, update=update))
    c, t = {}, {}
    for h in (1, 2):
        w, b = params["backbone.fc%d.weight" % h], params["backbone.fc%d.bias" % h]
        c["context_features_%d" % h] = F.linear(cf, w, b).reshape(-1, seq_len, 2048)
        t["target_features_%d" % h] = F.linear(tf, w, b).reshape(-1, seq_len, 2048)
    return c, t


def backbone_1fc(ctx, tgt, params, seq_len=8, training=True, update=True):
    """mobile_large.forward"""
    cf = pooled(features(ctx, params, training=training, update=update))
    tf = pooled(features(tgt, params, training=training, update=update))
    w, b = params["backbone.fc.weight"], params["backbone.fc.bias"]
    return F.linear(cf, w, b).reshape(-1, seq_len, 2048), F.linear(tf, w, b).reshape(-1, seq_len, 2048)
