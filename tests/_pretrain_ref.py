"""Plain torch / numpy restatements of what the teacher's pretraining and feature extraction compute, written from the behaviour the
modules document (litemkd_amd.pretrain, litemkd_amd.extract, teacher.action_recognition); shared by test_pretrain_host.py and
test_gpu_pretrain.py.  Nothing here imports the package."""
import io
import os
import random

import numpy as np
import torch
import torch.nn.functional as F


# ---- data rules ----
def get_seq_indices(n, seq_len, train):
    """the dataset's frame choice step by step for a video of n sorted frame files -> indices into them: more files than seq_len are
    first subsampled at int(linspace(0, n - 1, seq_len)); a list of exactly seq_len is taken whole; a shorter one goes through the
    start / end padding rule and its `end - start < seq_len` fallback; seq_len 1 draws between start and end - 1 (never reached:
    a list of one file is of exactly seq_len)."""
    files = list(range(n))
    if len(files) > seq_len:
        files = [files[int(i)] for i in np.linspace(0, len(files) - 1, seq_len).tolist()]
    m = len(files)
    if m == 0:
        raise Exception("No frames found")
    if m == seq_len:
        idxs = list(range(m))
    else:
        if train:
            excess_pad = int(min(5, (m - seq_len) / 2))
            if excess_pad < 1:
                start, end = 0, m - 1
            else:
                start, end = random.randint(0, excess_pad), random.randint(m - 1 - excess_pad, m - 1)
        else:
            start, end = 1, m - 2
        if end - start < seq_len:
            start, end = 0, m - 1
        idxs = [int(f) for f in np.linspace(start, end, num=seq_len)]
        if seq_len == 1:
            idxs = [random.randint(start, end - 1)]
    return [files[i] for i in idxs]


def parse_list(text):
    """the entries of a split list: spaces become '_', the first field of a line"""
    return [x.replace(" ", "_").strip().split(" ")[0] for x in text.strip().split("\n")]


def labels_by_first_appearance(text):
    d = {}
    for e in parse_list(text):
        c = e.split("/")[0]
        if c not in d:
            d[c] = len(d)
    return d


# ---- the torchvision resnet50 state dict, from its key and shape table alone ----
def torchvision_resnet50_shapes():
    shapes = {"conv1.weight": (64, 3, 7, 7)}

    def bn(prefix, c):
        for k, s in (("weight", (c,)), ("bias", (c,)), ("running_mean", (c,)), ("running_var", (c,)), ("num_batches_tracked", ())):
            shapes[prefix + "." + k] = s
    bn("bn1", 64)
    cin = 64
    for li, (width, n) in enumerate(((64, 3), (128, 4), (256, 6), (512, 3)), start=1):
        for b in range(n):
            p = "layer%d.%d" % (li, b)
            shapes[p + ".conv1.weight"] = (width, cin, 1, 1)
            bn(p + ".bn1", width)
            shapes[p + ".conv2.weight"] = (width, width, 3, 3)
            bn(p + ".bn2", width)
            shapes[p + ".conv3.weight"] = (4 * width, width, 1, 1)
            bn(p + ".bn3", 4 * width)
            if b == 0:
                shapes[p + ".downsample.0.weight"] = (4 * width, cin, 1, 1)
                bn(p + ".downsample.1", 4 * width)
            cin = 4 * width
    shapes["fc.weight"] = (1000, 2048)
    shapes["fc.bias"] = (1000,)
    return shapes


def torchvision_resnet50_state(seed=0):
    """a state dict with those keys and shapes; every tensor filled with its own position in the table, so a wrong mapping shows"""
    sd = {}
    for i, (k, s) in enumerate(torchvision_resnet50_shapes().items()):
        sd[k] = torch.full(s, i, dtype=torch.long) if k.endswith("num_batches_tracked") else torch.full(s, float(i + seed))
    return sd


def sequential_key(tv_key):
    """the key nn.Sequential(*list(resnet50.children())[:-1]) gives a torchvision key: children 0 conv1, 1 bn1, 2 relu, 3 maxpool,
    4..7 layer1..4, 8 avgpool"""
    head, rest = tv_key.split(".", 1)
    return {"conv1": "0", "bn1": "1", "layer1": "4", "layer2": "5", "layer3": "6", "layer4": "7"}[head] + "." + rest


# ---- the classifier over a trunk ----
def clip_logits(trunk, sd, x, num_frames, fc_w, fc_b, training=True):
    """x [B * T, 3, H, W] -> (logits [B, classes], per-frame features [B * T, 2048]): the trunk's map, its global average pool, the mean
    over each clip's frames, fc.  trunk: a function (x, state dict, training) -> NCHW map"""
    fm = trunk(x, sd, training)
    feat = fm.mean(dim=(2, 3))
    clip = feat.reshape(-1, num_frames, feat.shape[1]).mean(dim=1)
    return F.linear(clip, fc_w, fc_b), feat


def cross_entropy_parts(logits, labels):
    """-> (mean loss, its logits gradient, predictions (first maximal index), accuracy) in the dtype of the logits"""
    lg = logits.detach().clone().requires_grad_()
    loss = -F.log_softmax(lg, dim=1).gather(1, labels.view(-1, 1)).mean()
    loss.backward()
    mx = lg.detach().max(dim=1, keepdim=True).values
    first = (lg.detach() == mx).to(torch.int64).argmax(dim=1)      # argmax of a 0/1 tensor returns the first 1
    return loss.detach(), lg.grad, first, (first == labels).double().mean()


def sgd_momentum(params, grads_per_step, lr, momentum):
    """torch.optim.SGD(momentum) in fp64 over a list of gradient tensors, one per step -> (parameters, momentum buffer) after them"""
    p = torch.nn.Parameter(params.detach().double().clone())
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum)
    for g in grads_per_step:
        p.grad = g.detach().double().clone()
        opt.step()
    return p.detach(), opt.state[p]["momentum_buffer"].detach()


def step_lr_sequence(base_lr, epochs, step_size=10, gamma=0.1):
    """the learning rate each epoch trains with when StepLR is stepped at the START of every epoch"""
    import warnings
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base_lr, momentum=0.9)
    sch = torch.optim.lr_scheduler.StepLR(opt, step_size=step_size, gamma=gamma)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # torch warns about a scheduler stepped before its optimizer: that order is the point
        for _ in range(epochs):
            sch.step()
            out.append(opt.param_groups[0]["lr"])
    return out


# ---- a small JPEG tree ----
def write_jpeg_tree(root, lists, classes=("Apply Eye", "Bowl", "Climb"), videos=2, frames=(5, 4, 9), hw=(80, 96), seed=0):
    """<root>/<class with '_' for ' '>/<video>/img_%05d.jpg and {train,test}list03.txt under `lists`, the class names in the lists
    written WITH their spaces (the readers replace them) -> the entries as the readers see them"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    entries, lines = [], []
    os.makedirs(lists, exist_ok=True)
    for ci, cname in enumerate(classes):
        for v in range(videos):
            vid = "v_%s_g%02d" % (cname.split(" ")[0], v)
            d = os.path.join(root, cname.replace(" ", "_"), vid)
            os.makedirs(d, exist_ok=True)
            for f in range(frames[(ci * videos + v) % len(frames)]):
                yy, xx = np.mgrid[0:hw[0], 0:hw[1]]
                img = np.stack([(xx * 2 + 40 * ci + 3 * f) % 256, (yy * 2 + 25 * v) % 256, (xx + yy + 60 * ci) % 256], -1)
                img = np.clip(img + rng.integers(-6, 7, img.shape), 0, 255).astype(np.uint8)
                b = io.BytesIO()
                Image.fromarray(img).save(b, "JPEG", quality=80)
                with open(os.path.join(d, "img_%05d.jpg" % (f + 1)), "wb") as fh:
                    fh.write(b.getvalue())
            lines.append("%s/%s" % (cname, vid))      # the path alone: every space of a line becomes '_', a label field would join the name
            entries.append("%s/%s" % (cname.replace(" ", "_"), vid))
    for name in ("trainlist03.txt", "testlist03.txt"):
        with open(os.path.join(lists, name), "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return entries
