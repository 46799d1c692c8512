"""Teacher pretraining / feature extraction benchmark, one process on one GPU.  --part selects what is measured, so that each
part can run under a time limit of its own:

  extract  videos per second of Action_Recognition_Resnet50.extract_feature (trunk + global average pool, eval mode, the features copied
           to the host) on clips of 8 frames of 224 x 224 already on the device in the frame transform's NHWC4 layout, for 1, 8 and 25
           videos per call; JPEG reading, decoding and the transform are not part of it (tools/jpeg_bench.py measures those);
  step     milliseconds per pretraining step at batch 8 (64 frames of 224 x 224): forward, ops.softmax_ce, backward,
           trainloop.MomentumSGD.step(zero_grad=True);
  kernels  microseconds per launch of the three kernels of csrc/clipcls.hip, and the pool's achieved fraction of HBM bandwidth at
           [64, 7, 7, 2048] fp32: the launches rotate over 16 input tensors (411 MB) so that none is served from the 256 MiB Infinity Cache.

`extract` and `step` are also run with the same network built here from torch.nn (Conv2d / BatchNorm2d / ReLU / MaxPool2d /
AdaptiveAvgPool2d / Linear in torchvision's v1.5 arrangement, fp32, F.cross_entropy, two torch.optim.SGD(momentum=0.9)) on the same GPU.
HIP events around batches of back-to-back calls after a warm-up; median, minimum and maximum of the timings.

    python tools/pretrain_bench.py --part extract|step|kernels [--iters n] [--batches n] [--dtype fp32x3|fp32h2|fp32|bf16] [--out file.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12      # bytes / s a streaming kernel reaches on the MI355X (8e12 peak)
HBM_PEAK = 8.0e12


def stat(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "runs": v}


def events_ms(fn, iters, batches, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def nn_resnet50(num_classes):
    """torchvision's resnet50 (v1.5: the stride on conv2) written with torch.nn; forward(x [B, T, 3, H, W]) -> logits, features(x [F, 3, H, W])"""
    import torch.nn as nn

    class Bottleneck(nn.Module):
        def __init__(self, cin, width, stride):
            super().__init__()
            self.conv1, self.bn1 = nn.Conv2d(cin, width, 1, bias=False), nn.BatchNorm2d(width)
            self.conv2, self.bn2 = nn.Conv2d(width, width, 3, stride, 1, bias=False), nn.BatchNorm2d(width)
            self.conv3, self.bn3 = nn.Conv2d(width, 4 * width, 1, bias=False), nn.BatchNorm2d(4 * width)
            self.relu = nn.ReLU(inplace=True)
            self.downsample = None
            if stride != 1 or cin != 4 * width:
                self.downsample = nn.Sequential(nn.Conv2d(cin, 4 * width, 1, stride, bias=False), nn.BatchNorm2d(4 * width))

        def forward(self, x):
            idn = x if self.downsample is None else self.downsample(x)
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.relu(self.bn2(self.conv2(out)))
            return self.relu(self.bn3(self.conv3(out)) + idn)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            layers = [nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1)]
            cin = 64
            for width, n, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
                for i in range(n):
                    layers.append(Bottleneck(cin, width, stride if i == 0 else 1))
                    cin = 4 * width
            layers.append(nn.AdaptiveAvgPool2d(1))
            self.convnet = nn.Sequential(*layers)
            self.fc = nn.Linear(2048, num_classes)

        def features(self, x):
            return self.convnet(x).flatten(1)

        def forward(self, x):
            b, t = x.shape[:2]
            return self.fc(self.features(x.reshape((b * t,) + x.shape[2:])).view(b, t, -1).mean(dim=1))
    return Net()


def part_extract(a, dev, out):
    import torch
    from litemkd_amd.teacher.action_recognition import Action_Recognition_Resnet50
    model = Action_Recognition_Resnet50(argparse.Namespace(num_classes=64)).to(dev).eval()
    ref = nn_resnet50(64).to(dev).eval()
    res = {}
    for v in (1, 8, 25):
        x4 = torch.rand(v * 8, 224, 224, 4, device=dev)
        x4[..., 3] = 0
        x = x4[..., :3].permute(0, 3, 1, 2).contiguous()

        def hip():
            return model.extract_feature(x4).cpu()

        def tor():
            with torch.no_grad():
                return ref.features(x).cpu()
        assert tuple(hip().shape) == tuple(tor().shape) == (v * 8, 2048)
        h, t = stat(events_ms(hip, a.iters, a.batches, a.warmup)), stat(events_ms(tor, a.iters, a.batches, a.warmup))
        res["videos_per_call_%d" % v] = {"hip_ms_per_call": h, "torch_gpu_ms_per_call": t, "hip_videos_per_s": 1e3 * v / h["median"],
                                         "hip_videos_per_s_range": [1e3 * v / h["max"], 1e3 * v / h["min"]],
                                         "torch_gpu_videos_per_s": 1e3 * v / t["median"],
                                         "torch_gpu_videos_per_s_range": [1e3 * v / t["max"], 1e3 * v / t["min"]],
                                         "torch_over_hip_time": t["median"] / h["median"]}
    out["extract"] = res


def part_step(a, dev, out):
    import torch
    import torch.nn.functional as F
    from litemkd_amd import ops
    from litemkd_amd import pretrain as PT
    from litemkd_amd.teacher.action_recognition import Action_Recognition_Resnet50
    args = argparse.Namespace(num_classes=64, lr_1=1e-6, lr_2=1e-2)
    B, T = 8, 8
    x4 = torch.rand(B, T, 224, 224, 4, device=dev)
    x4[..., 3] = 0
    x = x4[..., :3].permute(0, 1, 4, 2, 3).contiguous()
    labels = torch.randint(0, 64, (B,))
    labels_d = labels.to(dev)
    model = Action_Recognition_Resnet50(args).to(dev).train()
    opt, _, _ = PT.build_optimizer(model, args)
    opt.zero_grad()

    def hip():
        loss, _ = ops.softmax_ce(model(x4), labels)
        loss.backward()
        opt.step(zero_grad=True)
        return loss
    h = stat(events_ms(hip, a.iters, a.batches, a.warmup))
    loss_hip = float(hip().detach())
    del model, opt
    torch.cuda.empty_cache()
    ref = nn_resnet50(64).to(dev).train()
    o1 = torch.optim.SGD(ref.convnet.parameters(), lr=args.lr_1, momentum=0.9)
    o2 = torch.optim.SGD(ref.fc.parameters(), lr=args.lr_2, momentum=0.9)

    def tor():
        o1.zero_grad()
        o2.zero_grad()
        loss = F.cross_entropy(ref(x), labels_d)
        loss.backward()
        o1.step()
        o2.step()
        return loss
    t = stat(events_ms(tor, a.iters, a.batches, a.warmup))
    out["step"] = {"batch": B, "frames": B * T, "hip_ms": h, "torch_gpu_ms": t, "torch_over_hip_time": t["median"] / h["median"],
                   "loss_hip": loss_hip, "loss_torch": float(tor().detach())}


def part_kernels(a, dev, out):
    import torch
    import litemkd_amd
    from litemkd_amd.ops import _p, _stream, _f32
    L = litemkd_amd.lib()
    F_, H, W, C = 64, 7, 7, 2048
    xs = [torch.randn(F_, H, W, C, device=dev) for _ in range(16)]
    res, it = {}, a.iters * 10
    for G in (1, 8):
        y = torch.empty(F_ // G, C, device=dev)
        dxs = [torch.empty_like(x) for x in xs]
        dy = torch.randn(F_ // G, C, device=dev)
        k = [0]

        def fwd():
            k[0] += 1
            L.call("lmkd_global_avgpool_fwd", _p(xs[k[0] % 16]), _p(y), F_, H, W, C, G, _stream())

        def bwd():
            k[0] += 1
            L.call("lmkd_global_avgpool_bwd", _p(dy), _p(dxs[k[0] % 16]), F_, H, W, C, G, _stream())
        nbytes = xs[0].numel() * 4 + y.numel() * 4
        for name, fn in (("fwd", fwd), ("bwd", bwd)):
            s = stat([1e3 * v for v in events_ms(fn, it, a.batches, a.warmup)])
            res["global_avgpool_%s_G%d_us" % (name, G)] = s
            res["global_avgpool_%s_G%d_bytes" % (name, G)] = nbytes
            res["global_avgpool_%s_G%d_fraction_of_achievable_hbm" % (name, G)] = nbytes / (s["median"] * 1e-6) / HBM_ACHIEVABLE
            res["global_avgpool_%s_G%d_fraction_of_peak_hbm" % (name, G)] = nbytes / (s["median"] * 1e-6) / HBM_PEAK
        del dxs
    for R_, Cc in ((8, 64), (8, 70), (8, 1000), (256, 1000)):
        lg = torch.randn(R_, Cc, device=dev)
        lab = torch.randint(0, Cc, (R_,), device=dev)
        o2, pred, g, rows = torch.empty(2, device=dev), torch.empty(R_, dtype=torch.int64, device=dev), torch.empty_like(lg), torch.empty(2 * R_, device=dev)

        def ce():
            L.call("lmkd_softmax_ce", _p(lg), _p(lab), None, _p(o2), _p(pred), _p(g), _p(rows), R_, Cc, _stream())
        res["softmax_ce_%dx%d_us" % (R_, Cc)] = stat([1e3 * v for v in events_ms(ce, it, a.batches, a.warmup)])
    n = 23508032 + 64 * 2048 + 64      # the parameters of Action_Recognition_Resnet50 at 64 classes
    p, gr, buf = (torch.randn(n, device=dev) for _ in range(3))

    def sgd():
        L.call("lmkd_sgd_momentum_step", _p(p), _p(gr), _p(buf), _f32(1e-6), _f32(0.9), n, 0, 1, _stream())
    s = stat([1e3 * v for v in events_ms(sgd, it, a.batches, a.warmup)])
    res["sgd_momentum_%d_us" % n] = s
    res["sgd_momentum_bytes"] = n * 4 * 6      # reads p, g, buf; writes p, g, buf
    res["sgd_momentum_fraction_of_achievable_hbm"] = n * 24 / (s["median"] * 1e-6) / HBM_ACHIEVABLE
    out["kernels"] = res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--part", choices=["extract", "step", "kernels"], required=True)
    p.add_argument("--iters", type=int, default=5, help="calls per timing (kernels: ten times as many)")
    p.add_argument("--batches", type=int, default=5, help="timings")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--dtype", default="fp32x3", choices=["fp32x3", "fp32h2", "fp32", "bf16"], help="arithmetic of the HIP convolutions")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import litemkd_amd
    from litemkd_amd import ops
    assert torch.cuda.is_available(), "pretrain_bench needs the GPU"
    litemkd_amd.lib().call("lmkd_device_check", 0)
    dev = torch.device("cuda", 0)
    if a.part != "kernels":      # the kernels part times fp32 tensors
        ops.set_conv_compute_dtype(a.dtype)
        if a.dtype == "bf16":
            ops.set_activation_dtype("bf16")
    torch.manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "part": a.part, "dtype": a.dtype,
           "timing": "%d timings of %d calls after %d warm-up calls; median, min, max" % (a.batches, a.iters * (10 if a.part == "kernels" else 1), a.warmup)}
    {"extract": part_extract, "step": part_step, "kernels": part_kernels}[a.part](a, dev, out)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
