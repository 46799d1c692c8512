"""Attention-map benchmark, one MI355X, ONE process, HIP events around batches of launches after a warm-up, each kernel
alternated with the torch expression of the same arithmetic on the same GPU:

(a) lmkd_gradcam_fwd, both modes, at 400 frames of 7 x 7 x 512 and 7 x 7 x 2048: microseconds per launch, the bytes it must move
    (2 F HW C 4 for A and dA + the outputs) and its share of the HBM bandwidth a streaming kernel reaches (tools/pretrain_bench.py's figure);
(b) lmkd_cam_overlay_u8 at 200 frames of 224 x 224 from 7 x 7 maps, beside torch's bilinear interpolate + table gather + float blend
    (the torch form is NOT bit-identical to Pillow; it is the cost of the same steps);
(c) a whole cam.grad_cam call (5-way 5-shot, 5 queries per class, 8 frames of 224 x 224, resnet18_2fc + TRX_2fcsup) beside the plain
    no-grad eval forward of the same episode.

    python tools/cam_bench.py [--seconds 1.0] [--batches 5] [--out profiles/cam_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12      # bytes / s a streaming kernel reaches on the MI355X (8e12 peak): tools/pretrain_bench.py


def stat(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "spread": (v[-1] - v[0]) / v[len(v) // 2], "runs": v}


def _time_us(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def alternate(fns, seconds, batches, warmup=10):
    """{name: fn} -> {name: stat of microseconds per call}: every fn warmed up, its iteration count sized to fill `seconds` over all
    batches, then the batches of the fns alternated"""
    iters = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn()
        one = _time_us(fn, 5)
        iters[name] = max(3, int(seconds * 1e6 / one / batches))
    runs = {name: [] for name in fns}
    for _ in range(batches):
        for name, fn in fns.items():
            runs[name].append(_time_us(fn, iters[name]))
    return {name: dict(stat(v), iterations_per_timing=iters[name]) for name, v in runs.items()}


def torch_gradcam(A, dA, mode):
    import torch
    F, C = A.shape[0], A.shape[-1]
    a, d = A.reshape(F, -1, C), dA.reshape(F, -1, C)
    w = d.mean(1)
    raw = torch.relu(torch.einsum("fc,fpc->fp", w, a) if mode == 0 else (d * a).sum(-1))
    mn, mx = raw.amin(1, keepdim=True), raw.amax(1, keepdim=True)
    return w, raw, (raw - mn) / (1e-7 + (mx - mn))


def kernel_cases(a, dev):
    import torch
    from litemkd_amd import ops
    out = {}
    for C in (512, 2048):
        F, h = 400, 7
        g = torch.Generator(device=dev).manual_seed(C)
        A = torch.randn(F, h, h, C, generator=g, device=dev)
        dA = torch.randn(F, h, h, C, generator=g, device=dev)
        nbytes = 2 * F * h * h * C * 4 + F * C * 4 + 2 * F * h * h * 4
        for mode, name in ((0, "gradcam"), (1, "hirescam")):
            r = alternate({"hip": lambda: ops.gradcam(A, dA, mode), "torch": lambda: torch_gradcam(A, dA, mode)}, a.seconds, a.batches)
            r["bytes"] = nbytes
            r["hip_fraction_of_achievable_hbm"] = nbytes / (r["hip"]["median"] * 1e-6) / HBM_ACHIEVABLE
            r["torch_over_hip"] = r["torch"]["median"] / r["hip"]["median"]
            out["%s_400x7x7x%d" % (name, C)] = r
    return out


def overlay_case(a, dev):
    import torch
    import torch.nn.functional as Fn
    from litemkd_amd import ops
    F, h, S = 200, 7, 224
    g = torch.Generator(device=dev).manual_seed(1)
    cam = torch.rand(F, h, h, generator=g, device=dev)
    frames = torch.randint(0, 256, (F, S, S, 3), generator=g, device=dev, dtype=torch.uint8)
    lut = ops.jet_lut(dev)
    lut_f = lut.float()

    def torch_form():
        q = (cam * 255 + 0.5).clamp(0, 255).floor()
        up = Fn.interpolate(q[:, None], size=(S, S), mode="bilinear", align_corners=False)[:, 0].round().long()
        return ((lut_f[up] * 128 + frames.float() * 128 + 128) / 256).to(torch.uint8)
    r = alternate({"hip": lambda: ops.cam_overlay(cam, frames, (S, S), lut=lut), "torch": torch_form}, a.seconds, a.batches)
    r["bytes"] = F * S * S * 3 * 2 + F * h * h * 4
    r["hip_fraction_of_achievable_hbm"] = r["bytes"] / (r["hip"]["median"] * 1e-6) / HBM_ACHIEVABLE
    r["torch_over_hip"] = r["torch"]["median"] / r["hip"]["median"]
    return r


def whole_call(a, dev):
    import torch
    from litemkd_amd import cam, trainloop as TL
    from litemkd_amd.model.model_select import Student
    from litemkd_amd.options import default_args
    args = default_args(device=dev, query_per_class_test=5)
    torch.manual_seed(3)
    student = Student(args).to(dev).eval()
    ep = TL.SyntheticEpisodes(args, base_seed=9, device=dev, train=False).episode(0)
    ci, ti, _, _, cl, _, _, _ = TL.prepare_task(ep, dev)

    def plain():
        with torch.no_grad():
            student(ci, cl, ti)
    r = alternate({"plain_eval_forward": plain, "grad_cam": lambda: cam.grad_cam(student, ci, cl, ti)}, a.seconds * 3, a.batches, warmup=3)
    r["grad_cam_over_plain"] = r["grad_cam"]["median"] / r["plain_eval_forward"]["median"]
    r["what"] = "5-way 5-shot, 5 queries per class, 400 frames of 224^2, resnet18_2fc + TRX_2fcsup, library default arithmetic; microseconds per call"
    return r


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seconds", type=float, default=1.0, help="timed launches per kernel fill about this long")
    p.add_argument("--batches", type=int, default=5)
    p.add_argument("--skip-call", action="store_true", help="(a) and (b) only")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import litemkd_amd
    assert torch.cuda.is_available(), "cam_bench needs the GPU"
    dev = torch.device("cuda", 0)
    litemkd_amd.lib().call("lmkd_device_check", 0)
    out = {"device": torch.cuda.get_device_name(0), "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "unit": "microseconds per launch",
           "gradcam": kernel_cases(a, dev), "overlay_200x224x224_from_7x7": overlay_case(a, dev)}
    if not a.skip_call:
        out["whole_call"] = whole_call(a, dev)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
