"""OTAM head benchmark, three measurements in ONE process:

(a) the head alone - forward + backward of ops.OtamFn at the workload's shape (5-way 5-shot, 25 queries, seq_len 8, D 2048; case 4 of
    tests/_otam_ref.py), HIP events around batches of iterations after a warm-up - beside the same computation written in torch
    (tests/_otam_ref.otam, the reference's way of doing it: hundreds of small launches per call) run by torch on the same GPU;
(b) training and inference episodes/s of resnet18_student + otam + KD (teacher test_teacher_otam) beside resnet18_student + e_dist + KD
    (teacher e_dist) on the path bench.py times (fp32h2, schedule.Schedule.from_env(), TL.make / PipelinedEpisodes / FusedOptimizer),
    alternated and repeated: the two differ only in the parameter-free head, so the difference is the head's cost inside the schedule;
(c) library calls and kernel launches per head call, from the tool's own count of lib().call (not a profiler run) and the launches each
    entry point makes (include/lmkd.h).

    python tools/otam_bench.py [--iters 200] [--batches 5] [--steps 32] [--warmup 6] [--repeats 3] [--out profiles/otam_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = {
    "otam": dict(model_backbone="resnet18_student", model_classifier="otam", model_teacher="test_teacher_otam", distill_name="KD"),
    "e_dist": dict(model_backbone="resnet18_student", model_classifier="e_dist", model_teacher="e_dist", distill_name="KD"),
}
LAUNCHES = {"lmkd_otam_frame_dist_fwd": 3, "lmkd_otam_align_fwd": 1, "lmkd_otam_align_bwd": 1, "lmkd_otam_frame_dist_bwd": 3}


def stat(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "runs": v} if v else None


def _events_us(fn, iters, batches, warmup):
    """microseconds per call: `batches` timings of `iters` back-to-back calls between two HIP events, after `warmup` calls"""
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
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return out


def head_alone(a, dev, counter):
    import torch
    import _otam_ref as R
    from litemkd_amd import _lib, ops
    way, L, sup, lab, qry = R.case_data(4)
    s, q = sup.to(dev).requires_grad_(), qry.to(dev).requires_grad_()
    plan = ops.ClassPlan(lab.to(dev), way, cpu_copy=lab)
    w = R.fixture_weights((qry.shape[0], way)).to(dev)
    lab_d = lab.to(dev)

    def hip():
        s.grad = q.grad = None
        ops.OtamFn.apply(s, q, plan)[0].backward(w)

    def torch_gpu():
        s.grad = q.grad = None
        R.otam(s, lab_d, q, way)[0].backward(w)
    names = []
    orig = _lib._Lib.call

    def spy(self, name, *args):
        names.append(name)
        return orig(self, name, *args)
    _lib._Lib.call = spy
    try:
        c0 = counter["n"]
        hip()
        calls = counter["n"] - c0
    finally:
        _lib._Lib.call = orig
    hip()
    g_hip = (s.grad.clone(), q.grad.clone())
    torch_gpu()
    err = max(float((g_hip[0] - s.grad).abs().max()) / float(s.grad.abs().max()), float((g_hip[1] - q.grad).abs().max()) / float(q.grad.abs().max()))
    t_hip = _events_us(hip, a.iters, a.batches, 20)
    t_torch = _events_us(torch_gpu, max(1, a.iters // 10), a.batches, 3)
    return {"shape": {"way": way, "Ns": sup.shape[0], "Nq": qry.shape[0], "seq_len": L, "D": sup.shape[2]},
            "hip_us_per_fwd_bwd": stat(t_hip), "torch_gpu_us_per_fwd_bwd": stat(t_torch),
            "iterations_per_timing": {"hip": a.iters, "torch": max(1, a.iters // 10)}, "timings": a.batches,
            "torch_over_hip": stat(t_torch)["median"] / stat(t_hip)["median"],
            "gradient_max_abs_difference_hip_vs_torch_gpu_over_max": err,
            "library_calls_per_fwd_bwd": calls, "library_calls": names,
            "kernel_launches_per_fwd_bwd": sum(LAUNCHES[n] for n in names), "launches_forward": sum(LAUNCHES[n] for n in names if n.endswith("_fwd")),
            "launches_backward": sum(LAUNCHES[n] for n in names if n.endswith("_bwd"))}


def episodes(a, dev, counter):
    import torch
    from litemkd_amd import ops, trainloop as TL
    from litemkd_amd.options import default_args
    from litemkd_amd.schedule import Schedule
    sched = Schedule.from_env()
    sched.apply(arithmetic=False)
    ops.set_conv_compute_dtype("fp32h2")
    ops.set_activation_dtype("fp32")
    runs = {}
    for name, names in CONFIGS.items():
        cfg = default_args(shot=a.shot, device=dev, trans_dropout=0.1, training_iterations=10 ** 9, print_freq=10 ** 9, **names)
        torch.manual_seed(1234)
        student, teacher, src, distiller, accuracy, _, opt, sch = TL.make(cfg, base_seed=2024)
        pool = [src.episode(e) for e in range(2)]
        pipe = TL.PipelinedEpisodes(student, teacher, distiller, accuracy, cfg) if sched.pipeline_episodes else None
        runs[name] = dict(cfg=cfg, student=student, teacher=teacher, distiller=distiller, accuracy=accuracy, opt=opt, sch=sch, pool=pool, pipe=pipe,
                          it=0, train=[], infer=[], calls=[], last=None)

    def train(r, n):
        cfg, pipe, every = r["cfg"], r["pipe"], r["cfg"].tasks_per_batch
        for i in range(n):
            r["it"] += 1
            ep = r["pool"][i % len(r["pool"])]
            if pipe is not None:
                r["last"] = pipe.push(ep) or r["last"]
            else:
                r["last"] = TL.train_task(ep, r["student"], r["teacher"], r["distiller"], r["accuracy"], cfg)
            if (r["it"] + 1) % every == 0:
                if pipe is not None:
                    r["last"] = pipe.flush() or r["last"]
                r["opt"].step()
                r["opt"].zero_grad()
            r["sch"].step()
        if pipe is not None:
            r["last"] = pipe.flush() or r["last"]

    def infer(r, n):
        r["student"].eval()
        with torch.no_grad():
            for i in range(n):
                ep = r["pool"][i % len(r["pool"])]
                r["student"](ep["support_set"][0], ep["support_labels"][0], ep["target_set"][0])
        r["student"].train()
    for r in runs.values():
        train(r, a.warmup)
        infer(r, 2)
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for r in runs.values():
            c0, t0 = counter["n"], time.perf_counter()
            train(r, a.steps)
            torch.cuda.synchronize()
            r["train"].append(a.steps / (time.perf_counter() - t0))
            r["calls"].append((counter["n"] - c0) / a.steps)
            t0 = time.perf_counter()
            infer(r, a.infer_steps)
            torch.cuda.synchronize()
            r["infer"].append(a.infer_steps / (time.perf_counter() - t0))
    out = {"what": "training and inference episodes/s, 5-way %d-shot, %d frames of 224^2, fp32h2, schedule %s; configurations alternated %d times, %d "
                   "timed training / %d inference episodes each (warm-up %d)" % (
                       a.shot, 8 * 5 * (a.shot + 5), "merged+pipelined" if sched.pipeline_episodes else "two-call", a.repeats, a.steps, a.infer_steps,
                       a.warmup)}
    for name, r in runs.items():
        out[name] = {"config": CONFIGS[name], "train_episodes_per_s": stat(r["train"]), "infer_episodes_per_s": stat(r["infer"]),
                     "library_calls_per_train_episode": r["calls"][-1], "loss_last": float(r["last"][0]) if r["last"] is not None else None}
    t = {k: out[k]["train_episodes_per_s"]["median"] for k in runs}
    i = {k: out[k]["infer_episodes_per_s"]["median"] for k in runs}
    out["train_ms_per_episode_otam_minus_e_dist"] = 1e3 / t["otam"] - 1e3 / t["e_dist"]
    out["infer_ms_per_episode_otam_minus_e_dist"] = 1e3 / i["otam"] - 1e3 / i["e_dist"]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200, help="(a): calls per timing of the HIP head (the torch version runs a tenth of them)")
    p.add_argument("--batches", type=int, default=5, help="(a): timings")
    p.add_argument("--steps", type=int, default=32)
    p.add_argument("--warmup", type=int, default=6)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--infer-steps", type=int, default=30)
    p.add_argument("--shot", type=int, default=5)
    p.add_argument("--skip-episodes", action="store_true", help="(a) and (c) only")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import litemkd_amd
    from mnv3_bench import _count_calls
    assert torch.cuda.is_available(), "otam_bench needs the GPU"
    dev = torch.device("cuda", 0)
    litemkd_amd.lib().call("lmkd_device_check", 0)
    counter = _count_calls()
    out = {"device": torch.cuda.get_device_name(0), "head_alone": head_alone(a, dev, counter)}
    if not a.skip_episodes:
        out["episodes"] = episodes(a, dev, counter)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
