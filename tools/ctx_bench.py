"""CTX head benchmark, measurements in ONE process:

(a) the head alone at the workload's shape (5-way 5-shot, 25 queries, seq_len 8, 2048 -> 1152; case 8 of tests/_ctx_ref.py) - forward +
    backward of ops.CtxLogitsFn, HIP events around batches of iterations after a warm-up - beside the same arithmetic written in torch
    (tests/_ctx_ref.ctx_head) run by torch on the same GPU, and beside ops.TRXLogitsFn with frame pairs on the same features (k / v
    projections 4096 -> 1152 with seeded weights);
(b) training and inference episodes/s of resnet18_student + CTX + KD (teacher test_teacher_ctx, a seeded checkpoint written to a
    temporary directory) beside the headline configuration bench.py times (resnet18_2fc + TRX_2fcsup + fc_2_sup_dist) on the same path
    (fp32h2, schedule.Schedule.from_env(), TL.make / PipelinedEpisodes / FusedOptimizer), alternated and repeated;
(c) library calls and kernel launches per head call, from the tool's own count of lib().call (not a profiler run) and the launches each
    entry point makes (include/lmkd.h).

    python tools/ctx_bench.py [--iters 200] [--batches 5] [--steps 32] [--warmup 6] [--repeats 3] [--out profiles/ctx_bench.json]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = {
    "ctx": dict(model_backbone="resnet18_student", model_classifier="CTX", model_teacher="test_teacher_ctx", distill_name="KD"),
    "headline": dict(model_backbone="resnet18_2fc", model_classifier="TRX_2fcsup", model_teacher="test_teacher_TRX_2fcsup_fixed",
                     distill_name="fc_2_sup_dist"),
}
LAUNCHES = {"lmkd_ctx_attend_bwd": 2}      # every other entry point the heads call is one launch


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
    import _ctx_ref as R
    from litemkd_amd import _lib, ops
    d = R.case_data(8)
    way, L = d["way"], d["L"]
    Ns, _, Din = d["sup"].shape
    Nq, D = d["qry"].shape[0], d["wk"].shape[0]
    leaves = {k: d[k].to(dev).requires_grad_() for k in ("sup", "qry") + R.PARAMS}
    pe = d["pe"][:L].contiguous().to(dev)
    plan = ops.ClassPlan(d["lab"].to(dev), way, cpu_copy=d["lab"])
    w = R.fixture_weights((Nq, way)).to(dev)
    lab_d = d["lab"].to(dev)
    g = torch.Generator().manual_seed(5)
    pair = {k: ((torch.rand(*shape, generator=g) * 2 - 1) / (2 * Din) ** 0.5).to(dev).requires_grad_()
            for k, shape in (("wk", (D, 2 * Din)), ("bk", (D,)), ("wv", (D, 2 * Din)), ("bv", (D,)))}

    def zero():
        for t in list(leaves.values()) + list(pair.values()):
            t.grad = None

    def hip():
        zero()
        ops.CtxLogitsFn.apply(leaves["sup"], leaves["qry"], *(leaves[k] for k in R.PARAMS), pe, None, plan).backward(w)

    def torch_gpu():
        zero()
        R.ctx_head(leaves["sup"], lab_d, leaves["qry"], way, *(leaves[k] for k in R.PARAMS), pe).backward(w)

    def trx_pairs():
        zero()
        ops.TRXLogitsFn.apply(leaves["sup"], leaves["qry"], pair["wk"], pair["bk"], pair["wv"], pair["bv"], leaves["gamma"], leaves["beta"], pe,
                              None, plan).backward(w)

    def count(fn):
        names = []
        orig = _lib._Lib.call

        def spy(self, name, *args):
            names.append(name)
            return orig(self, name, *args)
        _lib._Lib.call = spy
        try:
            fn()
        finally:
            _lib._Lib.call = orig
        return names
    hip()
    g_hip = (leaves["sup"].grad.clone(), leaves["qry"].grad.clone())
    torch_gpu()
    err = max(float((g_hip[0] - leaves["sup"].grad).abs().max()) / float(leaves["sup"].grad.abs().max()),
              float((g_hip[1] - leaves["qry"].grad).abs().max()) / float(leaves["qry"].grad.abs().max()))
    names, names_trx = count(hip), count(trx_pairs)
    nl = lambda ns: sum(LAUNCHES.get(n, 1) for n in ns)      # noqa: E731
    fwd_names = names[:names.index("lmkd_ctx_attend_fwd") + 1]
    t_hip = _events_us(hip, a.iters, a.batches, 20)
    t_trx = _events_us(trx_pairs, a.iters, a.batches, 20)
    t_torch = _events_us(torch_gpu, max(1, a.iters // 10), a.batches, 3)
    return {"shape": {"way": way, "Ns": Ns, "Nq": Nq, "seq_len": L, "Din": Din, "Dk": D},
            "hip_us_per_fwd_bwd": stat(t_hip), "torch_gpu_us_per_fwd_bwd": stat(t_torch), "trx_pairs_hip_us_per_fwd_bwd": stat(t_trx),
            "iterations_per_timing": {"hip": a.iters, "trx_pairs": a.iters, "torch": max(1, a.iters // 10)}, "timings": a.batches,
            "torch_over_hip": stat(t_torch)["median"] / stat(t_hip)["median"],
            "trx_pairs_over_ctx": stat(t_trx)["median"] / stat(t_hip)["median"],
            "gradient_max_abs_difference_hip_vs_torch_gpu_over_max": err,
            "library_calls": names, "kernel_launches_per_fwd_bwd": nl(names), "launches_forward": nl(fwd_names),
            "launches_backward": nl(names) - nl(fwd_names), "trx_pairs_kernel_launches_per_fwd_bwd": nl(names_trx)}


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
    tmp = tempfile.mkdtemp(prefix="ctx_bench_")
    torch.manual_seed(77)
    from litemkd_amd.model import classifiers as C
    ckpt = os.path.join(tmp, "two_ctx.pt")
    torch.save({"model_state_dict": {"bracnch." + k: v.clone() for k, v in C.CTX(default_args(device=torch.device("cpu"))).state_dict().items()}}, ckpt)
    for name, names in CONFIGS.items():
        cfg = default_args(shot=a.shot, device=dev, trans_dropout=0.1, training_iterations=10 ** 9, print_freq=10 ** 9,
                           teacher_checkpoint=ckpt if name == "ctx" else None, **names)
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
    out["train_ms_per_episode_ctx_minus_headline"] = 1e3 / t["ctx"] - 1e3 / t["headline"]
    out["infer_ms_per_episode_ctx_minus_headline"] = 1e3 / i["ctx"] - 1e3 / i["headline"]
    shutil.rmtree(tmp, ignore_errors=True)
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
    assert torch.cuda.is_available(), "ctx_bench needs the GPU"
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
