"""STRM student benchmark (strm18_student + strm_res18_sup + strm_fc_2_sup_dist, 5-way 5-shot, 400 frames of 224^2 per episode) beside
the headline configuration (resnet18_2fc + TRX_2fcsup + fc_2_sup_dist), both on the path bench.py times: bench.py's arithmetic (fp32h2),
its schedule (schedule.Schedule.from_env(): merged trunk call, pipelined episodes), TL.make / PipelinedEpisodes / FusedOptimizer with an
optimizer step every tasks_per_batch episodes.  The two configurations are alternated and repeated inside ONE process, so the ratio does
not depend on the box or on what else runs on it; bench.py itself stays the ResNet-18 headline.

    python tools/strm_bench.py --steps 32 --warmup 6 --repeats 3 [--infer-steps 30] [--out profiles/strm_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o strm -- python tools/strm_bench.py --only strm --steps 4 --warmup 2 --repeats 1 --infer-steps 0
(the second form: per-kernel time and counts of a short run; tools/strm_bench.py --summarize DIR --episodes 6 tabulates them per episode)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    "strm": dict(model_backbone="strm18_student", model_classifier="strm_res18_sup", distill_name="strm_fc_2_sup_dist"),
    "headline": dict(model_backbone="resnet18_2fc", model_classifier="TRX_2fcsup", distill_name="fc_2_sup_dist"),
}


def run(a):
    import torch
    import litemkd_amd
    from litemkd_amd import ops, trainloop as TL
    from litemkd_amd.options import default_args
    from litemkd_amd.schedule import Schedule
    from mnv3_bench import _count_calls
    assert torch.cuda.is_available(), "strm_bench needs the GPU"
    dev = torch.device("cuda", 0)
    litemkd_amd.lib().call("lmkd_device_check", 0)
    sched = Schedule.from_env()
    sched.apply(arithmetic=False)
    ops.set_conv_compute_dtype("fp32h2")
    ops.set_activation_dtype("fp32")
    counter = _count_calls()
    names = [a.only] if a.only else ["strm", "headline"]
    runs = {}
    for name in names:
        cfg = default_args(shot=a.shot, device=dev, trans_dropout=0.1, training_iterations=10 ** 9, print_freq=10 ** 9, **CONFIGS[name])
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

    for name in names:
        train(runs[name], a.warmup)
        if a.infer_steps > 0:
            infer(runs[name], 2)
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for name in names:
            r = runs[name]
            c0, t0 = counter["n"], time.perf_counter()
            train(r, a.steps)
            torch.cuda.synchronize()
            r["train"].append(a.steps / (time.perf_counter() - t0))
            r["calls"].append((counter["n"] - c0) / a.steps)
            if a.infer_steps > 0:
                t0 = time.perf_counter()
                infer(r, a.infer_steps)
                torch.cuda.synchronize()
                r["infer"].append(a.infer_steps / (time.perf_counter() - t0))

    def stat(v):
        v = sorted(v)
        return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "runs": v} if v else None
    out = {"what": "training and inference episodes/s, 5-way %d-shot, %d frames of 224^2, fp32h2, schedule %s; configurations alternated %d times in one "
                   "process, %d timed episodes each (warm-up %d)" % (a.shot, 8 * 5 * (a.shot + 5),
                                                                     "merged+pipelined" if sched.pipeline_episodes else "two-call", a.repeats, a.steps, a.warmup),
           "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    for name in names:
        r = runs[name]
        out[name] = {"config": CONFIGS[name], "train_episodes_per_s": stat(r["train"]), "infer_episodes_per_s": stat(r["infer"]),
                     "library_calls_per_train_episode": r["calls"][-1] if r["calls"] else None,
                     "loss_last": float(r["last"][0]) if r["last"] is not None else None}
    if len(names) == 2:
        out["train_ratio_strm_over_headline"] = out["strm"]["train_episodes_per_s"]["median"] / out["headline"]["train_episodes_per_s"]["median"]
        if a.infer_steps > 0:
            out["infer_ratio_strm_over_headline"] = out["strm"]["infer_episodes_per_s"]["median"] / out["headline"]["infer_episodes_per_s"]["median"]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=32)
    p.add_argument("--warmup", type=int, default=6)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--infer-steps", type=int, default=30)
    p.add_argument("--shot", type=int, default=5)
    p.add_argument("--only", choices=sorted(CONFIGS), default=None, help="time one configuration alone (kernel traces)")
    p.add_argument("--out", default=None)
    p.add_argument("--summarize", default=None, help="directory of a rocprofv3 --kernel-trace --stats run")
    p.add_argument("--episodes", type=int, default=6, help="--summarize: training episodes the traced run ran (warmup + steps)")
    a = p.parse_args()
    if a.summarize:
        from mnv3_bench import summarize
        summarize(a.summarize, a.episodes)
    else:
        run(a)


if __name__ == "__main__":
    main()
