"""Training rate of the headline student (resnet18_2fc + TRX_2fcsup + fc_2_sup_dist, 5-way 5-shot, 400 frames of 224^2 per episode) with
frame pairs alone (temp_set [2], what bench.py times) and with pairs plus triples (temp_set [2, 3]: student heads and frozen teacher head
each hold a second TemporalCrossTransformer over the 56 frame triples).  Both on the path bench.py times - its arithmetic (fp32h2), its
schedule (schedule.Schedule.from_env()), TL.make / PipelinedEpisodes / FusedOptimizer with an optimizer step every tasks_per_batch
episodes - alternated and repeated inside ONE process, so the ratio does not depend on the box or on what else runs on it.

    python tools/temp_set_bench.py --steps 32 --warmup 6 --repeats 3 [--out profiles/temp_set_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"pairs": [2], "pairs_triples": [2, 3]}


def run(a):
    import torch
    import litemkd_amd
    from litemkd_amd import ops, trainloop as TL
    from litemkd_amd.options import default_args
    from litemkd_amd.schedule import Schedule
    assert torch.cuda.is_available(), "temp_set_bench needs the GPU"
    dev = torch.device("cuda", 0)
    litemkd_amd.lib().call("lmkd_device_check", 0)
    sched = Schedule.from_env()
    sched.apply(arithmetic=False)
    ops.set_conv_compute_dtype("fp32h2")
    ops.set_activation_dtype("fp32")
    runs = {}
    for name, ts in CONFIGS.items():
        cfg = default_args(shot=a.shot, device=dev, trans_dropout=0.1, training_iterations=10 ** 9, print_freq=10 ** 9, temp_set=ts)
        torch.manual_seed(1234)
        student, teacher, src, distiller, accuracy, _, opt, sch = TL.make(cfg, base_seed=2024)
        pool = [src.episode(e) for e in range(2)]
        pipe = TL.PipelinedEpisodes(student, teacher, distiller, accuracy, cfg) if sched.pipeline_episodes else None
        runs[name] = dict(cfg=cfg, student=student, teacher=teacher, distiller=distiller, accuracy=accuracy, opt=opt, sch=sch, pool=pool, pipe=pipe,
                          it=0, train=[], last=None)

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

    for r in runs.values():
        train(r, a.warmup)
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for r in runs.values():
            t0 = time.perf_counter()
            train(r, a.steps)
            torch.cuda.synchronize()
            r["train"].append(a.steps / (time.perf_counter() - t0))

    def stat(v):
        v = sorted(v)
        return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "runs": v}
    out = {"what": "training episodes/s, 5-way %d-shot, %d frames of 224^2, fp32h2, schedule %s; temp_set [2] and [2, 3] alternated %d times in one "
                   "process, %d timed episodes each (warm-up %d)" % (a.shot, 8 * 5 * (a.shot + 5),
                                                                     "merged+pipelined" if sched.pipeline_episodes else "two-call", a.repeats, a.steps, a.warmup),
           "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    for name, r in runs.items():
        out[name] = {"temp_set": CONFIGS[name], "train_episodes_per_s": stat(r["train"]),
                     "head_parameters": sum(p.numel() for p in r["student"].classifier.parameters()),
                     "loss_last": float(r["last"][0]) if r["last"] is not None else None}
    out["train_ratio_pairs_triples_over_pairs"] = out["pairs_triples"]["train_episodes_per_s"]["median"] / out["pairs"]["train_episodes_per_s"]["median"]
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
    p.add_argument("--shot", type=int, default=5)
    p.add_argument("--out", default=None)
    run(p.parse_args())


if __name__ == "__main__":
    main()
