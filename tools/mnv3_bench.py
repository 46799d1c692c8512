"""MobileNetV3-Large student benchmark (moblienetv3_fc2 + TRX_2fcsup + fc_2_sup_dist, 5-way 5-shot, 400 frames of 224^2 per episode):
training episodes/s on the same TL.make / train_task / FusedOptimizer path bench.py times, inference episodes/s (student forward,
eval mode, no grad), and library calls per training episode.  bench.py itself stays the ResNet-18 headline.

    python tools/mnv3_bench.py --steps 30 --warmup 5 [--infer-steps 30] [--out profiles/mnv3_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o mnv3 -- python tools/mnv3_bench.py --steps 4 --warmup 2 --infer-steps 0
(the second form: per-kernel time and counts of a short run; tools/mnv3_bench.py --summarize DIR --episodes 6 tabulates them per episode)."""
import argparse
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _count_calls():
    """count the C-ABI calls (each launches one or more kernels) by wrapping _Lib.call"""
    from litemkd_amd import _lib
    counter = {"n": 0}
    orig = _lib._Lib.call

    def call(self, name, *args):
        counter["n"] += 1
        return orig(self, name, *args)
    _lib._Lib.call = call
    return counter


def run(a):
    import torch
    import litemkd_amd
    from litemkd_amd import trainloop as TL
    from litemkd_amd import ops
    from litemkd_amd.options import default_args
    assert torch.cuda.is_available(), "mnv3_bench needs the GPU"
    dev = torch.device("cuda", 0)
    litemkd_amd.lib().call("lmkd_device_check", 0)
    ops.reset_compute_dtypes()
    cfg = default_args(shot=a.shot, device=dev, trans_dropout=0.1, training_iterations=10 ** 9, print_freq=10 ** 9,
                       model_backbone="moblienetv3_fc2", model_classifier="TRX_2fcsup", distill_name="fc_2_sup_dist")
    torch.manual_seed(1234)
    student, teacher, src, distiller, accuracy, _, opt, sch = TL.make(cfg, base_seed=2024)
    pool = [src.episode(e) for e in range(2)]
    counter = _count_calls()
    every = cfg.tasks_per_batch

    def train(n, it0):
        last = None
        for i in range(n):
            last = TL.train_task(pool[i % len(pool)], student, teacher, distiller, accuracy, cfg)
            if (it0 + i + 1) % every == 0:
                opt.step()
                opt.zero_grad()
            sch.step()
        return last

    train(a.warmup, 0)
    torch.cuda.synchronize()
    c0 = counter["n"]
    t0 = time.perf_counter()
    last = train(a.steps, a.warmup)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    calls = (counter["n"] - c0) / max(1, a.steps)
    out = {"workload": "moblienetv3_fc2 + TRX_2fcsup + fc_2_sup_dist, 5-way %d-shot, %d frames of 224^2" % (a.shot, 8 * 5 * (a.shot + 5)),
           "train_episodes_per_s": a.steps / dt, "train_ms_per_episode": 1e3 * dt / a.steps, "library_calls_per_train_episode": calls,
           "steps": a.steps, "warmup": a.warmup, "loss_last": float(last[0]) if last is not None else None,
           "gemm_arithmetic": "lmkd_gemm_f32 default mode", "device": torch.cuda.get_device_name(0)}
    if a.infer_steps > 0:
        student.eval()
        with torch.no_grad():
            def infer(n):
                for i in range(n):
                    ep = pool[i % len(pool)]
                    student(ep["support_set"][0], ep["support_labels"][0], ep["target_set"][0])
            infer(2)
            torch.cuda.synchronize()
            c0 = counter["n"]
            t0 = time.perf_counter()
            infer(a.infer_steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        out.update({"infer_episodes_per_s": a.infer_steps / dt, "infer_ms_per_episode": 1e3 * dt / a.infer_steps,
                    "library_calls_per_infer_episode": (counter["n"] - c0) / a.infer_steps})
        student.train()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def summarize(d, episodes):
    """per-kernel launches and time of a rocprofv3 --kernel-trace run (its rocpd database, or the --stats CSV), per training episode"""
    import csv
    import sqlite3
    fam = {}
    dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
    if dbs:
        for p in dbs:
            con = sqlite3.connect(p)
            for name, n, t, mx in con.execute("select name, count(*), sum(duration), max(duration) from kernels group by name"):
                name = name.split("(")[0].replace("void ", "").strip()
                e = fam.setdefault(name, [0, 0.0, 0.0])
                e[0] += n
                e[1] += float(t)
                e[2] = max(e[2], float(mx))
    else:
        for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(p) as f:
                for r in csv.DictReader(f):
                    e = fam.setdefault(r["Name"].split("(")[0].replace("void ", "").strip(), [0, 0.0, 0.0])
                    e[0] += int(r["Calls"])
                    e[1] += float(r["TotalDurationNs"])
                    e[2] = max(e[2], float(r["MaxNs"]))
    tot = sum(v[1] for v in fam.values()) or 1.0
    print("%-72s %9s %11s %9s %6s" % ("kernel (per training episode)", "launches", "ms", "max us", "share"))
    for k, (n, t, mx) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
        print("%-72s %9.1f %11.3f %9.1f %5.1f%%" % (k[:72], n / episodes, t / 1e6 / episodes, mx / 1e3, 100 * t / tot))
    print("all kernels: %.1f launches, %.3f ms of kernel time per episode (%d episodes traced)"
          % (sum(v[0] for v in fam.values()) / episodes, tot / 1e6 / episodes, episodes))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--infer-steps", type=int, default=30)
    p.add_argument("--shot", type=int, default=5)
    p.add_argument("--out", default=None)
    p.add_argument("--summarize", default=None, help="directory of a rocprofv3 --kernel-trace --stats run")
    p.add_argument("--episodes", type=int, default=6, help="--summarize: training episodes the traced run ran (warmup + steps)")
    a = p.parse_args()
    if a.summarize:
        summarize(a.summarize, a.episodes)
    else:
        run(a)


if __name__ == "__main__":
    main()
