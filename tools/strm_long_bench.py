"""STRM students on clips of 8 / 12 / 16 frames: the token MLP (the 8-frame kernels against the family templated on the clip length), the
patch-distance forward (one-wave kernel against the LDS-tiled kernel, ops.set_patchdist_tiled(0) / (1)), and whole training / inference
episodes of the STRM student beside the headline student at each clip length.  Everything runs in ONE process, the variants of a group
alternate, and every figure is the min - median - max over the repeats (DESIGN.md 24 quotes the file this writes).

    python tools/strm_long_bench.py [--parent-lib PATH] [--out profiles/strm_long_bench.json] [--episodes-only | --kernels-only]

Kernel rows: `batch` back-to-back launches between two device events, per-launch microseconds.  The library is called through ctypes on
preallocated tensors, so a launch costs the host less than the kernel runs.  Bytes are what the operator must move (computed from the
shapes below), `copy_fraction` is the operator's bytes per second over those of torch's plain copy of the same number of bytes, measured
in the same alternation.

--parent-lib PATH: a liblmkd_hip.so built from the parent commit.  It is loaded beside the tree's library; the 8-frame outputs of the
token MLP (forward, backward) and of the patch distance must be bit-identical between the two builds, and the parent's patch-distance
kernel is timed at 12 and 16 frames as the reference for the rows of this build."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "strm": dict(model_backbone="strm18_student", model_classifier="strm_res18_sup", distill_name="strm_fc_2_sup_dist"),
    "headline": dict(model_backbone="resnet18_2fc", model_classifier="TRX_2fcsup", distill_name="fc_2_sup_dist"),
}
LENGTHS = (8, 12, 16)


def stat(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def _bind(cdll, protos, name):
    fn = getattr(cdll, name)
    fn.restype, fn.argtypes = protos[name]
    return fn


def kernels(a, out):
    import torch
    import litemkd_amd
    from litemkd_amd import _lib, ops
    dev = torch.device("cuda", 0)
    lib = litemkd_amd.lib()
    protos = lib.protos
    names = ("lmkd_strm_tokmlp_fwd", "lmkd_strm_tokmlp_bwd", "lmkd_strm_patchdist_fwd", "lmkd_strm_tokmlp_parts")
    own = {n: _bind(lib.cdll, protos, n) for n in names}
    parent = None
    if a.parent_lib:
        pc = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent = {n: _bind(pc, _lib.parse_header(), n) for n in names}
    p, st = ops._p, ops._stream()
    g = torch.Generator().manual_seed(7)

    def timed(fn, batch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / batch

    def alternate(variants, batch):
        """variants {name: fn} -> {name: [us per launch] * repeats}; one warm-up batch each, then the variants take turns"""
        for fn in variants.values():
            timed(fn, max(2, batch // 4))
        runs = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                runs[k].append(timed(fn, batch))
        return runs

    # ---- token MLP at V = 50, D = 2048 ------------------------------------------------------------------------------------------------
    V, D = 50, 2048
    tok, variants, check = {}, {}, {}
    for L in LENGTHS:
        t = {k: torch.randn(s, generator=g).to(dev) for k, s in (("x", (V, L, D)), ("pe", (L, D)), ("dy", (V, L, D)), ("w1", (L, L)), ("b1", (L,)),
                                                                ("w2", (L, L)), ("b2", (L,)))}
        nt = 2 * L * L + 2 * L
        t.update(xp=torch.empty(V, L, D, device=dev), y=torch.empty(V, L, D, device=dev), dx=torch.empty(V, L, D, device=dev),
                 part=torch.empty(own["lmkd_strm_tokmlp_parts"](V, D), nt, device=dev), dp=torch.empty(nt, device=dev))
        nbytes = 3 * V * L * D * 4      # forward: x in, xp and y out; backward: dy and xp in, dx out (tables, weights and partial rows are < 1 %)
        src, dst = torch.empty(nbytes // 8, device=dev), torch.empty(nbytes // 8, device=dev)
        tok[L] = (t, nbytes)

        def fwd(f=own, t=t, L=L):
            rc = f["lmkd_strm_tokmlp_fwd"](p(t["x"]), p(t["pe"]), None, p(t["w1"]), p(t["b1"]), p(t["w2"]), p(t["b2"]), p(t["xp"]), p(t["y"]), None, V, L, D, st)
            assert rc == 0, lib.last_error()

        def bwd(f=own, t=t, L=L):
            rc = f["lmkd_strm_tokmlp_bwd"](p(t["dy"]), p(t["xp"]), None, p(t["w1"]), p(t["b1"]), p(t["w2"]), p(t["dx"]), p(t["part"]), p(t["dp"]), V, L, D, st)
            assert rc == 0, lib.last_error()
        variants["fwd L=%d" % L], variants["bwd L=%d" % L] = fwd, bwd
        variants["copy L=%d" % L] = lambda src=src, dst=dst: dst.copy_(src)
        if L == 8 and parent:
            check["tok"] = (fwd, bwd, t)
    runs = alternate(variants, a.batch)
    rows = {}
    for L in LENGTHS:
        nbytes = tok[L][1]
        copy = stat(runs["copy L=%d" % L])
        for d in ("fwd", "bwd"):
            s = stat(runs["%s L=%d" % (d, L)])
            rows["%s L=%d" % (d, L)] = {"us": s, "bytes": nbytes, "ns_per_kilobyte": s["median"] * 1e3 / (nbytes / 1024.0),
                                         "copy_us": copy, "copy_fraction": copy["median"] / s["median"]}
    out["token_mlp"] = {"what": "V = 50, D = 2048, no dropout mask; L = 8 runs strm_tokmlp_fwd_k / _bwd_k, 12 and 16 the templated family; the "
                                "backward row includes strm_reduce_rows_k", "rows": rows}

    # ---- patch-distance forward at 25 x 25 videos -------------------------------------------------------------------------------------
    way, shot = 5, 5
    ns = nq = way * shot
    labels = torch.arange(way).repeat_interleave(shot).float()
    plan = ops.ClassPlan(labels.to(dev), way, labels)
    pd, variants = {}, {}
    for L in LENGTHS:
        T = L * (L - 1) // 2
        E = torch.relu(torch.randn((ns + nq) * T, 1024, generator=g)).to(dev)
        o = dict(dist=torch.empty(nq * T, way, device=dev), idx=torch.empty(nq * T, way, dtype=torch.int32, device=dev),
                 logits=torch.empty(nq, way, device=dev))
        pd[L] = (E, o)

        def run(f, mode, E=E, o=o, L=L):
            if mode is not None:
                lib.cdll.lmkd_patchdist_set_tiled(mode)
            rc = f["lmkd_strm_patchdist_fwd"](p(E), p(plan.order), p(o["dist"]), p(o["idx"]), p(o["logits"]), ns, nq, way, shot, L, 1024, st)
            assert rc == 0
        # the mode is process-wide and read at launch time: set it before every launch of a variant
        variants["plain L=%d" % L] = lambda run=run: run(own, 0)
        variants["tiled L=%d" % L] = lambda run=run: run(own, 1)
        if parent:
            variants["parent L=%d" % L] = lambda run=run: run(parent, None)
    try:
        runs = alternate(variants, max(4, a.batch // 4))
        same = {}
        for L in LENGTHS:      # the two kernels of this build, and the parent's, on the timed inputs
            E, o = pd[L]
            got = {}
            for k in ("plain", "tiled") + (("parent",) if parent else ()):
                variants["%s L=%d" % (k, L)]()
                torch.cuda.synchronize()
                got[k] = {n: v.clone() for n, v in o.items()}
            same[L] = {k: all(torch.equal(got[k][n], got["plain"][n]) for n in o) for k in got if k != "plain"}
    finally:
        lib.cdll.lmkd_patchdist_set_tiled(-1)
    rows = {}
    for L in LENGTHS:
        T = L * (L - 1) // 2
        r = {k: stat(runs["%s L=%d" % (k, L)]) for k in ("plain", "tiled") + (("parent",) if parent else ())}
        rows["L=%d" % L] = dict(r, T=T, row_pairs=nq * T * ns * T, bit_identical_to_plain=same[L],
                                tiled_median_below_plain_min=r["tiled"]["median"] < r["plain"]["min"])
    out["patch_distance_fwd"] = {"what": "5-way 5-shot, 25 query videos, 1024-wide pair rows; microseconds of lmkd_strm_patchdist_fwd (minimum kernel + "
                                         "strm_dist_logits_k); the measured dispatch sends an L > 8 to the tiled kernel only where its median is below the "
                                         "plain kernel's minimum", "rows": rows}

    # ---- parent build: the 8-frame outputs bit for bit --------------------------------------------------------------------------------
    if parent:
        fwd, bwd, t = check["tok"]
        res = {}
        for who, f in (("own", own), ("parent", parent)):
            for k in ("xp", "y", "dx", "dp"):
                t[k].fill_(float("nan"))
            fwd(f)
            bwd(f)
            torch.cuda.synchronize()
            res[who] = {k: t[k].clone() for k in ("xp", "y", "dx", "dp")}
        out["parent_check"] = {"token_mlp_L8_bit_identical": {k: bool(torch.equal(res["own"][k], res["parent"][k])) for k in res["own"]},
                               "patch_distance_L8_bit_identical": same[8]["parent"], "patch_distance_L12_L16_equal_parent": [same[12]["parent"], same[16]["parent"]]}
        assert all(out["parent_check"]["token_mlp_L8_bit_identical"].values()) and same[8]["parent"], out["parent_check"]


def episodes(a, out):
    import torch
    from litemkd_amd import ops, trainloop as TL
    from litemkd_amd.options import default_args
    from litemkd_amd.schedule import Schedule
    dev = torch.device("cuda", 0)
    sched = Schedule.from_env()
    sched.apply(arithmetic=False)
    ops.set_conv_compute_dtype("fp32h2")
    ops.set_activation_dtype("fp32")
    runs = {}
    for L in LENGTHS:
        for name in ("strm", "headline"):
            cfg = default_args(shot=5, device=dev, trans_dropout=0.1, training_iterations=10 ** 9, print_freq=10 ** 9, seq_len=L, **CONFIGS[name])
            torch.manual_seed(1234)
            student, teacher, src, distiller, accuracy, _, opt, sch = TL.make(cfg, base_seed=2024)
            pool = [src.episode(e) for e in range(2)]
            pipe = TL.PipelinedEpisodes(student, teacher, distiller, accuracy, cfg) if sched.pipeline_episodes else None
            runs[(name, L)] = dict(cfg=cfg, student=student, teacher=teacher, distiller=distiller, accuracy=accuracy, opt=opt, sch=sch, pool=pool,
                                   pipe=pipe, it=0, train=[], infer=[], last=None)

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
            t0 = time.perf_counter()
            train(r, a.steps)
            torch.cuda.synchronize()
            r["train"].append(a.steps / (time.perf_counter() - t0))
            t0 = time.perf_counter()
            infer(r, a.infer_steps)
            torch.cuda.synchronize()
            r["infer"].append(a.infer_steps / (time.perf_counter() - t0))
    rows = {}
    for (name, L), r in runs.items():
        rows["%s seq_len=%d" % (name, L)] = {"train_episodes_per_s": stat(r["train"]), "infer_episodes_per_s": stat(r["infer"]),
                                             "loss_last": float(r["last"][0]) if r["last"] is not None else None}
    for L in LENGTHS:
        rows["ratio strm / headline seq_len=%d" % L] = {
            k: rows["strm seq_len=%d" % L][k]["median"] / rows["headline seq_len=%d" % L][k]["median"] for k in ("train_episodes_per_s", "infer_episodes_per_s")}
    out["episodes"] = {"what": "5-way 5-shot, 224^2, fp32h2, schedule %s; the six configurations alternate %d times, %d training and %d inference "
                               "episodes each per turn (warm-up %d)" % ("merged+pipelined" if sched.pipeline_episodes else "two-call", a.repeats, a.steps,
                                                                        a.infer_steps, a.warmup), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblmkd_hip.so built from the parent commit")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=200, help="token-MLP launches per timed batch (a quarter of it for the patch distance)")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--infer-steps", type=int, default=16)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--episodes-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import litemkd_amd
    assert torch.cuda.is_available(), "strm_long_bench needs the GPU"
    litemkd_amd.lib().call("lmkd_device_check", 0)
    out = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats}
    if not a.episodes_only:
        kernels(a, out)
    if not a.kernels_only:
        episodes(a, out)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
