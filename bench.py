#!/usr/bin/env python
"""Benchmark of the Lite-MKD hot path on MI355X: episodes/sec, 5-way 5-shot, 8 x 224^2 frames, fp32
(BASELINE.json configs[1]).  One "step" = one training episode exactly as trainwandb.py:190-287 runs it:
student forward over 400 frames (two 200-frame BatchNorm batches), frozen TRX teacher head on the teacher
features, D2M loss fc_2_sup_dist, backward; plus the SGD step (and, for N>1, one RCCL all-reduce of the flat
gradient bucket) every tasks_per_batch/N episodes, as in trainwandb.py:141-143.

  python bench.py --gpus N --steps K --warmup W
N>1: one rank per GPU over RCCL.  Either the driver launches the ranks (python -m torch.distributed.run --nproc-per-node N
bench.py --gpus N ...: RANK / WORLD_SIZE are then in the environment), or a plain `python bench.py --gpus N` starts them itself
as a CHILD `python -m torch.distributed.run` process — before this process has made any GPU call — and exits with its code.

Prints ONE JSON line (rank 0).  A plain run does only what that line's headline needs: set-up, allocator priming, the W warm-up
steps, the K timed steps, --dump-outputs, the line.  `--full` adds everything else the benchmark measures, each in runs of its own
after the timed region: `repeat` (the K steps again), `host_enqueue_ms_per_episode`, the per-kernel `roofline` of serialized episodes
(with --serial the timed region itself), `other_modes` (the same job in the other arithmetics, N=1) and `cpu_baseline` (the CPU oracle
timed on the host's cores, rank 0, N=1 only)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
FWD_GFLOP_PER_FRAME = 3.627            # SURVEY.md 8d (ResNet-18 trunk, 224x224)


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a child torch.distributed.run and return its exit
    code.  Called before anything in this process touches the GPU (a process that has initialised HIP must never exec)."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # dmabuf IPC (RCCL across processes)
    env.setdefault("OMP_NUM_THREADS", "2")
    return subprocess.call(cmd, env=env)


def kernel_source_hash():
    """sha256 over the HIP sources the .so is built from: ties committed PMC numbers to the kernels they were measured on"""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "lite-mkd_amd", "csrc", "*"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shot", type=int, default=5)
    ap.add_argument("--pool", type=int, default=2, help="distinct resident synthetic episodes to cycle through")
    ap.add_argument("--full", action="store_true", help="after the headline measurement also run what it does not need: the repeat of the "
                    "timed steps, the host-enqueue probe, the per-kernel roofline pass, the other arithmetic modes and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--prime", type=int, default=160, help="at most this many untimed allocator-priming episodes in front of the warm-up (0: none)")
    ap.add_argument("--dropout", type=float, default=0.1, help="TRX dropout (reference default 0.1, active in train mode)")
    ap.add_argument("--serial", action="store_true", help="queue the two trunk calls on ONE stream (no kernel overlap); use this "
                    "mode under rocprofv3 so per-kernel durations are not inflated by concurrent kernels")
    ap.add_argument("--roofline-episodes", type=int, default=2, help="serialized episodes of the roofline pass (--full, --layer-table)")
    ap.add_argument("--dtype", choices=["f32", "f32native", "bf16", "bf16conv", "f32x3"], default="f32", help="f32 (headline, BASELINE "
                    "configs[1]): fp32 tensors, fp32 accumulation; f32x3's arithmetic with the trunk's convolution kernels (3x3 forward and data "
                    "gradient, every weight gradient, the stem: 97 %% of the trunk's flops) on TWO fp16 planes + power-of-two scales, three products per fp32 "
                    "product ('fp32h2', csrc/conv_patch16.h) - error vs fp64 at or below f32x3's on every layer (tests/test_gpu_h2.py, "
                    "profiles/r04_h2_error.txt); f32x3 (rounds 2-3's headline, the library default): the convolution products on the bf16 "
                    "matrix pipe from an EXACT 3-way bf16 split of both operands, 6 products per fp32 product (csrc/conv_x3.h, wgrad_x3.h; "
                    "error vs fp64 of the class of the native fp32 MFMA: tests/test_gpu_fullsize.py); f32native: the same "
                    "job on v_mfma_f32_32x32x2_f32 (round 1's headline arithmetic, reported under other_modes with --full); "
                    "bf16 (configs[2]): bf16 tensors in HBM for every activation / activation gradient of the trunk, bf16 MFMA with "
                    "fp32 accumulation, fp32 statistics, weights and heads; bf16conv: round 1's variant (fp32 tensors, only the "
                    "convolution operands rounded)")
    ap.add_argument("--xcd-mode", type=int, default=-1, help="tuning: lmkd_conv_set_xcd_mode (-1 auto, 0 plain tile orders, 1 auto without XCD-grouped weight-gradient splits)")
    ap.add_argument("--no-other-modes", action="store_true", help="--full without the short bf16 / f32x3 side measurements")
    ap.add_argument("--ew-wg", type=int, default=0, help="tuning: workgroups per CU of the HBM-bound kernels (lmkd_set_elementwise_wg_per_cu), 0 = default")
    ap.add_argument("--layer-table", action="store_true", help="print the per-layer-shape conv timing table of the roofline pass to stderr "
                    "(runs that pass without --full too)")
    ap.add_argument("--tile", type=int, default=0, help="tuning: force a conv tile configuration (lmkd_conv_set_tile), 0 = auto")
    ap.add_argument("--backbone", default="resnet18_2fc", help="resnet18_2fc (headline) or resnet50_2fc (BASELINE configs[4])")
    ap.add_argument("--live-mfm", action="store_true", help="fuse rgb/depth/flow teacher features with the MFM transformer "
                    "inside every episode (BASELINE configs[4]) instead of using precomputed fused features")
    ap.add_argument("--cpu-episodes", type=int, default=3, help="episodes of the bounded cpu_baseline sample (--full)")
    ap.add_argument("--graph", dest="graph", action="store_true", default=os.environ.get("LMKD_GRAPH", "0") == "1",
                    help="replay each resident episode as a captured hipGraph (trainloop.GraphedEpisode).  Same kernels, bit-identical results; "
                         "the ~560 launches of an episode leave the host path (1.3-2.0 ms of host time per episode instead of 8-11).  OFF by "
                         "default: on one MI355X with a free host the replay is 5 %% slower on the GPU side than the eager three-stream "
                         "launches (31.4 vs 33.0 episodes/s; bf16 66.5 vs 72.3) - for hosts with less than ~1 core per rank")
    ap.add_argument("--no-graph", dest="graph", action="store_false")
    ap.add_argument("--pipeline", dest="pipeline", action="store_true", default=None,
                    help="software pipelining across episodes (trainloop.PipelinedEpisodes): the forward of episode i + 1 runs beside the "
                         "backward of episode i on a second stream set; same kernels, bit-identical results, same optimizer cadence.  Default: "
                         "the schedule's (Schedule.bench(): ON together with the merged trunk call - 37.5 vs 37.0 episodes/s; with the "
                         "two-call schedule it is 5 %% slower, six streams of half-size launches disturb each other)")
    ap.add_argument("--no-pipeline", dest="pipeline", action="store_false")
    ap.add_argument("--graph-interval", action="store_true", help="with --graph: capture the episodes between two optimizer steps as ONE graph "
                    "(the weight-gradient stream keeps running under the next episode's forward, as in the eager loop)")
    ap.add_argument("--stream-inputs", action="store_true", help="extra measurement after the headline line: every episode's inputs arrive "
                    "from HOST memory - decoded uint8 frames (320x240, pinned) + teacher features go H2D on a copy stream, the GPU frame "
                    "transform (Resize 256 / crop 224 / flip / ToTensor, video_transform.py) runs there too, overlapped with the previous "
                    "episode's compute (trainwandb.py:419-443, video_reader.py:474-485); reported under `stream_inputs`, never as `value`")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps write what the timed path computed in its "
                    "last step as DIR/<name>.npy (rank 0): the episode's loss and accuracy, a fixed seeded sample of the trained weights and of "
                    "the accumulated gradient, the student's BatchNorm running statistics (dump_outputs below).  The priming then runs all "
                    "--prime episodes, so that runs with the same arguments compare output for output")
    ap.add_argument("--emulate-world", type=int, default=0, help="single-GPU rehearsal of the per-rank cadence of a W-rank run: the optimizer "
                    "step (+ weight re-pack) every tasks_per_batch / W episodes; no collective runs, `value` stays the 1-GPU figure of that cadence")
    a = ap.parse_args()
    if a.gpus > 1 and "RANK" not in os.environ:
        sys.exit(self_launch(a.gpus))

    import torch.distributed as dist
    import litemkd_amd  # noqa: F401
    from litemkd_amd import ops, trainloop as TL
    from litemkd_amd.parallel import init_distributed
    from litemkd_amd.model.model_select import Student, Teacher
    from litemkd_amd.distillers import Distiller
    from litemkd_amd.options import default_args
    from litemkd_amd.utils import aggregate_accuracy
    from litemkd_amd.model.backbone import resnet as R
    # the schedule the benchmark times: ONE object (lite-mkd_amd/schedule.py; defaults = Schedule.bench(), LMKD_* variables override single
    # switches for A/B runs) - tests/test_gpu_schedule.py compares exactly this schedule with the serial one at the benchmark's size
    from litemkd_amd.schedule import Schedule
    SCHED = Schedule.from_env()
    if a.serial:
        SCHED.overlap_trunk_calls = SCHED.side_wgrad = False
    SCHED.apply(arithmetic=False)
    if os.environ.get("LMKD_PRIO"):                                                         # stream priorities "lane0,lane1,wgrad" (-1 high, 0 default)
        pr = [int(v) for v in os.environ["LMKD_PRIO"].split(",")]
        ops.STREAM_PRIORITY.update({0: pr[0], 1: pr[1], "wgrad": pr[2]})
    if os.environ.get("LMKD_WGRAD_STEM", "1") == "0":                                     # the stem's weight gradient back on the im2col-gather kernel
        ops.lib().call("lmkd_conv_set_wgrad_stem", 0)
    if os.environ.get("LMKD_S2_PATCH", "1") == "0":                                       # stride-2 3x3 forward back on the im2col-gather kernel
        ops.lib().call("lmkd_conv_set_s2_patch", 0)
    if os.environ.get("LMKD_WIN16", "1") == "0":                                          # rolling-window weight gradient back on the 32x32x16 MFMA
        ops.lib().call("lmkd_conv_set_wgrad_win16", 0)

    from litemkd_amd import parallel as PAR
    rank, world, dev = init_distributed()
    assert dev.type == "cuda", "bench.py needs MI355X GPUs (the hot path has no CPU fallback)"
    assert world == a.gpus, "--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run --nproc-per-node %d" % (a.gpus, world, a.gpus)
    litemkd_amd.lib().call("lmkd_device_check", dev.index)
    litemkd_amd.lib().call("lmkd_conv_set_tile", a.tile)
    litemkd_amd.lib().call("lmkd_conv_set_xcd_mode", a.xcd_mode)
    if a.ew_wg > 0:
        litemkd_amd.lib().call("lmkd_set_elementwise_wg_per_cu", a.ew_wg)
    MODE = {"f32": "fp32h2", "f32x3": "fp32x3", "f32native": "fp32", "bf16": "bf16", "bf16conv": "bf16"}

    def set_mode(name):
        ops.set_conv_compute_dtype(MODE[name])
        ops.set_activation_dtype("bf16" if name == "bf16" else "fp32")
    set_mode(a.dtype)
    cfg = default_args(shot=a.shot, device=dev, trans_dropout=a.dropout, training_iterations=10 ** 9, print_freq=10 ** 9,
                       model_backbone=a.backbone)
    torch.manual_seed(1234)                                  # identical initial weights on every rank
    # the reference's make() (trainwandb.py:78-109): models, episode source, distiller, accuracy function, optimizer, scheduler
    student, teacher, src, distiller, aggregate_accuracy, _, opt, sch = TL.make(cfg, base_seed=2024)
    pool = [src.episode(e) for e in range(a.pool)]           # resident in HBM before the timed region
    mfm = None
    if a.live_mfm:
        import argparse as _ap
        from litemkd_amd.teacher import ThreeTRXShiftLoopTime
        mfm = ThreeTRXShiftLoopTime(_ap.Namespace(seq_len=cfg.seq_len, trans_num=2, shirt_num=1)).eval().to(dev)
        g = torch.Generator(device=dev).manual_seed(99 + rank)
        nv = cfg.way * (cfg.shot + cfg.query_per_class)
        mods = [{k: torch.randn(nv, cfg.seq_len, 2048, generator=g, device=dev).abs() for k in ("rgb", "depth", "flow")}
                for _ in range(a.pool)]
    every = max(1, cfg.tasks_per_batch // (a.emulate_world if a.emulate_world > 0 else world))
    if a.pipeline is not None:
        SCHED.pipeline_episodes = a.pipeline
    use_pipe = SCHED.pipeline_episodes and not a.serial and mfm is None
    use_graph = a.graph and not a.serial and mfm is None and not use_pipe
    if os.environ.get("LMKD_PIPE_DEPTH"):
        TL.PIPELINE_DEPTH = int(os.environ["LMKD_PIPE_DEPTH"])
    pipe = TL.PipelinedEpisodes(student, teacher, distiller, aggregate_accuracy, cfg) if use_pipe else None
    runners = {}      # one GraphedEpisode per arithmetic mode: a captured graph holds that mode's kernels and packed-weight buffers
    state = {"mode": a.dtype}

    def graph_runner():
        if not use_graph:
            return None
        if state["mode"] not in runners:
            runners[state["mode"]] = TL.GraphedEpisode(student, teacher, distiller, aggregate_accuracy, cfg, max_graphs=max(4, a.pool))
        return runners[state["mode"]]

    main_lane = os.environ.get("LMKD_MAIN_LANE", "0") == "1" and pipe is None      # the episode loop on lane 0's main stream (its priority)

    def run(n, it0):
        if not main_lane:
            return run_on_current(n, it0)
        ml = ops.lane_main(dev)
        ml.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(ml):
            it = run_on_current(n, it0)
        torch.cuda.current_stream(dev).wait_stream(ml)
        return it

    def run_intervals(n, it0):
        """--graph-interval: the episodes between two optimizer steps as ONE graph replay (GraphedEpisode.run_interval)"""
        it, i = it0, 0
        g = graph_runner()
        while i < n:
            k = min(every - ((it + 1) % every), n - i) or every      # up to the next optimizer step
            k = min(k, n - i)
            state["last"] = g.run_interval([pool[(it + j) % len(pool)] for j in range(k)])      # by the global episode count: the same interval comes round
            i += k
            it += k
            if (it + 1) % every == 0:
                opt.step()
                opt.zero_grad()
            for _ in range(k):
                sch.step()
        return it

    def run_on_current(n, it0):
        if use_graph and a.graph_interval and mfm is None:
            return run_intervals(n, it0)
        it = it0
        for i in range(n):
            it += 1
            ep = next(state["episodes"]) if state.get("episodes") is not None else pool[i % len(pool)]      # (--stream-inputs: from a StreamedEpisodes loader)
            if mfm is not None:      # live fusion: the teacher features of this episode come out of the MFM transformer
                fused = mfm.extract_feature(mods[i % len(pool)])
                ns = cfg.way * cfg.shot
                ep = dict(ep, support_set_feature_teacher=fused[:ns].unsqueeze(0), target_set_feature_teacher=fused[ns:].unsqueeze(0))
            graphed = graph_runner()
            if (it + 1) % every == 0 and graphed is None:
                opt.expect_step()                      # world > 1: the bucket's tail is all-reduced under this episode's backward pass (pipelined: it runs in the flush below)
            # state["last"]: what the caller receives for the most recent episode whose backward pass has been queued (--dump-outputs)
            if pipe is not None and state.get("pipe", True):
                state["last"] = pipe.push(ep) or state.get("last")
            elif graphed is not None:
                state["last"] = graphed(ep)
            else:
                state["last"] = TL.train_task(ep, student, teacher, distiller, aggregate_accuracy, cfg)
            if (it + 1) % every == 0:
                if pipe is not None:
                    state["last"] = pipe.flush() or state.get("last")       # the step needs the gradients of every episode up to this one
                opt.step()
                opt.zero_grad()
            sch.step()
        if pipe is not None:
            state["last"] = pipe.flush() or state.get("last")
        return it

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if world > 1:
        # the first all-reduce of a kind sets the backend up for it (gloo: staging buffers - a stall of seconds; RCCL: channels and
        # proxies for the stream): both collectives of an optimizer step - the bucket's tail on the early all-reduce's stream, the head
        # on the main stream - run once on the zeroed gradient buffers before the warm-up, so that a W too short to contain an
        # optimizer step (world 2: a step every 8 local episodes) does not move that one-time cost into the timed region
        opt.zero_grad()
        torch.cuda.synchronize()
        opt.early.arm()
        opt.early.launch()
        opt.bucket.allreduce_grads(opt.early.finish())
        torch.cuda.synchronize()
        opt.zero_grad()
        PAR.ALLREDUCE_TIMING = None
    # warm-up: with graphs every resident episode has to be seen twice before it replays (first eager, then captured)
    interval_mode = use_graph and a.graph_interval and mfm is None
    if interval_mode:      # whole optimizer intervals only: the interval that repeats is seen (eager), captured and replayed before the timed region
        a.steps = max(every, a.steps // every * every)
        it = run(every - 1 + 3 * every, 0)
    else:
        # allocator priming, before the W warm-up steps and outside every count: torch's caching allocator keeps one pool of blocks per
        # stream (a block freed on the weight-gradient stream cannot serve the forward's stream), and with two episodes in flight on five
        # streams the order in which blocks come back varies from episode to episode, so new device allocations keep trickling in for tens
        # of episodes (round 4: 246 - 331 hipMalloc calls inside a 16 - 20 step timed region).  Running the loop until an optimizer
        # interval passes without a device allocation puts that ramp in front of the measurement (`allocator_priming_episodes`).
        primed = 0
        it = 0
        if dev.type == "cuda" and not use_graph and a.prime > 0:
            quiet = 0      # consecutive optimizer intervals without a device allocation (one quiet interval was not enough: 145 allocations came back in a 20-step region)
            while primed < a.prime:
                m0 = torch.cuda.memory_stats(dev).get("num_device_alloc", 0)
                it = run(every, it)
                primed += every
                fence()
                still = 1 if torch.cuda.memory_stats(dev).get("num_device_alloc", 0) == m0 else 0
                if world > 1:      # every rank must leave the loop after the same interval: an interval holds an optimizer step's collectives
                    flag = torch.tensor([still], device=dev, dtype=torch.int32)
                    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                    still = int(flag.item())
                quiet = quiet + 1 if still else 0
                if quiet >= 3 and not a.dump_outputs:      # --dump-outputs: always --prime episodes, so that the state the timed steps start
                    break                                   # from depends on the arguments alone, not on when the allocator settled
        it = run(max(a.warmup, 2 * len(pool) + 1) if use_graph else a.warmup, it)
    fence()
    ops.CONV_TIMING = None if (use_graph or os.environ.get("LMKD_TIMED_EVENTS", "1") == "0") else []      # per-launch HIP events cannot be recorded into a captured graph (roofline_pass below times them)
    PAR.ALLREDUCE_TIMING = []
    steps0 = opt.steps
    mallocs0 = torch.cuda.memory_stats(dev).get("num_device_alloc", 0) if dev.type == "cuda" else 0
    t0 = time.perf_counter()
    it = run(a.steps, it)
    t_enq = time.perf_counter() - t0                 # host time to enqueue the timed region (before the fence)
    fence()
    dt = time.perf_counter() - t0
    mallocs_timed = (torch.cuda.memory_stats(dev).get("num_device_alloc", 0) - mallocs0) if dev.type == "cuda" else 0
    opt_steps_timed = opt.steps - steps0             # read HERE: the repeat and host-idle passes below step the optimizer too
    if a.dump_outputs and rank == 0:                 # before the repeat pass below trains on
        dump_outputs(a.dump_outputs, state.get("last"), opt.bucket, student)
    timed_events, ops.CONV_TIMING = (ops.CONV_TIMING or []), None
    # from here on, everything the headline does not need runs with --full only
    if a.full:
        # the same K steps once more, timed the same way (barrier + synchronize on both sides), WITHOUT the per-launch HIP events of the
        # roofline bookkeeping: reported as `repeat` (never as `value`) - two figures that agree say the timed region was undisturbed
        fence()
        t0r = time.perf_counter()
        it = run(a.steps, it)
        fence()
        dt_rep = time.perf_counter() - t0r
        if world > 1:
            tr = torch.tensor([dt_rep], device=dev, dtype=torch.float64)
            dist.all_reduce(tr, op=dist.ReduceOp.MAX)
            dt_rep = float(tr.item())
        # host cost of ONE episode's enqueue on an idle queue (nothing to wait for): what the Python / launch side needs per episode
        # when it is not throttled by a full launch queue
        host_idle = 0.0
        for _ in range(4):
            fence()
            th = time.perf_counter()
            it = run(every if interval_mode else 1, it)
            host_idle += (time.perf_counter() - th) / (every if interval_mode else 1)
        fence()
        host_idle /= 4
    ar_events, PAR.ALLREDUCE_TIMING = PAR.ALLREDUCE_TIMING, None
    dist_info = {"backend": None, "world": world, "devices": [torch.cuda.get_device_name(dev)], "allreduce_ms_per_optimizer_step": None,
                 "optimizer_steps_in_timed_region": opt_steps_timed, "allreduce_bucket_bytes": opt.bucket.numel * 4}
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        # evidence that the collective ran over `world` ranks on `world` distinct GPUs: backend, every rank's device, and a
        # checksum all-reduce (sum of rank+1 over the ranks must be world*(world+1)/2)
        names = [None] * world
        props = torch.cuda.get_device_properties(dev)
        dist.all_gather_object(names, "rank %d: cuda:%d %s (%s, pci %s)" % (rank, dev.index, props.name, getattr(props, "gcnArchName", "?"),
                                                                              getattr(props, "pci_bus_id", "?")))
        chk = torch.tensor([float(rank + 1)], device=dev)
        dist.all_reduce(chk)
        assert int(chk.item()) == world * (world + 1) // 2, "all-reduce checksum: %s" % chk.item()
        # per optimizer step: the part issued under the backward pass (EarlyAllReduce: overlapped with it) and the rest, issued at the step
        n_steps = max(1, sum(1 for e in ar_events if e[2] == "at step"))
        ms = {k: sum(e[0].elapsed_time(e[1]) for e in ar_events if e[2] == k) / n_steps for k in ("early", "at step")}
        ar = torch.tensor([ms["early"] + ms["at step"], ms["early"], ms["at step"]], device=dev, dtype=torch.float64)
        dist.all_reduce(ar, op=dist.ReduceOp.MAX)
        dist_info.update({"backend": dist.get_backend(), "devices": names, "allreduce_ms_per_optimizer_step": float(ar[0].item()),
                          "allreduce_ms_overlapped_with_backward": float(ar[1].item()), "allreduce_ms_at_step": float(ar[2].item()),
                          "allreduce_early_elements": opt.bucket.numel - opt.early.split, "allreduce_checksum_ok": True})
    conv_flops_timed = sum(r[1] for r in timed_events)
    # the same HIP-event measurement inside the timed region: with two streams a launch's interval also contains the other
    # stream's kernels, so this is a lower bound of the kernel's own rate (reported next to the serialized figure)
    cg_t = [(r[1], r[2].elapsed_time(r[3]) * 1e-3) for r in timed_events if r[0] in ("conv_gemm_kernel", "conv_patch_kernel")]
    achieved_timed = (sum(f for f, _ in cg_t) / max(sum(t for _, t in cg_t), 1e-12) / 1e12) if cg_t else None

    # Per-kernel roofline.  In the timed region the two trunk calls run on two streams, so kernels overlap and a single
    # launch's HIP-event duration includes time shared with the other stream's kernels.  The kernel-quality number is
    # therefore taken from `--roofline-episodes` extra episodes with the overlap switched off (same kernels, same shapes,
    # same process, right after the timed region); with --serial the timed region itself is used.
    def roofline_pass():
        """`--roofline-episodes` extra episodes with the stream overlap switched off -> per-launch HIP-event records"""
        R.OVERLAP_TRUNK_CALLS = False
        ops.SIDE_WGRAD = False
        ops.wait_weight_grads()
        ops.CONV_TIMING = []
        # optimizer steps are excluded here on purpose: this pass only prices kernels
        for i in range(a.roofline_episodes):
            TL.train_task(pool[i % len(pool)], student, teacher, distiller, aggregate_accuracy, cfg)
        opt.zero_grad()
        fence()
        rec, ops.CONV_TIMING = ops.CONV_TIMING, None
        R.OVERLAP_TRUNK_CALLS = SCHED.overlap_trunk_calls
        ops.SIDE_WGRAD = SCHED.side_wgrad
        return rec

    def families(rec):
        fam = {}
        for name, flops, e0, e1, nbytes in rec:
            f = fam.setdefault(name, [0.0, 0.0, 0, 0.0])
            f[0] += flops
            f[1] += e0.elapsed_time(e1) * 1e-3
            f[2] += 1
            f[3] += nbytes
        return fam

    # Forward + data-gradient convolutions run on two kernel families: conv_patch_x3_kernel (same-size 3x3 convolutions of the
    # bf16-plane modes, conv_patch.h) and the im2col-gather kernels (stride-2 / 1x1 / stem; every convolution in f32native).
    # The roofline is that of whichever takes more time; the other one is reported beside it.
    ZERO = [0.0, 1.0, 0, 0.0]

    def conv_families(fm):
        pk, gk = fm.get("conv_patch_kernel", ZERO), fm.get("conv_gemm_kernel", ZERO)
        patch_dominant = pk[2] > 0 and pk[1] >= gk[1]
        return (pk, gk, True) if patch_dominant else (gk, pk, False)
    # dense MFMA peaks (MI355X_MICROARCH.md); the 3xbf16 arithmetic issues 6 bf16 MFMA flops per algorithmic fp32 flop
    PEAK = {"f32": 2500.0 / 3, "f32x3": 2500.0 / 6, "f32native": PEAK_FP32_MFMA_TFLOPS, "bf16": 2500.0, "bf16conv": 2500.0}
    ARITH = {"f32": "v_mfma_f32_16x16x32_f16 x3 per fp32 product, two fp16 planes per operand (h0 + h1 = x 2^s to 2^-23, 2^s from the tensor's "
                    "maximum), fp32 accumulate; peak = dense fp16 MFMA peak / 3",
             "f32x3": "v_mfma_f32_16x16x32_bf16 x6 per fp32 product, exact 3-way bf16 operand split, fp32 accumulate; peak = dense bf16 MFMA peak / 6",
             "f32native": "v_mfma_f32_32x32x2_f32",
             "bf16": "one bf16 plane, bf16 tensors, v_mfma_f32_32x32x16_bf16",
             "bf16conv": "one bf16 plane, fp32 tensors, v_mfma_f32_32x32x16_bf16"}

    def kernel_name(mode, patch):
        if patch:
            return ("conv_patch16_x3_kernel + conv_patch_x3_kernel<.., 3, ..> (layer 1's launches, v_mfma_f32_32x32x16_f16, persistent workgroups: round 5)" if mode == "f32" else
                    "conv_patch16_x3_kernel" if mode == "f32x3" else "conv_patch_x3_kernel") + \
                " (3x3 conv fwd + dgrad from an LDS-resident input patch; stride-2 launches as parity classes): " + ARITH[mode]
        return ("conv_gemm_kernel" if mode == "f32native" else "conv_gemm_x3_kernel") + " (implicit-GEMM conv fwd + dgrad): " + ARITH[mode]

    # the per-kernel figures need per-launch records of serialized episodes: the timed region itself with --serial, else a pass of
    # their own (--full, or --layer-table alone); a plain run reports only what its timed region recorded
    timing = timed_events if a.serial else roofline_pass() if a.full or a.layer_table else None
    roofline = {}
    if timing is not None:
        # roofline of the dominant kernel family (implicit-GEMM conv fwd + dgrad, one template): algorithmic FLOPs / HIP-event time
        fam = families(timing)
        if a.layer_table and rank == 0:      # per distinct (kernel family, FLOPs, bytes) launch shape: where the conv time goes
            shp = {}
            for name, flops, e0, e1, nbytes in timing:
                g = shp.setdefault((name, flops, nbytes), [0.0, 0])
                g[0] += e0.elapsed_time(e1) * 1e-3
                g[1] += 1
            tot = sum(g[0] for g in shp.values())
            print("# kernel family | GFLOP/launch | MB/launch | launches | avg us | TFLOP/s | share of conv time", file=sys.stderr)
            for (name, flops, nbytes), (t, n) in sorted(shp.items(), key=lambda kv: -kv[1][0]):
                print("%-18s %7.2f %7.1f %4d %8.1f %6.1f %5.1f%%" % (name, flops / 1e9, nbytes / 1e6, n, t / n * 1e6, flops * n / t / 1e12,
                                                               100 * t / tot), file=sys.stderr)
        cg, cg_other, patch_dom = conv_families(fam)
        wg = fam.get("conv_wgrad_kernel", ZERO)
        achieved = cg[0] / cg[1] / 1e12
        PMC_KEY = ("conv_patch16_x3_kernel+conv_patch_x3_kernel" if a.dtype == "f32" else "conv_patch16_x3_kernel" if a.dtype == "f32x3" else "conv_patch_x3_kernel") if patch_dom else ("conv_gemm_kernel" if a.dtype == "f32native" else "conv_gemm_x3_kernel")
        peak = PEAK[a.dtype]
        # HBM-side traffic of the same kernel family: rocprofv3 PMC passes (FETCH_SIZE and WRITE_SIZE collected separately,
        # FETCH_SIZE doubled, as gfx950 counts the 128-B requests of 16-B/lane reads as 64 B) of `bench.py --serial`,
        # committed under profiles/ — counters cannot be read from inside this process.
        # The file records the hash of the kernel sources it was measured on; a number measured on other kernels is not reported.
        traffic, traffic_note = None, "no PMC file"
        import glob
        tfiles = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic.json")))
        if tfiles:
            tj = json.load(open(tfiles[-1]))
            if a.dtype != "f32":
                traffic_note = "%s holds the PMC passes of the headline arithmetic only" % os.path.relpath(tfiles[-1], ROOT)
            elif tj.get("kernel_src_hash") == kernel_source_hash():
                traffic = tj.get(PMC_KEY, {}).get("traffic_bytes_per_launch")
                traffic_note = "rocprofv3 FETCH_SIZE*2 + WRITE_SIZE per launch of %s, %s" % (PMC_KEY, os.path.relpath(tfiles[-1], ROOT))
            else:
                traffic_note = "%s was measured on other kernel sources (hash %s, now %s): not reported" % (
                    os.path.relpath(tfiles[-1], ROOT), tj.get("kernel_src_hash"), kernel_source_hash())
                print("bench.py: " + traffic_note, file=sys.stderr)
        roofline = {"bound": "mfma", "kernel": kernel_name(a.dtype, patch_dom),
                    "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                    "traffic": traffic, "traffic_unit": "bytes per launch", "traffic_note": traffic_note,
                    "kernel_src_hash": kernel_source_hash(),
                    "algorithmic_bytes_per_launch": cg[3] / max(cg[2], 1),
                    "launches": cg[2], "avg_launch_ms": cg[1] / max(cg[2], 1) * 1e3,
                    "other_conv_family": {"kernel": kernel_name(a.dtype, not patch_dom).split(":")[0], "launches": cg_other[2],
                                          "tflops": cg_other[0] / cg_other[1] / 1e12, "avg_launch_ms": cg_other[1] / max(cg_other[2], 1) * 1e3},
                    "wgrad_kernel_tflops": wg[0] / wg[1] / 1e12, "wgrad_avg_launch_ms": wg[1] / max(wg[2], 1) * 1e3,
                    "measured_on": "timed region (--serial)" if a.serial else "%d extra serialized episodes after the timed region" % a.roofline_episodes}
    frames = 8 * 5 * (a.shot + cfg.query_per_class)
    step_tflop = 3 * FWD_GFLOP_PER_FRAME * frames / 1e3
    roofline.update({"achieved_in_timed_region": achieved_timed,
                     "timed_region_conv_tflops_per_gpu": conv_flops_timed / dt / 1e12,
                     "episode_model_tflops": step_tflop * world * a.steps / dt})
    ops.h2_fence_step(wait=True)      # fp32h2: take in the range fence's last verdicts before they are reported
    out = {
        "metric": "episodes/sec (5-way %d-shot, 8x224^2 frames)" % a.shot, "value": world * a.steps / dt, "unit": "episodes/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
        "config": {"workload": "HMDB-shape 5-way %d-shot %s + TRX_2fcsup + D2M fc_2_sup_dist training episode%s, %s"
                               % (a.shot, a.backbone, " + live MFM fusion" if a.live_mfm else "",
                                  {"f32": "fp32", "f32x3": "fp32", "f32native": "fp32", "bf16": "bf16 tensors / fp32 accumulate", "bf16conv": "bf16 conv operands / fp32 tensors"}[a.dtype]),
                   "conv_arithmetic": {"f32": "fp32 tensors and accumulation.  The trunk's convolution kernels - 3x3 forward and data gradient, every weight "
                                              "gradient, the stem: 97 % of the trunk's flops - split each fp32 operand x into TWO fp16 planes, h0 = fp16(x 2^s), h1 = fp16(x 2^s - h0) "
                                              "(round to nearest: |x 2^s - h0 - h1| <= 2^-23 |x 2^s|, one fp32 ulp, zero for at least half of all fp32 values; 2^s a power of two from max |tensor|, which the kernel "
                                              "that writes the tensor records, so the scaling is exact) and form h0 w0 + h0 w1 + h1 w0 on "
                                              "v_mfma_f32_16x16x32_f16 with fp32 accumulation (the dropped h1 w1 <= 2^-22 of the product, zero-mean; the three-plane "
                                              "bf16 form drops <= 2^-23, all of one sign).  Everything else (the 1x1 forward of the downsample branches, the heads) runs f32x3's "
                                              "arithmetic.  Relative-L2 error vs fp64 on the trunk's four 3x3 shapes: forward 2.7e-7 .. 7.0e-7, data gradient "
                                              "2.7e-7 .. 7.1e-7, weight gradient 2.3e-7 .. 5.5e-7 - below f32x3's (3.5e-7 .. 9.6e-7 | 3.6e-7 .. 1.0e-6 | 2.9e-7 .. "
                                              "8.2e-7; profiles/r04_h2_error.txt, 40 frames, where torch's GPU fp32 convolution reads 3.0e-7 .. 8.0e-7).  Against the CPU "
                                              "ORACLE - the stated baseline - at the benchmark's 200 frames the pairs (HIP | torch-CPU fp32, both vs fp64) are in "
                                              "profiles/r05_parity_errors.txt: layers 1-2 level with it, layers 3-4 2-3x above (forward 7.0e-7 vs 2.3e-7 on layer 4): fp32-class - "
                                              "inside the fp64-anchored criterion 3 x CPU + 1e-6 of tests/test_gpu_fullsize.py, which also holds with trained-like "
                                              "statistics (log-normal activations, |gamma| in [0.2, 3], 2^6 weight-scale spread) - not 'at the oracle's level'.  A run-time "
                                              "range fence (DESIGN 11.2) counts what the two planes do not resolve and moves a tensor's convolutions to the three-plane "
                                              "form: h2_fallbacks below, 0 on this benchmark.  The same job in f32x3 (rounds 2-3's headline): other_modes.f32x3",
                                       "f32x3": "the library default: fp32 tensors and accumulation; every convolution (forward, data and weight "
                                              "gradient, stem included) forms its products on the bf16 matrix pipe from an exact 3-way bf16 split of "
                                              "both operands, 6 of 9 cross products; half the row tiles of a launch accumulate -y so that the MFMA's "
                                              "directional truncation cancels in sums over pixels (DESIGN 8.5).  Relative-L2 error vs fp64 at the "
                                              "benchmark's 200 frames: forward / data gradient <= 3 x torch-CPU-fp32's + 1e-6 (measured 1.2e-7 ... "
                                              "1.0e-6, torch-CPU 1.4e-7 ... 5e-7), weight gradient <= 3 x + 2e-6; measured pairs of every anchored test: "
                                              "profiles/r03_parity_errors.txt (tests/test_gpu_fullsize.py, test_gpu_ops.py, test_gpu_episode.py)",
                                       "f32native": "v_mfma_f32_32x32x2_f32 (exact fp32 products)",
                                       "bf16": "trunk activations and their gradients stored as bf16 in HBM, bf16 MFMA, fp32 accumulation; BatchNorm "
                                               "statistics, weights, weight gradients, heads and loss fp32",
                                       "bf16conv": "conv operands rounded to bf16 (RNE), fp32 accumulation; activations / BatchNorm / loss fp32"}[a.dtype],
                   "frames_per_episode": frames, "img": 224, "tasks_per_batch": cfg.tasks_per_batch, "optimizer": cfg.opt,
                   "episodes_per_optimizer_step_per_rank": every, "parallelism": "episode-parallel dp%d" % world,
                   "trans_dropout": a.dropout, "trunk_calls_overlapped_on_two_streams": not a.serial},
        "roofline": roofline,
        "distributed": dist_info,
        "device_mallocs_in_timed_region": mallocs_timed,
        "allocator_priming_episodes": primed if not interval_mode else 0,
        # HBM held by the caching allocator against what the tensors need at their peak: the gap is the allocator's per-stream pools (a block
        # belongs to the stream it was allocated on; five streams x the 6 GB of activations a trunk call saves, two or three episodes in flight)
        "hbm_GB": ({"reserved": round(torch.cuda.memory_stats(dev).get("reserved_bytes.all.peak", 0) / 2 ** 30, 1),
                    "allocated_peak": round(torch.cuda.memory_stats(dev).get("allocated_bytes.all.peak", 0) / 2 ** 30, 1)} if dev.type == "cuda" else None),
        # host side: the time the Python loop spent enqueueing the timed region - the host is throttled by the full launch queue there
        # whenever the GPU is the bottleneck (host_enqueue_ms_per_episode below, --full: the same on an idle queue)
        "host_loop_ms_per_episode_in_timed_region": t_enq / a.steps * 1e3,
        "episode_pipelining": bool(use_pipe),
        # after every episode and optimizer step this process has run so far (ReLU(NaN) = 0 keeps a loss finite on NaN weights)
        "weights_finite": bool(torch.isfinite(opt.bucket.flat).all()),
        # the range fence of the two-plane arithmetic (ops.h2_fence_step after every backward pass): launches that fell back to the three-plane
        # form because their tensor was flagged, and the flagged tensors ("y" | "a" | "d" | "p", BatchNorm) - expected 0 / none on this benchmark
        "h2_fallbacks": int(litemkd_amd.lib().value("lmkd_conv_h2_fallbacks")),
        "h2_fence_flagged_sites": len(ops.h2_fence_flagged()),
        "hipgraph": {"enabled": bool(use_graph), "replays": runners[a.dtype].replays if use_graph else 0,
                     "eager_episodes": runners[a.dtype].eager if use_graph else None, "graphs": len(runners[a.dtype].graphs) if use_graph else 0},
    }
    if a.full:
        out["repeat"] = {"value": world * a.steps / dt_rep, "unit": "episodes/s", "steps": a.steps,
                         "what": "the timed K steps run a second time right after the timed region, without per-launch timing events"}
        # time to ENQUEUE one episode on an idle queue (4 samples after the timed region; an optimizer step may fall on one of them)
        out["host_enqueue_ms_per_episode"] = host_idle * 1e3
    if a.emulate_world > 0:
        out["emulated_world"] = {"world": a.emulate_world, "episodes_per_optimizer_step": every,
                                 "note": "per-rank cadence of a %d-rank run rehearsed on ONE GPU (optimizer step + weight re-pack every %d episodes, "
                                         "no collective): value x %d would be the job's rate at perfect scaling" % (a.emulate_world, every, a.emulate_world)}
    if a.stream_inputs:
        out["stream_inputs"] = stream_inputs_pass(a, cfg, dev, run, state, fence, TL)
    if a.full and world == 1 and a.dtype == "f32" and not a.no_other_modes:
        # the same job in the two other arithmetic modes of the convolutions, for the record (never part of `value`):
        # short timed regions right here, same process, same resident episodes, each with its own per-kernel roofline pass
        other = {}
        ALG_BYTES_PER_EPISODE = 3 * 12.9e6 * frames      # 12.9 MB of bf16 activation traffic per frame forward, x3 for a step
        for name in ("f32x3", "f32native", "bf16"):
            set_mode(name)
            state["mode"] = name
            # the native fp32 MFMA mode has no two-segment kernels (resnet.merge_supported): it runs round 3's schedule - two trunk calls on
            # two streams, no pipelining (Schedule.two_call()), which is the faster one there
            state["pipe"] = name != "f32native"
            it = run(2 * len(pool) + 1 if use_graph else 2, it)
            fence()
            t1 = time.perf_counter()
            it = run(16, it)      # 16 consecutive episodes always contain exactly one optimizer step
            fence()
            v = 16 / (time.perf_counter() - t1)
            f2 = families(roofline_pass())
            g2, _, pd2 = conv_families(f2)
            w2 = f2.get("conv_wgrad_kernel", ZERO)
            ach = g2[0] / g2[1] / 1e12
            other[name] = {"value": v, "unit": "episodes/s", "steps": 16,
                           "roofline": {"bound": "mfma", "kernel": kernel_name(name, pd2), "achieved": ach, "peak": PEAK[name], "unit": "TFLOP/s",
                                        "frac": ach / PEAK[name], "avg_launch_ms": g2[1] / max(g2[2], 1) * 1e3,
                                        "wgrad_kernel_tflops": w2[0] / w2[1] / 1e12}}
        set_mode("f32")
        state["mode"] = "f32"
        state["pipe"] = True
        other["f32x3"]["what"] = ("rounds 2-3's headline arithmetic (the library default): every fp32 product from an exact 3-way bf16 split, "
                                  "six bf16 MFMA products")
        other["f32native"]["what"] = "round 1's headline arithmetic: every convolution on the fp32 MFMA (157.3 TFLOP/s peak)"
        other["bf16"]["what"] = "BASELINE configs[2]: bf16 tensors in HBM (activations and their gradients), bf16 MFMA, fp32 accumulate / statistics / weights"
        # configs[2] sits at the ridge of the bf16 roofline: report the HBM side as well, on algorithmic bytes
        gbs = ALG_BYTES_PER_EPISODE * other["bf16"]["value"] / 1e9
        other["bf16"]["roofline_hbm"] = {"bound": "hbm", "achieved": gbs, "peak": 8000.0, "unit": "GB/s", "frac": gbs / 8000.0,
                                         "algorithmic_bytes_per_episode": ALG_BYTES_PER_EPISODE,
                                         "note": "bf16 activations: 3 x 12.9 MB per frame (SURVEY 8d); whole-job average, not one kernel"}
        out["other_modes"] = other
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(a.shot, a.cpu_episodes)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def dump_outputs(out_dir, last, bucket, student, sample=1 << 22, seed=20240):
    """--dump-outputs: what the timed path computed, read right after its last step (the device is idle), as float32 .npy files:
    loss / accuracy of the last episode (what train_task returns), a sample of `sample` flat indices - fixed by `seed`, the same in every
    run - of the weights (bucket.flat, 22.7 M floats for the default student) and of the gradient accumulated since the last optimizer
    step (grad + the side streams' shadow), and the student's BatchNorm running statistics in state_dict order.  32 MB in all."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)

    def save(name, t):
        np.save(os.path.join(out_dir, name + ".npy"), torch.as_tensor(t).detach().float().cpu().reshape(-1).numpy())
    if last is not None:
        if isinstance(last, list):      # a pipeline flush or a graphed interval: one result per episode, the last one is the step's
            last = last[-1]
        save("loss", last[0])
        save("accuracy", last[1])
    n = bucket.flat.numel()
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:min(sample, n)].sort().values.to(bucket.flat.device)
    save("weights_sample", bucket.flat[idx])
    grad = bucket.grad if bucket.shadow is None else bucket.grad + bucket.shadow
    save("grad_sample", grad[idx])
    stats = [v.reshape(-1).float() for k, v in student.state_dict().items() if k.endswith(("running_mean", "running_var"))]
    if stats:
        save("bn_running_stats", torch.cat(stats))


class HostEpisodes:
    """what a loader's worker processes hand over (video_reader.py:474-485 before ToTensor): decoded uint8 frames of an episode's 50 videos
    (8 frames of 320x240x3 each, HMDB's resolution: 92 MB), the crop / flip draws, 3.3 MB of teacher features, shuffled labels - two
    seeded episodes in host memory, cycled"""

    def __init__(self, cfg, n=2, seed=4321):
        import random
        from litemkd_amd.video_transform import GpuFrameTransform
        way, L = cfg.way, cfg.seq_len
        ns, nq = way * cfg.shot, way * cfg.query_per_class
        g = torch.Generator().manual_seed(seed)
        tf = GpuFrameTransform(cfg.img_size, "cpu")
        state = random.getstate()
        random.seed(99)
        self.eps = [{"frames": torch.randint(0, 256, ((ns + nq) * L, 240, 320, 3), dtype=torch.uint8, generator=g).pin_memory(),      # (a worker that decodes into pinned memory)
                     "params": [tf.draw(240, 320, True) for _ in range(ns + nq)],
                     "features": torch.randn(ns + nq, L, 2048, generator=g).pin_memory(), "ns": ns,
                     "support_labels": torch.arange(way).repeat_interleave(cfg.shot)[torch.randperm(ns, generator=g)].float(),
                     "target_labels": torch.arange(way).repeat_interleave(cfg.query_per_class)[torch.randperm(nq, generator=g)].float()}
                    for _ in range(n)]
        random.setstate(state)
        self.i = 0

    def host_episode(self):
        e = self.eps[self.i % len(self.eps)]
        self.i += 1
        return e


def stream_inputs_pass(a, cfg, dev, run, state, fence, TL, episodes=None):
    """The input side inside the PRODUCT loop, under the schedule that is timed (trainwandb.py:87-88 the DataLoader worker, :419-443
    prepare_task, video_reader.py:474-485 the loader's output): trainloop.StreamedEpisodes - a prefetch thread pins the next host episodes,
    a copy stream uploads 92 MB of uint8 frames + 3.3 MB of teacher features per episode and runs Resize(256) -> crop 224 / flip ->
    ToTensor as HIP kernels into one of three static input sets, the compute streams wait for a set's `ready` event and hand it back
    through events of their own - feeding the same loop (`run`: cross-episode pipelining, optimizer cadence) as the headline line."""
    n = episodes or a.steps
    loader = TL.StreamedEpisodes(HostEpisodes(cfg), cfg, dev)
    state["episodes"] = iter(loader)
    try:
        it = run(3, 0)
        fence()
        t0 = time.perf_counter()
        run(n, it)
        fence()
        dt = time.perf_counter() - t0
    finally:
        state["episodes"] = None
        loader.close()
    s0 = loader.sets[0]
    nbytes = s0["u8"].numel() + 4 * s0["feat"].numel()
    return {"value": n / dt, "unit": "episodes/s", "steps": n, "h2d_bytes_per_episode": nbytes,
            "pcie_GBps_needed": nbytes * (n / dt) / 1e9,
            "what": "the headline loop (same schedule) with every episode's inputs streamed from host memory by trainloop.StreamedEpisodes (prefetch "
                    "thread, pinned uint8 frames 320x240 + teacher features, H2D + GPU frame transform on a copy stream, three static input "
                    "sets); compare with `value` (inputs resident in HBM)"}


def usable_cores():
    """cores this process may actually use: min(affinity mask, cgroup cpu quota), capped at 32 (the CPU convs do
    not scale beyond that; oversubscribing 256 hardware threads from a 16-core share made the first run 10x slower)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, min(n, 32))


def cpu_baseline(shot, episodes=3):
    """The CPU oracle (oracle/ref_cpu.py: torch-CPU fp32 restatement of the same training episode) timed on this
    box's host cores.  Bounded sample: `episodes` full training episodes of the benchmark workload (~5 s each on a
    16-core share), no warm-up, gradients accumulating as in the reference loop."""
    from oracle import ref_cpu as O
    n = usable_cores()
    torch.set_num_threads(n)
    params = O.make_student_params(11)
    for k, v in params.items():
        if v.is_floating_point() and "running" not in k and not k.endswith("pe.pe"):
            v.requires_grad_()
    tp = O.make_trx_params(torch.Generator().manual_seed(12))
    eps = [O.make_episode(7 + i, 5, shot, 5) for i in range(episodes)]
    t0 = time.perf_counter()
    for ep in eps:
        O.train_episode(ep, params, tp, 5, shot)
    dt = time.perf_counter() - t0
    return {"value": episodes / dt, "unit": "episodes/s", "cores": n, "kind": "port",
            "sample": "%d full 5-way %d-shot 224^2 training episodes (fwd+loss+bwd) on the torch-CPU fp32 oracle, %.1f s" % (episodes, shot, dt)}


if __name__ == "__main__":
    main()
