"""Measurements of the GPU JPEG decoder, on one MI355X:

    python tools/jpeg_bench.py [--out profiles/jpeg_bench.json] [--decode-only]

A seeded dataset of 320x240 4:2:0 frames at quality 75 and 90 (typical extracted frames), written with PIL under a temporary directory.
Reports, per quality:
  * decode_ms_per_400_frames: decode.jpeg_decode of one 400-frame batch (upload + three launches), device events, after warm-up;
  * plan_ms_per_400_frames: the host half (lmkd_jpeg_plan + packing), and host_episode_ms: JpegFrameEpisodes.host_episode() - file reads,
    plan, draws, features - what the prefetch thread does per 5-way 5-shot episode;
  * pil_ms_per_400_frames_16_threads: PIL decoding the same 400 frames on 16 host threads;
  * train episodes/s at 5-way 5-shot 224 through StreamedEpisodes with JpegFrameEpisodes, against the same decoded frames as .npy through
    ClipDirectoryEpisodes; the two runs alternate and repeat (--repeats) so the spread is visible.
--decode-only runs only the decode loop (for `rocprofv3 --kernel-trace --stats -- python tools/jpeg_bench.py --decode-only`: the time of
each of the three kernels)."""
import argparse
import io
import json
import os
import random
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame(seed, h=240, w=320):
    """a natural-looking synthetic frame: smooth shading, edges, texture"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = g.uniform(0, w), g.uniform(0, h)
    base = 120 + 80 * np.sin((x - cx) / g.uniform(15, 40)) * np.cos((y - cy) / g.uniform(15, 40))
    edges = 60 * (((x + 2 * y) // g.uniform(20, 60)) % 2)
    a = np.stack([base + edges, base * 0.8 + 40, 200 - base * 0.5 + edges * 0.5], -1) + g.normal(0, 8, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(img, q):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q, subsampling=2)
    return b.getvalue()


def decode_bench(blobs, reps=20):
    from litemkd_amd import decode
    for _ in range(3):
        decode.jpeg_decode(blobs, check=False)
    torch.cuda.synchronize()
    plans = [decode.JpegPlan(blobs) for _ in range(2)]
    t0 = time.perf_counter()
    for _ in range(reps):
        decode.JpegPlan(blobs, fallback=False)
    plan_ms = (time.perf_counter() - t0) / reps * 1e3
    out = torch.empty((len(blobs), 240, 320, 3), dtype=torch.uint8, device="cuda")
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for r in range(reps):
        p = plans[r % 2]
        torch.cuda.synchronize()
        s.record()
        p.decode(out=out, check=False)
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    return {"decode_ms_per_400_frames": float(np.median(times)), "decode_ms_min": float(np.min(times)), "plan_ms_per_400_frames": plan_ms,
            "compressed_MB_per_400_frames": sum(len(b) for b in blobs) / 1e6}


def pil_bench(blobs, threads=16, reps=3):
    from PIL import Image

    def dec(b):
        with Image.open(io.BytesIO(b)) as im:
            im.load()
            return im.size
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(dec, blobs))
        t0 = time.perf_counter()
        for _ in range(reps):
            list(ex.map(dec, blobs))
    return (time.perf_counter() - t0) / reps * 1e3


def make_tree(root, q, classes=5, videos=10, frames=12):
    """<root>/jpg/<class>/<video>/<frame>.jpg + the same decoded frames as <root>/npy/<class>/<video>.npy + teacher features"""
    from PIL import Image
    for c in range(classes):
        for v in range(videos):
            d = os.path.join(root, "jpg", "c%d" % c, "v%d_%d" % (c, v))
            fd = os.path.join(root, "feat", "c%d" % c, "v%d_%d" % (c, v))
            os.makedirs(d)
            os.makedirs(fd)
            os.makedirs(os.path.join(root, "npy", "c%d" % c), exist_ok=True)
            dec = []
            for f in range(frames):
                data = encode(frame(1000 * c + 10 * v + f), q)
                with open(os.path.join(d, "%05d.jpg" % f), "wb") as fh:
                    fh.write(data)
                dec.append(np.array(Image.open(io.BytesIO(data))))
            np.save(os.path.join(root, "npy", "c%d" % c, "v%d_%d.npy" % (c, v)), np.stack(dec))
            fe = np.random.default_rng(c * 100 + v).standard_normal((8, 2048)).astype(np.float32)
            np.save(os.path.join(root, "npy", "c%d" % c, "v%d_%d.feature.npy" % (c, v)), fe)
            np.save(os.path.join(fd, "feature.npy"), fe)


def train_rate(root, jpeg, n=64, warm=24):
    from litemkd_amd import trainloop as TL
    from litemkd_amd.options import default_args
    from litemkd_amd.schedule import Schedule
    from litemkd_amd.train import ClipDirectoryEpisodes, JpegFrameEpisodes
    dev = torch.device("cuda", 0)
    cfg = default_args(device=dev, training_iterations=n, print_freq=10 ** 9, save_freq=10 ** 9)
    sched = Schedule.bench(conv_dtype="fp32h2")
    torch.manual_seed(0)
    random.seed(0)
    stamps = []
    with sched.applied():
        student, teacher, _, distiller, acc_fn, _, opt, sch = TL.make(cfg)
        src = (JpegFrameEpisodes(cfg, os.path.join(root, "jpg"), teacher_path=os.path.join(root, "feat"), device=dev, length=n) if jpeg
               else ClipDirectoryEpisodes(cfg, os.path.join(root, "npy"), device=dev, length=n))
        loader = TL.StreamedEpisodes(src, cfg, dev)

        def timed():
            for td in loader:
                stamps.append(time.perf_counter())
                yield td
        TL.train(student, teacher, timed(), distiller, opt, sch, acc_fn, cfg, schedule=sched)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        loader.close()
    return (n - warm) / (t1 - stamps[warm])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--decode-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    res = {"frames": "320x240 4:2:0", "batch": 400}
    for q in (75, 90):
        blobs = [encode(frame(i), q) for i in range(400)]
        r = decode_bench(blobs, reps=50 if a.decode_only else 20)
        if not a.decode_only:
            r["pil_ms_per_400_frames_16_threads"] = pil_bench(blobs)
        res["q%d" % q] = r
        print(json.dumps({"q%d" % q: r}), flush=True)
    if not a.decode_only:
        from litemkd_amd.options import default_args
        from litemkd_amd.train import JpegFrameEpisodes
        with tempfile.TemporaryDirectory() as tmp:
            make_tree(tmp, 75)
            cfg = default_args(device="cuda")
            ds = JpegFrameEpisodes(cfg, os.path.join(tmp, "jpg"), teacher_path=os.path.join(tmp, "feat"), device="cuda")
            random.seed(0)
            for _ in range(4):
                ds.host_episode()["plan"].release()
            t0 = time.perf_counter()
            for _ in range(16):
                ds.host_episode()["plan"].release()
            res["host_episode_ms"] = (time.perf_counter() - t0) / 16 * 1e3
            rates = {"jpeg": [], "npy": []}
            for _ in range(a.repeats):
                for kind in ("npy", "jpeg"):
                    rates[kind].append(train_rate(tmp, kind == "jpeg"))
                    print(json.dumps({kind: rates[kind][-1]}), flush=True)
            res["train_episodes_per_s"] = rates
            res["jpeg_over_npy"] = float(np.median(rates["jpeg"]) / np.median(rates["npy"]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
