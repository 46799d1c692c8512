"""Measurements of the GPU PNG decoder, on one MI355X:

    python tools/png_bench.py [--out profiles/png_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/png_bench.py --decode-only
    python tools/png_bench.py --merge-kernel-stats DIR --out profiles/png_bench.json      (no GPU: adds the per-kernel times to the file)

The frames are those of tools/jpeg_bench.py (400 seeded frames of 320x240 RGB), written as PNG by PIL at its default compression level.
Reports:
  * compressed_MB_per_400_frames, decoded_MB_per_400_frames;
  * decode_ms_per_400_frames: PngPlan.decode of one 400-frame batch (upload + the two launches) by device events, after warm-up: median,
    min and max of --reps repeats;
  * plan_ms_per_400_frames: the host half (lmkd_png_plan: chunk walk, CRC-32, IDAT compaction, + packing);
  * pil_ms_per_400_frames_16_threads: PIL decoding the same 400 files on 16 host threads, in the same run (the median of three passes,
    all three in pil_ms_runs);
  * jpeg_q75: the same figures of the JPEG decoder for the same frames at quality 75, from the same process (context);
  * kernels (after --merge-kernel-stats): the average time of each kernel over the --decode-only run."""
import argparse
import csv
import glob
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def encode_png(img):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "PNG")
    return b.getvalue()


def decode_bench(blobs, reps):
    from litemkd_amd import decode
    for _ in range(3):
        decode.png_decode(blobs, check=False)
    torch.cuda.synchronize()
    frames, status = decode.png_decode(blobs, check=False)
    if int(status.cpu().abs().sum()) or decode.png_stats()["fallback"]:
        raise RuntimeError("the benchmark's frames must all decode on the GPU")
    plans = [decode.PngPlan(blobs) for _ in range(2)]
    t0 = time.perf_counter()
    for _ in range(max(3, reps // 4)):
        decode.PngPlan(blobs, fallback=False)
    plan_ms = (time.perf_counter() - t0) / max(3, reps // 4) * 1e3
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
    return {"decode_ms_per_400_frames": float(np.median(times)), "decode_ms_min": float(np.min(times)), "decode_ms_max": float(np.max(times)),
            "repeats": reps, "plan_ms_per_400_frames": plan_ms, "compressed_MB_per_400_frames": sum(len(b) for b in blobs) / 1e6,
            "decoded_MB_per_400_frames": out.numel() / 1e6}


def pil_runs(J, blobs, runs=3):
    """the host figure moves from run to run with what else the host does: the median of `runs`, and all of them"""
    t = sorted(J.pil_bench(blobs) for _ in range(runs))
    return {"pil_ms_per_400_frames_16_threads": t[len(t) // 2], "pil_ms_runs": t}


def merge_kernel_stats(directory, path):
    rows = {}
    for f in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = r.get("Name", "")
                if "png_" in name or "jpeg_" in name:
                    rows[name.replace("(anonymous namespace)::", "").split("(")[0]] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3,
                                                                 "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
    if not rows:
        raise RuntimeError("no kernel_stats.csv with the decoder's kernels under %s" % directory)
    with open(path) as fh:
        res = json.load(fh)
    res["kernels"] = rows
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--decode-only", action="store_true")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--merge-kernel-stats", default=None)
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a.merge_kernel_stats, a.out)
    import jpeg_bench as J
    import litemkd_amd
    litemkd_amd.lib().call("lmkd_device_check", 0)
    frames = [J.frame(i) for i in range(400)]
    blobs = [encode_png(f) for f in frames]
    res = {"frames": "320x240 RGB, PIL's default PNG encoder settings", "batch": 400}
    res.update(decode_bench(blobs, a.reps))
    if not a.decode_only:
        res.update(pil_runs(J, blobs))
        jb = [J.encode(f, 75) for f in frames]
        r = J.decode_bench(jb, reps=a.reps)
        r.update(pil_runs(J, jb))
        res["jpeg_q75"] = r
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
