"""Attention-map overlays of a trained student (reference: heatmap_vis.py:20-48, teacher/code/heatmap_vis.py:16-27, which lay
Grad-CAM of a torchvision network over one frame; here the maps are the few-shot student's own, cam.grad_cam).

    python -m litemkd_amd.heatmap --test_model_path model_save/<ckpt>.pt --out_dir heatmaps --episodes 4

takes the evaluator's flags (evaluate.py), so an evaluator command line can be reused as it is: --rgb_path (with --traintestlist /
--split) reads the test split of the reference's JPEG frame tree, without it synthetic test episodes; without --test_model_path the
student keeps its initial weights.  The maps are the student's: --test_model teacher is refused (teachers read features, not frames),
and --model_teacher, --teacher_checkpoint, --teacher_path and --num_test_tasks are accepted and unused (--episodes counts the episodes).
Per episode k:

    <out_dir>/ep<k>/q<i>_true<c>_pred<c'>/frame<j>.png     the frames of query video i under its map for class c' (--who query | both)
    <out_dir>/ep<k>/s<i>_class<c>/frame<j>.png             the frames of support video i under the evidence all queries drew (--who support | both)
    <out_dir>/ep<k>/maps.npz                               raw and normalised maps of both frame sets, logits, targets, labels"""
import os

import numpy as np
import torch

from . import cam, ops
from . import trainloop as TL
from .model.model_select import Student, load_student
from .options import default_args


def write_episode(out, images, labels, who, ep_dir, seq_len, image_weight):
    """the PNGs and maps.npz of one episode; images / labels: {"support": ..., "query": ...} -> the directories written"""
    from PIL import Image
    pred = out["target"].cpu().numpy()
    dirs = []
    for name in ("query", "support"):
        if who not in (name, "both"):
            continue
        x = images[name]
        u8 = cam.frames_to_u8(x)
        over = ops.cam_overlay(out[name]["cam"], u8, u8.shape[1:3], image_weight=image_weight).cpu().numpy()
        lab = labels[name].cpu().numpy().astype(np.int64)
        for i in range(over.shape[0] // seq_len):
            d = os.path.join(ep_dir, "q%d_true%d_pred%d" % (i, lab[i], pred[i]) if name == "query" else "s%d_class%d" % (i, lab[i]))
            os.makedirs(d, exist_ok=True)
            dirs.append(d)
            for j in range(seq_len):
                Image.fromarray(over[i * seq_len + j], "RGB").save(os.path.join(d, "frame%d.png" % j))
    np.savez(os.path.join(ep_dir, "maps.npz"), logits=out["logits"].cpu().numpy(), target=pred,
             support_labels=labels["support"].cpu().numpy(), query_labels=labels["query"].cpu().numpy(),
             **{"%s_%s" % (n, k): out[n][k].cpu().numpy() for n in ("support", "query") for k in ("raw", "cam")})
    return dirs


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser()
    base = default_args()
    for k in ("test_model", "test_model_path", "teacher_checkpoint", "model_backbone", "model_classifier", "model_teacher", "distill_name",
              "dataset", "mode"):
        ap.add_argument("--" + k, default=getattr(base, k))
    for k in ("num_test_tasks", "way", "shot", "query_per_class_test", "seq_len", "img_size", "trans_linear_out_dim"):
        ap.add_argument("--" + k, type=int, default=getattr(base, k))
    ap.add_argument("--rgb_path", default=None, help="<rgb_path>/<class>/<video>/<frame>.jpg or an uncompressed .zip of it")
    ap.add_argument("--traintestlist", default=None, help="directory of the split lists {train,test}list<split>.txt")
    ap.add_argument("--teacher_path", default=None, help="the evaluator's; unused here")
    ap.add_argument("--split", type=int, default=getattr(base, "split", 3))
    ap.add_argument("--temp_set", nargs="+", type=int, default=list(base.temp_set))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out_dir", default="heatmaps")
    ap.add_argument("--episodes", type=int, default=1)
    ap.add_argument("--method", choices=sorted(cam.METHODS), default="gradcam")
    ap.add_argument("--who", choices=("query", "support", "both"), default="query")
    ap.add_argument("--image_weight", type=float, default=0.5, help="share of the frame in the overlay")
    a = ap.parse_args(argv)
    if a.test_model != "student":
        ap.error("--test_model %s: attention maps are the student's (a teacher reads features, not frames)" % a.test_model)
    own = ("rgb_path", "traintestlist", "teacher_path", "seed", "out_dir", "episodes", "method", "who", "image_weight")
    args = default_args(**{k: v for k, v in vars(a).items() if k not in own})
    torch.manual_seed(a.seed)
    student = (load_student(args) if args.test_model_path else Student(args)).to(args.device)
    if a.rgb_path:
        import random
        from .train import JpegFrameEpisodes
        random.seed(a.seed)
        loader = JpegFrameEpisodes(args, a.rgb_path, a.traintestlist, None, split=a.split, device=args.device, train=False)
    else:
        loader = TL.SyntheticEpisodes(args, base_seed=777 + a.seed, device=args.device, train=False)
    written = []
    for k, task_dict in enumerate(loader):
        if k >= a.episodes:
            break
        (context_images, target_images, _, _, context_labels, target_labels, _, _) = TL.prepare_task(task_dict, args.device)
        out = cam.grad_cam(student, context_images, context_labels, target_images, method=a.method)
        ep_dir = os.path.join(a.out_dir, "ep%d" % k)
        os.makedirs(ep_dir, exist_ok=True)
        written += write_episode(out, {"support": context_images, "query": target_images}, {"support": context_labels, "query": target_labels},
                                 a.who, ep_dir, args.seq_len, a.image_weight)
        print("episode %d: %d query videos, accuracy %.2f -> %s" % (k, out["target"].numel(),
                                                                    (out["target"] == target_labels.to(out["target"].device)).float().mean().item(), ep_dir))
    return written


if __name__ == "__main__":
    main()
