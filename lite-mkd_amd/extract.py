"""Writes the teacher's features: `python -m litemkd_amd.extract --stage modality | fusion` (reference: teacher/code/extract_feature.py and
extract_multi_feature.py).

--stage modality: a pretrained Action_Recognition_Resnet50 (--checkpoint_dir: a best_checkpoint.pt of litemkd_amd.pretrain or the directory
holding it; or --init_weights alone) in eval mode over the videos of {mode}list{split:02d}.txt, frames chosen, decoded and transformed as
litemkd_amd.pretrain does, --videos_per_call videos per trunk call (eval BatchNorm makes frames independent) ->
<out>/<modality>/<class>/<video>/feature.npy, float32 [seq_len, 2048]: the tree train_teacher's --feature_save_path reads.
  Deviation: the reference assigns the STRING args.mode to dataset.train (extract_feature.py:81); a non-empty string is true, so it always
  extracts under the random flip and crop of training.  Here the default is Resize + CenterCrop, which makes the features reproducible;
  --augment --seed gives the reference's behaviour (the draws of one video in the reference's order: flip, then crop).

--stage fusion: the three modality trees <feature_save_path>/{rgb,depth,flow}/<class>/<video>/feature.npy and a train_teacher checkpoint
(checkpoint<N>.pt with its "model_state_dict", or the bare state dict of checkpoint_final.pt; the keys of the TRX head are not needed)
through ThreeTRXShiftLoopTime.extract_feature -> <out>/<class>/<video>/feature.npy, what train's --teacher_path reads.  The videos are
those of the rgb tree; the encoder depth is read from the checkpoint.

Both stages skip videos whose file exists under --resume, and print one JSON line at the end with counts and videos per second."""
import argparse
import json
import os
import random
import time

import numpy as np
import torch

from . import pretrain as PT

MODALITIES = ("rgb", "depth", "flow")      # the keys ThreeTRXShiftLoopTime.extract_feature reads (AuxDataset.get_feature_seq)


def build_parser():
    p = argparse.ArgumentParser(description="Extract per-modality or fused teacher features")
    p.add_argument("--stage", choices=["modality", "fusion"], default="modality")
    p.add_argument("--out", default=None, help="modality: root of <modality>/<class>/<video>/feature.npy; fusion: root of <class>/<video>/feature.npy")
    p.add_argument("--checkpoint_dir", default=None, help="the checkpoint file (modality: or the directory holding best_checkpoint.pt)")
    p.add_argument("--resume", action="store_true", help="skip videos whose feature.npy exists")
    p.add_argument("--seq_len", default=8, type=int)
    # stage modality
    p.add_argument("--path", default=None, help="frame folders <path>/<class>/<video>/*.{jpg,jpeg,png} of one modality; non-RGB frames (depth maps) are converted as "
                        "the reference's Image.open(path).convert('RGB') does")
    p.add_argument("--modality", default="rgb", type=str)
    p.add_argument("--traintestlist", default=None)
    p.add_argument("--split", default=3, type=int)
    p.add_argument("--mode", default="test")
    p.add_argument("--img_size", default=224, type=int)
    p.add_argument("--num_classes", type=int, default=64, help="without a checkpoint; a checkpoint's fc decides otherwise")
    p.add_argument("--init_weights", default=None, help="a torchvision resnet50 state-dict file, when there is no checkpoint")
    p.add_argument("--videos_per_call", type=int, default=8)
    p.add_argument("--augment", action="store_true", help="the reference's behaviour: random flip and crop")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--num_workers", type=int, default=1)
    # stage fusion
    p.add_argument("--feature_save_path", default=None, help="root of {rgb,depth,flow}/<class>/<video>/feature.npy")
    p.add_argument("--shirt_num", type=int, default=1)
    # accepted for the reference's command lines
    p.add_argument("--model", type=str, default=None)
    p.add_argument("--method", default="resnet50")
    p.add_argument("--getitem_name", type=str, default=None)
    p.add_argument("--num_gpus", type=int, default=1)
    p.add_argument("--dataset", type=str, default="hmdb")
    p.add_argument("--base_model", default="TRM", type=str)
    p.add_argument("--trans_num", default=None, type=int, help="ignored: the checkpoint's encoder depth is used")
    p.add_argument("--temp_set", nargs="+", type=int, default=[2])
    p.add_argument("--trans_linear_out_dim", type=int, default=1152)
    p.add_argument("--trans_dropout", type=float, default=0.1)
    return p


def args_check(parser, args):
    if not args.out:
        parser.error("--out is needed")
    if args.stage == "modality":
        if not args.path or not args.traintestlist:
            parser.error("--stage modality needs --path and --traintestlist")
        if not args.checkpoint_dir and not args.init_weights:
            parser.error("--stage modality needs --checkpoint_dir or --init_weights")
        if args.videos_per_call < 1:
            parser.error("--videos_per_call must be at least 1")
    else:
        if not args.feature_save_path or not args.checkpoint_dir:
            parser.error("--stage fusion needs --feature_save_path and --checkpoint_dir")
        from .ops import MFM_MAX_L
        if not 1 <= args.seq_len <= MFM_MAX_L:
            parser.error("--seq_len %d: the fusions take clips of 1 to %d frames" % (args.seq_len, MFM_MAX_L))
    return args


def _save(path, feature):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = path + ".tmp.npy"
    np.save(tmp, np.ascontiguousarray(feature, dtype=np.float32))
    os.replace(tmp, path)      # a run that is cut short leaves no half-written file for --resume to skip


def _summary(stage, written, skipped, t0, **extra):
    dt = time.time() - t0
    rec = {"stage": stage, "written": written, "skipped": skipped, "seconds": round(dt, 3), "videos_per_s": round(written / dt, 3) if dt > 0 else None}
    rec.update(extra)
    print(json.dumps(rec), flush=True)
    return rec


# ---- stage modality ----
def modality_checkpoint_state(path):
    """-> the model state dict of a pretrain checkpoint file, or of <path>/best_checkpoint.pt"""
    if os.path.isdir(path):
        path = os.path.join(path, "best_checkpoint.pt")
    ck = torch.load(path, map_location="cpu")
    return ck["model_state_dict"] if "model_state_dict" in ck else ck


def build_modality_model(args, device):
    sd = modality_checkpoint_state(args.checkpoint_dir) if args.checkpoint_dir else None
    if sd is not None:
        args.num_classes = int(sd["fc.weight"].shape[0])
    model = PT.build_model(args, device)      # --init_weights first, the checkpoint over it
    if sd is not None:
        from . import ops
        with torch.no_grad():
            model.load_state_dict(sd, strict=True)
        ops.WEIGHT_EPOCH[0] += 1
    return model.eval()


def extract_modality(model, args, device, load_batch=None):
    """the walk of the stage: the list in order, --videos_per_call videos per model call.  load_batch(entries) -> the model's input for
    those videos, [len(entries) * seq_len, ...] (default: read, decode and transform the frames) -> the summary record"""
    entries = PT.read_video_list(args.traintestlist, args.mode, args.split)
    root = os.path.join(args.out, args.modality)
    t0 = time.time()
    todo, skipped = [], 0
    for e in entries:
        if args.resume and os.path.isfile(os.path.join(root, e, "feature.npy")):
            skipped += 1
        else:
            todo.append(e)
    if load_batch is None:
        tf = PT.frame_transform(args.img_size, device)

        def load_batch(batch):
            return PT.load_clips(PT.plan_clips(args.path, batch, args.seq_len), len(batch), args.seq_len, tf, bool(args.augment))[0]
    written, calls = 0, 0
    for o in range(0, len(todo), args.videos_per_call):
        batch = todo[o:o + args.videos_per_call]
        feats = model.extract_feature(load_batch(batch)).reshape(len(batch), args.seq_len, -1).cpu().numpy()
        calls += 1
        for e, f in zip(batch, feats):
            _save(os.path.join(root, e, "feature.npy"), f)
            written += 1
    return _summary("modality", written, skipped, t0, modality=args.modality, mode=args.mode, model_calls=calls, out=root)


# ---- stage fusion ----
def fusion_checkpoint_state(path):
    """-> the fusion's state dict from checkpoint<N>.pt ({"model_state_dict": ...}) or checkpoint_final.pt (the state dict alone), without
    the keys of the TRX head"""
    ck = torch.load(path, map_location="cpu")
    sd = ck["model_state_dict"] if isinstance(ck, dict) and "model_state_dict" in ck else ck
    sd = {k: v for k, v in sd.items() if not k.startswith("bracnch.")}
    if not any(k.startswith("three_fusion.") for k in sd) or not any(k.startswith("fusion.") for k in sd):
        raise KeyError("%s holds no `fusion.*` / `three_fusion.*` entries: not a checkpoint of the MFM teacher" % path)
    return sd


def build_fusion_model(args, device):
    from .teacher.mfm import ThreeTRXShiftLoopTime
    sd = fusion_checkpoint_state(args.checkpoint_dir)
    layers = {int(k.split(".")[3]) for k in sd if k.startswith("fusion.transformer_encoder.layers.")}
    args.trans_num = len(layers)
    with torch.device(device):      # constructed where it runs: the default initialisation of 10^8 weights is then a device fill
        model = ThreeTRXShiftLoopTime(args)
    with torch.no_grad():
        model.load_state_dict(sd, strict=True)
    return model.eval()


def feature_tree_videos(root):
    """[(class, video)] of one modality tree, sorted"""
    out = []
    for cname in sorted(os.listdir(root)):
        d = os.path.join(root, cname)
        if os.path.isdir(d):
            out += [(cname, v) for v in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, v, "feature.npy"))]
    return out


def extract_fusion(model, args, device):
    first = os.path.join(args.feature_save_path, MODALITIES[0])
    if not os.path.isdir(first):
        raise ValueError("no %s features under %s" % (MODALITIES[0], args.feature_save_path))
    t0 = time.time()
    written = skipped = 0
    for cname, vid in feature_tree_videos(first):
        dst = os.path.join(args.out, cname, vid, "feature.npy")
        if args.resume and os.path.isfile(dst):
            skipped += 1
            continue
        feature = {}
        for m in MODALITIES:      # AuxDataset.get_feature_seq: all three are read, a missing one raises
            f = np.load(os.path.join(args.feature_save_path, m, cname, vid, "feature.npy"))
            if f.shape != (args.seq_len, 2048):
                raise ValueError("%s/%s/%s: feature of shape %s, expected (%d, 2048)" % (m, cname, vid, f.shape, args.seq_len))
            feature[m] = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).unsqueeze(0).to(device)
        out = model.extract_feature(feature)
        _save(dst, out.reshape(args.seq_len, -1).cpu().numpy())
        written += 1
    return _summary("fusion", written, skipped, t0, out=args.out)


def main(argv=None):
    parser = build_parser()
    args = args_check(parser, parser.parse_args(argv))
    if not torch.cuda.is_available():
        raise RuntimeError("extract needs the GPU: the trunk and the fusions have no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if args.stage == "modality":
        return extract_modality(build_modality_model(args, dev), args, dev)
    return extract_fusion(build_fusion_model(args, dev), args, dev)


if __name__ == "__main__":
    main()
