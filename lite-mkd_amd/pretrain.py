"""Pretrains the teacher's per-modality feature extractor as a clip classifier (reference: teacher/code/pretrain/pretrain.py with
AuxDataset.get_video_with_label), on one GPU: `python -m litemkd_amd.pretrain`.  The model is teacher.action_recognition.
Action_Recognition_Resnet50; the loss ops.softmax_ce (any class count), the optimizer trainloop.MomentumSGD with the groups `convnet`
(lr_1) and `fc` (lr_2), each under a trainloop.StepLR(10, 0.1).

Data: the videos of {mode}list{split:02d}.txt under --traintestlist (spaces become '_', the first field of a line is <class>/<video>),
a label being the class's index in order of first appearance in trainlist03.txt (utils.parsing_label); the frames
<path>/<class>/<video>/*.jpg, *.jpeg and *.png, sorted by name (any modality: a depth tree of single-channel PNGs is converted to RGB
as AuxDataset.read_single_image does, Image.open(path).convert("RGB")); the frame choice AuxDataset.get_seq's, which followed through is int(linspace(0, n - 1, seq_len))
in every mode and for every n (a longer video is first subsampled to seq_len files and then taken whole; a shorter one falls through to
the same linspace, frames repeating).  Frames are decoded on the GPU (decode.ImagePlan: JPEG and PNG) and transformed by GpuFrameTransform: Resize,
random flip and crop in --mode train, centre crop otherwise.  An --img_size other than 84 / 224 resizes to round(img_size * 8 / 7).

The loop keeps pretrain.py as it behaves:
  * both schedulers step at the START of each epoch (:108-109), so the first epoch already counts towards the 10;
  * the evaluation pass after each epoch runs the model in eval mode over the SAME loader, shuffle and training augmentation included:
    `video_loader.train = False` (:145) sets an attribute nothing reads;
  * its accuracy divides by 8 per batch (:162) whatever the batch holds (a smaller last batch, another --batch_size);
  * best_checkpoint.pt {iteration (the epoch, from 1), model_state_dict, optimizer1_state_dict, optimizer2_state_dict, scheduler1,
    scheduler2} is written when that accuracy improves on the best of THIS run (:166-169);
  * --resume loads that file and the epochs count from 1 again, with the restored schedulers continuing (:185-193 reads start_iteration
    and nothing uses it).
The reference's `pretrained=True` downloads ImageNet weights; here --init_weights names a torchvision resnet50 state-dict file, and
without it the trunk keeps its own initialisation.  Loss and accuracy stay on the device between prints (every 50 batches, :135-139)."""
import argparse
import json
import os
import random
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import decode, ops
from . import trainloop as TL

PRINT_EVERY = 50      # pretrain.py:135
ACC_DENOMINATOR = 8      # pretrain.py:162


def _flag(v):
    return str(v).lower() in ("1", "true", "yes", "y", "t")


def build_parser():
    p = argparse.ArgumentParser(description="Pretrain the teacher's per-modality ResNet-50 as a clip classifier")
    p.add_argument("--path", type=str, help="frame folders <path>/<class>/<video>/*.{jpg,jpeg,png} of one modality (RGB, depth, flow, ...)")
    p.add_argument("--modality", default="rgb", type=str)
    p.add_argument("--traintestlist", default="splits/pretrain/kinetics", type=str)
    p.add_argument("--split", default=3, type=int)
    p.add_argument("--mode", default="train")
    p.add_argument("--seq_len", default=8, type=int)
    p.add_argument("--img_size", default=224, type=int)
    p.add_argument("--num_classes", type=int, default=64)
    p.add_argument("--lr_1", type=float, default=0.000001, help="learning rate of the trunk")
    p.add_argument("--lr_2", type=float, default=0.01, help="learning rate of fc")
    p.add_argument("--checkpoint_dir", "-c", type=str, help="where best_checkpoint.pt is written")
    p.add_argument("--resume", "-r", type=_flag, nargs="?", const=True, default=False)
    p.add_argument("--num_workers", type=int, default=1, help="host threads reading and planning the next batches")
    p.add_argument("--init_weights", default=None, help="a torchvision resnet50 state-dict file for the trunk (the reference downloads one)")
    p.add_argument("--epochs", type=int, default=50)
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--seed", type=int, default=0)
    # accepted for the reference's command lines; one model, one GPU here
    p.add_argument("--model", type=str, default="Action_Recognition_Resnet50")
    p.add_argument("--method", default="resnet50")
    p.add_argument("--getitem_name", type=str, default="get_video_with_label")
    p.add_argument("--num_gpus", type=int, default=1)
    p.add_argument("--dataset", type=str, default="hmdb")
    p.add_argument("--learning_rate", "-lr", type=float, default=0.1)
    p.add_argument("--temp_set", nargs="+", type=int, default=[2])
    p.add_argument("--trans_linear_out_dim", type=int, default=1152)
    p.add_argument("--trans_dropout", type=float, default=0.1)
    return p


def args_check(parser, args):
    if args.model != "Action_Recognition_Resnet50":
        parser.error("--model %s: this module trains Action_Recognition_Resnet50" % args.model)
    if not args.path or not args.checkpoint_dir:
        parser.error("--path and --checkpoint_dir are needed")
    return args


# ---- data ----
def frame_indices(n, seq_len):
    """AuxDataset.get_seq followed through for a video of n frames (module docstring)"""
    if n < 1:
        raise ValueError("No frames found")
    return [int(f) for f in np.linspace(0, n - 1, seq_len)]


def _list_entries(path):
    with open(path) as f:
        data = [x.replace(" ", "_") for x in f.readlines()]
    return [x.strip().split(" ")[0] for x in data if x.strip()]


def read_video_list(traintestlist, mode, split):
    """AuxDataset._select_fold: the <class>/<video> entries of {mode}list{split:02d}.txt"""
    return _list_entries(os.path.join(traintestlist, "{}list{:02d}.txt".format(mode, split)))


def class_index(traintestlist):
    """utils.parsing_label on trainlist03.txt: {class: its position in order of first appearance}"""
    d = {}
    for e in _list_entries(os.path.join(traintestlist, "trainlist03.txt")):
        d.setdefault(e.split("/")[0], len(d))
    return d


FRAME_EXTENSIONS = (".jpg", ".jpeg", ".png")


def video_frames(root, entry):
    """the frame files of a video folder, sorted by name: *.jpg, *.jpeg, *.png (AuxDataset.py:129-136 takes every file of the folder)"""
    d = os.path.join(root, entry)
    files = sorted(f for f in os.listdir(d) if f.endswith(FRAME_EXTENSIONS))
    if not files:
        raise ValueError("No frames found for video %s" % entry)
    return [os.path.join(d, f) for f in files]


def frame_transform(img_size, device):
    from .video_transform import GpuFrameTransform, _RESIZE_FOR
    return GpuFrameTransform(img_size, device, resize=_RESIZE_FOR.get(img_size, int(round(img_size * 8 / 7))))


def plan_clips(root, entries, seq_len):
    """the host half of a batch: the chosen frame files of every video, read and planned for the decoder (a malformed header raises,
    naming its file) -> decode.ImagePlan over len(entries) x seq_len frames, video-major.  convert_rgb: a frame the GPU does not decode
    (grayscale JPEG, 16-bit or interlaced PNG, ...) goes through PIL's convert("RGB"), as AuxDataset.read_single_image converts"""
    names = []
    for e in entries:
        paths = video_frames(root, e)
        names += [paths[i] for i in frame_indices(len(paths), seq_len)]
    blobs = []
    for p in names:
        with open(p, "rb") as f:
            blobs.append(f.read())
    plan = decode.ImagePlan(blobs, names=names, convert_rgb=True)
    plan.check()
    return plan


def load_clips(plan, n_videos, seq_len, tf, train, check=True):
    """decode a planned batch (n_videos x seq_len JPEG / PNG frames, video-major) and transform it -> (NHWC4 [n_videos * seq_len, S, S, 4], the
    decoder's status words); check=False leaves reading them (a synchronisation) to the caller: plan.raise_on_status(status.cpu())"""
    frames, status = plan.decode(check=check)
    return tf(decode.split_videos(frames, seq_len), train=train), status


class ClipBatches:
    """DataLoader(AuxDataset, batch_size, shuffle=True) with getitem get_video_with_label: every pass is a fresh permutation of the list,
    the last batch may be smaller.  A batch: (NHWC4 frames [B * T, S, S, 4] on the device, int64 labels [B] on the host, the entries).
    The files of the next batches are read and planned (decode.ImagePlan) on `workers` host threads while the current one runs."""

    def __init__(self, args, device, shuffle=True):
        self.args, self.device, self.shuffle = args, device, shuffle
        self.entries = read_video_list(args.traintestlist, args.mode, args.split)
        self.labels = class_index(args.traintestlist)
        missing = sorted({e.split("/")[0] for e in self.entries} - set(self.labels))
        if missing:
            raise ValueError("classes without a label in trainlist03.txt: %s" % ", ".join(missing[:5]))
        self.train = args.mode == "train"
        self.tf = frame_transform(args.img_size, device)
        self.workers = max(1, int(args.num_workers))
        self._decoded = []      # (plan, status words) of the batches whose decode has not been checked yet

    def check_decoded(self):
        """read the status words of the batches decoded since the last call (one synchronisation); a malformed frame raises, named"""
        pending, self._decoded = self._decoded, []
        for plan, status in pending:
            plan.raise_on_status(status.cpu())

    def __len__(self):
        return (len(self.entries) + self.args.batch_size - 1) // self.args.batch_size

    def _host(self, batch):
        return plan_clips(self.args.path, batch, self.args.seq_len)

    def __iter__(self):
        order = list(range(len(self.entries)))
        if self.shuffle:
            random.shuffle(order)
        bs = self.args.batch_size
        batches = [[self.entries[i] for i in order[o:o + bs]] for o in range(0, len(order), bs)]
        with ThreadPoolExecutor(self.workers) as pool:
            pending = [pool.submit(self._host, b) for b in batches[:self.workers + 1]]
            for i, batch in enumerate(batches):
                plan = pending.pop(0).result()
                if i + self.workers + 1 < len(batches):
                    pending.append(pool.submit(self._host, batches[i + self.workers + 1]))
                x, status = load_clips(plan, len(batch), self.args.seq_len, self.tf, self.train, check=False)
                self._decoded.append((plan, status))
                labels = torch.tensor([self.labels[e.split("/")[0]] for e in batch], dtype=torch.int64)
                yield x, labels, batch


# ---- model, optimizer, checkpoints ----
def build_model(args, device):
    from .teacher.action_recognition import Action_Recognition_Resnet50
    model = Action_Recognition_Resnet50(args)
    if getattr(args, "init_weights", None):
        model.load_torchvision_resnet50(args.init_weights)
    return model.to(device)


def build_optimizer(model, args):
    """-> (optimizer, scheduler of the trunk, scheduler of fc): pretrain.py:31-38"""
    opt = TL.MomentumSGD(model, {"convnet": ("convnet.", args.lr_1, 0.9), "fc": ("fc.", args.lr_2, 0.9)})
    return opt, TL.StepLR(opt, "convnet", 10, 0.1), TL.StepLR(opt, "fc", 10, 0.1)


def save_checkpoint(model, optimizer, sched1, sched2, epoch, checkpoint_dir):
    os.makedirs(checkpoint_dir, exist_ok=True)
    d = {"iteration": epoch, "model_state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
         "optimizer1_state_dict": optimizer.state("convnet"), "optimizer2_state_dict": optimizer.state("fc"),
         "scheduler1": sched1.state(), "scheduler2": sched2.state()}
    torch.save(d, os.path.join(checkpoint_dir, "best_checkpoint.pt"))


def load_checkpoint(model, optimizer, sched1, sched2, checkpoint_dir):
    ck = torch.load(os.path.join(checkpoint_dir, "best_checkpoint.pt"), map_location="cpu")
    with torch.no_grad():      # into the optimizer's flat buffers: load_state_dict copies in place
        model.load_state_dict(ck["model_state_dict"], strict=True)
    optimizer.load_state("convnet", ck["optimizer1_state_dict"])
    optimizer.load_state("fc", ck["optimizer2_state_dict"])
    sched1.load_state(ck["scheduler1"])
    sched2.load_state(ck["scheduler2"])
    ops.WEIGHT_EPOCH[0] += 1
    return int(ck["iteration"])


def _clip_view(x, n_videos, seq_len):
    return x.view((n_videos, seq_len) + tuple(x.shape[1:]))


def train_epoch(model, loader, optimizer, args, log=None, epoch=1):
    """pretrain.py:104-139 -> the (loss, accuracy) of every batch as floats"""
    model.train()
    out, window = [], []
    optimizer.zero_grad()
    n = len(loader)
    for i, (x, labels, batch) in enumerate(loader):
        logits = model(_clip_view(x, len(batch), args.seq_len))
        loss, acc = ops.softmax_ce(logits, labels)
        loss.backward()
        optimizer.step(zero_grad=True)
        window.append((loss.detach(), acc))
        if (i + 1) % PRINT_EVERY == 0:
            vals = [(float(a), float(b)) for a, b in window]      # the only device reads of the batch loop, with the decoder's status
            loader.check_decoded()
            out += vals
            window = []
            if log is not None:
                log({"epoch": epoch, "batch": i + 1, "batches": n, "loss": round(sum(v[0] for v in vals) / PRINT_EVERY, 3),
                     "accuracy": sum(v[1] for v in vals) / PRINT_EVERY})
    loader.check_decoded()
    return out + [(float(a), float(b)) for a, b in window]


def evaluate(model, loader, args):
    """pretrain.py:142-163: eval mode over the same loader -> right answers / (8 x batches)"""
    model.eval()
    right, batches = None, 0
    with torch.no_grad():
        for x, labels, batch in loader:
            _, acc = ops.softmax_ce(model(_clip_view(x, len(batch), args.seq_len)), labels)
            r = acc * len(batch)
            right = r if right is None else right + r
            batches += 1
    loader.check_decoded()
    return float(right) / (ACC_DENOMINATOR * batches) if batches else 0.0


def train(model, loader, optimizer, sched1, sched2, args, log=None):
    """pretrain.py:94-170 -> {"losses", "accuracies" (per batch), "eval" (per epoch), "best"}"""
    hist = {"losses": [], "accuracies": [], "eval": [], "best": 0.0}
    for epoch in range(args.epochs):
        sched1.step()
        sched2.step()
        vals = train_epoch(model, loader, optimizer, args, log, epoch + 1)
        hist["losses"] += [v[0] for v in vals]
        hist["accuracies"] += [v[1] for v in vals]
        acc = evaluate(model, loader, args)
        hist["eval"].append(acc)
        saved = acc > hist["best"]
        if saved:
            hist["best"] = acc
            save_checkpoint(model, optimizer, sched1, sched2, epoch + 1, args.checkpoint_dir)
        if log is not None:
            log({"epoch": epoch + 1, "eval_accuracy": acc, "saved": saved, "lr_1": optimizer.groups["convnet"]["lr"],
                 "lr_2": optimizer.groups["fc"]["lr"]})
    return hist


def main(argv=None):
    parser = build_parser()
    args = args_check(parser, parser.parse_args(argv))
    if not torch.cuda.is_available():
        raise RuntimeError("pretrain needs the GPU: the trunk, the pool and the loss have no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    model = build_model(args, dev)
    loader = ClipBatches(args, dev)
    optimizer, sched1, sched2 = build_optimizer(model, args)
    start = load_checkpoint(model, optimizer, sched1, sched2, args.checkpoint_dir) if args.resume else 0
    t0 = time.time()

    def log(rec):
        rec["time"] = round(time.time() - t0, 3)
        print(json.dumps(rec, default=float), flush=True)
    hist = train(model, loader, optimizer, sched1, sched2, args, log)
    print(json.dumps({"resumed_from_epoch": start, "epochs": args.epochs, "best_accuracy": hist["best"],
                      "checkpoint": os.path.join(args.checkpoint_dir, "best_checkpoint.pt") if hist["best"] > 0 else None}), flush=True)
    return hist, model, optimizer


if __name__ == "__main__":
    main()
