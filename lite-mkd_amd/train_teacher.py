"""Trains the MFM teacher (reference: teacher/code/multi_run.py:361-396 run, :440-474 train_task, :596-619 checkpoints) from
per-modality features on disk, on one GPU: `python -m litemkd_amd.train_teacher`.  The model is teacher.mfm.ThreeTRXShiftLoopTime with its
TRX head (`head=True`): both fusions and the head run forward and backward on the HIP kernels; the loss is the reference's summed
cross-entropy (lmkd_d2m_loss with the query count as the weight of its mean) divided by tasks_per_batch, the optimizer trainloop.FusedOptimizer, the schedule
trainloop.MultiStepLR stepped every episode, the accuracy ops.accuracy.

The loop keeps the reference's counting: `iteration` is incremented before the episode runs, the optimizer steps when
(iteration + 1) % tasks_per_batch == 0 or iteration == training_iterations - 1, and a checkpoint labelled iteration + 1 is written
when (iteration + 1) % save_freq == 0 and iteration + 1 != training_iterations; a resumed run continues counting from that label.

Data (multi_video_reader.py:254-283): <feature_save_path>/<modality>/<class>/<video>/feature.npy, float [seq_len, 2048]; the videos are
those of the first modality's tree, kept when the split list names them; a second or third modality without a file reads as zeros.
The class and video draws are train.ClipDirectoryEpisodes'.  --synthetic draws seeded class-dependent features instead.

Checkpoints: every save_freq iterations {"iteration", "model_state_dict", "optimizer_state_dict", "scheduler"} as checkpoint<N>.pt and
checkpoint.pt, keys `fusion.*`, `three_fusion.*`, `bracnch.transformers.<i>.*` (what model_select.load_teacher and a default-constructed
ThreeTRXShiftLoopTime read); the final file checkpoint_final.pt holds the state dict alone (multi_run.py:436)."""
import argparse
import json
import os
import random
import time

import numpy as np
import torch

from . import ops
from . import trainloop as TL
from .distillers import _terms
from .train import ClipDirectoryEpisodes, read_split_lists


def build_parser():
    p = argparse.ArgumentParser(description="Train the MFM teacher on per-modality features")
    p.add_argument("--way", type=int, default=5)
    p.add_argument("--shot", type=int, default=5)
    p.add_argument("--query_per_class", type=int, default=5)
    p.add_argument("--seq_len", type=int, default=8)
    p.add_argument("--trans_linear_out_dim", type=int, default=1152)
    p.add_argument("--trans_dropout", type=float, default=0.1)
    p.add_argument("--temp_set", nargs="+", type=int, default=[2], help="frame-tuple cardinalities of the TRX head")
    p.add_argument("--tasks_per_batch", type=int, default=16)
    p.add_argument("--training_iterations", "-i", type=int, default=100020)
    p.add_argument("--save_freq", type=int, default=5000)
    p.add_argument("--print_freq", type=int, default=1000)
    p.add_argument("--split", type=int, default=3)
    p.add_argument("--traintestlist", default=None, help="directory of the split lists {train,test}list<split>.txt")
    p.add_argument("--checkpoint_dir", "-c", default=None)
    p.add_argument("--resume_from_checkpoint", "-r", action="store_true", help="continue from <checkpoint_dir>/checkpoint.pt")
    p.add_argument("--feature_save_path", default=None, help="root of <modality>/<class>/<video>/feature.npy")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--m1", default="rgb")
    p.add_argument("--m2", default="depth")
    p.add_argument("--m3", default="flow")
    p.add_argument("--shirt_num", type=int, default=1, help="frames the second modality is rolled by")
    p.add_argument("--trans_num", type=int, default=2, help="encoder layers per fusion")
    p.add_argument("--opt", choices=["adam", "sgd"], default="sgd")
    p.add_argument("--learning_rate", "-lr", type=float, default=0.0001)
    p.add_argument("--sch", nargs="+", type=int, default=[1000000], help="iterations at which the learning rate drops by 10")
    p.add_argument("--log_jsonl", default=None, help="append one JSON line per print_freq iterations")
    p.add_argument("--no_save", action="store_true", help="write no checkpoints")
    p.add_argument("--synthetic", action="store_true", help="seeded synthetic features instead of --feature_save_path")
    return p


def args_check(parser, args):
    if not args.synthetic and not args.feature_save_path:
        parser.error("--feature_save_path (or --synthetic) is needed")
    if args.checkpoint_dir is None and not args.no_save:
        parser.error("--checkpoint_dir is needed unless --no_save")
    if args.resume_from_checkpoint and args.checkpoint_dir is None:
        parser.error("--resume_from_checkpoint reads <checkpoint_dir>/checkpoint.pt")
    if not 1 <= args.seq_len <= ops.MFM_MAX_L:
        parser.error("--seq_len %d: the fusions take clips of 1 to %d frames" % (args.seq_len, ops.MFM_MAX_L))
    if not args.shirt_num < args.seq_len:
        parser.error("--shirt_num %d must be below --seq_len %d" % (args.shirt_num, args.seq_len))
    args.trans_linear_in_dim = 2048
    args.query_per_class_test = args.query_per_class
    return args


# ---- data ----
class FeatureTreeEpisodes(ClipDirectoryEpisodes):
    """Episodes of per-modality features (multi_video_reader.py:254-283).  Draws: ClipDirectoryEpisodes._draw (classes, videos, the two
    shuffles; a feature holds its seq_len frames already, so no frame draw).  episode() -> {"context_features": {modality: [Ns, L, 2048]},
    "context_labels": [Ns], "target_features": {...}, "target_labels": [Nq]} on the device."""

    def __init__(self, config, feature_save_path, traintestlist=None, split=None, device="cuda", length=10 ** 9, train=True):
        # the parent's constructor scans a clip directory and builds the frame transform, neither of which exists here; of the parent,
        # only _draw and _frame_idxs are used, and they read self.c, _classes() and _open() alone
        self.c, self.root, self.device, self.length, self.train = config, feature_save_path, device, length, train
        self.dataset = self
        self.modalities = (config.m1, config.m2, config.m3)
        first = os.path.join(feature_save_path, config.m1)
        if not os.path.isdir(first):
            raise ValueError("no features of the first modality under %s" % first)
        lists = read_split_lists(traintestlist, getattr(config, "split", 3) if split is None else split) if traintestlist else None
        self.splits = {True: {}, False: {}}
        for cname in sorted(os.listdir(first)):
            d = os.path.join(first, cname)
            if not os.path.isdir(d):
                continue
            for vid in sorted(os.listdir(d)):
                if not os.path.isfile(os.path.join(d, vid, "feature.npy")):
                    continue
                modes = (True, False) if lists is None else (True,) if vid.lower() in lists["train"] else (False,) if vid.lower() in lists["test"] else ()
                for m in modes:
                    self.splits[m].setdefault(cname, []).append(vid)
        if len(self.splits[bool(train)]) < config.way:
            raise ValueError("%s holds %d classes for this split, the episodes need %d" % (first, len(self.splits[bool(train)]), config.way))

    def _classes(self, train):
        return self.splits[bool(train)]

    def _open(self, cname, vid):
        return None, self.c.seq_len

    def read(self, cname, vid):
        """-> one float tensor [seq_len, 2048] per modality; a second or third modality without a file is zeros (:266-273)"""
        out = []
        for i, m in enumerate(self.modalities):
            try:
                f = np.load(os.path.join(self.root, m, cname, vid, "feature.npy"))
            except FileNotFoundError:
                if i == 0:
                    raise
                f = np.zeros((self.c.seq_len, 2048), dtype=np.float32)
            if f.shape != (self.c.seq_len, 2048):
                raise ValueError("%s/%s/%s: feature of shape %s, expected (%d, 2048)" % (m, cname, vid, f.shape, self.c.seq_len))
            out.append(f)
        return [torch.from_numpy(np.ascontiguousarray(f)).float() for f in out]

    def episode(self):
        sup, tgt = self._draw(self.train)

        def stack(videos):
            feats = [self.read(v[0], v[1]) for v in videos]
            return {m: torch.stack([f[i] for f in feats]).to(self.device) for i, m in enumerate(self.modalities)}
        return {"context_features": stack(sup), "context_labels": torch.FloatTensor([v[4] for v in sup]).to(self.device),
                "target_features": stack(tgt), "target_labels": torch.FloatTensor([v[4] for v in tgt]).to(self.device)}


class SyntheticFeatureEpisodes:
    """Seeded episodes without a dataset: every class of a pool has one prototype per modality, a video is |prototype + noise|
    (post-ReLU-like features), so the classes are separable and the loss falls; with proto_scale 0 they cannot be told apart and the
    loss does not saturate.  Same dictionary as FeatureTreeEpisodes."""

    def __init__(self, config, seed=0, device="cuda", length=10 ** 9, classes=16, noise=0.5, proto_scale=1.0):
        self.c, self.device, self.length, self.noise = config, device, length, noise
        self.dataset = self
        self.modalities = (config.m1, config.m2, config.m3)
        self.g = torch.Generator().manual_seed(seed)
        self.proto = proto_scale * torch.randn(max(classes, config.way), 3, config.seq_len, 2048, generator=self.g)

    def episode(self):
        c = self.c
        classes = torch.randperm(self.proto.shape[0], generator=self.g)[:c.way]

        def draw(per_class):
            lab = torch.arange(c.way).repeat_interleave(per_class)
            lab = lab[torch.randperm(lab.numel(), generator=self.g)]
            x = (self.proto[classes[lab]] + self.noise * torch.randn(lab.numel(), 3, c.seq_len, 2048, generator=self.g)).abs()
            return {m: x[:, i].contiguous().to(self.device) for i, m in enumerate(self.modalities)}, lab.float().to(self.device)
        cf, cl = draw(c.shot)
        tf, tl = draw(c.query_per_class)
        return {"context_features": cf, "context_labels": cl, "target_features": tf, "target_labels": tl}

    def __iter__(self):
        for _ in range(self.length):
            yield self.episode()


# ---- model, loop, checkpoints ----
def build_model(args, device):
    """ThreeTRXShiftLoopTime with its head, constructed on the device (its default initialisation draws from the device generator)"""
    from .teacher.mfm import ThreeTRXShiftLoopTime
    from .model.classifiers.TRX_2fcsup import PositionalEncoding
    with torch.device(device):
        model = ThreeTRXShiftLoopTime(args, head=True)
    for t in model.bracnch.transformers:      # the sinusoid table as every other module of the project holds it: computed on the host
        t.pe.pe.copy_(PositionalEncoding(2048, t.pe.p, max_len=t.pe.pe.shape[1]).pe)
    return model.train()


def optimizer_steps_at(iteration, args):
    """multi_run.py:391-393, `iteration` counted from 1"""
    return (iteration + 1) % args.tasks_per_batch == 0 or iteration == args.training_iterations - 1


def optimizer_state(optimizer):
    s = {"opt": optimizer.opt, "lr": optimizer.lr, "steps": optimizer.steps}
    if optimizer.opt == "adam":
        s.update(exp_avg=optimizer.m.clone(), exp_avg_sq=optimizer.v.clone())
    return s


def load_optimizer_state(optimizer, s):
    if s["opt"] != optimizer.opt:
        raise ValueError("checkpoint of a %s optimizer, this run uses %s" % (s["opt"], optimizer.opt))
    optimizer.lr, optimizer.steps = float(s["lr"]), int(s["steps"])
    if optimizer.opt == "adam":
        optimizer.m.copy_(s["exp_avg"])
        optimizer.v.copy_(s["exp_avg_sq"])


def save_checkpoint(model, optimizer, scheduler, iteration, checkpoint_dir):
    """multi_run.py:596-608"""
    os.makedirs(checkpoint_dir, exist_ok=True)
    d = {"iteration": iteration, "model_state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
         "optimizer_state_dict": optimizer_state(optimizer), "scheduler": {"n": scheduler.n, "base": scheduler.base}}
    torch.save(d, os.path.join(checkpoint_dir, "checkpoint%d.pt" % iteration))
    torch.save(d, os.path.join(checkpoint_dir, "checkpoint.pt"))


def load_checkpoint(model, optimizer, scheduler, checkpoint_dir):
    """multi_run.py:610-619 -> the iteration to continue from"""
    ck = torch.load(os.path.join(checkpoint_dir, "checkpoint.pt"), map_location="cpu")
    with torch.no_grad():      # into the optimizer's flat buffers: load_state_dict copies in place
        model.load_state_dict(ck["model_state_dict"], strict=True)
    load_optimizer_state(optimizer, ck["optimizer_state_dict"])
    scheduler.n, scheduler.base = ck["scheduler"]["n"], ck["scheduler"]["base"]
    ops.WEIGHT_EPOCH[0] += 1
    return int(ck["iteration"])


def summed_cross_entropy(logits, labels):
    """the teacher's `loss` (teacher/code/utils.py:177-189) for its one sample of logits: the SUM over the queries of the cross-entropy.
    lmkd_d2m_loss's cross-entropy term is the mean over the queries (the student's distillers), so its weight carries the count."""
    return _terms(s_ce=logits, labels=labels, w_ce=float(logits.shape[0]))[0]


def train_task(model, task, args):
    """multi_run.py:440-478 -> (loss / tasks_per_batch as a float tensor, accuracy tensor); the backward has run"""
    logits = model(task["context_features"], task["context_labels"], task["target_features"])["logits"]
    labels = task["target_labels"].long()
    loss = summed_cross_entropy(logits, labels) / args.tasks_per_batch
    acc, _ = ops.accuracy(logits.detach(), None, labels)
    loss.backward()
    return loss.detach(), acc


def train(model, loader, optimizer, scheduler, args, log=None, start_iteration=0, on_step=None):
    """multi_run.py:361-396, 423-426.  -> (losses, accuracies) of the episodes run, as floats"""
    losses, accs, window = [], [], []
    iteration, total = start_iteration, args.training_iterations
    optimizer.zero_grad()
    for task in loader:
        if iteration >= total:
            break
        iteration += 1
        loss, acc = train_task(model, task, args)
        window.append((loss, acc))
        if optimizer_steps_at(iteration, args):
            optimizer.step()
            optimizer.zero_grad()
            if on_step is not None:
                on_step(iteration)
        scheduler.step()
        if (iteration + 1) % args.print_freq == 0 or iteration >= total:
            vals = [(float(a), float(b)) for a, b in window]      # the only device reads of the loop
            losses += [v[0] for v in vals]
            accs += [v[1] for v in vals]
            if log is not None and vals and (iteration + 1) % args.print_freq == 0:
                log(iteration + 1, sum(v[0] for v in vals) / len(vals), sum(v[1] for v in vals) / len(vals))
            window = []
        if (iteration + 1) % args.save_freq == 0 and iteration + 1 != total and not args.no_save:
            save_checkpoint(model, optimizer, scheduler, iteration + 1, args.checkpoint_dir)
    vals = [(float(a), float(b)) for a, b in window]
    return losses + [v[0] for v in vals], accs + [v[1] for v in vals]


def main(argv=None):
    parser = build_parser()
    args = args_check(parser, parser.parse_args(argv))
    if not torch.cuda.is_available():
        raise RuntimeError("train_teacher needs the GPU: the fusions and the head have no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    args.device = dev
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    model = build_model(args, dev)
    loader = (SyntheticFeatureEpisodes(args, args.seed, dev) if args.synthetic
              else FeatureTreeEpisodes(args, args.feature_save_path, args.traintestlist, args.split, dev))
    optimizer = TL.FusedOptimizer(model, args.opt, args.learning_rate)
    scheduler = TL.MultiStepLR(optimizer, args.sch, episodes_per_step=1)
    start = load_checkpoint(model, optimizer, scheduler, args.checkpoint_dir) if args.resume_from_checkpoint else 0
    t0 = time.time()

    def log(iteration, loss, acc):
        rec = {"iteration": iteration, "loss": loss, "accuracy": acc, "time": round(time.time() - t0, 3), "lr": optimizer.lr}
        print(json.dumps(rec, default=float), flush=True)
        if args.log_jsonl:
            with open(args.log_jsonl, "a") as f:
                f.write(json.dumps(rec, default=float) + "\n")
    losses, accs = train(model, loader, optimizer, scheduler, args, log=log, start_iteration=start)
    if not args.no_save:
        os.makedirs(args.checkpoint_dir, exist_ok=True)
        path = os.path.join(args.checkpoint_dir, "checkpoint_final.pt")
        torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, path)      # multi_run.py:436: the state dict alone
        print(json.dumps({"checkpoint": path, "start_iteration": start, "optimizer_steps": optimizer.steps}), flush=True)
    return losses, accs, model, optimizer


if __name__ == "__main__":
    main()
