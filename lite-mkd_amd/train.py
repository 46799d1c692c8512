"""Training entry point with the reference's command line (trainwandb.py:1-109 `main` / `make`, options.py:7-76 `parse_train_args`,
train_wandb.sh):

    python -m litemkd_amd.train --dataset hmdb --shot 5 --model_backbone resnet18_2fc --model_classifier TRX_2fcsup \
        --model_teacher test_teacher_TRX_2fcsup_fixed --distill_name fc_2_sup_dist --learning_rate 0.0001 \
        --checkpoint_dir hmdb_checkpoint/ --training_iterations 70010 --temp_set 2 --trans_linear_in_dim 2048

Every flag of the reference's parser is accepted under its own name and default (so train_wandb.sh's command line parses unchanged);
the defaults of the three plugin names are train_wandb.sh's values instead of the parser's (`strm18_student` / `TRX` / `test_teacher`:
the STRM student is available under its own names, `--model_backbone strm18_student --model_classifier strm_res18_sup --distill_name
strm_fc_2_sup_dist`).  What the reference does around the loop and this build does not: wandb logging (a
JSON-lines log instead, --log_jsonl).  Episodes come from SyntheticEpisodes, from the reference's own JPEG frame tree (--rgb_path,
--traintestlist, --teacher_path: JpegFrameEpisodes, decoded on the GPU) or, with --data_dir, from a directory of decoded uint8 clips;
the frame transform runs on the GPU.  One process per GPU: under torchrun every rank runs this script on its own episode stream
and the optimizer step all-reduces the gradient bucket (parallel.py).

Extra flags (not in the reference): --dtype, --two_call, --serial (schedule.Schedule), --data_dir / --feature_dir, --log_jsonl,
--seed, --no_save.  --rgb_path / --traintestlist / --teacher_path carry the names of the reference's dataset attributes."""
import argparse
import json
import os
import random
import sys
import time
import zipfile

import numpy as np
import torch

from . import trainloop as TL
from .options import DEFAULT_CFG
from .schedule import Schedule


def _bool(v):
    """the reference declares `type=bool` flags (options.py:40,52): any non-empty string is True there - `--debug False` included; here
    the usual spellings of false are honoured"""
    return str(v).lower() not in ("", "0", "false", "no", "none")


def build_parser():
    """options.py:7-76: parse_common_args + parse_train_args, flag for flag"""
    p = argparse.ArgumentParser(prog="python -m litemkd_amd.train", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    # few-shot setting
    p.add_argument("--way", type=int, default=5, help="Way of each task.")
    p.add_argument("--shot", type=int, default=5, help="Shots per class.")
    p.add_argument("--query_per_class", type=int, default=5, help="Target samples (i.e. queries) per class used for training.")
    p.add_argument("--query_per_class_test", type=int, default=1, help="Target samples (i.e. queries) per class used for testing.")
    # rarely changed
    p.add_argument("--tasks_per_batch", type=int, default=16, help="Number of tasks between parameter optimizations.")
    p.add_argument("--print_freq", type=int, default=10, help="print and log every n iterations.")
    p.add_argument("--seq_len", type=int, default=8, help="Frames per video.")
    p.add_argument("--num_workers", type=int, default=1, help="Num dataloader workers.")
    p.add_argument("--trans_linear_out_dim", type=int, default=1152, help="Transformer linear_out_dim")
    p.add_argument("--trans_linear_in_dim", type=int, default=2048, help="Transformer linear_in_dim")
    p.add_argument("--img_size", type=int, default=224, help="Input image size to the CNN after cropping.")
    p.add_argument("--temp_set", nargs="+", type=int, default=[2], help="cardinalities e.g. 2,3 is pairs and triples")
    p.add_argument("--trans_dropout", type=float, default=0.1, help="Transformer dropout")
    p.add_argument("--save_freq", type=int, default=10000, help="Number of iterations between checkpoint saves.")
    p.add_argument("--split", type=int, default=3, help="Dataset split.")
    p.add_argument("--sch", nargs="+", type=int, default=[20000, 40000], help="iters to drop learning rate")
    p.add_argument("--num_test_tasks", type=int, default=5000, help="number of random tasks to test on.")
    p.add_argument("--device", default=dev, help="device")
    # changed per experiment
    p.add_argument("--method", choices=["resnet18", "resnet34", "resnet50"], default="resnet18", help="method")
    p.add_argument("--num_gpus", type=int, default=1, help="(reference: GPUs to split the ResNet over with DataParallel; here ranks come from torchrun)")
    p.add_argument("--dataset", choices=["ssv2", "kinetics", "hmdb", "ucf"], default="kinetics", help="Dataset to use.")
    p.add_argument("--mode", default="KD_KL_meta", help="experiment description")
    p.add_argument("--debug", type=_bool, default=False, help="debug mode: no checkpoints")
    p.add_argument("--distill_name", default="fc_2_sup_dist", help="distill experiment name (a Distiller method)")
    p.add_argument("--model_backbone", default="resnet18_2fc", help="backbone name")
    p.add_argument("--model_classifier", default="TRX_2fcsup", help="classifier name")
    p.add_argument("--model_teacher", default="test_teacher_TRX_2fcsup_fixed", help="teacher name")
    p.add_argument("--teacher_checkpoint", default=None, help="teacher checkpoint (MFM layout)")
    p.add_argument("--test_model", choices=["teacher", "student", "extract_feature"], default="student", help="test who")
    p.add_argument("--soft_loss_weight", default=1, help="experiment hyperparameter")
    p.add_argument("--hard_loss_weight", default=1, help="experiment hyperparameter")
    p.add_argument("--test", type=_bool, default=False, help="experiment hyperparameter")
    p.add_argument("--cfg", type=json.loads, default=dict(DEFAULT_CFG), help="loss weights / temperature as a JSON object")
    # parse_train_args
    p.add_argument("--checkpoint_dir", "-c", default=None, help="Directory to save checkpoint to.")
    p.add_argument("--training_iterations", "-i", type=int, default=100010, help="Number of meta-training iterations.")
    p.add_argument("--resume_from_checkpoint", "-r", dest="resume_from_checkpoint", default=False, action="store_true", help="Restart from latest checkpoint.")
    p.add_argument("--test_iters", nargs="+", type=int, default=[10000, 15000, 20000, 30000, 35000, 40000, 50000, 60000, 70000, 80000, 90000, 100000],
                   help="iterations to test at.")
    p.add_argument("--learning_rate", "-lr", type=float, default=0.0001, help="Learning rate.")
    p.add_argument("--opt", choices=["adam", "sgd"], default="sgd", help="Optimizer")
    # ---- not in the reference
    p.add_argument("--dtype", choices=["f32", "f32h2", "f32x3", "f32native", "bf16"], default="f32", help="arithmetic: f32 = f32h2 (default, what bench.py times): "
                   "fp32 tensors and accumulation, the trunk's convolutions on two fp16 planes + power-of-two scales from the tensors' maxima (DESIGN 10): "
                   "full precision for elements within 2^17 of their tensor's maximum, an absolute 2^-40 of the maximum below; a run-time range fence "
                   "(ops.h2_fence_step, once per episode) counts what that leaves under-resolved and moves a tensor whose under-resolved elements would add more "
                   "than a quarter to its rounding error to f32x3's kernels from the next episode on (INTEGRATION.md, 'range fence'); "
                   "f32x3 = every fp32 product from an exact 3-way bf16 split, six products (the library's default arithmetic); "
                   "f32native = v_mfma_f32_32x32x2_f32, bf16 = bf16 tensors + bf16 MFMA (the reference's autocast path, trainwandb.py:20,126)")
    p.add_argument("--no_stream_inputs", dest="stream_inputs", action="store_false", help="with --data_dir: read, upload and transform every episode on "
                   "the training thread (default: a prefetch thread + copy stream + four static input sets, trainloop.StreamedEpisodes; needs one "
                   "frame resolution per episode)")
    p.add_argument("--serial", action="store_true", help="single-stream schedule (Schedule.serial())")
    p.add_argument("--two_call", action="store_true", help="round 3's schedule (two trunk calls on two streams, no cross-episode pipelining) instead of "
                   "the default merged + pipelined one (Schedule.bench())")
    p.add_argument("--data_dir", default=None, help="directory of decoded clips: <data_dir>/<class>/<video>.npy, uint8 [T, H, W, 3]")
    p.add_argument("--feature_dir", default=None, help="teacher features: <feature_dir>/<class>/<video>.npy, float [seq_len, 2048] (default: next to the clips, <video>.feature.npy)")
    p.add_argument("--rgb_path", default=None, help="the reference's frame tree: <rgb_path>/<class>/<video>/<frame>.jpg, or an uncompressed "
                   ".zip of it (JpegFrameEpisodes: decoded on the GPU); exclusive with --data_dir")
    p.add_argument("--traintestlist", default=None, help="with --rgb_path: directory of the split lists {train,test}list<split>.txt (--split)")
    p.add_argument("--teacher_path", default=None, help="with --rgb_path: teacher features <teacher_path>/<class>/<video>/<file>.npy")
    p.add_argument("--log_jsonl", default=None, help="append one JSON line per print_freq iterations (the reference logs to wandb)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--no_save", action="store_true", help="write no checkpoints")
    return p


def args_check(args):
    """options.py:86-112 `args_cheak` as far as it concerns the hot path"""
    if args.checkpoint_dir is None and not (args.debug or args.no_save):
        print("need to specify a checkpoint dir")
        sys.exit(1)
    if args.model_backbone.startswith("resnet"):          # every backbone of this build projects to 2048 (resnet18_2fc.py:27)
        args.trans_linear_in_dim = 2048
    args.save_dir = args.checkpoint_dir or "model_save"
    args.test_model_path = None
    if args.debug or args.no_save:
        args.save_freq = 0
    return args


class ClipDirectoryEpisodes:
    """Episodes from a directory of DECODED clips (video_reader.VideoDataset.__getitem__, video_reader.py:398-485, with the JPEG decoding
    done beforehand): <root>/<class>/<video>.npy = uint8 [T, H, W, 3]; teacher features [seq_len, 2048] float next to them
    (<video>.feature.npy) or under `feature_root`.  The class / video / frame draws follow the reference (`random.sample` of `way` classes,
    of shot + queries videos per class, get_seq's start / end / linspace frame choice :345-375, the two shuffles :454-460); Resize ->
    crop / flip -> ToTensor run on the GPU (video_transform.GpuFrameTransform), so `support_set` / `target_set` arrive as NHWC4 float
    tensors, which the backbones accept in place of [F, 3, S, S]."""

    def __init__(self, config, root, feature_root=None, device="cuda", length=10 ** 9, train=True):
        from .video_transform import GpuFrameTransform
        self.c, self.root, self.froot, self.device, self.length, self.train = config, root, feature_root, device, length, train
        self.dataset = self
        self.classes = {}
        for cname in sorted(os.listdir(root)):
            d = os.path.join(root, cname)
            if os.path.isdir(d):
                vids = sorted(f[:-4] for f in os.listdir(d) if f.endswith(".npy") and not f.endswith(".feature.npy"))
                if vids:
                    self.classes[cname] = vids
        if len(self.classes) < config.way:
            raise ValueError("%s holds %d classes, the episodes need %d" % (root, len(self.classes), config.way))
        self.tf = GpuFrameTransform(config.img_size, device)

    def _frame_idxs(self, n, train):
        """get_seq's frame choice (video_reader.py:345-375) for a video of n frames"""
        L = self.c.seq_len
        if n == L:
            return list(range(n))
        if train:
            excess_pad = int(min(5, (n - L) / 2))
            if excess_pad < 1:
                start, end = 0, n - 1
            else:
                start = random.randint(0, excess_pad)
                end = random.randint(n - 1 - excess_pad, n - 1)
        else:
            start, end = 1, n - 2
        if end - start < L:
            start, end = 0, n - 1
        return [int(f) for f in np.linspace(start, end, num=L)]

    def _frames(self, clip, train=None):
        return clip[self._frame_idxs(clip.shape[0], self.train if train is None else train)]

    def _classes(self, train):
        """{class: [videos]} the draws of a `train` / test episode choose from"""
        return self.classes

    def _open(self, cname, vid):
        """-> (handle, frame count) of one video: here the memory-mapped clip"""
        clip = np.load(os.path.join(self.root, cname, vid + ".npy"), mmap_mode="r")
        return clip, clip.shape[0]

    def _feature(self, cname, vid):
        path = (os.path.join(self.froot, cname, vid + ".npy") if self.froot else os.path.join(self.root, cname, vid + ".feature.npy"))
        return torch.from_numpy(np.load(path)).float()

    def _draw(self, train):
        """the draws of one episode in the reference's order - classes, videos, each video's frames, the two shuffles - for both
        episode() and host_episode(), and for JpegFrameEpisodes: -> (support, query) lists of (class, video, handle, frame indices,
        label).  The per-video flip / crop draws follow (GpuFrameTransform.draw, support videos first)."""
        c = self.c
        nq = c.query_per_class if train else c.query_per_class_test
        classes = self._classes(train)
        batch_classes = random.sample(list(classes), c.way)
        sup, tgt = [], []
        for bl, bc in enumerate(batch_classes):
            vids = classes[bc]
            if len(vids) < c.shot + nq:
                raise ValueError("class %s has %d videos, an episode needs %d" % (bc, len(vids), c.shot + nq))
            idxs = random.sample(range(len(vids)), c.shot + nq)
            for j, i in enumerate(idxs):
                h, n = self._open(bc, vids[i])
                (sup if j < c.shot else tgt).append((bc, vids[i], h, self._frame_idxs(n, train), bl))
        random.shuffle(sup)
        random.shuffle(tgt)
        return sup, tgt

    @staticmethod
    def _labels(sup, tgt, way):
        return {"support_labels": torch.FloatTensor([v[4] for v in sup]), "target_labels": torch.FloatTensor([v[4] for v in tgt]),
                "real_target_labels": torch.FloatTensor([v[4] for v in tgt]), "batch_class_list": torch.arange(way).float()}

    def host_episode(self):
        """the HOST half of episode() for trainloop.StreamedEpisodes (a prefetch thread calls it): the same draws in the same order - classes,
        videos, frames, the two shuffles, then per video flip / crop (support videos first) - but no device work: the decoded frames of all
        videos as ONE uint8 tensor (they must share a resolution: one H2D copy, one resize launch), the crop parameters, the features"""
        train = self.train                  # read once: an episode is wholly of one mode
        sup, tgt = self._draw(train)
        vids = [torch.from_numpy(np.ascontiguousarray(v[2][v[3]])) for v in sup + tgt]
        if len({tuple(v.shape[1:3]) for v in vids}) != 1:
            raise ValueError("StreamedEpisodes needs one frame resolution per episode (got %s): run with --no_stream_inputs"
                             % sorted({tuple(v.shape[1:3]) for v in vids}))
        params = [self.tf.draw(v.shape[1], v.shape[2], train) for v in vids]
        d = {"frames": torch.cat(vids, 0), "params": params, "features": torch.stack([self._feature(v[0], v[1]) for v in sup + tgt]),
             "ns": len(sup)}
        d.update(self._labels(sup, tgt, self.c.way))
        return d

    def _task(self, sup_videos, tgt_videos, sup, tgt, train):
        # one transform call per set: the per-video flip / crop draws come in the reference's order (support videos, then query videos)
        d = {"support_set": self.tf(sup_videos, train=train), "target_set": self.tf(tgt_videos, train=train),
             "support_set_feature_teacher": torch.stack([self._feature(s[0], s[1]) for s in sup]).to(self.device),
             "target_set_feature_teacher": torch.stack([self._feature(t[0], t[1]) for t in tgt]).to(self.device)}
        d.update(self._labels(sup, tgt, self.c.way))
        return {k: v.unsqueeze(0) for k, v in d.items()}

    def episode(self):
        train = self.train
        sup, tgt = self._draw(train)
        clip = lambda v: torch.from_numpy(np.ascontiguousarray(v[2][v[3]]))      # noqa: E731
        return self._task([clip(s) for s in sup], [clip(t) for t in tgt], sup, tgt, train)

    def __iter__(self):
        for _ in range(self.length):
            yield self.episode()


FRAME_EXTENSIONS = (".jpg", ".jpeg", ".png")      # decoded on the GPU (decode.ImagePlan sorts a batch by file signature)


def jpeg_frame_index(rgb_path):
    """read_dir (video_reader.py:118-196) without the split: -> ({class: {video: [frame file names]}}, {(class, video): [paths]}) of a
    directory <rgb_path>/<class>/<video>/<frame>.jpg (or .jpeg / .png) or an uncompressed .zip of the same tree (a member's last three
    path components; the paths are then member names).  Classes, videos and frames sorted; the index of a directory equals that of its
    .zip."""
    idx = {}
    if rgb_path.endswith(".zip"):
        with zipfile.ZipFile(rgb_path) as zf:
            for name in zf.namelist():
                parts = name.split("/")
                if len(parts) >= 3 and parts[-1].endswith(FRAME_EXTENSIONS):
                    idx.setdefault(parts[-3], {}).setdefault(parts[-2], []).append((parts[-1], name))
    else:
        for cname in os.listdir(rgb_path):
            d = os.path.join(rgb_path, cname)
            if not os.path.isdir(d):
                continue
            for vid in os.listdir(d):
                vd = os.path.join(d, vid)
                if os.path.isdir(vd):
                    idx.setdefault(cname, {})[vid] = [(f, os.path.join(vd, f)) for f in os.listdir(vd) if f.endswith(FRAME_EXTENSIONS)]
    index, paths = {}, {}
    for cname in sorted(idx):
        index[cname] = {}
        for vid in sorted(idx[cname]):
            frames = sorted(idx[cname][vid])
            index[cname][vid] = [f for f, _ in frames]
            paths[(cname, vid)] = [p for _, p in frames]
    return index, paths


def read_split_lists(traintestlist, split):
    """_select_fold (video_reader.py:305-319): {train,test}list{split:02d}.txt -> {"train": set, "test": set} of video names, normalised
    as the reference does (spaces to '_', lower case, first token, basename without extension); a video folder v is matched as v.lower()"""
    lists = {}
    for name in ("train", "test"):
        with open(os.path.join(traintestlist, "{}list{:02d}.txt".format(name, split))) as f:
            data = [x.replace(" ", "_").lower() for x in f.readlines()]
        data = [x.strip().split(" ")[0] for x in data]
        lists[name] = {os.path.splitext(os.path.split(x)[1])[0] for x in data}
    return lists


class JpegFrameEpisodes(ClipDirectoryEpisodes):
    """Episodes from the reference's own data layout (video_reader.VideoDataset, video_reader.py:118-485): JPEG or PNG frames
    <rgb_path>/<class>/<video>/<frame>.jpg (.jpeg, .png) or an uncompressed .zip of that tree, split into train / test videos by the split lists
    ({train,test}list{split:02d}.txt under `traintestlist`; without them every video serves both modes), teacher features from
    <teacher_path>/<class>/<video>/ (the first file in sorted order, a float [seq_len, 2048] .npy).

    Features are matched to videos BY NAME and a missing one raises.  The reference matches them by position in two separately built
    lists (:197-260, :388-396), which silently pairs a video with another video's feature when a folder is missing on one side.

    The draws are ClipDirectoryEpisodes' own (_draw: classes, videos, frames, shuffles, then flip / crop), so a seeded run picks the same
    episode from a JPEG tree as from the .npy tree of the same decoded frames; only the seq_len selected files of a video are read.  The
    frames are decoded on the GPU (decode.ImagePlan: csrc/jpeg.hip, csrc/png.hip; bit-identical to PIL; a frame that PIL does not decode as
    RGB raises, since the reference's student reader, video_reader.py:334-343, does not convert): episode() decodes and transforms on the current
    stream; host_episode() hands trainloop.StreamedEpisodes the compressed bytes of the episode, packed into one pinned buffer with
    their decode plan, in place of "frames"."""

    def __init__(self, config, rgb_path, traintestlist=None, teacher_path=None, split=None, device="cuda", length=10 ** 9, train=True):
        from . import decode
        from .video_transform import GpuFrameTransform
        self.c, self.root, self.froot, self.device, self.length, self.train = config, rgb_path, teacher_path, device, length, train
        self.dataset = self
        self.index, self._paths = jpeg_frame_index(rgb_path)
        self.class_folders = list(self.index)          # the class id of the reference = the position in this list
        self._zip = zipfile.ZipFile(rgb_path) if rgb_path.endswith(".zip") else None
        lists = read_split_lists(traintestlist, getattr(config, "split", 3) if split is None else split) if traintestlist else None
        self.splits = {True: {}, False: {}}
        for cname, vids in self.index.items():
            for vid, frames in vids.items():
                if len(frames) < config.seq_len:
                    continue
                if lists is None:
                    modes = (True, False)
                else:
                    v = vid.lower()
                    modes = (True,) if v in lists["train"] else (False,) if v in lists["test"] else ()
                for m in modes:
                    self.splits[m].setdefault(cname, []).append(vid)
        self._feat = {}
        if teacher_path is not None:
            for m in (True, False):
                for cname, vids in self.splits[m].items():
                    for vid in vids:
                        d = os.path.join(teacher_path, cname, vid)
                        files = sorted(os.listdir(d)) if os.path.isdir(d) else []
                        if not files:
                            raise ValueError("no teacher feature for video %s/%s under %s" % (cname, vid, teacher_path))
                        self._feat[(cname, vid)] = os.path.join(d, files[0])
        if len(self.splits[bool(train)]) < config.way:
            raise ValueError("%s holds %d classes in the %s split, the episodes need %d"
                             % (rgb_path, len(self.splits[bool(train)]), "train" if train else "test", config.way))
        self.tf = GpuFrameTransform(config.img_size, device)
        self._ring = decode.PinnedRing(6)

    @property
    def classes(self):
        return self.splits[bool(self.train)]

    def _classes(self, train):
        return self.splits[bool(train)]

    def _open(self, cname, vid):
        p = self._paths[(cname, vid)]
        return p, len(p)

    def _read(self, path):
        if self._zip is not None:
            return self._zip.read(path)
        with open(path, "rb") as f:
            return f.read()

    def _feature(self, cname, vid):
        if self.froot is None:              # (the evaluator of a student needs no teacher features)
            return torch.zeros(self.c.seq_len, 2048)
        return torch.from_numpy(np.load(self._feat[(cname, vid)])).float()

    def _plan(self, train):
        from . import decode
        sup, tgt = self._draw(train)
        names = [v[2][i] for v in sup + tgt for i in v[3]]
        plan = decode.ImagePlan([self._read(p) for p in names], names=names, ring=self._ring if torch.cuda.is_available() else None,
                                convert_rgb=False)
        plan.check()                        # a malformed header names its file here
        return sup, tgt, plan

    def host_episode(self):
        train = self.train                  # read once: an episode is wholly of one mode
        sup, tgt, plan = self._plan(train)
        shapes = plan.shapes()
        if len(set(shapes)) != 1:
            raise ValueError("StreamedEpisodes needs one frame resolution per episode (got %s): run with --no_stream_inputs"
                             % sorted(set(shapes)))
        L = self.c.seq_len
        params = [self.tf.draw(shapes[i * L][0], shapes[i * L][1], train) for i in range(len(sup) + len(tgt))]
        d = {"plan": plan, "params": params, "features": torch.stack([self._feature(v[0], v[1]) for v in sup + tgt]), "ns": len(sup)}
        d.update(self._labels(sup, tgt, self.c.way))
        return d

    def episode(self):
        train = self.train
        sup, tgt, plan = self._plan(train)
        from . import decode
        frames, _ = plan.decode(check=True)
        videos = decode.split_videos(frames, self.c.seq_len)
        return self._task(videos[:len(sup)], videos[len(sup):], sup, tgt, train)


def schedule_from_args(args):
    conv = {"f32": "fp32h2", "f32h2": "fp32h2", "f32x3": "fp32x3", "f32native": "fp32", "bf16": "bf16"}[args.dtype]
    act = "bf16" if args.dtype == "bf16" else "fp32"
    if args.serial:
        return Schedule.serial(conv_dtype=conv, act_dtype=act)
    if args.two_call or conv == "fp32":          # the native fp32 MFMA mode has no two-segment kernels
        return Schedule.two_call(conv_dtype=conv, act_dtype=act)
    return Schedule.from_env(conv_dtype=conv, act_dtype=act)


def main(argv=None):
    parser = build_parser()
    args = args_check(parser.parse_args(argv))
    if args.rgb_path and args.data_dir:
        parser.error("--rgb_path and --data_dir are exclusive")
    if args.rgb_path and not args.teacher_path:
        parser.error("--rgb_path needs --teacher_path (the distillation loss reads the teacher features)")
    from .parallel import init_distributed
    rank, world, dev = init_distributed()
    args.device = dev
    random.seed(args.seed + rank)
    np.random.seed(args.seed + rank)
    torch.manual_seed(args.seed)                  # identical initial weights on every rank (make() also broadcasts them)
    sched = schedule_from_args(args)
    loader = None
    if args.data_dir or args.rgb_path:
        loader = (JpegFrameEpisodes(args, args.rgb_path, args.traintestlist, args.teacher_path, split=args.split, device=dev) if args.rgb_path
                  else ClipDirectoryEpisodes(args, args.data_dir, args.feature_dir, device=dev))
        if args.stream_inputs and torch.device(dev).type == "cuda":
            # the loader beside the compute (trainwandb.py:87-88: a DataLoader worker): a prefetch thread reads and pins the next episodes,
            # a copy stream uploads the uint8 frames and runs the frame transform into one of four static input sets
            loader = TL.StreamedEpisodes(loader, args, dev)
    student, teacher, loader, distiller, accuracy_fn, _, optimizer, scheduler = TL.make(args, video_loader=loader, base_seed=args.seed, schedule=sched)
    if args.teacher_checkpoint:
        from .model.model_select import load_teacher, load_teacher_ctx
        # (a CTX teacher's checkpoint is a TwoCTXShuffleTime one: `bracnch.transformers.*` without an index)
        load = load_teacher_ctx if args.model_teacher in ("train_teacher_ctx", "test_teacher_ctx") else load_teacher
        load(teacher.classifier if hasattr(teacher, "classifier") else teacher, args)
    t0 = time.time()

    def log(iteration, a, b):
        rec = ({"iteration": iteration, "loss": a, "accuracy": b} if b is not None else {"iteration": iteration, "test": a})
        rec.update(time=round(time.time() - t0, 3), rank=rank, world=world, lr=optimizer.lr)
        if rank == 0:
            print(json.dumps(rec, default=float), flush=True)
            if args.log_jsonl:
                with open(args.log_jsonl, "a") as f:
                    f.write(json.dumps(rec, default=float) + "\n")
    losses, accs = TL.train(student, teacher, loader, distiller, optimizer, scheduler, accuracy_fn, args, log=log, schedule=sched)
    if not (args.debug or args.no_save):
        path = TL.checkpoint_all_ranks(student, len(losses), args)      # trainwandb.py:183-186: the final checkpoint
        if rank == 0:
            print(json.dumps({"checkpoint": path}), flush=True)
    return losses, accs


if __name__ == "__main__":
    main()
