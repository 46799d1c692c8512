"""Attention maps of a student: Grad-CAM / HiResCAM on the map that enters the pooled head (the last trunk stage, [F, H/32, W/32, C]).

The reference's heatmap_vis.py:20-48 and teacher/code/heatmap_vis.py:16-27 take Grad-CAM on `layer4` of a torchvision ImageNet network
through pytorch_grad_cam and cv2; here the same construction runs on the few-shot student itself: the score is a query's logit for a
class of the episode, so the support frames get maps as well (the evidence a query draws from them).

    out = grad_cam(student, context_images, context_labels, target_images)        # inputs as trainloop.prepare_task returns them
    out["query"]["cam"]      # [Nq * L, h, w] in [0, 1]
    ops.cam_overlay(out["query"]["cam"], frames_u8, (H, W))

The backward ends at the recorded maps (ops.cam_tap): no trunk backward is entered, no parameter receives a gradient, no running
statistic changes.  The arithmetic of the maps is lmkd_gradcam_fwd's (include/lmkd.h)."""
import torch

from . import ops
from .model.model_select import name2strm_backbone

METHODS = {"gradcam": ops.CAM_GRADCAM, "hirescam": ops.CAM_HIRESCAM}
# The forward whose gradient gives the maps sums the GEMMs of the Linear heads and the TRX matcher (forward and backward) in blocks of this
# many terms (ops.module_k_block, as the MFM trainer's head).  A map is normalised frame by frame, so a frame whose channel sum nearly
# cancels shows the gradient's rounding error at full scale, and that error is made in the FORWARD: with one accumulator over the K = 4096
# of the matcher's projections the gradient is 2.2 x as far from fp64 as a blocked CPU GEMM's (1.1e-5 against 5e-6 relative L2 at the test
# shapes; blocking the backward alone changes nothing), in blocks it is closer than that (3.6e-6).  The blocked logits differ from the
# evaluator's by the evaluator's own rounding (measured up to 1.1e-5 of the largest logit), so a call also runs the evaluator's plain
# forward: the "logits" and the predicted class it returns are the evaluator's, the maps the gradient of the blocked "scored_logits".
K_BLOCK = 128


def accuracy_logits(logits, logits_fn=None):
    """the [Nq, way] logits the episode loop's accuracy uses (trainwandb.py:247-257): kl + ce for a dict with both, kl alone, or the tensor
    itself; any other dict needs logits_fn(dict) -> tensor"""
    if logits_fn is not None:
        return logits_fn(logits)
    if isinstance(logits, dict):
        if "kl" not in logits:
            raise ValueError("the classifier returns logits %s without 'kl': pass logits_fn= to choose the scored tensor" % sorted(logits))
        return logits["kl"] + logits["ce"] if "ce" in logits else logits["kl"]
    return logits


def frames_to_u8(images):
    """float frames in [0, 1], NCHW [F, 3, H, W] or NHWC4 [F, H, W, 4] -> uint8 RGB [F, H, W, 3] = (int)(x * 255 + 0.5)"""
    if images.dim() == 4 and images.shape[-1] == 4 and images.shape[1] != 3:
        x = images[..., :3]
    else:
        x = images.permute(0, 2, 3, 1)
    return (x * 255.0 + 0.5).clamp(0, 255).to(torch.uint8).contiguous()


def grad_cam(student, context_images, context_labels, target_images, target=None, query=None, method="gradcam", logits_fn=None,
             keep=False):
    """-> {"logits" [Nq, way], "target" [Nq], "scored_logits" [Nq, way], "support": {"raw", "cam"}, "query": {"raw", "cam"}} with maps
    [N * L, h, w]; keep=True adds "map", "grad" ([N * L, h, w, C]) and "weights" ([N * L, C]) per frame set.

    "logits" are the evaluator's (its plain no-grad forward); target = their predicted class (None) or a [Nq] tensor of classes in
    [0, way).  The score is S = sum_q z[q, target[q]] over the queries (query=i: that query alone), z = "scored_logits": accuracy_logits
    of the student's output in the forward that records the maps, whose GEMMs are summed in blocks (K_BLOCK)."""
    backbone = getattr(student.args, "model_backbone", None)
    if backbone in name2strm_backbone:
        raise NotImplementedError("backbone plugin '%s' pools patches, not the 4 x 4 adaptive maximum whose input Grad-CAM reads here" % backbone)
    if method not in METHODS:
        raise ValueError("method %r: one of %s" % (method, sorted(METHODS)))
    modes = [(m, m.training) for m in student.modules()]
    flags = [(p, p.requires_grad) for p in student.parameters()]
    try:
        student.eval()
        for p, _ in flags:
            p.requires_grad_(False)
        with torch.no_grad():
            logits = accuracy_logits(student(context_images, context_labels, target_images)["logits"], logits_fn)
        if logits.dim() != 2:
            raise ValueError("the scored logits must be [Nq, way], got %s" % (tuple(logits.shape),))
        n_query, way = logits.shape
        if target is None:
            target = logits.argmax(-1)
        else:          # checked on the host: a class outside [0, way) must not reach the device's gather
            host = torch.as_tensor(target).detach().cpu()
            if host.is_floating_point() or host.dtype == torch.bool or tuple(host.shape) != (n_query,):
                raise ValueError("target must hold one integer class per query (%d), got %s %s" % (n_query, host.dtype, tuple(host.shape)))
            if n_query and (int(host.min()) < 0 or int(host.max()) >= way):
                raise ValueError("target classes must lie in [0, %d), got %s" % (way, host.tolist()))
            target = host.long().to(logits.device)
        if query is not None and not 0 <= int(query) < n_query:
            raise ValueError("query %r: the episode has %d queries" % (query, n_query))
        with ops.module_k_block(student, K_BLOCK), torch.enable_grad(), ops.cam_tap(context_images.shape[0]) as tap:
            z = accuracy_logits(student(context_images, context_labels, target_images)["logits"], logits_fn)
            picked = z.gather(1, target[:, None])[:, 0]
            score = picked.sum() if query is None else picked[int(query)]
            grads = torch.autograd.grad(score, tap.leaves)
    finally:
        for m, t in modes:
            m.training = t
        for p, f in flags:
            p.requires_grad_(f)
    # the query frames' map and its gradient come from the side stream of the two-call schedule: the map kernel runs behind both
    cur = torch.cuda.current_stream(z.device)
    for s in ops.lane_streams(z.device):
        if s.cuda_stream != cur.cuda_stream:
            cur.wait_stream(s)
    for t in tuple(tap.leaves) + tuple(grads):
        t.record_stream(cur)
    out = {"logits": logits, "target": target, "scored_logits": z.detach()}
    for name, A, dA in zip(("support", "query"), tap.split(), tap.split(grads)):
        A, dA = A.detach().contiguous(), dA.contiguous()
        weights, raw, cam = ops.gradcam(A, dA, METHODS[method])
        out[name] = {"raw": raw, "cam": cam}
        if keep:
            out[name].update(map=A, grad=dA, weights=weights)
    return out
