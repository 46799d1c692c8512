"""MFM teacher training benchmark, measurements in ONE process on one GPU:

(a) one teacher training episode - 5-way 5-shot, 25 support + 25 query videos, seq_len 8, width 2048, trans_num 2, training mode with
    every dropout drawn: ThreeTRXShiftLoopTime.forward (head=True), the summed cross-entropy, backward - on the HIP path
    (teacher/mfm.py, ops.TRXLogitsFn, train_teacher.summed_cross_entropy);
(b) the same episode with the same nn containers run by torch on the same GPU: nn.Embedding / nn.LayerNorm / nn.Dropout /
    nn.TransformerEncoder / nn.Linear of the same module in training mode, the TRX head as tests/_trx_card_ref.trx_logits writes it in
    torch, F.cross_entropy;
(c) forward + backward of one three-modality fusion call over the 50 videos, both ways.

The episode's features carry no class (SyntheticFeatureEpisodes(proto_scale=0)): on separable classes the cross-entropy is exactly 0 and so
is every gradient.  In eval mode both sides must give the same logits and the same non-zero loss (asserted, recorded).  --k_block sets
ops.MFM_K_BLOCK for the run (the blocks the teacher's GEMMs are summed in; 0: one launch per GEMM).

HIP events around batches of back-to-back calls after a warm-up; medians of the timings.  Gradients are left to accumulate as between two
optimizer steps; the optimizer step is not part of either side.

    python tools/mfm_train_bench.py [--iters 10] [--batches 5] [--k_block n] [--out profiles/mfm_train_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stat(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "runs": v}


def events_ms(fn, iters, batches, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10, help="calls per timing")
    p.add_argument("--batches", type=int, default=5, help="timings")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=None)
    p.add_argument("--k_block", type=int, default=None, help="ops.MFM_K_BLOCK for this run (default: the library's)")
    a = p.parse_args()
    import torch
    import torch.nn.functional as F
    import litemkd_amd
    import _trx_card_ref as TC
    from litemkd_amd import train_teacher as TT
    assert torch.cuda.is_available(), "mfm_train_bench needs the GPU"
    litemkd_amd.lib().call("lmkd_device_check", 0)
    dev = torch.device("cuda", 0)
    from litemkd_amd import ops
    if a.k_block is not None:
        ops.MFM_K_BLOCK = a.k_block
    ps = TT.build_parser()
    args = TT.args_check(ps, ps.parse_args(["--synthetic", "--no_save", "--way", "5", "--shot", "5", "--query_per_class", "5", "--trans_num", "2", "--trans_dropout", "0.0"]))      # the head without dropout on both sides (the torch head has none)
    torch.manual_seed(3)
    model = TT.build_model(args, dev)
    task = TT.SyntheticFeatureEpisodes(args, 3, dev, proto_scale=0.0).episode()      # classes that cannot be told apart: the loss does not saturate
    labels = task["target_labels"].long()
    L, s, way = args.seq_len, args.shirt_num, args.way
    ns = task["context_labels"].numel()
    mods = [torch.cat((task["context_features"][m], task["target_features"][m])) for m in (args.m1, args.m2, args.m3)]

    def nn_fusion(f, xs):      # the module's own containers, training mode (torch draws the dropouts)
        hs = []
        for i, x in enumerate(xs):
            pe = getattr(f, "positionEncoding%d" % (i + 1))
            hs.append(pe.dropout(pe.LayerNorm(x + pe.position_embeddings(torch.arange(L, device=dev)))))
        return f.dropout(f.f1(f.transformer_encoder(torch.cat(hs, dim=-1))))

    got = {}

    def hip_episode():
        got["hip"] = model(task["context_features"], task["context_labels"], task["target_features"])["logits"]
        loss = TT.summed_cross_entropy(got["hip"], labels)
        loss.backward()
        return loss

    def torch_episode():
        first, second, third = mods
        rolled = torch.cat((second[:, s:], second[:, :s]), dim=1)
        fused = nn_fusion(model.three_fusion, (first, second, third)) + nn_fusion(model.fusion, (first, rolled)) + nn_fusion(model.fusion, (first, third))
        t = model.bracnch.transformers[0]
        hp = {k: v for k, v in t.state_dict(keep_vars=True).items()}
        logits = TC.trx_logits(fused[:ns], task["context_labels"], fused[ns:], hp, way, L, 2)
        got["torch"] = logits
        loss = F.cross_entropy(logits, labels, reduction="sum")
        loss.backward()
        return loss
    w = torch.randn(mods[0].shape, device=dev)

    def hip_fusion():
        model.three_fusion(*mods).backward(w)

    def torch_fusion():
        nn_fusion(model.three_fusion, mods).backward(w)
    model.eval()      # dropout off once: both sides compute the same logits and the same, non-zero, loss
    l_hip, l_torch = float(hip_episode()), float(torch_episode())
    logits_rel = float((got["hip"] - got["torch"]).norm() / got["torch"].norm())
    assert l_torch > 0.1 and abs(l_hip - l_torch) < 1e-3 * l_torch and logits_rel < 1e-4, (l_hip, l_torch, logits_rel)
    for prm in model.parameters():
        prm.grad = None
    model.train()
    out = {"device": torch.cuda.get_device_name(0),
           "what": "teacher training episode, 5-way 5-shot, 25 + 25 videos, seq_len 8, width 2048, trans_num 2, training mode: forward + "
                   "summed cross-entropy + backward; milliseconds per call, %d timings of %d calls after %d warm-up calls" % (a.batches, a.iters, a.warmup),
           "parameters": sum(p.numel() for p in model.parameters()),
           "k_block": ops.MFM_K_BLOCK, "eval_mode_loss_hip": l_hip, "eval_mode_loss_torch": l_torch, "eval_mode_logits_rel_diff": logits_rel}
    res = {}
    for name, fn in (("episode_hip_ms", hip_episode), ("episode_torch_gpu_ms", torch_episode), ("three_fusion_fwd_bwd_hip_ms", hip_fusion),
                     ("three_fusion_fwd_bwd_torch_gpu_ms", torch_fusion)):
        res[name] = stat(events_ms(fn, a.iters, a.batches, a.warmup))
        for prm in model.parameters():
            prm.grad = None
    out.update(res)
    out["episode_torch_over_hip"] = res["episode_torch_gpu_ms"]["median"] / res["episode_hip_ms"]["median"]
    out["three_fusion_torch_over_hip"] = res["three_fusion_fwd_bwd_torch_gpu_ms"]["median"] / res["three_fusion_fwd_bwd_hip_ms"]["median"]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
