"""Benchmark of the MFM attention for clips of up to 16 frames, measurements in ONE process on one GPU:

(a) the three entry points of the 16-token family (lmkd_mha_seq, lmkd_mha_seq_train_fwd with a mask, lmkd_mha_seq_bwd) at B = 50 videos,
    (D, H) = (6144, 3) and (4096, 2), L = 8, 12, 16: microseconds per launch, and the bytes every launch has to move (each operand once:
    qkv in and out out for a forward; qkv, dO in and dqkv out for the backward; P and the mask are counted too) divided by that time,
    against the 6.29 TB/s a float4 copy reaches on this GPU;
(b) the three entry points of the 8-token family (lmkd_mha_small*) at L = 8 on the same buffers;
(c) torch.nn.functional.scaled_dot_product_attention on the same shapes (q, k, v the [B, H, L, hd] views of the same qkv buffer, no
    dropout): forward, and forward + backward;
(d) one teacher training episode (5-way 5-shot, 25 + 25 videos, width 2048, trans_num 2, training mode with every dropout drawn; the loop of
    tools/mfm_train_bench.py) at seq_len 8, 12 and 16.

The operands of one call fit the 256 MiB Infinity Cache (59 MB of qkv at L = 16, D = 6144), so every timed launch works on the next of
enough buffer sets that the sets together hold more than --rotate_mb (default 768 MB): by the time a set comes round again it has been
evicted, and the figures are HBM figures.  --rotate_mb 0 uses one set (cache figures).

HIP events around batches of back-to-back launches after a warm-up; median, minimum and maximum over the batches.

    python tools/mfm_long_bench.py [--iters 20] [--batches 7] [--no_episode] [--out profiles/mfm_long_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_TBS = 6.29      # achievable HBM bandwidth of the MI355X (float4 copy)
B = 50
WIDTHS = ((6144, 3), (4096, 2))
LENGTHS = (8, 12, 16)


def stat(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "runs": v}


def events_us(fn, iters, batches, warmup):
    """fn(i) is launch number i -> microseconds per launch of each batch"""
    import torch
    n = 0
    for _ in range(warmup):
        fn(n)
        n += 1
    torch.cuda.synchronize()
    out = []
    for _ in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn(n)
            n += 1
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / iters)
    return out


def with_rate(us, nbytes):
    s = stat(us)
    s["bytes"] = nbytes
    s["TB_per_s"] = nbytes / (s["median"] * 1e-6) / 1e12
    s["of_hbm"] = s["TB_per_s"] / HBM_TBS
    return s


def attention(a, dev):
    import torch
    import torch.nn.functional as F
    import litemkd_amd
    from litemkd_amd import ops
    lib, p, st = litemkd_amd.lib(), ops._p, ops._stream()
    res = {}
    for D, H in WIDTHS:
        for L in LENGTHS:
            hd = D // H
            per_set = 4 * B * L * D * 8 + 4 * B * H * (256 + L * L)
            sets = max(1, -(-a.rotate_mb * 1000000 // per_set)) if a.rotate_mb else 1
            g = torch.Generator(device=dev).manual_seed(L + D)
            S = []
            for _ in range(sets):
                S.append(dict(qkv=torch.randn(B * L, 3 * D, device=dev, generator=g), dO=torch.randn(B * L, D, device=dev, generator=g),
                              mask=(torch.rand(B * H, L, L, device=dev, generator=g) >= 0.1).float() / 0.9,
                              out=torch.empty(B * L, D, device=dev), dqkv=torch.empty(B * L, 3 * D, device=dev),
                              P16=torch.zeros(B * H, 16, 16, device=dev), P8=torch.zeros(B * H, 8, 8, device=dev)))
            f4 = 4 * B * L * D
            nbytes = {"fwd": 4 * f4, "train_fwd": 4 * f4 + 4 * B * H * L * L, "bwd": 7 * f4 + 4 * B * H * L * L}      # + P below
            entry = {"B": B, "L": L, "D": D, "H": H, "buffer_sets": sets, "MB_per_set": per_set / 1e6}
            families = [("seq", "P16", 256)] + ([("small", "P8", 64)] if L <= 8 else [])
            for fam, pk, pn in families:
                for s in S:      # the backward reads the probabilities of its own set
                    lib.call("lmkd_mha_%s_train_fwd" % fam, p(s["qkv"]), p(s["mask"]), p(s["out"]), p(s[pk]), B, L, D, H, st)
                infer = "lmkd_mha_seq" if fam == "seq" else "lmkd_mha_small"
                calls = {
                    "fwd": lambda i: lib.call(infer, p(S[i % sets]["qkv"]), p(S[i % sets]["out"]), B, L, D, H, st),
                    "train_fwd": lambda i: lib.call("lmkd_mha_%s_train_fwd" % fam, p(S[i % sets]["qkv"]), p(S[i % sets]["mask"]),
                                                    p(S[i % sets]["out"]), p(S[i % sets][pk]), B, L, D, H, st),
                    "bwd": lambda i: lib.call("lmkd_mha_%s_bwd" % fam, p(S[i % sets]["qkv"]), p(S[i % sets][pk]), p(S[i % sets]["mask"]),
                                              p(S[i % sets]["dO"]), p(S[i % sets]["dqkv"]), B, L, D, H, st),
                }
                for name, fn in calls.items():
                    extra = 0 if name == "fwd" else 4 * B * H * pn
                    entry["%s_%s_us" % (fam, name)] = with_rate(events_us(fn, a.iters, a.batches, a.warmup), nbytes[name] + extra)
            # torch's attention on the same buffers
            leaves = [s["qkv"].clone().requires_grad_() for s in S]
            gos = [s["dO"].reshape(B, L, H, hd).transpose(1, 2) for s in S]

            def sdpa(i, backward):
                x = leaves[i % sets]
                q, k, v = (t.reshape(B, L, H, hd).transpose(1, 2) for t in x.chunk(3, dim=-1))
                if not backward:
                    with torch.no_grad():
                        return F.scaled_dot_product_attention(q, k, v)
                x.grad = None
                F.scaled_dot_product_attention(q, k, v).backward(gos[i % sets])
            entry["torch_sdpa_fwd_us"] = stat(events_us(lambda i: sdpa(i, False), a.iters, a.batches, a.warmup))
            entry["torch_sdpa_fwd_bwd_us"] = stat(events_us(lambda i: sdpa(i, True), a.iters, a.batches, a.warmup))
            entry["seq_train_fwd_plus_bwd_us"] = entry["seq_train_fwd_us"]["median"] + entry["seq_bwd_us"]["median"]
            entry["torch_fwd_over_seq_fwd"] = entry["torch_sdpa_fwd_us"]["median"] / entry["seq_fwd_us"]["median"]
            entry["torch_fwd_bwd_over_seq_fwd_bwd"] = entry["torch_sdpa_fwd_bwd_us"]["median"] / entry["seq_train_fwd_plus_bwd_us"]
            res["D%d_H%d_L%d" % (D, H, L)] = entry
            print(json.dumps({k: (round(v["median"], 2) if isinstance(v, dict) else v) for k, v in entry.items()}), flush=True)
            del S, leaves, gos
            torch.cuda.empty_cache()
    return res


def episodes(a, dev):
    import torch
    from litemkd_amd import train_teacher as TT
    res = {}
    for L in LENGTHS:
        ps = TT.build_parser()
        args = TT.args_check(ps, ps.parse_args(["--synthetic", "--no_save", "--way", "5", "--shot", "5", "--query_per_class", "5", "--trans_num", "2",
                                                "--seq_len", str(L)]))
        torch.manual_seed(3)
        model = TT.build_model(args, dev)
        task = TT.SyntheticFeatureEpisodes(args, 3, dev, proto_scale=0.0).episode()      # classes that cannot be told apart: the loss does not saturate
        labels = task["target_labels"].long()

        def episode(_):
            loss = TT.summed_cross_entropy(model(task["context_features"], task["context_labels"], task["target_features"])["logits"], labels)
            loss.backward()
            return loss
        first = float(episode(0))
        assert first == first and first > 0.0, first
        res["seq_len_%d" % L] = {"first_loss": first, "episode_ms": stat([t / 1e3 for t in events_us(episode, a.episode_iters, a.batches, 2)])}
        print(json.dumps({"seq_len": L, "episode_ms": res["seq_len_%d" % L]["episode_ms"]["median"]}), flush=True)
        del model, task
        torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20, help="launches per timing")
    p.add_argument("--episode_iters", type=int, default=3, help="episodes per timing")
    p.add_argument("--batches", type=int, default=7, help="timings")
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rotate_mb", type=int, default=768, help="the buffer sets together hold at least this much; 0: one set")
    p.add_argument("--no_episode", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import litemkd_amd
    assert torch.cuda.is_available(), "mfm_long_bench needs the GPU"
    litemkd_amd.lib().call("lmkd_device_check", 0)
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "what": "MFM attention for up to 16 tokens: microseconds per launch, %d timings of %d launches after %d warm-up launches, every launch "
                   "on the next of `buffer_sets` operand sets (%s); TB_per_s = the bytes one launch must move / the median time, of_hbm = "
                   "that / %.2f TB/s; teacher training episodes in milliseconds, %d timings of %d episodes"
                   % (a.batches, a.iters, a.warmup, "together over %d MB: HBM figures" % a.rotate_mb if a.rotate_mb else "one set: cache figures",
                      HBM_TBS, a.batches, a.episode_iters),
           "attention": attention(a, dev)}
    if not a.no_episode:
        out["teacher_episode"] = episodes(a, dev)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print("written" if a.out else line, flush=True)


if __name__ == "__main__":
    main()
