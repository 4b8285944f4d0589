#!/usr/bin/env python3
"""Train-step time at both ends of the ViT patch-grid range; prints ONE JSON line and writes it to
profiles/grids_bench.json (--out).

Per grid, in bf16 and f16: the graph-replayed RPO train step (K = 24, 19 classes, synthetic weights, images resident in
HBM) -- ViT-L/14@336px at B = 16 and ViT-B/32 at B = 32, next to ViT-L/14 (224 px, B = 16) and ViT-B/16 (B = 32) from the
same process -- as time per step (host clock around --steps steps that end in a device synchronise, after --warmup;
median / min / max over --repeats), images/s, the step's algorithmic FLOPs (config.flops_step) and the whole step's
algorithmic FLOP/s over the 2.5 PFLOP/s dense 16-bit peak (an end-to-end rate, not a kernel's share of peak).  And, per
launch, the long-sequence attention forward at N = 577 against the all-keys-in-LDS forward at N = 257 (B = 16, 16 heads,
K = 24): HIP events around 100 back-to-back launches after 10 warm-up launches, 5 repeats.  No threshold is asserted.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PEAK_FLOPS = 2.5e15


def _ms(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def step_times(torch, cfg, sd, toks, B, act, steps, warmup, repeats):
    from rpo_amd import synth
    from rpo_amd.trainer import RPO
    pool = 3
    imgs = [torch.from_numpy(synth.images(cfg, B, seed=1234 + 17 * i)).cuda() for i in range(pool)]
    labs = [torch.from_numpy(synth.labels(cfg, B, seed=4321 + 17 * i)).cuda() for i in range(pool)]
    tr = RPO(cfg, sd, toks, None, "cuda:0", act, batch_size=B, num_batches=10 ** 9, prompts=synth.prompts(cfg, sd, seed=7))
    step = lambda i: tr.step_async(imgs[i % pool], labs[i % pool], imgs[(i + 1) % pool])
    for i in range(warmup):
        step(i)
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(i)
        tr._join_side()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    loss = float(tr.engine.loss.item())
    del tr, imgs, labs
    torch.cuda.empty_cache()
    return out, loss


def attn_launch_us(torch, ops, N, act, B=16, H=16, Kp=24, launches=100, warmup=10, repeats=5):
    d = 64 * H
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B * (N + Kp), 3 * d, generator=g).to("cuda:0", act)
    out = torch.empty(B * (N + Kp), d, dtype=act, device="cuda:0")
    run = lambda: ops.attn_readonly_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], out, B, H, N, Kp)
    for _ in range(warmup):
        run()
    res = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            run()
        e1.record()
        e1.synchronize()
        res.append(1e3 * e0.elapsed_time(e1) / launches)
    flops = 4.0 * B * H * (N + Kp) * N * 64
    return {"us_per_launch": _ms(res), "tflops_at_median": round(flops / (statistics.median(res) * 1e-6) / 1e12, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grids_bench.json"))
    a = ap.parse_args()
    import torch
    from rpo_amd import ops, synth
    from rpo_amd.config import flops_step, vit_b16, vit_b32, vit_l14, vit_l14_336
    assert torch.cuda.is_available(), "bench_grids needs cuda:0"
    torch.cuda.set_device(0)
    toks = synth.oxford_pets_base_tokens()
    lens = synth.len_prompts(toks)
    out = {"metric": "grids_bench", "device": torch.cuda.get_device_name(0), "K": 24, "n_cls": 19,
           "steps_per_repeat": a.steps, "warmup": a.warmup, "repeats": a.repeats, "peak_flops": PEAK_FLOPS,
           "timing": "host clock around graph-replayed steps ending in a device synchronise; attention: HIP events "
                     "around 100 back-to-back launches after 10 warm-up launches",
           "steps": {}, "attention_forward": {}}
    for make, B in ((vit_l14_336, 16), (vit_b32, 32), (vit_l14, 16), (vit_b16, 32)):
        cfg = make(K=24)
        sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
        fl = flops_step(cfg, B, lens)
        rec = {"batch": B, "image_size": cfg.image_size, "patch": cfg.patch, "n_frozen": cfg.n_frozen,
               "algorithmic_gflop_per_step": round(fl / 1e9, 2)}
        for name, act in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            t, loss = step_times(torch, cfg, sd, toks, B, act, a.steps, a.warmup, a.repeats)
            med = statistics.median(t)
            rec[name] = {"step_ms": _ms(t), "images_s": round(B / (med * 1e-3), 1),
                         "fraction_of_peak": round(fl / (med * 1e-3) / PEAK_FLOPS, 4), "last_loss": round(loss, 5)}
        out["steps"][cfg.name] = rec
        del sd
    for name, act in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        out["attention_forward"][name] = {
            "N577_chunked_attn_fwd_long_kernel": attn_launch_us(torch, ops, 577, act),
            "N257_keys_in_lds_attn_fwd_kernel": attn_launch_us(torch, ops, 257, act)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
