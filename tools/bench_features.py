#!/usr/bin/env python3
"""Measurements of DESIGN.md section 9n on one MI355X, one process: writes profiles/features_bench.json.

Zero-shot CLIP on full-size ViT-B/16 (bf16, e = 512), a synthetic resident set of `--images` decoded images, class sets of
C = 19 (the Oxford-Pets base prompts) and C = 1000 (synthetic prompts of 8-20 tokens), S = 1, 8, 81 classifiers
(S = 1: the model's own text features; more: seeded random classifiers -- the cost does not depend on the values):

  (a) `test(set)` with the image pass: what ONE classifier costs today (S classifiers: S such passes, stated as S x).
  (b) the comparator on the CACHED features, written here from existing ops: per chunk of 100 rows and per classifier the
      existing cosine head (rpo_head_fwd_bwd, K = 1, eval) and rpo_eval_accumulate -- 2 S n / 100 launches, the logits
      through memory.
  (c) the fused call: ONE rpo_features_classify launch for all S.

(b) and (c) are timed from the first enqueue to a device synchronise with zeroed counters in place; the read-back of
counts and confusion matrices is the same bytes for both and is timed on its own.  Short arms are repeated inside the
timed window until it holds about 0.1 s.  Every arm runs untimed first; (b) and (c) alternate; medians with min-max.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, torch, inner=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def stats(v):
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), repeats=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--test-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_bench.json"))
    a = ap.parse_args()
    import torch
    from rpo_amd import ops, synth
    from rpo_amd.config import vit_b16
    from rpo_amd.features import ImageFeatures
    from rpo_amd.input_pipeline import DeviceImageSet
    from rpo_amd.zeroshot import ZeroshotCLIP
    assert torch.cuda.is_available(), "bench_features.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    n, chunk = a.images, 100
    cfg = vit_b16(K=1)
    e = cfg.embed
    rng = np.random.default_rng(2024)
    images = [rng.integers(0, 256, (375, 500, 3), dtype=np.uint8) for _ in range(n)]
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, images=n, embed=e, act="bf16", chunk=chunk,
               backbone="ViT-B/16 (synthetic weights)", cases=[])
    token_sets = {19: synth.oxford_pets_base_tokens(),
                  1000: synth.synthetic_tokens(cfg, [8 + (5 * c) % 13 for c in range(1000)], seed=31)}
    rows = sorted(set(np.unique(np.concatenate([t.ravel() for t in token_sets.values()])).tolist() + [49407]))
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=rows)
    for C, tokens in token_sets.items():
        zs = ZeroshotCLIP(sd, tokens, dev, torch.bfloat16, max_batch=chunk)
        ds = DeviceImageSet(images, [i % C for i in range(n)], dev)
        zs.test(ds, batch_size=chunk, verbose=False)
        t_a = [timed(lambda: zs.test(ds, batch_size=chunk, verbose=False), torch) for _ in range(a.test_repeats)]
        t_build = timed(lambda: ImageFeatures.build(zs, ds, batch_size=chunk), torch)
        F = ImageFeatures.build(zs, ds, batch_size=chunk)
        own, _, _, _, scale = zs.classifier()
        logits = torch.empty(chunk, C, dtype=torch.float32, device=dev)
        ws = torch.empty(ops.head_workspace_floats(chunk, C, 1, e), dtype=torch.float32, device=dev)
        for S in (1, 8, 81):
            g = torch.Generator().manual_seed(100 * C + S)
            cls = own.unsqueeze(0).clone() if S == 1 else torch.randn(S, C, e, generator=g).to(dev)
            counts_b = torch.zeros(S, 2, dtype=torch.int64, device=dev)
            cmat_b = torch.zeros(S, C * C, dtype=torch.int32, device=dev)
            counts_c, cmat_c = torch.zeros_like(counts_b), torch.zeros_like(cmat_b)

            def arm_b():
                for b0 in range(0, n, chunk):
                    B = min(chunk, n - b0)
                    for s in range(S):
                        ops.head_fwd_bwd(F.feat[b0:b0 + B].view(B, 1, e), cls[s].view(C, 1, e), None, scale, logits[:B], None,
                                         None, None, ws)
                        ops.eval_accumulate(logits[:B], F.labels_dev[b0:b0 + B], counts_b[s], cmat_b[s])

            def arm_c():
                ops.features_classify(F.feat, cls, None, F.labels_dev, scale, True, True, counts_c, cmat_c)

            arm_b(); arm_c()                                              # untimed: code objects, first touches
            torch.cuda.synchronize()
            # one pass each into fresh counters: how many of the S x n predictions the two paths share
            counts_b.zero_(); cmat_b.zero_(); counts_c.zero_(); cmat_c.zero_()
            arm_b(); arm_c()
            torch.cuda.synchronize()
            cells_differ = int((cmat_b != cmat_c).sum().item()) // 2      # a differing prediction moves one count: two cells
            inner_b = max(1, min(50, math.ceil(100.0 / max(timed(arm_b, torch), 1e-3))))
            inner_c = max(1, min(500, math.ceil(100.0 / max(timed(arm_c, torch), 1e-3))))
            tb, tc = [], []
            for _ in range(a.repeats):                                     # alternating
                tb.append(timed(arm_b, torch, inner_b))
                tc.append(timed(arm_c, torch, inner_c))
            t_rb = [timed(lambda: (counts_c.cpu(), cmat_c.cpu()), torch) for _ in range(3)]
            a_ms, b_ms, c_ms = statistics.median(t_a), statistics.median(tb), statistics.median(tc)
            res["cases"].append(dict(
                C=C, S=S, a_test_with_image_pass_one_classifier=stats(t_a), a_times_S_ms=round(a_ms * S, 3),
                features_build_ms=round(t_build, 3), b_head_plus_eval_per_chunk=stats(tb), b_launches=2 * S * math.ceil(n / chunk),
                b_inner=inner_b, c_fused=stats(tc), c_launches=1, c_inner=inner_c, readback=stats(t_rb),
                c_over_b=round(c_ms / b_ms, 4), c_over_a=round(c_ms / (a_ms * S), 6),
                c_plus_readback_over_a=round((c_ms + statistics.median(t_rb)) / (a_ms * S), 6),
                predictions_differing_b_vs_c=cells_differ, predictions=S * n))
            print(json.dumps(res["cases"][-1]), flush=True)
        del zs, F, ds
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
