#!/usr/bin/env python3
"""Step time of the multi-run RPO trainer against the single-run step it replaces; prints ONE JSON line.

Workload: ViT-B/16, K = 24, --n-cls classes (19: the Oxford-Pets base split), synthetic weights and images resident in HBM,
graph-replayed steps, per dtype in --dtypes.  Two arms alternate repeat by repeat in one process (the convention of 9f):
  multi    RPOMulti(n_runs=S, batch_size=B).step_async            one step advances S members
  single   RPO(batch_size=B).step_async(next_image=...)            the existing step, as bench.py --batch B times it;
                                                                   S runs one after the other cost S of these
Each repeat times --steps steps with a host clock around work that ends in a device synchronise.  Condition, in 9f's form
(`multi_median_below_S_x_single_best`): the multi arm's MEDIAN time per step is below S x the single arm's BEST repeat.
Also: S = 1 against the single arm (what the grouped seams and the one-graph step cost), images/s per member and in total,
C-ABI calls per step, HBM bytes.  --single-bench-ms: the figure `python bench.py --batch B` gave on the parent commit in the
same session, written into the JSON next to this tool's single arm.

--trace S: only the multi arm at S, a few steps (run under `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time_steps(step, n, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        step(i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def _abi_calls(fn):
    """C-ABI calls one eager enqueue makes (a call is one launch, except the head: 2 launches up to 128 classes, 6 above)."""
    from rpo_amd import _lib, ops
    n = [0]
    real = _lib.check

    def counting(rc, what=""):
        n[0] += 1
        return real(rc, what)
    ops.check = counting
    try:
        fn()
    finally:
        ops.check = real
    return n[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, nargs="+", default=[1, 2, 3, 4, 8])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--n-cls", type=int, default=19)
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "f16"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--single-bench-ms", type=float, default=None)
    ap.add_argument("--trace", type=int)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from rpo_amd import synth
    from rpo_amd.config import vit_b16
    from rpo_amd.multi import RPOMulti
    from rpo_amd.trainer import RPO, OptimConfig
    assert torch.cuda.is_available(), "bench_multi needs cuda:0"
    torch.cuda.set_device(0)
    dev, B = "cuda:0", a.batch
    cfg = vit_b16(K=24, n_cls=a.n_cls)
    toks = synth.default_tokens(cfg)
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
    DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
    pool, Smax = 4, max(a.S if not a.trace else [a.trace])
    imgs = [torch.from_numpy(np.concatenate([synth.images(cfg, B, seed=1234 + 17 * i + 1000 * s) for s in range(Smax)])).to(dev)
            for i in range(pool)]
    labs = [torch.from_numpy(np.concatenate([synth.labels(cfg, B, seed=4321 + 17 * i + 1000 * s) for s in range(Smax)])).to(dev)
            for i in range(pool)]
    prompts = [synth.prompts(cfg, sd, seed=7 + s) for s in range(Smax)]
    oc = OptimConfig()

    def multi_arm(S, dt):
        tr = RPOMulti(cfg, sd, toks, n_runs=S, batch_size=B, prompts=prompts[:S], optim=oc, device=dev, act_dtype=DT[dt],
                      num_batches=10 ** 9)
        ims = [im[:S * B].contiguous() for im in imgs]
        lbs = [lb[:S * B].contiguous() for lb in labs]
        return tr, (lambda i: tr.step_async(ims[i % pool], lbs[i % pool]))

    if a.trace:
        tr, step = multi_arm(a.trace, a.dtypes[0])
        for i in range(12):
            step(i)
        torch.cuda.synchronize()
        return
    out = {"metric": "multi_bench", "device": torch.cuda.get_device_name(0), "model": "ViT-B/16", "K": 24, "n_cls": a.n_cls,
           "batch_per_member": B, "steps_per_repeat": a.steps, "repeats": a.repeats, "warmup": a.warmup,
           "timing": "host clock around graph-replayed steps ending in a device synchronise; arms alternate per repeat",
           "single_bench_py_ms_parent_commit": a.single_bench_ms, "dtypes": {}}
    for dt in a.dtypes:
        single = RPO(cfg, sd, toks, oc, dev, DT[dt], batch_size=B, num_batches=10 ** 9, prompts=prompts[0])
        s_im, s_lb = [im[:B].contiguous() for im in imgs], [lb[:B].contiguous() for lb in labs]
        single_step = lambda i: single.step_async(s_im[i % pool], s_lb[i % pool], s_im[(i + 1) % pool])
        for i in range(a.warmup):
            single_step(i)
        rows, single_all = {}, []
        for S in a.S:
            tr, step = multi_arm(S, dt)
            for i in range(a.warmup):
                step(i)
            tm, ts = [], []
            for r in range(a.repeats):
                tm.append(_time_steps(step, a.steps, torch))
                ts.append(_time_steps(single_step, a.steps, torch))
            single_all += ts
            med, best1 = statistics.median(tm), min(ts)
            eager = RPOMulti(cfg, sd, toks, n_runs=S, batch_size=B, prompts=prompts[:S], optim=oc, device=dev,
                             act_dtype=DT[dt], num_batches=10 ** 9, use_graph=False)
            eager.step_async(imgs[0][:S * B].contiguous(), labs[0][:S * B].contiguous())
            calls = _abi_calls(lambda: eager.step_async(imgs[1][:S * B].contiguous(), labs[1][:S * B].contiguous()))
            torch.cuda.synchronize()
            rows[str(S)] = {
                "multi_ms": {"median": round(med, 4), "min": round(min(tm), 4), "max": round(max(tm), 4)},
                "single_ms": {"median": round(statistics.median(ts), 4), "min": round(best1, 4), "max": round(max(ts), 4)},
                "S_x_single_best_ms": round(S * best1, 4),
                "multi_median_over_S_x_single_best": round(med / (S * best1), 4),
                "multi_median_below_S_x_single_best": bool(med < S * best1),
                "images_s_per_member": round(B / (med * 1e-3), 1), "images_s_total": round(S * B / (med * 1e-3), 1),
                "abi_calls_per_step": calls,
                "hbm_bytes": int(tr.engine.hbm_bytes() + tr.engine.multi_hbm_bytes()),
                "hbm_bytes_multi_setup": int(tr.engine.multi_hbm_bytes()),
                "last_loss": [round(float(v), 5) for v in tr.engine.m_loss.tolist()]}
            del tr, step, eager
            torch.cuda.empty_cache()
        calls1 = None
        if not single.use_graph:
            calls1 = _abi_calls(lambda: single_step(0))
        out["dtypes"][dt] = {"S": rows, "single_ms_all_repeats": {"median": round(statistics.median(single_all), 4),
                                                                  "min": round(min(single_all), 4)},
                             "single_hbm_bytes": int(single.engine.hbm_bytes()), "single_abi_calls_per_step": calls1}
        del single
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
