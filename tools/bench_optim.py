#!/usr/bin/env python3
"""rpo_optim_step_sets against rpo_sgd_step_sets, and the RPO step with Adam against the RPO step with SGD, on one MI355X
(DESIGN.md section 9k); writes profiles/optim_bench.json (or --out).

  kernel  device time of one optimiser call, graph-replayed (launch cost as inside a step), HIP event pairs around a batch
          of replays: rpo_sgd_step_sets vs rpo_optim_step_sets with kind SGD and with kind Adam, elementwise and guarded,
          at RPO's 30 720 floats x {1, 8} sets and LP's 262 656 floats x 1 set
  step    the RPO step (ViT-B/16, K = 24, bf16, batch 4 and 32) with name="sgd" (the unchanged path) against name="adam":
          HIP event pairs around `steps` graph-replayed steps per repeat

One process, the arms alternate per repeat after a warm-up round; every figure is the median over the repeats with min /
max, and `sgd_spread` is (max - min) / median of the SGD arm: the yardstick for the adam / sgd ratio.
Usage: python tools/bench_optim.py [--steps 100] [--repeats 7] [--out profiles/optim_bench.json]"""
import argparse
import json
import os
import socket
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rpo_amd import ops, optim, synth  # noqa: E402
from rpo_amd.config import vit_b16  # noqa: E402
from rpo_amd.trainer import RPO, OptimConfig  # noqa: E402

DEV = "cuda:0"


def _events(fn, n: int) -> float:
    """Mean device ms per call of fn over n calls (one HIP event pair on the current stream)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def _stat(v, scale=1.0, nd=3):
    return {"median": round(statistics.median(v) * scale, nd), "min": round(min(v) * scale, nd), "max": round(max(v) * scale, nd)}


def _graph(fn):
    fn()                                            # (an eager launch first: kernel load outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        fn()
    return g


def bench_kernel(n: int, sets: int, guarded: bool, replays: int, repeats: int) -> dict:
    z = lambda: torch.zeros(sets, n, device=DEV)
    p, g, buf, s1 = 0.02 * torch.randn(sets, n, device=DEV), 1e-3 * torch.randn(sets, n, device=DEV), z(), z()
    found = torch.zeros(sets, 2, dtype=torch.int32, device=DEV) if guarded else None
    hyper4 = torch.tensor([[0.01, 0.9, 5e-4, 1.0]] * sets, dtype=torch.float32, device=DEV)
    arms = {"sgd_step_sets": lambda: ops.sgd_step_sets(p, g, buf, hyper4, n, 0, first_step=False, found_inf=found)}
    for name in ("sgd", "adam"):
        ocs = [OptimConfig(name=name)] * sets
        kind, hyper = optim.kind_table(ocs).to(DEV), optim.hyper_table(ocs, 1).to(DEV)
        step = torch.ones(sets, dtype=torch.int32, device=DEV)
        arms[f"optim_step_sets_{name}"] = (lambda kind=kind, hyper=hyper, step=step: ops.optim_step_sets(
            p, g, buf, s1, None, kind, hyper, step, n, 0, found_inf=found))
    graphs = {k: _graph(fn) for k, fn in arms.items()}
    times = {k: [] for k in arms}
    for r in range(repeats + 1):                    # round 0 is the warm-up round
        for k, gr in graphs.items():
            t = _events(gr.replay, replays)
            if r:
                times[k].append(t)
    out = {k: _stat(v, 1e3, 2) for k, v in times.items()}           # us per call
    base = statistics.median(times["sgd_step_sets"])
    out["ratio_optim_sgd"] = round(statistics.median(times["optim_step_sets_sgd"]) / base, 3)
    out["ratio_optim_adam"] = round(statistics.median(times["optim_step_sets_adam"]) / base, 3)
    return out


def bench_step(B: int, steps: int, warmup: int, repeats: int) -> dict:
    cfg = vit_b16(K=24)
    toks = synth.default_tokens(cfg)
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
    prompts = synth.prompts(cfg, sd, seed=7)
    pool = 4
    imgs = [torch.from_numpy(synth.images(cfg, B, seed=1234 + 17 * i)).to(DEV) for i in range(pool)]
    labs = [torch.from_numpy(synth.labels(cfg, B, seed=4321 + 17 * i)).to(DEV) for i in range(pool)]
    trs = {name: RPO(cfg, sd, toks, OptimConfig(name=name, lr=0.01 if name == "sgd" else 1e-3), DEV, torch.bfloat16,
                     batch_size=B, num_batches=10 ** 9, prompts=prompts) for name in ("sgd", "adam")}
    it = {k: 0 for k in trs}

    def one(name):
        i = it[name] = it[name] + 1
        trs[name].step_async(imgs[i % pool], labs[i % pool])

    for name in trs:
        for _ in range(warmup):
            one(name)
    torch.cuda.synchronize()
    times = {k: [] for k in trs}
    for r in range(repeats + 1):                    # round 0 is the warm-up round
        for name in trs:
            t = _events(lambda: one(name), steps)
            trs[name]._join_side()
            torch.cuda.synchronize()
            if r:
                times[name].append(t)
    loss = {k: float(tr.engine.loss.item()) for k, tr in trs.items()}
    sgd = statistics.median(times["sgd"])
    out = {"sgd_ms": _stat(times["sgd"], nd=4), "adam_ms": _stat(times["adam"], nd=4),
           "ratio_adam_sgd": round(statistics.median(times["adam"]) / sgd, 4),
           "sgd_spread": round((max(times["sgd"]) - min(times["sgd"])) / sgd, 4),
           "early_text": {k: bool(getattr(tr, "_early_text", False)) for k, tr in trs.items()},
           "loss": {k: round(v, 4) for k, v in loss.items()}, "finite": all(np.isfinite(v) for v in loss.values())}
    del trs
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optim needs cuda:0"
    torch.cuda.set_device(0)
    res = {"metric": "optim_bench", "device": torch.cuda.get_device_name(0), "host": socket.gethostname(),
           "timing": "HIP event pairs; one process; arms alternate per repeat after a warm-up round; median / min / max over "
                     "the repeats", "repeats": a.repeats, "replays_per_repeat": a.replays, "steps_per_repeat": a.steps,
           "kernel_us": {}, "step": {}}
    for n, sets, what in ((30720, 1, "rpo_k24"), (30720, 8, "rpo_k24_x8"), (262656, 1, "lp")):
        for guarded in (False, True):
            res["kernel_us"][f"{what}_{'guarded' if guarded else 'elementwise'}"] = bench_kernel(n, sets, guarded, a.replays,
                                                                                                 a.repeats)
    for B in (4, 32):
        res["step"][f"vit_b16_k24_bf16_b{B}"] = bench_step(B, a.steps, a.warmup, a.repeats)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
