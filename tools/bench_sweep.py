#!/usr/bin/env python3
"""Step time of the sweep trainer (rpo_amd/sweep.py); prints ONE JSON line (--out: also written to a file).

Workload, as 9f / 9g: ViT-B/16, --n-cls classes (19: the Oxford-Pets base split), B = 4 per member, bf16, synthetic weights
and images resident in HBM, graph-replayed steps; the arms of a comparison alternate repeat by repeat in one process; each
repeat times --steps steps (after --warmup) with a host clock around work that ends in a device synchronise.

  (a) what the device tables cost: RPOSweep with three identical K = 24 members and one shared OptimConfig against
      RPOMulti(S = 3).  Reported: the sweep arm's MEDIAN against the RPOMulti arm's min - max over its repeats
      (`sweep_median_within_multi_spread`; outside: by how much).
  (b) a real sweep: RPOSweep with K = 24 / 16 / 8 and three learning rates against the three standalone RPO(K_s) arms.
      Condition in 9g's form (`sweep_median_below_sum_of_single_bests`): the sweep's MEDIAN time per step below the SUM of the
      standalone arms' BEST repeats.
  captures: HIP-graph captures over 8 steps of 2-batch epochs (4 learning rates): RPOSweep's against RPOMulti's.
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


def _ms(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--n-cls", type=int, default=19)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import dataclasses
    import torch
    from rpo_amd import synth
    from rpo_amd.config import vit_b16
    from rpo_amd.multi import RPOMulti
    from rpo_amd.sweep import RPOSweep
    from rpo_amd.trainer import RPO, OptimConfig
    assert torch.cuda.is_available(), "bench_sweep needs cuda:0"
    torch.cuda.set_device(0)
    dev, B, S, Ks = "cuda:0", a.batch, 3, (24, 16, 8)
    act = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    cfg = vit_b16(K=24, n_cls=a.n_cls)
    toks = synth.default_tokens(cfg)
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
    pool = 4
    imgs = [torch.from_numpy(np.concatenate([synth.images(cfg, B, seed=1234 + 17 * i + 1000 * s) for s in range(S)])).to(dev)
            for i in range(pool)]
    labs = [torch.from_numpy(np.concatenate([synth.labels(cfg, B, seed=4321 + 17 * i + 1000 * s) for s in range(S)])).to(dev)
            for i in range(pool)]
    oc = OptimConfig()
    same_prompts = [synth.prompts(cfg, sd, seed=7 + s) for s in range(S)]
    kcfgs = [dataclasses.replace(cfg, K=k) for k in Ks]
    k_prompts = [synth.prompts(kcfgs[s], sd, seed=7 + s) for s in range(S)]
    k_optims = [OptimConfig(lr=0.01), OptimConfig(lr=0.02), OptimConfig(lr=0.005)]

    def sweep(prompts, ks, optims, num_batches=10 ** 9):
        return RPOSweep(cfg, sd, toks, members=[dict(prompts=prompts[s], K=ks[s], optim=optims[s]) for s in range(S)],
                        batch_size=B, device=dev, act_dtype=act, num_batches=num_batches)

    def multi(num_batches=10 ** 9):
        return RPOMulti(cfg, sd, toks, n_runs=S, batch_size=B, prompts=same_prompts, optim=oc, device=dev, act_dtype=act,
                        num_batches=num_batches)

    member_step = lambda tr: (lambda i: tr.step_async(imgs[i % pool], labs[i % pool]))
    out = {"metric": "sweep_bench", "device": torch.cuda.get_device_name(0), "model": "ViT-B/16", "n_cls": a.n_cls,
           "batch_per_member": B, "members": S, "dtype": a.dtype, "steps_per_repeat": a.steps, "repeats": a.repeats,
           "warmup": a.warmup,
           "timing": "host clock around graph-replayed steps ending in a device synchronise; arms alternate per repeat"}
    # ---- (a) identical members: the device tables and the _k head against RPOMulti
    sw, mu = sweep(same_prompts, (24,) * S, [oc] * S), multi()
    steps = [member_step(sw), member_step(mu)]
    for st in steps:
        for i in range(a.warmup):
            st(i)
    t_sw, t_mu = [], []
    for r in range(a.repeats):
        t_sw.append(_time_steps(steps[0], a.steps, torch))
        t_mu.append(_time_steps(steps[1], a.steps, torch))
    med = statistics.median(t_sw)
    inside = min(t_mu) <= med <= max(t_mu)
    out["a_identical_members"] = {
        "sweep_ms": _ms(t_sw), "multi_ms": _ms(t_mu), "sweep_median_within_multi_spread": bool(inside),
        "sweep_median_outside_by_ms": 0.0 if inside else round(med - max(t_mu) if med > max(t_mu) else med - min(t_mu), 4),
        "sweep_median_over_multi_median": round(med / statistics.median(t_mu), 4),
        "captures": {"sweep": sw.captures, "multi": mu.captures}}
    del sw, mu, steps
    torch.cuda.empty_cache()
    # ---- (b) K = 24 / 16 / 8 with three learning rates against the three standalone runs
    sw = sweep(k_prompts, Ks, k_optims)
    solos = [RPO(kcfgs[s], sd, toks, k_optims[s], dev, act, batch_size=B, num_batches=10 ** 9, prompts=k_prompts[s])
             for s in range(S)]
    s_im = [[im[s * B:(s + 1) * B].contiguous() for im in imgs] for s in range(S)]
    s_lb = [[lb[s * B:(s + 1) * B].contiguous() for lb in labs] for s in range(S)]
    solo_step = lambda s: (lambda i: solos[s].step_async(s_im[s][i % pool], s_lb[s][i % pool], s_im[s][(i + 1) % pool]))
    steps = [member_step(sw)] + [solo_step(s) for s in range(S)]
    for st in steps:
        for i in range(a.warmup):
            st(i)
    times = [[] for _ in steps]
    for r in range(a.repeats):
        for t, st in zip(times, steps):
            t.append(_time_steps(st, a.steps, torch))
    med, bests = statistics.median(times[0]), [min(t) for t in times[1:]]
    out["b_K_24_16_8_three_rates"] = {
        "member_K": list(Ks), "member_lr": [o.lr for o in k_optims], "sweep_ms": _ms(times[0]),
        "single_ms": {str(Ks[s]): _ms(times[1 + s]) for s in range(S)}, "sum_of_single_bests_ms": round(sum(bests), 4),
        "sweep_median_over_sum_of_single_bests": round(med / sum(bests), 4),
        "sweep_median_below_sum_of_single_bests": bool(med < sum(bests)),
        "images_s_total": round(S * B / (med * 1e-3), 1), "captures": {"sweep": sw.captures},
        "last_loss": [round(float(v), 5) for v in sw.engine.m_loss.tolist()]}
    del sw, solos, steps
    torch.cuda.empty_cache()
    # ---- captures per run: 8 steps of 2-batch epochs = 4 learning rates
    caps = {}
    for name, tr in (("sweep", sweep(k_prompts, Ks, k_optims, num_batches=2)), ("multi", multi(num_batches=2))):
        for i in range(8):
            tr.step_async(imgs[i % pool], labs[i % pool])
            tr._loop_advance()
        torch.cuda.synchronize()
        caps[name] = tr.captures
        del tr
    out["captures_over_4_learning_rates"] = caps
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
