#!/usr/bin/env python3
"""Step time of the shared-batch sweep (rpo_amd/shared_sweep.py) against the own-batch sweep fed the same
images; prints ONE JSON line (--out: also written to a file, default profiles/shared_sweep_bench.json).

Workload, the conventions of tools/bench_sweep.py: ViT-B/16, 12 + 12 layers, K = 24 for every member, bf16, 19 classes
(the Oxford-Pets base split), synthetic weights and images resident in HBM, graph-replayed steps; every arm is warmed
before anything is timed; the arms of a configuration alternate repeat by repeat in one process; each repeat times --steps
steps with a host clock around work that ends in a device synchronise and reports the mean step time of the repeat.

Per B in --batches (4: the reference's main_K24.yaml; 32) and S in --members (1, 4, 8):
  (a) RPOSweep of the S members, each fed the SAME B images: the batch replicated to S x B, member-major (what the trainer
      could do before the shared-batch step)
  (b) RPOSharedSweep of the same members on the ONE batch
  (c) one standalone RPO step at batch B, for scale (once per B)
Condition: at S = 8 the SLOWEST (b) repeat below the FASTEST (a) repeat, at both B (`b_slowest_below_a_fastest`).
S = 1 is expected to lose to (c) -- a whole pass plus the prompt-row pass -- and is reported as it comes.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_steps(step, n, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        step(i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def _ms(v):
    return {"repeats": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,32")
    ap.add_argument("--members", default="1,4,8")
    ap.add_argument("--n-cls", type=int, default=19)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_sweep_bench.json"))
    a = ap.parse_args()
    import torch
    from rpo_amd import synth
    from rpo_amd.config import vit_b16
    from rpo_amd.engine_prompt_train import prompt_train_bytes
    from rpo_amd.shared_sweep import RPOSharedSweep
    from rpo_amd.sweep import RPOSweep
    from rpo_amd.trainer import RPO, OptimConfig
    assert torch.cuda.is_available(), "bench_shared_sweep needs cuda:0"
    torch.cuda.set_device(0)
    dev, K = "cuda:0", 24
    act = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    cfg = vit_b16(K=K, n_cls=a.n_cls)
    toks = synth.default_tokens(cfg)
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
    pool = 4
    out = {"metric": "shared_sweep_bench", "device": torch.cuda.get_device_name(0), "model": "ViT-B/16", "layers": [12, 12],
           "K": K, "n_cls": a.n_cls, "dtype": a.dtype, "steps_per_repeat": a.steps, "repeats": a.repeats, "warmup": a.warmup,
           "timing": "host clock around graph-replayed steps ending in a device synchronise; mean step time per repeat; "
                     "arms alternate per repeat; every arm warmed before the first timed repeat",
           "configs": []}
    for B in (int(v) for v in a.batches.split(",")):
        imgs = [torch.from_numpy(synth.images(cfg, B, seed=1234 + 17 * i)).to(dev) for i in range(pool)]
        labs = [torch.from_numpy(synth.labels(cfg, B, seed=4321 + 17 * i)).to(dev) for i in range(pool)]
        solo = RPO(cfg, sd, toks, OptimConfig(lr=0.01), dev, act, batch_size=B, num_batches=10 ** 9,
                   prompts=synth.prompts(cfg, sd, seed=7))
        solo_step = lambda i: solo.step_async(imgs[i % pool], labs[i % pool], imgs[(i + 1) % pool])
        for S in (int(v) for v in a.members.split(",")):
            members = [dict(prompts=synth.prompts(cfg, sd, seed=7 + s), K=K, optim=OptimConfig(lr=0.01 / (1 + s))) for s in range(S)]
            own = RPOSweep(cfg, sd, toks, members=members, batch_size=B, device=dev, act_dtype=act, num_batches=10 ** 9)
            shared = RPOSharedSweep(cfg, sd, toks, members=members, batch_size=B, device=dev, act_dtype=act, num_batches=10 ** 9)
            rep_i = [im.repeat(S, 1, 1, 1).contiguous() for im in imgs]           # the same B images for every member
            rep_l = [lb.repeat(S).contiguous() for lb in labs]
            steps = {"a_own_batch_sweep": lambda i: own.step_async(rep_i[i % pool], rep_l[i % pool]),
                     "b_shared_sweep": lambda i: shared.step_async(imgs[i % pool], labs[i % pool]),
                     "c_standalone": solo_step}
            for st in steps.values():
                for i in range(a.warmup):
                    st(i)
            torch.cuda.synchronize()
            times = {k: [] for k in steps}
            for r in range(a.repeats):
                for k, st in steps.items():
                    times[k].append(_time_steps(st, a.steps, torch))
            ta, tb, tc = times["a_own_batch_sweep"], times["b_shared_sweep"], times["c_standalone"]
            rec = {"B": B, "S": S, "a_own_batch_sweep_ms": _ms(ta), "b_shared_sweep_ms": _ms(tb), "c_standalone_ms": _ms(tc),
                   "a_over_b_medians": round(statistics.median(ta) / statistics.median(tb), 4),
                   "b_over_c_medians": round(statistics.median(tb) / statistics.median(tc), 4),
                   "b_slowest_below_a_fastest": bool(max(tb) < min(ta)),
                   "bytes": {"a_engine": own.engine.hbm_bytes(), "a_members": own.engine.multi_hbm_bytes(),
                             "b_engine": shared.engine.hbm_bytes(), "b_members": shared.engine.multi_hbm_bytes(),
                             "b_prompt_rows": shared.engine.prompt_train_hbm_bytes(),
                             "b_prompt_rows_formula": prompt_train_bytes(cfg, S, B, act), "c_engine": solo.engine.hbm_bytes()},
                   "captures": {"a": own.captures, "b": shared.captures},
                   "last_loss": {"a": [round(float(v), 5) for v in own.engine.m_loss.tolist()],
                                 "b": [round(float(v), 5) for v in shared.engine.m_loss.tolist()]}}
            out["configs"].append(rec)
            print(f"# B={B} S={S}: a {rec['a_own_batch_sweep_ms']['median']} b {rec['b_shared_sweep_ms']['median']} "
                  f"c {rec['c_standalone_ms']['median']} ms; a/b {rec['a_over_b_medians']}", file=sys.stderr, flush=True)
            del own, shared, steps, rep_i, rep_l
            torch.cuda.empty_cache()
        del solo
        torch.cuda.empty_cache()
    s8 = [c for c in out["configs"] if c["S"] == 8]
    out["condition_S8_b_slowest_below_a_fastest_at_every_B"] = bool(s8) and all(c["b_slowest_below_a_fastest"] for c in s8)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
