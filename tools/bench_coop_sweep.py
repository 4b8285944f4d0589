#!/usr/bin/env python3
"""Measurements of DESIGN.md section 9s on one MI355X, one process: writes profiles/coop_sweep_bench.json.

The CoOp train step (full ViT-B/16, bf16, B = 32, n_ctx 16 prompts, inputs resident on the device, the step replayed from one
HIP graph) for S members in one CoOpSweep step on ONE shared batch, next to ONE standalone CoOp step in the same process:

  classes  the 19 Oxford-Pets base prompts (rpo_amd/data/) and 100 synthetic prompts (class names of 4 + (7 c) % 22 tokens)
  arms     S = 1, 4, 8, 16 with every member at n_ctx 16; S = 4, 8, 16 with the members alternating n_ctx 16 / 4 ("mix");
           S = 8 with shared_prefix=True (beside a standalone run that shares too)

Per arm both trainers live side by side; `--warmup` steps each (step 0 eager, step 1 captures), then `--repeats` rounds that
alternate the standalone and the sweep trainer, `--steps` steps per round between a host clock's reads, ending in a device
synchronise.  Median of the rounds with min .. max.  `sweep_over_S_standalone` = (ms of one sweep step) / (S x ms of one
standalone step): below 1, the S runs are faster together than one after the other.  The file is rewritten after every arm."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--classes", default="pets19,100")
    ap.add_argument("--arms", default="1,4,8,16,4:mix,8:mix,16:mix,8:shared")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coop_sweep_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from rpo_amd import synth
    from rpo_amd.config import vit_b16
    from rpo_amd.coop import CoOp
    from rpo_amd.coop_sweep import CoOpSweep
    from rpo_amd.trainer import OptimConfig
    assert torch.cuda.is_available(), "bench_coop_sweep.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n_max, n_short, B = 16, 4, 32
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, repeats=a.repeats, steps=a.steps,
               warmup=a.warmup, model="ViT-B/16", act="bf16", hip_graph=True, n_ctx=n_max, n_ctx_mix=[n_max, n_short],
               batch=B, rows=[])

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for cls in a.classes.split(","):
        if cls == "pets19":
            base = synth.oxford_pets_base_tokens()
        else:
            n = int(cls)
            base = synth.synthetic_tokens(vit_b16(K=1, n_cls=n), [4 + (7 * c) % 22 for c in range(n)], seed=17)
        cfg = vit_b16(K=1, n_cls=base.shape[0])
        toks = synth.coop_tokens(base, n_max)
        sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
        oc = OptimConfig(lr=0.002, warmup_epoch=0, lr_scheduler="constant", max_epoch=50)
        pool = 4
        imgs = [torch.from_numpy(synth.images(cfg, B, seed=1234 + 17 * i)).to(dev) for i in range(pool)]
        labs = [torch.from_numpy(synth.labels(cfg, B, seed=4321 + 17 * i)).to(dev) for i in range(pool)]
        for arm in a.arms.split(","):
            S, kind = int(arm.split(":")[0]), (arm.split(":") + ["same"])[1]
            shared = kind == "shared"
            n_ctxs = [n_short if (kind == "mix" and s % 2) else n_max for s in range(S)]
            torch.manual_seed(0)
            solo = CoOp(sd, toks, n_max, oc, dev, torch.bfloat16, batch_size=B, num_batches=10 ** 9, cfg=cfg, use_graph=True,
                        shared_prefix=shared)
            sweep = CoOpSweep(sd, toks, [dict(seed=s, n_ctx=n, optim=oc) for s, n in enumerate(n_ctxs)], n_ctx=n_max,
                              batch_size=B, num_batches=10 ** 9, act_dtype=torch.bfloat16, use_graph=True,
                              shared_prefix=shared, cfg=cfg, device=dev)
            trs = dict(standalone=solo, sweep=sweep)
            for tr in trs.values():
                for i in range(max(a.warmup, 2)):
                    tr.step_async(imgs[i % pool], labs[i % pool])
            torch.cuda.synchronize()
            assert sweep.captures == 1
            t = {k: [] for k in trs}
            for _ in range(a.repeats):
                for k, tr in trs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(a.steps):
                        out = tr.step_async(imgs[i % pool], labs[i % pool])
                    torch.cuda.synchronize()
                    t[k].append(1e3 * (time.perf_counter() - t0) / a.steps)
                assert bool(torch.isfinite(out).all())
            eng = sweep.engine
            times = {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                             all_ms=[round(x, 4) for x in v]) for k, v in t.items()}
            ratio = times["sweep"]["median_ms"] / (S * times["standalone"]["median_ms"])
            rec = dict(classes=cls, n_cls=cfg.n_cls, S=S, arm=kind, n_ctx_members=n_ctxs, shared_prefix=shared, Lmax=eng.Lmax,
                       text_rows=int(eng.cx[0].shape[0]), ms_per_step=times,
                       ms_per_member_step=round(times["sweep"]["median_ms"] / S, 4), sweep_over_S_standalone=round(ratio, 4))
            res["rows"].append(rec)
            dump()
            print(f"[{cls} S={S} {kind}] text rows {rec['text_rows']}: standalone {times['standalone']['median_ms']:.3f} ms ("
                  f"{times['standalone']['min_ms']:.3f} .. {times['standalone']['max_ms']:.3f}); sweep "
                  f"{times['sweep']['median_ms']:.3f} ms ({times['sweep']['min_ms']:.3f} .. {times['sweep']['max_ms']:.3f}) = "
                  f"{rec['ms_per_member_step']:.3f} per member -> sweep / (S x standalone) {ratio:.3f}", flush=True)
            del trs, solo, sweep, eng, tr
            torch.cuda.empty_cache()
    dump()
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}))


if __name__ == "__main__":
    main()
