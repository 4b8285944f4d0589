#!/usr/bin/env python3
"""Measurements of DESIGN.md section 9q on one MI355X, one process: writes profiles/coop_prefix_bench.json.

The CoOp / CoCoOp train step (bench.py --trainer coop / cocoop's: full ViT-B/16, bf16, inputs resident on the device, the
step replayed from one HIP graph) with the text tower on the dense row layout (`shared_prefix=False`, n_cls * Lmax rows per
replica) and on the shared-prefix layout (`shared_prefix=True`, P + n_cls * S rows), on the same tokens and from the same
start:

  coop    B 32, n_ctx 16: the 19 Oxford-Pets base prompts (rpo_amd/data/), synthetic class sets of 100, 397 and 1000 prompts
          (class names of 4 + (7 c) % 22 tokens with SOS / '.' / EOT, i.e. prompts of 20-41 tokens)
  cocoop  B 1, n_ctx 4: the 19 Oxford-Pets base prompts and the 100 synthetic prompts

Both trainers of a row live side by side; `--warmup` steps each (step 0 eager, step 1 captures), then `--repeats` rounds
that alternate dense and shared, `--steps` steps per round between a host clock's reads, ending in a synchronise.  Median
of the rounds with min .. max, the rows of each layout beside the times, and the largest loss difference between the two
trainers over the timed steps (they see the same batches)."""
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
    ap.add_argument("--rows", default="coop:pets19,coop:100,coop:397,coop:1000,cocoop:pets19,cocoop:100")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coop_prefix_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from rpo_amd import synth
    from rpo_amd.config import vit_b16
    from rpo_amd.coop import CoCoOp, CoOp
    from rpo_amd.engine_coop import shared_rows
    from rpo_amd.trainer import OptimConfig
    assert torch.cuda.is_available(), "bench_coop_prefix.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, repeats=a.repeats, steps=a.steps,
               warmup=a.warmup, model="ViT-B/16", act="bf16", hip_graph=True, rows=[])
    for row in a.rows.split(","):
        kind, cls = row.split(":")
        coop = kind == "coop"
        n_ctx, B = (16, 32) if coop else (4, 1)
        if cls == "pets19":
            base = synth.oxford_pets_base_tokens()
        else:
            n = int(cls)
            base = synth.synthetic_tokens(vit_b16(K=1, n_cls=n), [4 + (7 * c) % 22 for c in range(n)], seed=17)
        cfg = vit_b16(K=1, n_cls=base.shape[0])
        toks = synth.coop_tokens(base, n_ctx)
        sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
        oc = OptimConfig(lr=0.002, warmup_epoch=0, lr_scheduler="constant")
        Tr = CoOp if coop else CoCoOp
        trs = {}
        for name, shared in (("dense", False), ("shared", True)):
            torch.manual_seed(0)                              # the same initial ctx / meta-net draws
            trs[name] = Tr(sd, toks, n_ctx, oc, dev, torch.bfloat16, batch_size=B, num_batches=10 ** 9, cfg=cfg,
                           use_graph=True, shared_prefix=shared)
        pool = 4
        imgs = [torch.from_numpy(synth.images(cfg, B, seed=1234 + 17 * i)).to(dev) for i in range(pool)]
        labs = [torch.from_numpy(synth.labels(cfg, B, seed=4321 + 17 * i)).to(dev) for i in range(pool)]
        for tr in trs.values():
            for i in range(max(a.warmup, 2)):
                tr.step_async(imgs[i % pool], labs[i % pool])
        torch.cuda.synchronize()
        t = {k: [] for k in trs}
        loss = {}
        for _ in range(a.repeats):
            for k, tr in trs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.steps):
                    out = tr.step_async(imgs[i % pool], labs[i % pool])
                torch.cuda.synchronize()
                t[k].append(1e3 * (time.perf_counter() - t0) / a.steps)
                loss[k] = float(out.item())
        eng = trs["dense"].engine
        R = 1 if coop else B
        rows = dict(dense=R * cfg.n_cls * eng.Lmax, shared=shared_rows(R, cfg.n_cls, eng.Lmax, n_ctx))
        assert trs["shared"].engine.cx[0].shape[0] == rows["shared"] and eng.cx[0].shape[0] == rows["dense"]
        times = {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                         all_ms=[round(x, 4) for x in v]) for k, v in t.items()}
        rec = dict(trainer=kind, classes=cls, n_cls=cfg.n_cls, batch=B, n_ctx=n_ctx, Lmax=eng.Lmax, rows=rows,
                   row_ratio=round(rows["dense"] / rows["shared"], 3), ms_per_step=times,
                   dense_over_shared=round(times["dense"]["median_ms"] / times["shared"]["median_ms"], 4),
                   final_loss=loss, final_loss_diff=abs(loss["dense"] - loss["shared"]))
        res["rows"].append(rec)
        print(f"[{kind} {cls}] n_cls {cfg.n_cls} B {B} n_ctx {n_ctx} Lmax {eng.Lmax}: rows dense {rows['dense']} shared "
              f"{rows['shared']} (x{rec['row_ratio']}); ms/step dense {times['dense']['median_ms']:.3f} "
              f"({times['dense']['min_ms']:.3f} .. {times['dense']['max_ms']:.3f}) shared {times['shared']['median_ms']:.3f} "
              f"({times['shared']['min_ms']:.3f} .. {times['shared']['max_ms']:.3f}) -> dense / shared "
              f"{rec['dense_over_shared']:.3f}; final loss {loss['dense']:.5f} / {loss['shared']:.5f}", flush=True)
        del trs, tr, eng
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}))


if __name__ == "__main__":
    main()
