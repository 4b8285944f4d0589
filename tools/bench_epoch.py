#!/usr/bin/env python3
"""Epoch-level throughput of the training / test loops on one MI355X; prints ONE JSON line per call.

Workload: ViT-B/16, K = 24, batch 32, bf16, 19 classes, a synthetic DECODED few-shot set (304 uint8 images of 375 x 500 from
a seeded generator: 16 shots x 19 classes), synthetic full-size CLIP weights.  An epoch (9 batches; the 16 left-over images
are dropped, as drop_last does) is timed end to end with host clocks around a final device sync.

  --arm A   today's loop: `for batch: trainer.forward_backward({"img": [decoded images] | staged floats, "label": ...})`.
            Uses only the API of the commit BEFORE the epoch loops, so it can (and for the committed figures did) run from
            a checkout of that commit:  --root <that checkout>  selects the package tree that is imported.
  --arm B   `trainer.run_epoch(DeviceImageSet)`: resident set, lookahead, no per-step read-back.
  --arm C   the ceiling: `step_async` (RPO: with `next_image`) on float batches already on the device -- what bench.py times.
  --arm D   C plus the epoch's LR update behind its last step (the bookkeeping of forward_backward / run_epoch): CoOp, CoCoOp
            and LP capture the learning rate in their step graph and recapture it when it changes, i.e. once per epoch.
  --arm BC / BCD  the arms alternating in one process (one trainer each).

  --what rpo | coop | test     RPO (K = 24) / CoOp (n_ctx 16; arm A feeds float tensors from the staging transform) / the test
                               loop at batch 100 over the same 304 images (A: model_inference + argmax + .item() per batch;
                               B: trainer.test(); no arm C)

`--merge a.json b.json ...` folds the lines of several calls (alternating rounds of processes) into the committed table:
per arm the median, min and max of all repeats, B / A, B / C, and whether B's median exceeds A's by more than the spread
(max - min) of A's own repeats.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def _decoded_set(n=304, n_cls=19, seed=2024):
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (375, 500, 3), dtype=np.uint8) for _ in range(n)]
    labels = [i % n_cls for i in range(n)]
    return images, labels


def _order(n, bs, epoch):
    """A shuffled epoch's batches (numpy; the order does not matter for the timing, and arm A's tree has no epoch_indices)."""
    perm = np.random.default_rng(100 + epoch).permutation(n).tolist()
    return [perm[i:i + bs] for i in range(0, n - bs + 1, bs)]


def _timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["A", "B", "C", "D", "BC", "BCD"])
    ap.add_argument("--what", choices=["rpo", "coop", "test"], default="rpo")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--merge", nargs="+")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge)
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from rpo_amd import synth
    from rpo_amd.config import vit_b16
    assert torch.cuda.is_available(), "bench_epoch needs cuda:0"
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    dev, B = "cuda:0", a.batch
    images, labels = _decoded_set()
    n = len(images)
    nb = n // B
    toks = synth.oxford_pets_base_tokens()

    def make_trainer(batch_size):
        if a.what == "coop":
            from rpo_amd.coop import CoOp
            cfg = vit_b16(K=1)
            ctoks = synth.coop_tokens(toks, 16)
            sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(ctoks).tolist() + [49407])
            ctx = np.random.default_rng(3).normal(0, 0.02, (16, cfg.d_t)).astype(np.float32)
            return cfg, CoOp(sd, ctoks, 16, None, dev, torch.bfloat16, batch_size=batch_size, num_batches=nb, ctx=ctx,
                             use_graph=True)
        from rpo_amd.trainer import RPO
        cfg = vit_b16(K=24)
        sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
        return cfg, RPO(cfg, sd, toks, None, dev, torch.bfloat16, batch_size=batch_size, num_batches=nb, use_graph=True,
                        prompts=synth.prompts(cfg, sd, seed=7))

    arms = list(a.arm)                               # "BC" -> ["B", "C"]
    runs = {}
    if a.what == "test":
        TB = 100
        cfg, tr = make_trainer(TB)
        if "A" in arms:
            def epoch_a(_):
                correct = 0
                for b0 in range(0, n, TB):
                    lab = torch.tensor(labels[b0:b0 + TB], device=dev)
                    logits = tr.model_inference(images[b0:b0 + TB])          # decoded images: eval transform on the device
                    correct += int((logits.argmax(1) == lab).sum().item())
                return correct
            runs["A"] = epoch_a
        if "B" in arms:
            from rpo_amd.input_pipeline import DeviceImageSet
            ds = DeviceImageSet(images, labels, dev)
            runs["B"] = lambda _: tr.test(ds, batch_size=TB, verbose=False)
        images_per_epoch = n
    else:
        trainers = {}
        for arm in arms:
            cfg, trainers[arm] = make_trainer(B)
        images_per_epoch = nb * B
        if "A" in arms:
            tr_a = trainers["A"]
            if a.what == "rpo":
                def epoch_a(e):
                    for batch in _order(n, B, e):
                        tr_a.forward_backward({"img": [images[i] for i in batch],
                                               "label": torch.tensor([labels[i] for i in batch])})
            else:
                from rpo_amd.input_pipeline import InputConfig, build_transform
                tf = build_transform(InputConfig(), True, dev, B)

                def epoch_a(e):
                    for batch in _order(n, B, e):
                        tr_a.forward_backward({"img": tf([images[i] for i in batch]),
                                               "label": torch.tensor([labels[i] for i in batch])})
            runs["A"] = epoch_a
        if "B" in arms:
            from rpo_amd.input_pipeline import DeviceImageSet
            ds = DeviceImageSet(images, labels, dev)
            tr_b = trainers["B"]
            runs["B"] = lambda _: tr_b.run_epoch(ds)
        if "C" in arms:
            tr_c = trainers["C"]
            fl = [torch.from_numpy(synth.images(cfg, B, seed=1234 + 31 * i)).to(dev) for i in range(4)]
            lb = [torch.tensor(labels[i * B:(i + 1) * B], device=dev) for i in range(4)]
            if a.what == "rpo":
                def epoch_c(e):                  # (the next batch is named across the epoch boundary too, as bench.py does)
                    for k in range(e * nb, (e + 1) * nb):
                        tr_c.step_async(fl[k % 4], lb[k % 4], next_image=fl[(k + 1) % 4])
            else:
                def epoch_c(_):
                    for t in range(nb):
                        tr_c.step_async(fl[t % 4], lb[t % 4])
            runs["C"] = epoch_c
        if "D" in arms:
            tr_d = trainers["D"]
            fd = [torch.from_numpy(synth.images(cfg, B, seed=1234 + 31 * i)).to(dev) for i in range(4)]
            ld = [torch.tensor(labels[i * B:(i + 1) * B], device=dev) for i in range(4)]
            kw = (lambda k: {"next_image": fd[(k + 1) % 4]}) if a.what == "rpo" else (lambda k: {})

            def epoch_d(e):
                for k in range(e * nb, (e + 1) * nb):
                    tr_d.step_async(fd[k % 4], ld[k % 4], **kw(k))
                    tr_d._loop_advance()
            runs["D"] = epoch_d

    times = {k: [] for k in runs}
    with torch.cuda.device(0):
        for e in range(a.warmup):
            for k, fn in runs.items():
                _timed(lambda: fn(e), torch)
        for e in range(a.repeats):                   # the arms of one process alternate, epoch by epoch
            for k, fn in runs.items():
                times[k].append(_timed(lambda: fn(a.warmup + e), torch))
    here = os.path.abspath(a.root) == os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {"metric": "epoch_bench", "what": a.what, "device": torch.cuda.get_device_name(0), "batch": B if a.what != "test" else 100,
           "images_per_epoch": images_per_epoch, "tree": "this tree" if here else "another checkout",
           "epoch_ms": {k: [round(1e3 * t, 3) for t in v] for k, v in times.items()}}
    print(json.dumps(out))


def merge(paths):
    tables = {}
    for p in paths:
        for line in open(p):
            line = line.strip()
            if not line.startswith("{"):
                continue
            r = json.loads(line)
            t = tables.setdefault(r["what"], {"images_per_epoch": r["images_per_epoch"], "batch": r["batch"], "device": r["device"],
                                              "epoch_ms": {}, "arm_A_tree": None})
            for arm, v in r["epoch_ms"].items():
                t["epoch_ms"].setdefault(arm, []).extend(v)
                if arm == "A":
                    t["arm_A_tree"] = r["tree"]
    out = {"metric": "epoch_bench", "tables": {}}
    for what, t in tables.items():
        row = {"images_per_epoch": t["images_per_epoch"], "batch": t["batch"], "device": t["device"], "arm_A_tree": t["arm_A_tree"]}
        for arm, v in sorted(t["epoch_ms"].items()):
            med = statistics.median(v)
            row[arm] = {"repeats": len(v), "median_ms": round(med, 3), "min_ms": min(v), "max_ms": max(v),
                        "images_s_median": round(t["images_per_epoch"] / (med * 1e-3), 1),
                        "images_s_min": round(t["images_per_epoch"] / (max(v) * 1e-3), 1),
                        "images_s_max": round(t["images_per_epoch"] / (min(v) * 1e-3), 1)}
        if "A" in row and "B" in row:
            ra, rb = row["A"], row["B"]
            row["B_over_A"] = round(rb["images_s_median"] / ra["images_s_median"], 3)
            spread = ra["images_s_max"] - ra["images_s_min"]
            row["A_spread_images_s"] = round(spread, 1)
            row["B_beats_A_by_more_than_A_spread"] = bool(rb["images_s_median"] - ra["images_s_median"] > spread)
        for ceil in ("C", "D"):
            if "B" in row and ceil in row:
                row[f"B_over_{ceil}"] = round(row["B"]["images_s_median"] / row[ceil]["images_s_median"], 3)
        out["tables"][what] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
