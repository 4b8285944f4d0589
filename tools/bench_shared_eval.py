#!/usr/bin/env python3
"""Evaluation of all RPOMulti members per frozen image pass against the per-member loop it replaces;
prints ONE JSON line.

Workload: ViT-B/16, 12 + 12 layers, K = 24, 19 classes, synthetic weights, --images synthetic images resident in HBM
(`DeviceImageSet`), chunks of --batch images, per S in --S.  Three arms alternate repeat by repeat in one process:
  (a) per_member   S calls of `test(image_set, member=s)`: the existing path -- the whole image tower once per member
  (b) live         `test_all(image_set)`: one frozen pass per chunk, then one prompt-row pass for all S members
  (c) cached       `test_all(image_set, frozen=FrozenImageKV.build(...))`: no image pass at all
Every arm is run once before timing (graph captures, kernel attributes), then --repeats times; a repeat is a host clock
around one whole pass over the set, which ends in the evaluator's read-back (a device synchronise).  The engine is built
with max_batch >= --batch (members' training batch ceil(batch / S)), so all arms run the same chunks.
Condition (`live_beats_per_member`): the SLOWEST (b) repeat is below the FASTEST (a) repeat.

--trace S: only arm (b) at S, three passes (run under `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _stat(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, nargs="+", default=[1, 3, 8])
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", type=int)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from rpo_amd import synth
    from rpo_amd.config import vit_b16
    from rpo_amd.frozen_kv import FrozenImageKV
    from rpo_amd.input_pipeline import DeviceImageSet
    from rpo_amd.multi import RPOMulti
    assert torch.cuda.is_available(), "bench_shared_eval needs cuda:0"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
    cfg = vit_b16(K=24, n_cls=19)
    toks = synth.default_tokens(cfg)
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
    rng = np.random.default_rng(0)
    size = cfg.image_size
    images = [rng.integers(0, 256, (size, size, 3), dtype=np.uint8) for _ in range(a.images)]
    labels = rng.integers(0, cfg.n_cls, a.images).tolist()
    ds = DeviceImageSet(images, labels, dev)
    del images

    def trainer(S):
        B = -(-a.batch // S)                                        # S * B >= batch: the engine takes chunks of `batch`
        return RPOMulti(cfg, sd, toks, n_runs=S, batch_size=B, prompts=[synth.prompts(cfg, sd, seed=7 + s) for s in range(S)],
                        device=dev, act_dtype=DT[a.dtype], num_batches=10 ** 9)

    if a.trace:
        tr = trainer(a.trace)
        for _ in range(3):
            tr.test_all(ds, a.batch, verbose=False)
        torch.cuda.synchronize()
        return
    out = {"metric": "shared_eval_bench", "device": torch.cuda.get_device_name(0), "model": "ViT-B/16", "layers": "12 + 12",
           "K": 24, "n_cls": 19, "dtype": a.dtype, "images": a.images, "batch": a.batch, "repeats": a.repeats,
           "timing": "host clock around one pass over the resident set, ending in the evaluator's read-back; arms alternate "
                     "per repeat; every arm run once before timing",
           "S": {}}
    for S in a.S:
        tr = trainer(S)
        t_build = _timed(lambda: FrozenImageKV.build(tr.engine, ds, a.batch), torch)          # (also the warm-up of the pass)
        cache = FrozenImageKV.build(tr.engine, ds, a.batch)
        arms = {
            "per_member": lambda: [tr.test(ds, member=s, batch_size=a.batch, verbose=False) for s in range(S)],
            "live": lambda: tr.test_all(ds, a.batch, verbose=False),
            "cached": lambda: tr.test_all(ds, a.batch, frozen=cache, verbose=False),
        }
        res = {k: fn() for k, fn in arms.items()}                  # warm-up of every arm and shape
        ts = {k: [] for k in arms}
        for _ in range(a.repeats):
            for k, fn in arms.items():
                ts[k].append(_timed(fn, torch))
        agree = [[r["correct"] for r in res[k]] for k in arms]
        ta, tb, tc = ts["per_member"], ts["live"], ts["cached"]
        out["S"][str(S)] = {
            "per_member_ms": _stat(ta), "live_ms": _stat(tb), "cached_ms": _stat(tc),
            "live_over_per_member": round(statistics.median(tb) / statistics.median(ta), 4),
            "cached_over_per_member": round(statistics.median(tc) / statistics.median(ta), 4),
            "live_beats_per_member": bool(max(tb) < min(ta)),
            "cached_beats_per_member": bool(max(tc) < min(ta)),
            "cache_build_ms_first_call": round(t_build, 3), "cache_bytes": int(cache.nbytes()),
            "engine_max_batch": int(tr.engine.max_batch),
            "correct_per_member": {"per_member": agree[0], "live": agree[1], "cached": agree[2]},
        }
        del tr, cache, arms
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
