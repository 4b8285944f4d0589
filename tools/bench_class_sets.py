#!/usr/bin/env python3
"""Measurements of DESIGN.md section 9m on one MI355X, one process: writes profiles/classset_bench.json.

  (a) `Engine.encode_text` at 1000 classes x 7 and x 80 templates (7 000 / 80 000 prompts of 8-20 tokens, full ViT-B/16 text
      tower, bf16): the device gather (rpo_text_embed) against RPO_TEXT_EMBED_HOST=1.
  (b) base-to-new on 19 + 18 classes, 1000 synthetic resident images per split, full ViT-B/16, K = 24, bf16, a trainer of
      batch 32 (so `test` runs chunks of 32):
      `base_to_new` on ONE trainer (the class-set build included) against `test(base)` + building a second trainer on the
      new tokens + its `test(new)`; and `hbm_bytes()` of the class set against the second engine.

Arms alternate, every arm runs once before timing, five repeats each, median with min-max; host clocks around a device
sync.  (c), `bench.py` against the parent commit, is two checkouts alternating and is not run from here."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(arms, repeats, torch):
    """arms: name -> callable.  Every arm once untimed, then `repeats` alternating rounds: name -> {median, min, max, all} ms."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            t[k].append(timed(fn, torch))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), all_ms=[round(x, 3) for x in v])
            for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--images", type=int, default=1000, help="(b): images per split")
    ap.add_argument("--skip", default="", help="comma list of a, b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classset_bench.json"))
    a = ap.parse_args()
    import torch
    from rpo_amd import synth
    from rpo_amd.config import vit_b16
    from rpo_amd.engine import Engine
    from rpo_amd.evaluator import base_to_new
    from rpo_amd.input_pipeline import DeviceImageSet
    from rpo_amd.trainer import RPO
    assert torch.cuda.is_available(), "bench_class_sets.py needs a GPU"
    dev = torch.device("cuda:0")
    skip = set(a.skip.split(","))
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, repeats=a.repeats)
    cfg = vit_b16(K=24)
    sd = synth.clip_state_dict(cfg, seed=0)
    base_t = synth.oxford_pets_base_tokens()

    if "a" not in skip:
        eng = Engine(cfg, sd, base_t, dev, torch.bfloat16, max_batch=4)
        res["encode_text"] = {}
        for T in (7, 80):
            P = 1000 * T
            lens = np.random.default_rng(T).integers(8, 21, P).tolist()
            toks = synth.synthetic_tokens(cfg, lens, seed=T)

            def run(host):
                if host:
                    os.environ["RPO_TEXT_EMBED_HOST"] = "1"
                else:
                    os.environ.pop("RPO_TEXT_EMBED_HOST", None)
                eng.encode_text(toks)
                os.environ.pop("RPO_TEXT_EMBED_HOST", None)
            r = alternate({"device": lambda: run(False), "host": lambda: run(True)}, a.repeats, torch)
            r["device_not_above_host"] = r["device"]["median_ms"] <= r["host"]["median_ms"]
            res["encode_text"][f"1000x{T}"] = r
            print(f"(a) {P} prompts: device {r['device']['median_ms']:.1f} ms [{r['device']['min_ms']:.1f}, "
                  f"{r['device']['max_ms']:.1f}], host {r['host']['median_ms']:.1f} ms [{r['host']['min_ms']:.1f}, "
                  f"{r['host']['max_ms']:.1f}]", flush=True)
        del eng
        torch.cuda.empty_cache()

    if "b" not in skip:
        gold = os.path.join(ROOT, "tests", "golden", "ref_classset_rpo.npz")
        new_t = np.load(gold)["tokens"] if os.path.exists(gold) else synth.synthetic_tokens(cfg, [9 + c % 5 for c in range(18)])
        rng = np.random.default_rng(5)

        def split(n_cls):
            imgs = [rng.integers(0, 256, (224, 224, 3), dtype=np.uint8) for _ in range(a.images)]
            return DeviceImageSet(imgs, [i % n_cls for i in range(a.images)], dev)
        base_set, new_set = split(19), split(new_t.shape[0])
        prompts = synth.prompts(cfg, sd, seed=7)
        tr = RPO(cfg, sd, base_t, None, dev, torch.bfloat16, batch_size=32, num_batches=1, prompts=prompts)
        sizes = {}

        def class_set_route():
            out = base_to_new(tr, base_set, new_set, new_t, batch_size=100, verbose=False)      # (builds the class set)
            class_set_route.last = out

        def second_trainer_route():
            b = tr.test(base_set, batch_size=100, verbose=False)
            cfg2 = dataclasses.replace(cfg, n_cls=int(new_t.shape[0]))
            tr2 = RPO(cfg2, sd, new_t, None, dev, torch.bfloat16, batch_size=32, num_batches=1, prompts=prompts)
            n = tr2.test(new_set, batch_size=100, verbose=False)
            torch.cuda.synchronize()
            sizes["second_engine_hbm_bytes"] = tr2.engine.hbm_bytes()
            second_trainer_route.last = dict(base=b["accuracy"], new=n["accuracy"])
            del tr2
            torch.cuda.empty_cache()
        r = alternate({"class_set": class_set_route, "second_trainer": second_trainer_route}, a.repeats, torch)
        cs = tr.class_set(new_t)
        tr.test(new_set, batch_size=100, verbose=False, classes=cs)
        sizes["class_set_hbm_bytes"] = cs.hbm_bytes()
        sizes["first_engine_hbm_bytes"] = tr.engine.hbm_bytes()
        r.update(sizes)
        r["class_set_not_slower"] = r["class_set"]["median_ms"] <= r["second_trainer"]["median_ms"]
        r["accuracies"] = dict(class_set={k: class_set_route.last[k] for k in ("base", "new", "H")},
                               second_trainer=second_trainer_route.last)
        res["base_to_new"] = r
        print(f"(b) base-to-new, {a.images} images per split: class set {r['class_set']['median_ms']:.1f} ms "
              f"[{r['class_set']['min_ms']:.1f}, {r['class_set']['max_ms']:.1f}], second trainer "
              f"{r['second_trainer']['median_ms']:.1f} ms [{r['second_trainer']['min_ms']:.1f}, {r['second_trainer']['max_ms']:.1f}]; "
              f"class set {sizes['class_set_hbm_bytes'] / 1e6:.1f} MB, second engine {sizes['second_engine_hbm_bytes'] / 1e6:.1f} MB",
              flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k in ("device", "repeats")}))


if __name__ == "__main__":
    main()
