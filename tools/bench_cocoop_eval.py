#!/usr/bin/env python3
"""Measurements of DESIGN.md section 9p on one MI355X, one process: writes profiles/cocoop_eval_bench.json.

CoCoOp inference over 100 images (the reference's TEST.BATCH_SIZE), full ViT-B/16, bf16, a trainer of batch 1 (the
reference's training batch), on two class sets -- the 19 Oxford-Pets base classes (`synth.coop_tokens(.., 4)` of the ids in
rpo_amd/data/) and 100 synthetic classes of 8-29 tokens:

  dense      `model(image)`: today's path, the image tower and B * n_cls * Lmax text rows per chunk of the training batch
  prefix@k   `model_inference(image, classes=ccs)` on the SAME tokens with images_per_pass = k: the image tower in the same
             chunks, then k * (P + n_cls * S) text rows per pass
  image      the plain image tower alone, in the same chunks (what both paths share)

Arms alternate, every arm runs once before timing, `--repeats` rounds, median with min-max; host clock around a device
sync.  The rows per pass of both paths are recorded next to the times."""
import argparse
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--sweep", default="1,4,16,50,100", help="images_per_pass values")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cocoop_eval_bench.json"))
    a = ap.parse_args()
    import torch
    from rpo_amd import synth
    from rpo_amd.config import vit_b16
    from rpo_amd.coop import CoCoOp
    assert torch.cuda.is_available(), "bench_cocoop_eval.py needs a GPU"
    dev = torch.device("cuda:0")
    sweep = [int(s) for s in a.sweep.split(",")]
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, repeats=a.repeats, images=a.images,
               model="ViT-B/16", act="bf16", n_ctx=4, sets={})
    n_ctx = 4
    sets = {"oxford_pets_base_19": lambda cfg: synth.coop_tokens(synth.oxford_pets_base_tokens(), n_ctx),
            "synthetic_100": lambda cfg: synth.coop_tokens(
                synth.synthetic_tokens(cfg, [4 + (7 * c) % 22 for c in range(100)], seed=17), n_ctx)}
    for name, make in sets.items():
        n_cls = 19 if name.startswith("oxford") else 100
        cfg = vit_b16(K=1, n_cls=n_cls)
        toks = make(cfg)
        sd = synth.clip_state_dict(cfg, seed=0)
        torch.manual_seed(0)
        tr = CoCoOp(sd, toks, n_ctx=n_ctx, device=dev, act_dtype=torch.bfloat16, batch_size=1, cfg=cfg)
        eng = tr.engine
        image = torch.from_numpy(synth.images(cfg, a.images, seed=3)).to(dev)
        ccs = {k: tr.conditional_class_set(toks, images_per_pass=k) for k in sweep}
        default = tr.conditional_class_set(toks)

        def image_only():
            with torch.cuda.device(dev):
                for b0 in range(0, a.images, eng.max_batch):
                    eng._plain_image_features(image[b0:b0 + eng.max_batch])
        arms = {"dense": lambda: tr.model_inference(image), "image": image_only}
        for k in sweep:
            arms[f"prefix@{k}"] = (lambda c: lambda: tr.model_inference(image, classes=c))(ccs[k])
        arms["prefix@default"] = lambda: tr.model_inference(image, classes=default)
        r = alternate(arms, a.repeats, torch)
        one = ccs[sweep[0]]
        worst = float((tr.model_inference(image, classes=one) - tr.model_inference(image)).abs().max())
        rows = dict(P=one.P, S=one.S, Lmax=one.Lmax, n_cls=one.n,
                    dense_rows_per_image=one.n * one.Lmax, prefix_rows_per_image=one.P + one.n * one.S,
                    row_ratio=one.n * one.Lmax / (one.P + one.n * one.S),
                    dense_rows_per_pass=eng.coop_replicas * one.n * one.Lmax,
                    prefix_rows_per_pass={str(k): ccs[k].rows_per_pass(min(k, a.images)) for k in sweep},
                    classes_per_pass={str(k): ccs[k].classes_per_pass for k in sweep},
                    default_images_per_pass=default.images_per_pass, default_classes_per_pass=default.classes_per_pass,
                    default_rows_per_pass=default.rows_per_pass(min(default.images_per_pass, a.images)),
                    row_budget=default.ROW_BUDGET)
        img = r["image"]["median_ms"]
        ratios = {k: dict(end_to_end=r["dense"]["median_ms"] / v["median_ms"],
                          text_side=(r["dense"]["median_ms"] - img) / max(v["median_ms"] - img, 1e-9))
                  for k, v in r.items() if k.startswith("prefix@")}
        res["sets"][name] = dict(times=r, rows=rows, dense_over_prefix=ratios, worst_logits_diff_vs_dense=worst)
        print(f"[{name}] rows per image: dense {rows['dense_rows_per_image']}, prefix {rows['prefix_rows_per_image']} "
              f"(ratio {rows['row_ratio']:.2f}); dense {r['dense']['median_ms']:.1f} ms, image tower {img:.1f} ms; " +
              "; ".join(f"{k} {r[k]['median_ms']:.1f} ms (x{ratios[k]['end_to_end']:.2f}, text side x{ratios[k]['text_side']:.2f})"
                        for k in ratios) + f"; worst |logits diff| {worst:.3e}", flush=True)
        del tr, eng, ccs, default, arms
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k in ("device", "repeats", "images")}))


if __name__ == "__main__":
    main()
