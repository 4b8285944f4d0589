#!/usr/bin/env python3
"""Linear-probe (rpo_amd/lp.py) throughput on one MI355X; prints ONE JSON line.

  step_img_s   LP training step (plain ViT-B/16 image tower + LP head + SGD), graph-replayed, B = 32, for C = 19 (Oxford-Pets
               base) and C = 1000 (ImageNet-sized class set), in the f32 and bf16 modes
  head_sgd_us  device time of rpo_lp_head_fwd_bwd + rpo_sgd_step alone (HIP events over repeated launches), and its share of
               the step's device time
  eval_img_s   model_inference at the yaml's test batch of 100 (C = 19)

Synthetic full-size CLIP weights (rpo_amd/synth.py); the numbers are throughput, not accuracy.
Usage: python tools/bench_lp.py [--steps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpo_amd import ops, synth  # noqa: E402
from rpo_amd.config import vit_b16  # noqa: E402
from rpo_amd.lp import LP  # noqa: E402


def _tokens(cfg, n_cls: int) -> np.ndarray:
    if n_cls == 19:
        return synth.oxford_pets_base_tokens()
    rng = np.random.default_rng(5)
    return synth.synthetic_tokens(cfg, rng.integers(6, 12, n_cls).tolist())


def _time(fn, n: int) -> float:
    """Mean device ms per call of fn over n calls (HIP events on the current stream)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def bench_step(act, n_cls: int, B: int, steps: int, warmup: int) -> dict:
    cfg = vit_b16(K=1, n_cls=n_cls)
    toks = _tokens(cfg, n_cls)
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist())
    tr = LP(sd, toks, None, "cuda:0", act, batch_size=B, num_batches=10 ** 9, use_graph=True, max_batch=100)
    eng = tr.engine
    img = torch.from_numpy(synth.images(cfg, B)).cuda()
    lab = torch.from_numpy(synth.labels(cfg, B) % n_cls).cuda()
    for _ in range(warmup):
        tr.step_async(img, lab)
    torch.cuda.synchronize()
    step_ms = _time(lambda: tr.step_async(img, lab), steps)
    loss = float(eng.loss.item())
    oc = tr.optim_cfg

    def head_sgd():
        ops.lp_head_fwd_bwd(eng.img_cls_f[:B], eng.lp_w, eng.lp_b, eng.lp_text_f_n, lab, eng.logit_scale_exp, eng.lp_z[:B],
                            eng.logits[:B], eng.loss, eng.lp_gw, eng.lp_gb, eng.lp_ws)
        ops.sgd_step(eng.lp_params, eng.lp_grads, eng.lp_moms, tr.lr, oc.momentum, oc.weight_decay, 1.0, False)
    g = torch.cuda.CUDAGraph()                        # launch cost as in the step: the pair replayed from a graph
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        head_sgd()
    for _ in range(warmup):
        g.replay()
    hs_ms = _time(g.replay, 50)
    out = dict(step_img_s=round(B / (step_ms * 1e-3), 1), step_ms=round(step_ms, 3), head_sgd_us=round(hs_ms * 1e3, 1),
               head_sgd_share=round(hs_ms / step_ms, 4), loss=round(loss, 4), finite=bool(np.isfinite(loss)))
    ev = None
    if n_cls == 19:
        ev_img = torch.from_numpy(synth.images(cfg, 100)).cuda()
        tr.model_inference(ev_img)
        torch.cuda.synchronize()
        ev = 100 / (_time(lambda: tr.model_inference(ev_img), max(3, steps // 4)) * 1e-3)
    del tr, eng
    torch.cuda.empty_cache()
    return out, ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lp needs cuda:0"
    torch.cuda.set_device(0)
    res = {"metric": "lp_step", "batch": a.batch, "steps": a.steps, "device": torch.cuda.get_device_name(0), "modes": {}}
    for name, act in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        for n_cls in (19, 1000):
            r, ev = bench_step(act, n_cls, a.batch, a.steps, a.warmup)
            res["modes"][f"{name}_c{n_cls}"] = r
            if ev is not None:
                res["modes"][f"{name}_c{n_cls}"]["eval_b100_img_s"] = round(ev, 1)
    res["head_sgd_share_max_bf16"] = max(res["modes"][f"bf16_c{c}"]["head_sgd_share"] for c in (19, 1000))
    res["target_share"] = 0.05
    print(json.dumps(res))


if __name__ == "__main__":
    main()
