#!/usr/bin/env python3
"""In-step event figures (us, one column per image block, last block first) of the image tower's ln_2 backward and of the
attention backward behind it, from eager steps of the default bench workload with the text tower running beside.  Reads the
engine's switches from the environment like bench.py.  Usage: python tools/probe_ln2_bwd.py [--batch 32] [--dtype bf16]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench
from rpo_amd import synth
from rpo_amd.config import vit_b16
from rpo_amd.trainer import RPO, OptimConfig
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
a = ap.parse_args()
cfg = vit_b16(); toks = synth.default_tokens(cfg)
sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
dev = torch.device("cuda:0"); torch.cuda.set_device(dev)
tr = RPO(cfg, sd, toks, OptimConfig(), dev, {"bf16": torch.bfloat16, "f16": torch.float16}[a.dtype], batch_size=a.batch,
         num_batches=10**9, prompts=synth.prompts(cfg, sd, seed=7))
img = torch.from_numpy(synth.images(cfg, a.batch)).to(dev); lab = torch.from_numpy(synth.labels(cfg, a.batch)).to(dev)
eng = tr.engine
for _ in range(3): eng.forward_backward(img, lab)
torch.cuda.synchronize()
STEPS = 5
p = bench.KernelProbe(); eng.probe = p
for _ in range(STEPS): eng.forward_backward(img, lab)
eng.probe = None; torch.cuda.synchronize()
for k in ("ln2_bwd", "attn_bwd_proj"):
    ts = np.array([1e3 * s.elapsed_time(e) for s, e in p.ev[k]]).reshape(STEPS, -1)
    print(f"{k:14s} mean/block {ts[1:].mean():5.2f}  sum/step {ts[1:].sum(1).mean():6.1f}  last step: " + " ".join(f"{t:5.1f}" for t in ts[-1]))
