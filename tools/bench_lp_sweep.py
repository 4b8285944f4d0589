#!/usr/bin/env python3
"""`LPSweep` (rpo_amd/lp_sweep.py) against S standalone `LP` steps, on one MI355X; prints ONE JSON line.

  sweep     ViT-B/16, bf16, B in {32, 1}, C in {19, 1000}, S in {1, 4, 16}: ms per graph-replayed `LPSweep` step beside
            S x the ms of a graph-replayed standalone `LP` step timed in the same process.  Host clock around `--steps` steps
            after `--warmup` steps; the median of `--repeats` repeats with min .. max.  The one bound: at S = 4 and S = 16
            the sweep is faster than S standalone steps one after the other (`bound_ok`).
  existing  rpo_lp_head_fwd_bwd of this tree's library against `--parent-lib` (the parent commit's librpo_hip.so), one call
            captured into a HIP graph each, replayed alternately: us per call, median with min .. max, for both.

Synthetic full-size CLIP weights (rpo_amd/synth.py); the numbers are time, not accuracy.
Usage: python tools/bench_lp_sweep.py [--steps 200] [--warmup 20] [--repeats 5] [--parent-lib PATH] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rpo_amd import _lib, ops, synth  # noqa: E402
from rpo_amd.config import vit_b16  # noqa: E402
from rpo_amd.lp import LP, lp_optim_config  # noqa: E402
from rpo_amd.lp_sweep import LPSweep  # noqa: E402


def _tokens(cfg, n_cls: int) -> np.ndarray:
    if n_cls == 19:
        return synth.oxford_pets_base_tokens()
    rng = np.random.default_rng(5)
    return synth.synthetic_tokens(cfg, rng.integers(6, 12, n_cls).tolist())


def _stat(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def _ms_per_call(fn, n: int) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def _members(S: int):
    """The points of a learning-rate x weight-decay grid around the yaml's recipe."""
    import dataclasses
    base = lp_optim_config()
    return [dict(optim=dataclasses.replace(base, lr=base.lr * (0.5 + 0.25 * (s % 4)), weight_decay=5e-4 * (s // 4)))
            for s in range(S)]


def bench_sweep(n_cls: int, B: int, sizes, steps: int, warmup: int, repeats: int) -> dict:
    cfg = vit_b16(K=1, n_cls=n_cls)
    toks = _tokens(cfg, n_cls)
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist())
    img = torch.from_numpy(synth.images(cfg, B)).cuda()
    lab = torch.from_numpy(synth.labels(cfg, B) % n_cls).cuda()
    trainers = {0: LP(sd, toks, None, "cuda:0", torch.bfloat16, batch_size=B, num_batches=10 ** 9, use_graph=True, max_batch=100)}
    for S in sizes:
        trainers[S] = LPSweep(sd, toks, _members(S), "cuda:0", torch.bfloat16, batch_size=B, num_batches=10 ** 9,
                              use_graph=True, max_batch=100)
    for tr in trainers.values():
        for _ in range(warmup):
            tr.step_async(img, lab)
    times = {k: [] for k in trainers}
    for _ in range(repeats):                                   # alternating: every repeat times every trainer once
        for k, tr in trainers.items():
            times[k].append(_ms_per_call(lambda: tr.step_async(img, lab), steps))
    solo = _stat(times[0])
    out = {"standalone_ms": solo}
    for S in sizes:
        st = _stat(times[S])
        loss = trainers[S].engine.lps_loss.tolist()
        out[f"S{S}"] = dict(sweep_ms=st, standalone_x_S_ms=round(S * solo["median"], 4),
                            speedup=round(S * solo["median"] / st["median"], 2),
                            vs_one_step=round(st["median"] / solo["median"], 3), finite=bool(np.isfinite(loss).all()),
                            captures=trainers[S].captures)
    del trainers
    torch.cuda.empty_cache()
    return out


def bench_existing(parent_lib: str, steps: int, warmup: int, repeats: int) -> dict:
    """rpo_lp_head_fwd_bwd, this tree's library and the parent's: one captured call each, replayed alternately."""
    new = _lib.load()
    old = ctypes.CDLL(parent_lib)
    restype, argtypes = _lib.SIGNATURES["rpo_lp_head_fwd_bwd"]
    old.rpo_lp_head_fwd_bwd.restype, old.rpo_lp_head_fwd_bwd.argtypes = restype, argtypes
    out = {}
    e = 512
    for B, C in ((32, 19), (32, 1000), (1, 19)):
        g = torch.Generator().manual_seed(B + C)
        x = torch.randn(B, e, generator=g).cuda()
        w = (torch.eye(e) + 0.01 * torch.randn(e, e, generator=g)).cuda()
        bias, t = torch.zeros(e).cuda(), torch.nn.functional.normalize(torch.randn(C, e, generator=g), dim=1).cuda()
        lab = torch.randint(0, C, (B,), generator=g).cuda()
        graphs, outs = {}, {}
        for name, lib in (("parent", old), ("this", new)):
            z, logits, loss = torch.empty(B, e).cuda(), torch.empty(B, C).cuda(), torch.empty(1).cuda()
            gr, ws = torch.empty(e * e + e).cuda(), torch.empty(ops.lp_head_workspace_floats(B, C, e)).cuda()

            def call(lib=lib, z=z, logits=logits, loss=loss, gr=gr, ws=ws):
                rc = lib.rpo_lp_head_fwd_bwd(x.data_ptr(), w.data_ptr(), bias.data_ptr(), t.data_ptr(), lab.data_ptr(), 100.0,
                                             z.data_ptr(), logits.data_ptr(), loss.data_ptr(), gr.data_ptr(),
                                             gr.data_ptr() + 4 * e * e, B, C, e, ws.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc
            call()
            torch.cuda.synchronize()
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg, capture_error_mode="thread_local"):
                call()
            graphs[name], outs[name] = cg, (z, logits, loss, gr)
            for _ in range(warmup):
                cg.replay()
        times = {"parent": [], "this": []}
        for _ in range(repeats):
            for name in ("parent", "this"):
                times[name].append(_ms_per_call(graphs[name].replay, steps) * 1e3)
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs["parent"], outs["this"]))
        out[f"B{B}_C{C}"] = dict(parent_us=_stat(times["parent"]), this_us=_stat(times["this"]), same_bits=bool(same))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lp_sweep needs cuda:0"
    torch.cuda.set_device(0)
    sizes = (1, 4, 16)
    res = {"metric": "lp_sweep_step", "mode": "bf16", "backbone": "ViT-B/16", "steps": a.steps, "warmup": a.warmup,
           "repeats": a.repeats, "clock": "host, graph-replayed steps", "device": torch.cuda.get_device_name(0), "sweep": {}}
    for B in (32, 1):
        for n_cls in (19, 1000):
            res["sweep"][f"B{B}_C{n_cls}"] = bench_sweep(n_cls, B, sizes, a.steps, a.warmup, a.repeats)
            print(f"B{B} C{n_cls}: {json.dumps(res['sweep'][f'B{B}_C{n_cls}'])}", file=sys.stderr, flush=True)
    res["bound_ok"] = all(r[f"S{S}"]["sweep_ms"]["median"] < r[f"S{S}"]["standalone_x_S_ms"]
                          for r in res["sweep"].values() for S in (4, 16))
    if a.parent_lib:
        res["existing_entry"] = bench_existing(a.parent_lib, a.steps, a.warmup, a.repeats)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)
    assert res["bound_ok"], "at S = 4 or S = 16 the sweep is not faster than S standalone steps"


if __name__ == "__main__":
    main()
