#!/usr/bin/env python3
"""Time to build the prompt-ensemble classifier (rpo_amd.zeroshot.ZeroshotCLIP2); prints ONE JSON line
(--out: also written to a file).

Workload: ViT-B/16's text tower (12 layers, d_t = 512), bf16, synthetic weights; the image tower plays no part and is
built 2 layers deep.  Configurations: n_cls = 1000 with T = 7 and T = 80 templates (token lengths 8 .. 20, SOT .. EOT, as
ImageNet's class-name prompts under a template have) and the 19 Oxford-Pets base classes with T = 8 (lengths 10 .. 16).

Arms, on the same code base:
  ensemble  `encode_text` over all T * n_cls prompts (host embedding gather and upload included) + the two ensemble
            kernels: what ZeroshotCLIP2.__init__ runs after the engine is built.  hipEvent timing, arms alternating
            repeat by repeat after --warmup untimed rounds.  Also at 256 / 1024 / 4096 prompts per pass (3 repeats each).
  single    one `cache_text_kv` + EOT feature tail of an engine built on ONE template's n_cls prompts -- the only route
            to text features before `encode_text`; the ensemble by that route costs T of them (reported: T x the median)
            plus T engine builds and a host-side combine that are NOT in the figure.
  cpu       the reference's loop restated with the float32 CPU oracle (oracle/rpo_oracle.py): per template, the whole
            77-position context of every class through the text tower, normalise, add; host clock.  n_cls = 1000 runs
            ONE template and reports T x that (`extrapolated`), n_cls = 19 runs all 8.
No condition is evaluated: the tool reports times."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _ms(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def _event_ms(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _cpu_template(sd_t, tokens, torch, oracle):
    """Normalised text features [n, e] of one template's prompts, float32 on the CPU (clip/model.py:344-356)."""
    tok = torch.from_numpy(tokens)
    x = (sd_t["token_embedding.weight"][tok] + sd_t["positional_embedding"]).permute(1, 0, 2)
    L = x.shape[0]
    causal = torch.full((L, L), float("-inf")).triu_(1)
    for blk in oracle._blocks(sd_t, "transformer.resblocks."):
        x = oracle.res_block(x, blk, sd_t["ln_final.weight"].shape[0] // oracle.HEAD_DIM, causal)
    x = oracle.layer_norm(x.permute(1, 0, 2), sd_t["ln_final.weight"], sd_t["ln_final.bias"])
    f = x[torch.arange(x.shape[0]), tok.argmax(dim=-1)] @ sd_t["text_projection"]
    return f / f.norm(dim=-1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default="19x8,1000x7,1000x80", help="comma-separated n_cls x T")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from oracle import rpo_oracle as oracle
    from rpo_amd import ops, synth
    from rpo_amd.config import vit_b16
    from rpo_amd.zeroshot import ZeroshotCLIP
    assert torch.cuda.is_available(), "bench_ensemble needs cuda:0"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    act = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    out = {"metric": "ensemble_bench", "device": torch.cuda.get_device_name(0), "host": os.uname().nodename,
           "model": "ViT-B/16 text tower (12 layers, d_t 512, e 512); image tower 2 layers, unused", "dtype": a.dtype,
           "warmup": a.warmup, "repeats": a.repeats,
           "timing": "hipEvent pairs around each arm, arms alternating per repeat; cpu arm: host clock", "configs": {}}
    sd = None
    for spec in a.configs.split(","):
        n, T = (int(v) for v in spec.split("x"))
        cfg = vit_b16(layers_v=2, K=1, n_cls=n)
        if sd is None:
            sd = synth.clip_state_dict(cfg, seed=0)                      # the whole token table: the ids are random
        rng = np.random.default_rng(5 + n + T)
        lo, hi = (10, 16) if n == 19 else (8, 20)
        tokens = synth.synthetic_tokens(cfg, rng.integers(lo, hi + 1, size=T * n).tolist(), seed=99 + T).reshape(T, n, 77)
        m = ZeroshotCLIP(sd, tokens[0], dev, act, max_batch=4, cfg=cfg)
        eng = m.engine
        flat = tokens.reshape(T * n, 77)
        acc = torch.empty(n, cfg.embed, dtype=torch.float32, device=dev)
        single_f = torch.empty(n, cfg.embed, dtype=torch.float32, device=dev)

        def ensemble(chunk=None):
            f = eng.encode_text(flat, chunk)
            ops.text_ensemble_accumulate(f, n, acc, first=True)
            ops.text_ensemble_finish(acc, T)

        def kernels_only(f):
            ops.text_ensemble_accumulate(f, n, acc, first=True)
            ops.text_ensemble_finish(acc, T)

        def single():
            eng.cache_text_kv()
            eng._text_eot_features(eng.text_x_final, eng.len_i32, n, eng.Lmax, single_f)

        for _ in range(a.warmup):
            ensemble(); single()
        t_ens, t_single = [], []
        for _ in range(a.repeats):
            t_ens.append(_event_ms(ensemble, torch))
            t_single.append(_event_ms(single, torch))
        feats = eng.encode_text(flat)
        t_kern = [_event_ms(lambda: kernels_only(feats), torch) for _ in range(a.repeats + 1)][1:]
        rec = {"n_cls": n, "T": T, "prompts": T * n, "token_lengths": [lo, hi], "chunk": eng.TEXT_CHUNK,
               "ensemble_ms": _ms(t_ens), "ensemble_kernels_only_ms": _ms(t_kern), "single_template_pass_ms": _ms(t_single),
               "T_x_single_template_median_ms": round(T * statistics.median(t_single), 3),
               "ensemble_median_over_T_x_single_median": round(statistics.median(t_ens) / (T * statistics.median(t_single)), 4)}
        if T * n > 256:                       # what the chunk costs: the same arm at other prompts-per-pass values
            sweep = {}
            for c in (256, 1024, 4096):
                ensemble(c)
                sweep[str(c)] = _ms([_event_ms(lambda: ensemble(c), torch) for _ in range(3)])
            rec["ensemble_ms_by_chunk"] = sweep
        if not a.no_cpu:
            sd_t = {k: torch.from_numpy(np.ascontiguousarray(v)).float() for k, v in sd.items() if not k.startswith("visual.")}
            t_run = T if n == 19 else 1
            with torch.no_grad():
                t0 = time.perf_counter()
                mean = 0
                for t in range(t_run):
                    mean = mean + _cpu_template(sd_t, tokens[t], torch, oracle)
                mean = mean / t_run
                mean = mean / mean.norm(dim=-1, keepdim=True)
                dt = 1e3 * (time.perf_counter() - t0)
            rec["cpu_loop_ms"] = round(dt * T / t_run, 1)
            rec["cpu_loop_templates_run"] = t_run
            rec["cpu_loop_extrapolated"] = t_run != T
            rec["cpu_threads"] = torch.get_num_threads()
            if t_run == T:                                                # the arms compute the same thing
                rec["ensemble_vs_cpu_max_abs"] = float((acc.cpu() - mean).abs().max())
        out["configs"][spec] = rec
        del m, eng, feats
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
