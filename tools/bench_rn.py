#!/usr/bin/env python3
"""The CLIP ResNet image tower (rpo_amd/engine_rn.py) at the reference's test batch of 100: images/s, ms, algorithmic
GFLOP (config.flops_rn_image), achieved TFLOP/s and the fraction of the 2.5 PF bf16 / 157 TF f32 peak, eager and
graph-replayed, for RN50 and RN101 in bf16 / f16 / f32; ZeroshotCLIP.model_inference at B = 100; the conv tile
geometries against rpo_conv2d_plan's choice (RN50, bf16); the CoOp RN50 step at batch 32, n_ctx 16, graph-replayed.

Comparator (never on the product path): torch's own conv stack in the same process on the same inputs -- a functional
restatement of the forward with BatchNorm folded as the engine folds it, every weight a device tensor in the act dtype
(channels_last) made ONCE before timing, F.conv2d -> MIOpen, F.multi_head_attention_forward for the pool.
--trace: one RN50 B = 100 bf16 forward only (run under rocprofv3 --kernel-trace --stats).  Writes profiles/rn_bench.json."""
import json, os, sys
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rpo_amd import synth  # noqa: E402
from rpo_amd.config import flops_coop_step, flops_rn_image, rn_clip, rn_plan  # noqa: E402
from rpo_amd.engine_rn import fold_bn  # noqa: E402
from rpo_amd.zeroshot import ZeroshotCLIP  # noqa: E402

PEAK = {"bf16": 2.5e15, "f16": 2.5e15, "f32": 157e12}
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def row(name, mode, B, ms, fl_per_image, **extra):
    tf = fl_per_image * B / (ms * 1e-3) / 1e12
    r = dict(case=name, dtype=mode, batch=B, ms=round(ms, 4), images_per_s=round(B / (ms * 1e-3), 1),
             gflop=round(fl_per_image * B / 1e9, 2), tflops=round(tf, 2), frac_peak=round(tf * 1e12 / PEAK[mode], 4), **extra)
    print(json.dumps(r), flush=True)
    return r


class TorchRN:
    """The comparator: folded weights uploaded once; forward = F.conv2d / avg_pool2d / relu / attention pool."""

    def __init__(self, sd, cfg, dtype):
        dev = "cuda"
        self.cfg, self.dt = cfg, dtype

        def conv(c, bn):
            wf, b = fold_bn(sd[c], sd[bn + "weight"], sd[bn + "bias"], sd[bn + "running_mean"], sd[bn + "running_var"])
            w = torch.from_numpy(wf.transpose(0, 3, 1, 2).astype(np.float32)).to(dev, dtype)
            return w.contiguous(memory_format=torch.channels_last), torch.from_numpy(b.astype(np.float32)).to(dev, dtype)
        self.stem = [conv(f"visual.conv{i}.weight", f"visual.bn{i}.") for i in (1, 2, 3)]
        self.blocks = []
        for b in rn_plan(cfg):
            p = f"visual.{b['name']}."
            self.blocks.append(dict(b, c1=conv(p + "conv1.weight", p + "bn1."), c2=conv(p + "conv2.weight", p + "bn2."),
                                    c3=conv(p + "conv3.weight", p + "bn3."),
                                    ds=conv(p + "downsample.0.weight", p + "downsample.1.") if b["down"] else None))
        t = lambda k: torch.from_numpy(np.asarray(sd["visual.attnpool." + k])).to(dev, dtype)
        self.ap = {k: t(k) for k in ("positional_embedding", "q_proj.weight", "k_proj.weight", "v_proj.weight",
                                     "c_proj.weight", "c_proj.bias")}
        self.ap["in_bias"] = torch.cat([t("q_proj.bias"), t("k_proj.bias"), t("v_proj.bias")])

    @torch.no_grad()
    def __call__(self, x):
        (w1, b1), (w2, b2), (w3, b3) = self.stem
        x = F.relu(F.conv2d(x, w1, b1, stride=2, padding=1))
        x = F.relu(F.conv2d(x, w2, b2, padding=1))
        x = F.avg_pool2d(F.relu(F.conv2d(x, w3, b3, padding=1)), 2)
        for b in self.blocks:
            out = F.relu(F.conv2d(x, *b["c1"]))
            out = F.relu(F.conv2d(out, *b["c2"], padding=1))
            if b["stride"] > 1:
                out = F.avg_pool2d(out, b["stride"])
            out = F.conv2d(out, *b["c3"])
            idn = x
            if b["ds"] is not None:
                idn = F.conv2d(F.avg_pool2d(x, b["stride"]) if b["stride"] > 1 else x, *b["ds"])
            x = F.relu(out + idn)
        a = self.ap
        B, C, H, W = x.shape
        x = x.reshape(B, C, H * W).permute(2, 0, 1)
        x = torch.cat([x.mean(dim=0, keepdim=True), x], dim=0) + a["positional_embedding"][:, None, :]
        y, _ = F.multi_head_attention_forward(
            query=x[:1], key=x, value=x, embed_dim_to_check=C, num_heads=C // 64, q_proj_weight=a["q_proj.weight"],
            k_proj_weight=a["k_proj.weight"], v_proj_weight=a["v_proj.weight"], in_proj_weight=None,
            in_proj_bias=a["in_bias"], bias_k=None, bias_v=None, add_zero_attn=False, dropout_p=0.0,
            out_proj_weight=a["c_proj.weight"], out_proj_bias=a["c_proj.bias"], use_separate_proj_weight=True,
            training=False, need_weights=False)
        return y[0]


def coop_step(sd, cfg, mode, iters):
    from rpo_amd.coop import CoOp
    from rpo_amd.trainer import OptimConfig
    toks = synth.coop_tokens(synth.oxford_pets_base_tokens(), 16)
    tr = CoOp(sd, toks, 16, OptimConfig(lr=0.002, warmup_epoch=0, lr_scheduler="constant"), "cuda:0", DT[mode],
              batch_size=32, num_batches=10 ** 9, use_graph=True)
    img = torch.from_numpy(synth.images(cfg, 32)).cuda()
    lab = torch.from_numpy(synth.labels(cfg, 32)).cuda()
    ms = timed(lambda: tr.step_async(img, lab), iters)
    # per image: the RN forward + a 32nd of the dense text forward / backward and the head (flops_coop_step with no image)
    fl = flops_rn_image(cfg) + (flops_coop_step(cfg, 0, synth.len_prompts(toks)) + 4.0 * 32 * cfg.n_cls * cfg.embed) / 32
    return row("RN50 CoOp step (graph, B 32, n_ctx 16)", mode, 32, ms, fl)


def main():
    iters = int(os.environ.get("RN_BENCH_ITERS", "20"))
    B, out = 100, []
    cfg50 = rn_clip()
    if "--trace" in sys.argv:
        sd = synth.rn_clip_state_dict(cfg50, seed=0, token_rows=[49406, 49407], check=False)
        m = ZeroshotCLIP(sd, device="cuda:0", act_dtype=torch.bfloat16, max_batch=B)
        img = torch.from_numpy(synth.images(cfg50, B)).cuda()
        m.engine.rn_forward(img)
        torch.cuda.synchronize()
        return
    for cfg in (cfg50, rn_clip((3, 4, 23, 3), 64, 512)):
        sd = synth.rn_clip_state_dict(cfg, seed=0, token_rows=None if cfg is cfg50 else [49406, 49407], check=False)
        fl = flops_rn_image(cfg)
        img = torch.from_numpy(synth.images(cfg, B)).cuda()
        for mode in ("bf16", "f16", "f32"):
            m = ZeroshotCLIP(sd, device="cuda:0", act_dtype=DT[mode], max_batch=B)
            eng = m.engine
            out.append(row(f"{cfg.name} tower eager", mode, B, timed(lambda: eng.rn_forward(img), iters), fl))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                eng.rn_forward(img)
            out.append(row(f"{cfg.name} tower graph", mode, B, timed(g.replay, iters), fl))
            if mode == "bf16":
                out.append(row(f"{cfg.name} ZeroshotCLIP.model_inference", mode, B, timed(lambda: m.model_inference(img), iters), fl))
                if cfg is cfg50:                         # conv tile geometry: forced against rpo_conv2d_plan's choice (0)
                    for tc in (1, 3, 2):
                        eng.rn_tile_config = tc
                        out.append(row(f"{cfg.name} tower eager, every conv on tile_config {tc}", mode, B,
                                       timed(lambda: eng.rn_forward(img), iters), fl))
                    eng.rn_tile_config = 0
            del m, eng, g
            torch.cuda.empty_cache()
            if mode != "f32":
                ref = TorchRN(sd, cfg, DT[mode])
                x = img.to(DT[mode]).contiguous(memory_format=torch.channels_last)
                out.append(row(f"{cfg.name} torch F.conv2d comparator (not product)", mode, B, timed(lambda: ref(x), iters), fl))
                del ref
                torch.cuda.empty_cache()
        if cfg is cfg50:
            for mode in ("bf16", "f16"):
                out.append(coop_step(sd, cfg, mode, iters))
    with open(os.path.join(ROOT, "profiles", "rn_bench.json"), "w") as f:
        json.dump(dict(tool="tools/bench_rn.py", device=torch.cuda.get_device_name(0), results=out), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
