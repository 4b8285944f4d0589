"""The CLIP ResNet image tower (clip/model.py:10-152, ModifiedResNet) on the engine: frozen and forward-only, for the
trainers that take whatever `clip_model.visual` is (zero-shot CLIP, CoOp).  Mixed into rpo_amd.engine.Engine; its
`_pack` / `_alloc` call `_rn_pack` / `_rn_alloc` instead of building the ViT tower when the config is a ResNet.

Data layout: NHWC in the act dtype (row = pixel, channels contiguous), so a 1x1 convolution is a GEMM
[B*H*W, Cin] x [Cout, Cin]^T and a 3x3 one an implicit GEMM over (tap, channel) (csrc/conv.hip).  Eval-mode BatchNorm
is folded into every convolution at load, in float64: W' = W gamma / sqrt(var + eps) rounded to the act dtype, b' = beta -
mean gamma / sqrt(var + eps) in fp32; weights are stored [Cout, kh, kw, Cin].  The forward enqueues kernels only (no
host sync, no allocation), so it can be captured in a graph."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import ops
from ._lib import EPI_BIAS
from .config import rn_plan

BN_EPS = 1e-5


def fold_bn(w: np.ndarray, gamma: np.ndarray, beta: np.ndarray, mean: np.ndarray, var: np.ndarray, eps: float = BN_EPS):
    """(W' [Cout, kh, kw, Cin] float64, b' [Cout] float64) with conv(x, W') + b' = BatchNorm_eval(conv(x, W))."""
    g = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    wf = np.asarray(w, np.float64) * g[:, None, None, None]
    b = np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * g
    return np.ascontiguousarray(wf.transpose(0, 2, 3, 1)), b


def rn_unsupported(cfg, act_dtype) -> Optional[str]:
    """Why the conv kernels cannot run this ResNet (None: they can).  rpo_conv2d_nhwc takes Cin % 32 (16-bit) / % 16
    (f32) == 0 and Cout % 32 == 0, the stem Cout % 8 == 0 up to 128, the attention pool at most 256 tokens: RN50 / RN101
    fit; RN50x4 (stem 40, planes 80, ...) and RN50x16 (stem 48, ...) do not."""
    ck = 16 if act_dtype == torch.float32 else 32
    w = cfg.rn_width
    convs = [(w // 2, w // 2), (w // 2, w)]
    for b in rn_plan(cfg):
        p = b["planes"]
        convs += [(b["cin"], p), (p, p), (p, 4 * p)] + ([(b["cin"], 4 * p)] if b["down"] else [])
    bad = sorted({(ci, co) for ci, co in convs if ci % ck or co % 32})
    if bad or (w // 2) % 8 or w // 2 > 128:
        return (f"channel counts (Cin, Cout) {bad[:4]} of the stem width {w}: the conv kernels need Cin % {ck} == 0 and "
                f"Cout % 32 == 0")
    if cfg.n_frozen > 256:
        return f"{cfg.n_frozen} attention-pool tokens (at most 256)"
    return None


class RnEngineMixin:
    # conv tile geometry of every launch: 0 = rpo_conv2d_plan's choice; 1 / 2 / 3 force 64x64 / 128x128 / 128x64
    # (bit-identical results; tools/bench_rn.py measures them against the heuristic)
    rn_tile_config = 0

    def _rn_conv(self, sd, conv: str, bn: str):
        wf, b = fold_bn(sd[conv], sd[bn + "weight"], sd[bn + "bias"], sd[bn + "running_mean"], sd[bn + "running_var"])
        w = torch.from_numpy(wf.astype(np.float32)).to(self.dev)
        return self._act(w.reshape(w.shape[0], -1)).view(w.shape), self._f32(b)

    def _rn_pack(self, sd) -> None:
        cfg = self.cfg
        why = rn_unsupported(cfg, self.act)
        if why is not None:
            raise NotImplementedError(f"{cfg.name}: the ResNet tower supports RN50 / RN101-shaped models; this one has {why}")
        self.rn_stem = [self._rn_conv(sd, f"visual.conv{i}.weight", f"visual.bn{i}.") for i in (1, 2, 3)]
        self.rn_blocks: List[Dict] = []
        for b in rn_plan(cfg):
            p = f"visual.{b['name']}."
            blk = dict(b, c1=self._rn_conv(sd, p + "conv1.weight", p + "bn1."), c2=self._rn_conv(sd, p + "conv2.weight", p + "bn2."),
                       c3=self._rn_conv(sd, p + "conv3.weight", p + "bn3."))
            if b["down"]:
                blk["ds"] = self._rn_conv(sd, p + "downsample.0.weight", p + "downsample.1.")
            self.rn_blocks.append(blk)
        a = "visual.attnpool."
        self.rn_pos = self._f32(sd[a + "positional_embedding"])
        self.rn_wq, self.rn_bq = self._act(self._f32(sd[a + "q_proj.weight"])), self._f32(sd[a + "q_proj.bias"])
        self.rn_wkv = self._act(self._f32(np.concatenate([sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]])))
        self.rn_bkv = self._f32(np.concatenate([sd[a + "k_proj.bias"], sd[a + "v_proj.bias"]]))
        self.rn_wc, self.rn_bc = self._act(self._f32(sd[a + "c_proj.weight"])), self._f32(sd[a + "c_proj.bias"])

    def _rn_alloc(self) -> None:
        """Ping-pong NHWC buffers for max_batch, each as large as the largest activation of the tower."""
        cfg, B, act = self.cfg, self.max_batch, self.act
        w, h1 = cfg.rn_width, cfg.image_size // 2
        big = h1 * h1 * w                                                  # stem conv3 output
        for b in self.rn_blocks:
            big = max(big, b["H"] * b["H"] * max(b["cin"], b["planes"]), (b["H"] // b["stride"]) ** 2 * 4 * b["planes"])
        a = lambda n: torch.empty(B * n, dtype=act, device=self.dev)
        self.rn_buf = [a(big) for _ in range(5)]                          # x, out, t1, t2 / pooled, identity
        self.rn_pool = a(big // 4)
        C, T = cfg.d_v, cfg.n_frozen
        self.rn_tok = torch.empty(B, T, C, dtype=act, device=self.dev)
        self.rn_kv = torch.empty(B * T, 2 * C, dtype=act, device=self.dev)
        self.rn_q = torch.empty(B, C, dtype=torch.float32, device=self.dev)
        self.rn_att = torch.empty(B, C, dtype=act, device=self.dev)
        self.rn_img_f = torch.empty(B, cfg.embed, dtype=torch.float32, device=self.dev)       # = Engine.img_cls_f

    def _nhwc(self, i: int, B: int, H: int, C: int, pool: bool = False) -> torch.Tensor:
        buf = self.rn_pool if pool else self.rn_buf[i]
        return buf[:B * H * H * C].view(B, H, H, C)

    def rn_forward(self, image: torch.Tensor) -> int:
        """ModifiedResNet.forward (clip/model.py:138-152) of image [B, 3, R, R] fp32 -> self.img_cls_f[:B] (fp32)."""
        cfg = self.cfg
        B = image.shape[0]
        assert image.is_cuda and image.dtype == torch.float32 and image.is_contiguous() and 1 <= B <= self.max_batch
        assert tuple(image.shape[1:]) == (3, cfg.image_size, cfg.image_size)
        assert image.device == self.dev and torch.cuda.current_device() == self.dev.index
        w, H = cfg.rn_width, cfg.image_size // 2
        (w1, b1), (w2, b2), (w3, b3) = self.rn_stem
        s1 = ops.conv_stem(image, w1, b1, self._nhwc(2, B, H, w // 2))
        tc = self.rn_tile_config
        s2 = ops.conv2d_nhwc(s1, w2, b2, self._nhwc(3, B, H, w // 2), tile_config=tc)
        s3 = ops.conv2d_nhwc(s2, w3, b3, self._nhwc(2, B, H, w), tile_config=tc)
        H //= 2
        x = ops.avgpool_nhwc(s3, self._nhwc(0, B, H, w), 2)
        cur = 0
        for blk in self.rn_blocks:
            s, p, cin = blk["stride"], blk["planes"], blk["cin"]
            Ho, nxt = H // s, 1 - cur
            t1 = ops.conv2d_nhwc(x, *blk["c1"], self._nhwc(2, B, H, p), tile_config=tc)
            t2 = ops.conv2d_nhwc(t1, *blk["c2"], self._nhwc(3, B, H, p), tile_config=tc)
            if s > 1:
                t2 = ops.avgpool_nhwc(t2, self._nhwc(2, B, Ho, p), s)
            idn = x
            if blk["down"]:
                xd = ops.avgpool_nhwc(x, self._nhwc(0, B, Ho, cin, pool=True), s) if s > 1 else x
                idn = ops.conv2d_nhwc(xd, *blk["ds"], self._nhwc(4, B, Ho, 4 * p), relu=False, tile_config=tc)
            x = ops.conv2d_nhwc(t2, *blk["c3"], self._nhwc(nxt, B, Ho, 4 * p), resid=idn, tile_config=tc)
            cur, H = nxt, Ho
        # attention pool (clip/model.py:66-91): only token 0's query is needed
        C, T, heads = cfg.d_v, cfg.n_frozen, cfg.heads_v
        tok = ops.attnpool_tokens(x, self.rn_pos, self.rn_tok[:B])
        ops.gemm_nt(tok.view(B * T, C), self.rn_wkv, self.rn_kv[:B * T], EPI_BIAS, bias=self.rn_bkv)
        ops.gemm_nt(tok[:, 0, :], self.rn_wq, self.rn_q[:B], EPI_BIAS, bias=self.rn_bq)
        ops.attnpool_attn(self.rn_q[:B], self.rn_kv[:B * T].view(B, T, 2 * C), self.rn_att[:B], heads, (C // heads) ** -0.5)
        ops.gemm_nt(self.rn_att[:B], self.rn_wc, self.img_cls_f[:B], EPI_BIAS, bias=self.rn_bc)
        return B
