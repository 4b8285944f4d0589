"""The prompt-row pass of the image tower that TRAINS: the members of a sweep on ONE shared batch.
Mixed into rpo_amd.engine.Engine next to `engine_prompt_rows.PromptRowsEngineMixin`, whose inference-only pass this is the
training twin of.

When the S members of a step see the same B augmented images, the frozen rows of the image tower and their per-block K / V
are the same for all of them (no frozen image token reads a prompt): the frozen pass runs ONCE for the B
images, and only the S * B * K prompt rows differ.  Per block and image the own-batch sweep (`multi_forward_backward`: "ONE
batch of S * B images") costs S (N + K) 24 d^2 multiply-adds, this step (N + K) 24 d^2 + S K 20 d^2 -- the two figures of
engine_prompt_rows.py's docstring.  The sharing is within one step on one augmented batch, so it is exact: nothing is cached
across steps.

    text tower     S * n_cls virtual classes on the side stream, exactly as `multi_forward_backward` (`_multi_mode`)
    frozen pass    the existing `_image_forward` for the B images; the single-run `img_prompt` rides in its rows N .. N + K
                   (the frozen rows' bits do not depend on it; K / (N + K) of that pass is wasted)
    prompt rows    the GEMM calls and the LayerNorm fold of `image_prompt_rows` over `live_kv()`, saving per block what
                   `_rows_backward` reads: the stream at the block boundary, the stream after attention, q, the QuickGELU operand
    head           rpo_head_fwd_bwd_grouped: S groups of B images, the labels shared, k_used = the members' own K
    backward       `_rows_backward` on the R = S B K rows; per block ONE rpo_attn_prompt_bwd serves all members from one
                   staging of an image's K / V; d out-proj is its own GEMM (fold_out = False)
    tail           ln_pre backward, then reduce_groups_sets(..., m_g_img, B)

Row layout of every buffer here: set-major, row (s * B + b) * K + j, as in engine_prompt_rows.py.  Results land where
`multi_forward_backward` leaves them: m_loss [S], m_logits [S * B, n_cls], m_grads [S, text | img].
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch

from . import ops
from .config import refuse_long_grid
from ._lib import EPI_BIAS, EPI_BIAS_QGELU, EPI_BIAS_RESID, EPI_LN_BIAS, EPI_LN_BIAS_QGELU, EPI_NONE

SCALE = 0.125                       # 1 / sqrt(head_dim = 64)
DY_SLABS = 4                        # split-K slabs of the chain's fp32 dX GEMMs (Engine._alloc: max(SPLIT_FC, SPLIT_Q, 4))


def prompt_train_bytes(cfg, S: int, B: int, act_dtype: torch.dtype = torch.bfloat16, aux_f32: bool = False) -> int:
    """Bytes `prompt_train_setup(S, B)` allocates for R = S B K prompt rows -- arithmetic on the configuration, nothing is
    touched.  Per row and block: the two fp32 streams, q and the QuickGELU operand (13 824 B at ViT-B/16 in the 16-bit modes:
    165 888 B per row over 12 blocks, 1.02 GB at S = 8, B = 32, K = 24); beside them the last boundary, the ln_pre input,
    the forward's temporaries, the head gradients and the chain's workspaces."""
    a = 4 if act_dtype == torch.float32 else 2
    au = 4 if aux_f32 else a
    R, dv, e, L = S * B * cfg.K, cfg.d_v, cfg.embed, cfg.layers_v
    per_block = 4 * dv + 4 * dv + a * dv + au * 4 * dv                     # x[l], xm[l], q[l], u[l]
    saves = L * per_block + 4 * dv + 4 * dv                                # + x[L], x_pre
    forward = a * dv + 4 * (dv // 64) * 2 + a * dv + a * 4 * dv + a * dv + 4 * e     # h, st, att, g, y_post, img_f
    head = 4 * e + a * e                                                   # d_img_f, d_img_f_a
    chain = 4 * dv * 2 + a * dv + a * 4 * dv + a * dv * 2 + 4 * dv * DY_SLABS       # dxa, dxb, dxc, du, da, dq, dy
    return R * (saves + forward + head + chain)


class PromptTrainEngineMixin:
    pt_rows = 0                         # rows `prompt_train_setup` sized the buffers for, 0 before it
    pt_S = pt_B = 0

    def prompt_train_setup(self, S: int, B: int, member_K: Optional[Sequence[int]] = None) -> None:
        """Buffers of the shared-batch step for S members on ONE batch of B images.  Touches no existing buffer.  The
        members' parameters, gradients, losses, logits and S-fold text buffers are `multi_setup`'s (called here unless it
        has been, for the same S, B and member_K); the image tower is the engine's own, built for B images."""
        self._refuse_rn("prompt_train_setup")
        refuse_long_grid(self.cfg, "Engine.prompt_train_setup")
        if S < 1 or B < 1:
            raise ValueError(f"prompt_train_setup: S = {S}, B = {B}: both must be >= 1")
        if B > self.max_batch:
            raise ValueError(f"prompt_train_setup: B = {B} images per step, the engine was built with max_batch = "
                             f"{self.max_batch}")
        mk = None if member_K is None else [int(k) for k in member_K]
        if not (self.multi_S == S and self.multi_B == B and getattr(self, "multi_K", None) == mk):
            # `multi_setup` sizes the members' buffers for an own-batch step of S * B images through the image tower and
            # checks the tower for them; here the tower sees B, so for that one call the check is given S * B
            cap = self.max_batch
            self.max_batch = max(cap, S * B)
            try:
                self.multi_setup(S, B, **({} if mk is None else dict(member_K=mk)))
            finally:
                self.max_batch = cap
        cfg, dev, act = self.cfg, self.dev, self.act
        K, dv, e, L = cfg.K, cfg.d_v, cfg.embed, cfg.layers_v
        R = S * B * K
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        a = lambda *s: torch.empty(*s, dtype=act, device=dev)
        au = f32 if os.environ.get("RPO_AUX_F32") == "1" else a
        t = {}
        t["x"] = [f32(R, dv) for _ in range(L + 1)]        # the fp32 stream at the block boundaries
        t["xm"] = [f32(R, dv) for _ in range(L)]           # ... after attention
        t["q"] = [a(R, dv) for _ in range(L)]
        t["u"] = [au(R, 4 * dv) for _ in range(L)]         # QuickGELU operand (16-bit modes: the derivative itself)
        t["x_pre"] = f32(R, dv)                            # the sets' rows once per image: ln_pre's input
        t["h"], t["st"] = a(R, dv), f32(R, dv // 64, 2)
        t["att"], t["g"], t["y_post"] = a(R, dv), a(R, 4 * dv), a(R, dv)
        t["img_f"] = f32(R, e)
        t["d_img_f"], t["d_img_f_a"] = f32(R, e), a(R, e)
        t["dxa"], t["dxb"], t["dxc"] = f32(R, dv), f32(R, dv), a(R, dv)
        t["du"], t["da"], t["dq"] = a(R, 4 * dv), a(R, dv), a(R, dv)
        t["dy"] = f32(DY_SLABS, R, dv)
        self._pt = t
        self._pt_label = torch.zeros(S * B, dtype=torch.int64, device=dev)     # the batch's labels once per member
        self.pt_rows, self.pt_S, self.pt_B = R, S, B

    def prompt_train_hbm_bytes(self) -> int:
        """Bytes `prompt_train_setup` added beside `multi_setup`'s (`multi_hbm_bytes`): `prompt_train_bytes` says the same."""
        tot = 0
        for v in self._pt.values():
            for x in (v if isinstance(v, list) else [v]):
                tot += x.numel() * x.element_size()
        return tot

    # ------------------------------------------------------------------ the pass
    def _prompt_rows_train_forward(self, B: int, img_prompts: torch.Tensor) -> torch.Tensor:
        """`image_prompt_rows` over `live_kv()` in train mode: the same launches, with every block's x / xm / q kept and
        `aux=` on c_fc.  img_f [S*B*K, e]."""
        cfg, t = self.cfg, self._pt
        S, K, dv, H, N = img_prompts.shape[0], cfg.K, cfg.d_v, cfg.heads_v, cfg.n_frozen
        kv = self.live_kv()
        h, st, att, g = t["h"], t["st"], t["att"], t["g"]
        ops.broadcast_rows_sets(img_prompts, t["x_pre"], B)
        ops.layernorm_fwd(t["x_pre"], self.ln_pre[0], self.ln_pre[1], t["x"][0])         # rpo.py:206
        fold, last = self.fold_ln, len(self.vis) - 1
        for l, blk in enumerate(self.vis):
            k, v = kv.layers[l]
            x, xm, xo, q = t["x"][l], t["xm"][l], t["x"][l + 1], t["q"][l]
            if fold and l > 0:
                self._gemm(h, blk.w_in_ln[:dv], q, EPI_LN_BIAS, bias=blk.b_in_ln[:dv], ln_stats=st, ln_colsum=blk.s_in[:dv])
            else:
                ops.layernorm_fwd(x, blk.ln1_w, blk.ln1_b, h)
                self._gemm(h, blk.w_in[:dv], q, EPI_BIAS, bias=blk.b_in[:dv])
            ops.attn_prompt_fwd(q, k, v, att, B, H, N, K, S, first_image=None, scale=SCALE, kv_images=kv.n_images)
            prod = dict(out2=h, ln_stats=st) if fold else {}
            self._gemm(att, blk.w_out, xm, EPI_BIAS_RESID, bias=blk.b_out, resid=x, **prod)
            if fold:
                self._gemm(h, blk.w_fc_ln, g, EPI_LN_BIAS_QGELU, bias=blk.b_fc_ln, aux=t["u"][l], aux_row0=0, ln_stats=st,
                           ln_colsum=blk.s_fc)
            else:
                ops.layernorm_fwd(xm, blk.ln2_w, blk.ln2_b, h)
                self._gemm(h, blk.w_fc, g, EPI_BIAS_QGELU, bias=blk.b_fc, aux=t["u"][l], aux_row0=0)
            prod = dict(out2=h, ln_stats=st) if (fold and l < last) else {}
            self._gemm(g, blk.w_proj, xo, EPI_BIAS_RESID, bias=blk.b_proj, resid=xm, **prod)
        ops.layernorm_fwd(t["x"][-1], self.ln_post[0], self.ln_post[1], t["y_post"])     # rpo.py:210
        self._gemm(t["y_post"], self.img_proj_t, t["img_f"], EPI_NONE)
        return t["img_f"]

    def _shared_head(self, label: torch.Tensor) -> None:
        """The S heads in the launches of one: member s pairs the B shared images' prompt rows of ITS set with its own text
        features; `label` [S * B] repeats the batch's labels per member."""
        S, B, K, e, n = self.pt_S, self.pt_B, self.cfg.K, self.cfg.embed, self.cfg.n_cls
        t, mb = self._pt, self._multi_bufs
        act = {} if self.act == torch.float32 else dict(d_img_f_act=t["d_img_f_a"], d_text_f_act=mb["d_text_f_a"])
        ops.head_fwd_bwd_grouped(t["img_f"].view(S * B, K, e), mb["text_f"].view(S * n, K, e), label, self.logit_scale_exp,
                                 self.m_logits, self.m_loss, t["d_img_f"].view(S * B, K, e), mb["d_text_f"].view(S * n, K, e),
                                 self.m_head_ws, S, k_used=self.m_k_used, **act)

    def _prompt_rows_backward(self, B: int) -> None:
        """The image tower's prompt-row chain for all S members: `_image_backward_rows` on the R rows of the buffers here."""
        cfg, t = self.cfg, self._pt
        S, K, dv, H, N = self.pt_S, cfg.K, cfg.d_v, cfg.heads_v, cfg.n_frozen
        f32m = self.act == torch.float32
        kv = self.live_kv()
        dxa, dxb, dxc, dy = t["dxa"], t["dxb"], t["dxc"], t["dy"]
        self._gemm(t["d_img_f"] if f32m else t["d_img_f_a"], self.img_proj, dy[0], EPI_NONE,
                   prefetch=self.vis[-1].w_proj_t if self._pf_chains else None)
        ops.layernorm_bwd(dy[0], t["x"][-1], self.ln_post[0], None, dxa, None if f32m else dxc)

        def attn_bwd(l, da, dq):
            k, v = kv.layers[l]
            ops.attn_prompt_bwd(t["q"][l], k, v, da, dq, B, H, N, K, S, first_image=None, scale=SCALE, kv_images=kv.n_images)

        dx = self._rows_backward(self.vis, t["x"][:-1], t["xm"], t["u"], dxa, dxb, dxc, t["du"], t["da"], t["dq"], dy, attn_bwd,
                                 fold_out=False)
        ops.layernorm_bwd(dx, t["x_pre"], self.ln_pre[0], None, dxb)                     # through ln_pre (rpo.py:206)
        ops.reduce_groups_sets(dxb, self.m_g_img, B)                                     # .repeat over the batch (rpo.py:204)

    def shared_forward_backward(self, image: torch.Tensor, label: torch.Tensor) -> None:
        """Enqueue loss + both prompt gradients of every member on ONE batch: image [B, 3, H, W] and label [B], shared by
        the S members.  Results land in m_loss [S], m_logits [S*B, n_cls], m_grads [S, text | img].  Capturable in a HIP
        graph; the stream structure is `multi_forward_backward`'s: text tower on the side stream, image tower on the
        current one."""
        S, B = self.pt_S, self.pt_B
        if not self.pt_rows:
            raise RuntimeError("prompt_train_setup(S, B) has not been called on this engine")
        assert image.shape[0] == B, f"the shared-batch step takes the ONE batch of B = {B} images"
        assert label.dtype == torch.int64 and label.shape == (B,) and label.is_contiguous()
        self._check(image)
        self.text_f_version = -1
        main = torch.cuda.current_stream()
        self.side.wait_stream(main)
        with self._multi_mode(), torch.cuda.stream(self.side):
            self._text_forward(train=True)
        # (outside `_multi_mode`: the frozen pass is the single-run image forward, its embedding the single-run one)
        self._image_forward(image, train=False)
        self._prompt_rows_train_forward(B, self.m_img_prompt)
        labels = self._pt_labels(label)
        main.wait_stream(self.side)
        self._shared_head(labels)
        self.side.wait_stream(main)
        with self._multi_mode(), torch.cuda.stream(self.side):
            self._text_backward()
        self._prompt_rows_backward(B)
        main.wait_stream(self.side)

    def _pt_labels(self, label: torch.Tensor) -> torch.Tensor:
        """label [B] once per member ([S * B], what the grouped head reads): one small copy on the step's stream."""
        self._pt_label.view(self.pt_S, self.pt_B).copy_(label)
        return self._pt_label
