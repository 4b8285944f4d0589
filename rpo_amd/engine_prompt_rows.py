"""The prompt-row pass of the image tower: the prompt rows of S prompt sets on buffers of their own, reading the frozen
rows' K / V of a frozen image pass that has already been run -- or of a cache of one (rpo_amd/frozen_kv.py).  Mixed
into rpo_amd.engine.Engine; the image tower's twin of `_text_forward_`, which runs the text tower's prompt rows on
`cache_text_kv`'s cache every step.

No frozen image token reads a prompt (the visual mask puts -inf on every prompt column for every
row), so after any `_image_forward` the columns [d_v, 3 d_v) of `qkv[l][:B*N]` hold the per-block K / V of the frozen
rows, a function of the image alone, and the K prompt rows of ANY prompt set follow from them alone:
q-proj -> attention over the N frozen keys (rpo_attn_prompt_fwd) -> out-proj -> MLP, (N + K) / K * 24 / 20 ~ 11 times
less arithmetic per block than the whole pass at ViT-B/16, K = 24.  Evaluation of S prompt sets (the members of an
`RPOMulti`) is then ONE frozen pass per chunk and ONE prompt-row pass of S * B * K rows; with a cache, no image pass.

Row layout of every buffer here: set-major, row (s * B + b) * K + j = prompt row j of set s for image b of the chunk
(what rpo_broadcast_rows_sets writes and the grouped head reads: group s pairs its B images with its own text features).
Inference only: nothing is saved for a backward; training keeps its path.
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch

from . import ops
from .config import refuse_long_grid
from ._lib import EPI_BIAS, EPI_BIAS_QGELU, EPI_BIAS_RESID, EPI_LN_BIAS, EPI_LN_BIAS_QGELU, EPI_NONE

SCALE = 0.125                       # 1 / sqrt(head_dim = 64)


class PromptKV:
    """Where the prompt-row pass reads the frozen K / V: per block the views (k, v) [n_images * N, .] with one leading
    dimension, and `first` -- an int32 device scalar naming the first image of the chunk (None: image 0).  `graphs` keeps
    the captured prompt-row pass per (sets, B): the pointers a graph bakes in are this object's."""

    def __init__(self, layers: List[tuple], n_images: int, first: Optional[torch.Tensor] = None):
        self.layers, self.n_images, self.first = layers, n_images, first
        self.graphs = {}

    def set_first(self, b0: int, B: int) -> None:
        if b0 < 0 or b0 + B > self.n_images:
            raise ValueError(f"images [{b0}, {b0 + B}) of a K / V source that holds {self.n_images}")
        if self.first is None:
            if b0 != 0:
                raise ValueError("the live K / V of a frozen pass start at image 0")
            return
        self.first.fill_(b0)


class PromptRowsEngineMixin:
    pr_rows = 0                         # rows `prompt_rows_setup` sized the buffers for, 0 before it
    pr_S = pr_B = pr_gen = 0

    def prompt_rows_setup(self, S: int, B: int) -> None:
        """Buffers of the prompt-row pass for S prompt sets and chunks of up to B images.  Allocates nothing the existing
        paths use and changes none of their buffers; a second call with a smaller or equal problem keeps what is there."""
        self._refuse_rn("prompt_rows_setup")
        refuse_long_grid(self.cfg, "Engine.prompt_rows_setup")
        if S < 1 or B < 1:
            raise ValueError(f"prompt_rows_setup: S = {S}, B = {B}: both must be >= 1")
        cfg, dev, act = self.cfg, self.dev, self.act
        K, dv, e, n = cfg.K, cfg.d_v, cfg.embed, cfg.n_cls
        if self.pr_rows and S <= self.pr_S and B <= self.pr_B:
            return
        S, B = max(S, self.pr_S), max(B, self.pr_B)          # (grows, never shrinks: one allocation per trainer in practice)
        R = S * B * K
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        a = lambda *s: torch.empty(*s, dtype=act, device=dev)
        self.pr_x, self.pr_xm = f32(R, dv), f32(R, dv)       # the fp32 stream at the block boundary / after attention
        self.pr_h = a(R, dv)                                 # its 16-bit copy (or the LayerNorm output): the GEMMs' A operand
        self.pr_st = f32(R, dv // 64, 2)                     # row statistics of what pr_h copies (LayerNorm fold)
        self.pr_q, self.pr_att = a(R, dv), a(R, dv)
        self.pr_g = a(R, 4 * dv)
        self.pr_y_post = a(R, dv)
        self.pr_img_f = f32(R, e)
        self.pr_logits = f32(S * B, n)
        self.pr_head_ws = f32(S * ops.head_workspace_floats(B, n, K, e))
        self.pr_rows, self.pr_S, self.pr_B = R, S, B
        self.pr_gen += 1                                     # (captured graphs hold the old buffers' addresses: new keys)

    def live_kv(self) -> PromptKV:
        """The frozen K / V the last `_image_forward` left in `qkv[l]` (leading dimension 3 d_v), images [0, B)."""
        if getattr(self, "_pr_live", None) is None:
            dv = self.cfg.d_v
            rows = self.max_batch * self.cfg.n_frozen
            self._pr_live = PromptKV([(q[:rows, dv:2 * dv], q[:rows, 2 * dv:]) for q in self.qkv], self.max_batch)
        return self._pr_live

    def frozen_pass(self, image: torch.Tensor) -> None:
        """The existing image pass for a chunk (the captured eval forward): afterwards `live_kv()` is this chunk's."""
        self.forward_eval(image)

    def eval_text_features(self) -> torch.Tensor:
        """text_f [n_cls * K, e] of the single-run prompts, recomputed only when the prompts changed (as `forward_eval`)."""
        if not self.text_cache_ready:
            self.cache_text_kv()
        if self.text_f_version != self.params_version:
            self._text_forward(train=False)
            self.text_f_version = self.params_version
        return self.text_f

    def multi_text_features(self) -> torch.Tensor:
        """text_f [S * n_cls * K, e] of the S members' current prompts (`multi_setup`'s buffers): one text pass for all."""
        if not self.text_cache_ready:
            self.cache_text_kv()
        with self._multi_mode():
            self._text_forward(train=False)
        return self._multi_bufs["text_f"]

    # ------------------------------------------------------------------ the pass
    def image_prompt_rows(self, B: int, kv: PromptKV, img_prompts: torch.Tensor) -> torch.Tensor:
        """img_f [S*B*K, e] of the prompt rows of the S sets `img_prompts` [S, K, d_v] (sets possibly strided) for the B
        images whose frozen K / V `kv` names.  Enqueue only, current stream, capturable."""
        cfg = self.cfg
        S, K, dv, H, N = img_prompts.shape[0], cfg.K, cfg.d_v, cfg.heads_v, cfg.n_frozen
        assert tuple(img_prompts.shape[1:]) == (K, dv) and img_prompts.dtype == torch.float32
        R = S * B * K
        if R > self.pr_rows:
            raise RuntimeError(f"image_prompt_rows: {S} sets x {B} images x K = {K} rows; prompt_rows_setup sized the "
                               f"buffers for {self.pr_rows}")
        if len(kv.layers) != len(self.vis) or B > kv.n_images:
            raise ValueError(f"image_prompt_rows: K / V of {len(kv.layers)} blocks and {kv.n_images} images for "
                             f"{len(self.vis)} blocks and a chunk of {B}")
        x, xm, h, st = self.pr_x[:R], self.pr_xm[:R], self.pr_h[:R], self.pr_st[:R]
        q, att, g = self.pr_q[:R], self.pr_att[:R], self.pr_g[:R]
        # the prompt rows carry no positional embedding (trainers/rpo.py:201-204): the set's rows once per image, then ln_pre
        ops.broadcast_rows_sets(img_prompts, xm, B)
        ops.layernorm_fwd(xm, self.ln_pre[0], self.ln_pre[1], x)                        # rpo.py:206
        fold, last = self.fold_ln, len(self.vis) - 1
        for l, blk in enumerate(self.vis):
            k, v = kv.layers[l]
            # ln_1 + q-proj (K / V of a prompt row are never read).  Folded as in the whole pass: from block 1 on pr_h holds
            # the 16-bit copy of the stream and pr_st its row statistics, left by the c_proj before.
            if fold and l > 0:
                self._gemm(h, blk.w_in_ln[:dv], q, EPI_LN_BIAS, bias=blk.b_in_ln[:dv], ln_stats=st, ln_colsum=blk.s_in[:dv])
            else:
                ops.layernorm_fwd(x, blk.ln1_w, blk.ln1_b, h)
                self._gemm(h, blk.w_in[:dv], q, EPI_BIAS, bias=blk.b_in[:dv])
            ops.attn_prompt_fwd(q, k, v, att, B, H, N, K, S, first_image=kv.first, scale=SCALE, kv_images=kv.n_images)
            prod = dict(out2=h, ln_stats=st) if fold else {}
            self._gemm(att, blk.w_out, xm, EPI_BIAS_RESID, bias=blk.b_out, resid=x, **prod)
            if fold:
                self._gemm(h, blk.w_fc_ln, g, EPI_LN_BIAS_QGELU, bias=blk.b_fc_ln, aux=None, aux_row0=R, ln_stats=st,
                           ln_colsum=blk.s_fc)
            else:
                ops.layernorm_fwd(xm, blk.ln2_w, blk.ln2_b, h)
                self._gemm(h, blk.w_fc, g, EPI_BIAS_QGELU, bias=blk.b_fc, aux=None, aux_row0=R)
            prod = dict(out2=h, ln_stats=st) if (fold and l < last) else {}
            self._gemm(g, blk.w_proj, x, EPI_BIAS_RESID, bias=blk.b_proj, resid=xm, **prod)
        ops.layernorm_fwd(x, self.ln_post[0], self.ln_post[1], self.pr_y_post[:R])      # rpo.py:210
        self._gemm(self.pr_y_post[:R], self.img_proj_t, self.pr_img_f[:R], EPI_NONE)
        return self.pr_img_f[:R]

    def _prompt_rows_body(self, B: int, kv: PromptKV, img_prompts: torch.Tensor, text_f: torch.Tensor, k_used=None,
                          n: Optional[int] = None, logits: Optional[torch.Tensor] = None, head_ws=None) -> None:
        """n / logits / head_ws: a class set's count and buffers (shared_eval_logits(classes=...)); default: the built-in's."""
        S, K, e = img_prompts.shape[0], self.cfg.K, self.cfg.embed
        n = self.cfg.n_cls if n is None else n
        logits, head_ws = (self.pr_logits, self.pr_head_ws) if logits is None else (logits, head_ws)
        img_f = self.image_prompt_rows(B, kv, img_prompts)
        ops.head_fwd_bwd_grouped(img_f.view(S * B, K, e), text_f.view(S * n, K, e), None, self.logit_scale_exp,
                                 logits[:S * B], None, None, None, head_ws, S, k_used=k_used)

    def _shared_eval_logits_cs(self, B: int, kv: PromptKV, img_prompts: torch.Tensor, text_f: torch.Tensor, use_graph: bool,
                               cs) -> torch.Tensor:
        """`shared_eval_logits` against a class set: the prompt-row pass is the engine's own, the grouped head reads the
        set's features and writes the set's logits.  Graphs are keyed per (S, B, K / V source) and live on the class set
        (with the K / V source they read, so neither outlives the other's addresses)."""
        self._cs_check(cs)
        S, n = img_prompts.shape[0], cs.n
        assert text_f.shape[0] == S * n * self.cfg.K and text_f.is_contiguous()
        if B > self.pr_B or S > self.pr_S:
            raise RuntimeError(f"shared_eval_logits: S = {S}, B = {B}; prompt_rows_setup({self.pr_S}, {self.pr_B})")
        sh = cs.shared_buffers(S, B)
        body = lambda: self._prompt_rows_body(B, kv, img_prompts, text_f, None, n, sh["logits"], sh["head_ws"])
        if not use_graph or os.environ.get("RPO_NO_EVAL_GRAPH") == "1":
            body()
            return sh["logits"][:S * B].view(S, B, n)
        key = ("shared", id(kv), self.pr_gen, sh["gen"], S, B, img_prompts.data_ptr(), img_prompts.stride(0), text_f.data_ptr())
        entry = cs.graphs.get(key)
        if entry is None:
            body()                                                             # eager warm-up: sets kernel attributes
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                body()
            entry = cs.graphs[key] = (g, kv)
        entry[0].replay()
        return sh["logits"][:S * B].view(S, B, n)

    def shared_eval_logits(self, B: int, kv: PromptKV, img_prompts: torch.Tensor, text_f: torch.Tensor,
                           use_graph: bool = True, k_used: Optional[torch.Tensor] = None, classes=None) -> torch.Tensor:
        """logits [S, B, n_cls] (the engine's own buffer, valid until the next call) of the S prompt sets for the chunk `kv`
        names: the prompt-row pass and the grouped head, ONE HIP graph per (S, B) and K / V source on the current
        stream -- eager warm-up first, then capture, as `forward_eval`.  text_f [S * n_cls * K, e]: the sets' text features.
        k_used: int32 [S] on the device -- set s averages over its first k_used[s] pairs (rpo_head_fwd_bwd_grouped_k).
        classes: a `ClassSet` of this engine -- logits [S, B, n'] in its buffer, text_f [S * n' * K, e] its features."""
        if classes is not None:
            if k_used is not None:
                raise NotImplementedError("shared_eval_logits(classes=...) with k_used: members that use fewer than the "
                                          "engine's K pairs (RPOSweep) are not built for class sets")
            return self._shared_eval_logits_cs(B, kv, img_prompts, text_f, use_graph, classes)
        S, n = img_prompts.shape[0], self.cfg.n_cls
        assert text_f.shape[0] == S * n * self.cfg.K and text_f.is_contiguous()
        if S * B > self.pr_logits.shape[0] or B > self.pr_B or S > self.pr_S:
            raise RuntimeError(f"shared_eval_logits: S = {S}, B = {B}; prompt_rows_setup({self.pr_S}, {self.pr_B})")
        if not use_graph or os.environ.get("RPO_NO_EVAL_GRAPH") == "1":
            self._prompt_rows_body(B, kv, img_prompts, text_f, k_used)
            return self.pr_logits[:S * B].view(S, B, n)
        key = (self.pr_gen, S, B, img_prompts.data_ptr(), img_prompts.stride(0), text_f.data_ptr()) + (
            () if k_used is None else (k_used.data_ptr(),))
        g = kv.graphs.get(key)
        if g is None:
            self._prompt_rows_body(B, kv, img_prompts, text_f, k_used)         # eager warm-up: sets kernel attributes
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._prompt_rows_body(B, kv, img_prompts, text_f, k_used)
            kv.graphs[key] = g
        g.replay()
        return self.pr_logits[:S * B].view(S, B, n)
