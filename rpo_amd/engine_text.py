"""The plain text tower of the engine (rpo_amd/engine.py mixes this in): the ONE block loop (`_text_blocks`) and EOT
feature tail (`_text_eot_tail`) that every plain-tower pass runs -- `cache_text_kv`, `forward_plain`, class sets, the dense
and shared-prefix CoOp / CoCoOp passes -- then `encode_text` on top of the two for prompts the engine was NOT built with
(any [P, 77] token ids, chunked), and the caller-given classifier of `forward_plain`.  Prompt ensembling
(rpo_amd.zeroshot.ZeroshotCLIP2) is built on it."""
from __future__ import annotations

import os
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import EPI_BIAS, EPI_BIAS_QGELU, EPI_BIAS_RESID, EPI_NONE

SCALE = 0.125                       # 1 / sqrt(head_dim = 64)


class TextEncodeEngineMixin:
    def _text_blocks(self, xs: Sequence[torch.Tensor], xms: Sequence[torch.Tensor], qkvs: Sequence[torch.Tensor],
                     h: torch.Tensor, att: torch.Tensor, g: torch.Tensor, attn: Callable,
                     kv: Optional[List[torch.Tensor]] = None, aux: Optional[Sequence[torch.Tensor]] = None) -> None:
        """The plain text blocks (clip/model.py:171-186) over R rows: block l reads xs[l] [R, d_t] fp32 and writes
        xs[l + 1], with xms[l] (fp32, the residual after attention) and qkvs[l] [R, 3 d_t] as its buffers.  A pass that
        keeps nothing gives the same tensor for every layer, so x is updated in place; a training pass gives the lists the
        backward re-reads.  h, att [R, d_t] and g [R, 4 d_t] are workspace.  attn(q, k, v, out): the attention of the row
        layout.  kv: per layer [R, 2 d_t], receives that layer's K | V.  aux: per layer [R, 4 d_t], receives the QuickGELU
        operand (training only)."""
        dt, R = self.cfg.d_t, h.shape[0]
        for l, blk in enumerate(self.txt):
            x, xm, qkv = xs[l], xms[l], qkvs[l]
            ops.layernorm_fwd(x, blk.ln1_w, blk.ln1_b, h)
            ops.gemm_nt(h, blk.w_in, qkv, EPI_BIAS, bias=blk.b_in)
            attn(qkv[:, :dt], qkv[:, dt:2 * dt], qkv[:, 2 * dt:], att)
            if kv is not None:
                kv[l].copy_(qkv[:, dt:])
            ops.gemm_nt(att, blk.w_out, xm, EPI_BIAS_RESID, bias=blk.b_out, resid=x)
            ops.layernorm_fwd(xm, blk.ln2_w, blk.ln2_b, h)
            ops.gemm_nt(h, blk.w_fc, g, EPI_BIAS_QGELU, bias=blk.b_fc, aux=None if aux is None else aux[l],
                        aux_row0=R if aux is None else 0)
            ops.gemm_nt(g, blk.w_proj, xs[l + 1], EPI_BIAS_RESID, bias=blk.b_proj, resid=xm)

    def _text_blocks_plain(self, x: torch.Tensor, len_i32: torch.Tensor, n: int, L: int,
                           kv: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
        """The text blocks over the first L positions of n prompts, x [n * L, d_t] fp32 updated in place to the last
        block's output, under the causal AND col < len mask.  kv: per layer [n * L, 2 d_t], receives that layer's K | V."""
        dt, H, Lt = self.cfg.d_t, self.cfg.heads_t, len(self.txt)
        a = lambda w: torch.empty(n * L, w, dtype=self.act, device=self.dev)
        attn = lambda q, k, v, out: ops.text_attn_fwd(q, k, v, out, len_i32, n, L, L, H, causal=True, scale=SCALE)
        self._text_blocks([x] * (Lt + 1), [torch.empty_like(x)] * Lt, [a(3 * dt)] * Lt, a(dt), a(dt), a(4 * dt), attn, kv)
        return x

    def _text_eot_tail(self, x: torch.Tensor, rows: torch.Tensor, x_eot: torch.Tensor, y_eot: torch.Tensor,
                       out: torch.Tensor) -> torch.Tensor:
        """out [n, e] fp32 = text_projection of ln_final of rows `rows` [n] (the EOT tokens) of x (clip/model.py:352-354);
        x_eot [n, d_t] fp32 keeps the gathered rows (the backward re-reads them), y_eot [n, d_t] is workspace."""
        torch.index_select(x, 0, rows, out=x_eot)
        ops.layernorm_fwd(x_eot, self.ln_final[0], self.ln_final[1], y_eot)
        return ops.gemm_nt(y_eot, self.text_proj_t, out, EPI_NONE)

    def _text_eot_features(self, x: torch.Tensor, len_i32: torch.Tensor, n: int, L: int, out: torch.Tensor) -> torch.Tensor:
        """out [n, e] fp32 = `_text_eot_tail` of every prompt's EOT row of x [n * L, d_t]."""
        rows = torch.arange(n, device=self.dev) * L + (len_i32.to(torch.int64) - 1)            # EOT positions
        return self._text_eot_tail(x, rows, torch.empty(n, self.cfg.d_t, dtype=torch.float32, device=self.dev),
                                   torch.empty(n, self.cfg.d_t, dtype=self.act, device=self.dev), out)

    def _text_tables(self):
        """(token_embedding.weight [vocab, d_t], positional_embedding [context, d_t]) as fp32 device tensors for
        rpo_text_embed: uploaded on the first call that needs them (101 MB at CLIP's vocabulary) and kept; attributes of
        the engine, so `hbm_bytes()` counts them."""
        if getattr(self, "_tok_emb_dev", None) is None:
            self._tok_emb_dev = self._f32(np.asarray(self._tok_emb_host))
            self._pos_dev = self._f32(np.asarray(self._pos_host))
        return self._tok_emb_dev, self._pos_dev

    # prompts per pass of encode_text: bounds its workspace to TEXT_CHUNK * 77 rows of [fp32 x 2 | act x 9] d_t-wide
    # buffers -- 0.26 GB in the 16-bit modes and 0.44 GB in f32 at d_t = 512 if every prompt filled the context; a chunk
    # allocates for its own longest prompt (class-name prompts: 10-20 tokens, a quarter of that).  Measured at 7 000 and
    # 80 000 prompts of 8-20 tokens (profiles/ensemble_bench.json): 256 per pass is faster than 1024 or 4096 (50 / 159 /
    # 147 ms at 7 000), so the smaller bound costs nothing
    TEXT_CHUNK = 256

    @torch.no_grad()
    def encode_text(self, tokens: np.ndarray, chunk: Optional[int] = None) -> torch.Tensor:
        """Plain `CLIP.encode_text` (clip/model.py:344-356) of ANY prompts: tokens int64 [P, 77] -> [P, e] fp32 on the
        device, un-normalised as the reference's.  P has nothing to do with cfg.n_cls, and the engine may hold any model
        (RPO / CoOp / LP): nothing of its own text state is read or written (K / V cache, frozen-token rows, cached
        features, prompts versions).  A learned CoOp context (`set_context`) is not applied.
        `chunk` prompts run per pass (default TEXT_CHUNK = 256, which bounds the workspace by the chunk instead of P:
        see the note at TEXT_CHUNK); each pass runs the positions up to ITS longest prompt -- what follows a prompt's
        EOT cannot reach the EOT row under the causal mask -- through the block sequence of `cache_text_kv`, keeps no
        K / V, and ends in ln_final + text_projection of the EOT rows as `forward_plain` does.  The token embeddings of
        a chunk are gathered on the device (rpo_text_embed: the pass uploads its int32 ids; the fp32 table and the
        positional embedding are uploaded once, on the first call that needs them); RPO_TEXT_EMBED_HOST=1 gathers them on
        the host from the state dict's table (held by reference, never copied) and uploads the rows -- the same bits."""
        cfg = self.cfg
        tokens = np.asarray(tokens)
        assert tokens.ndim == 2 and tokens.shape[1] == cfg.context and tokens.shape[0] >= 1, \
            f"tokens: [P, {cfg.context}] prompt ids"
        assert np.issubdtype(tokens.dtype, np.integer), "tokens: integer prompt ids"
        tokens = tokens.astype(np.int64, copy=False)
        assert int(tokens.min()) >= 0 and int(tokens.max()) < self._tok_emb_host.shape[0], "token id outside the vocabulary"
        P = tokens.shape[0]
        chunk = self.TEXT_CHUNK if chunk is None else int(chunk)
        assert chunk >= 1, "chunk: prompts per pass, >= 1"
        lens = tokens.argmax(-1) + 1                                   # EOT has the highest id (clip/model.py:354)
        host = os.environ.get("RPO_TEXT_EMBED_HOST") == "1"
        if host:
            # host tensors over the state dict's own memory (no copy of the table): torch's embedding gathers a pass's rows
            # on the host's threads, numpy's fancy index on one (7 000 prompts: 68 -> 50 ms)
            table, pos = torch.as_tensor(np.asarray(self._tok_emb_host)), torch.as_tensor(np.asarray(self._pos_host))
            ids = torch.from_numpy(np.ascontiguousarray(tokens))
        else:
            ids = torch.from_numpy(np.ascontiguousarray(tokens.astype(np.int32)))
        with torch.cuda.device(self.dev):
            if not host:
                table, pos = self._text_tables()
            out = torch.empty(P, cfg.embed, dtype=torch.float32, device=self.dev)
            for p0 in range(0, P, chunk):
                p1 = min(P, p0 + chunk)
                n, L = p1 - p0, int(lens[p0:p1].max())
                if host:
                    emb = torch.nn.functional.embedding(ids[p0:p1, :L], table) + pos[None, :L]
                    x = emb.reshape(n * L, cfg.d_t).to(device=self.dev, dtype=torch.float32)
                else:
                    x = torch.empty(n * L, cfg.d_t, dtype=torch.float32, device=self.dev)
                    ops.text_embed(ids[p0:p1].to(self.dev), table, pos, x, L)
                len_i32 = torch.tensor(lens[p0:p1], dtype=torch.int32, device=self.dev)
                self._text_blocks_plain(x, len_i32, n, L)
                self._text_eot_features(x, len_i32, n, L, out[p0:p1])
        return out

    def plain_text_features(self) -> torch.Tensor:
        """The classifier of `forward_plain`, [n_cls, e] un-normalised (the engine's own buffer): the caller's
        (`set_plain_text_features`), else the EOT features of the frozen-token pass, computed once per context."""
        n, e = self.cfg.n_cls, self.cfg.embed
        if not self.text_cache_ready:
            self.cache_text_kv()
        if self.plain_text_f is None:
            self.plain_text_f = self._text_eot_features(self.text_x_final, self.len_i32, n, self.Lmax,
                                                        torch.empty(n, e, dtype=torch.float32, device=self.dev))
        return self.plain_text_f if self.plain_text_override is None else self.plain_text_override

    def set_plain_text_features(self, features: Optional[torch.Tensor]) -> None:
        """The classifier of `forward_plain` becomes `features` [n_cls, e] (the head normalises them) instead of the
        engine's own prompts' text features, until None is passed; `cache_text_kv` leaves the override alone."""
        if features is None:
            self.plain_text_override = None
            return
        f = torch.as_tensor(features, dtype=torch.float32, device=self.dev)
        assert tuple(f.shape) == (self.cfg.n_cls, self.cfg.embed), f"features: [{self.cfg.n_cls}, {self.cfg.embed}]"
        self.plain_text_override = f.contiguous().clone()
