"""The linear probe's share of the engine (trainers/linear_prob.py): frozen plain CLIP towers, a trained dense e x e layer
plus bias on the UN-normalised image feature, logits against text features computed once.  Mixed into
rpo_amd.engine.Engine, whose plain image tower, text cache and streams these methods use; nothing here is allocated
unless `lp_setup` is called."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from ._lib import EPI_NONE


class LpEngineMixin:
    def lp_setup(self) -> None:
        """Buffers of the linear probe: the trained layer as ONE flat fp32 buffer `lp_params` = [W (e x e, out x in) | b (e)]
        with matching gradient and momentum buffers (one SGD launch, one all-reduce, no copies: rpo_lp_head_fwd_bwd writes
        g_w and g_bias into `lp_grads` directly), the normalised text features [n_cls, e] (preprocess, :77-83: once), and
        the head's z / workspace sized for max_batch."""
        cfg, dev = self.cfg, self.dev
        e, n = cfg.embed, cfg.n_cls
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        tot = e * e + e
        self.lp_params = torch.zeros(tot, dtype=torch.float32, device=dev)
        self.lp_grads = torch.zeros(tot, dtype=torch.float32, device=dev)
        self.lp_moms = torch.zeros(tot, dtype=torch.float32, device=dev)
        self.lp_w, self.lp_b = self.lp_params[:e * e].view(e, e), self.lp_params[e * e:]
        self.lp_gw, self.lp_gb = self.lp_grads[:e * e].view(e, e), self.lp_grads[e * e:]
        self.lp_z = f32(self.max_batch, e)
        self.lp_ws = f32(ops.lp_head_workspace_floats(self.max_batch, n, e))
        if self.img_cls_f is None:
            self.img_cls_f = f32(self.max_batch, e)
        self.lp_text_f_n = self._lp_text_features()

    def _lp_text_features(self) -> torch.Tensor:
        """TextEncoder on the prompts of the caller's token ids (EOT row -> ln_final -> text_projection, :47-58), divided by
        its norm (:81): the plain text tower of the frozen-token pass, as forward_plain computes it."""
        cfg = self.cfg
        n, e = cfg.n_cls, cfg.embed
        if not self.text_cache_ready:
            self.cache_text_kv()
        rows = torch.arange(n, device=self.dev) * self.Lmax + (self.len_i32.to(torch.int64) - 1)   # EOT positions
        eot = self.text_x_final.index_select(0, rows).contiguous()
        y = torch.empty(n, cfg.d_t, dtype=self.act, device=self.dev)
        ops.layernorm_fwd(eot, self.ln_final[0], self.ln_final[1], y)
        tf = torch.empty(n, e, dtype=torch.float32, device=self.dev)
        ops.gemm_nt(y, self.text_proj_t, tf, EPI_NONE)
        return (tf / tf.norm(dim=-1, keepdim=True)).contiguous()

    def lp_forward_backward(self, image: torch.Tensor, label: Optional[torch.Tensor]) -> torch.Tensor:
        """trainers/linear_prob.py:85-95 (+ F.cross_entropy and backward, :176-178): logits = exp(logit_scale) *
        lp_layer(encode_image(image)) @ text_features^T; with `label` also the mean cross-entropy (self.loss) and the
        gradient of [W | b] (self.lp_grads).  Capturable in a HIP graph.  Returns self.logits[:B]."""
        B = self._plain_image_features(image)
        train = label is not None
        ops.lp_head_fwd_bwd(self.img_cls_f[:B], self.lp_w, self.lp_b, self.lp_text_f_n, label, self.logit_scale_exp,
                            self.lp_z[:B], self.logits[:B], self.loss if train else None, self.lp_gw if train else None,
                            self.lp_gb if train else None, self.lp_ws)
        return self.logits[:B]

    # ---- the members of a sweep (rpo_amd/lp_sweep.py): S layers behind ONE image pass -------------
    def lp_sweep_setup(self, S: int) -> None:
        """Buffers of S linear probes on the shared image feature: `lps_params` / `lps_grads` / `lps_moms` [S, stride] fp32,
        row s = [W_s (e x e, out x in) | b_s (e)] (stride = e e + e, a multiple of 32: every row is 16-byte aligned and the
        rows are the optimiser's sets), `lps_z` [S, max_batch, e], `lps_logits` [S, max_batch, n_cls], `lps_loss` [S] and
        the grouped head's workspace.  Nothing here is allocated unless this is called; `lp_setup`'s buffers stay as they
        are (the text features are its own, shared)."""
        cfg, dev = self.cfg, self.dev
        e, n, mb = cfg.embed, cfg.n_cls, self.max_batch
        if not 1 <= S <= 1024:
            raise ValueError(f"lp_sweep_setup: {S} members (rpo_lp_head_fwd_bwd_grouped takes 1 .. 1024 groups)")
        if getattr(self, "lp_text_f_n", None) is None:
            self.lp_setup()
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        self.lps_S, self.lps_stride = S, e * e + e
        self.lps_params = torch.zeros(S, self.lps_stride, dtype=torch.float32, device=dev)
        self.lps_grads = torch.zeros(S, self.lps_stride, dtype=torch.float32, device=dev)
        self.lps_moms = torch.zeros(S, self.lps_stride, dtype=torch.float32, device=dev)
        self.lps_w = self.lps_params[:, :e * e].view(S, e, e)                # (views: member s's weight [e, e], bias [e])
        self.lps_b = self.lps_params[:, e * e:]
        self.lps_z, self.lps_logits, self.lps_loss = f32(S, mb, e), f32(S, mb, n), torch.zeros(S, dtype=torch.float32, device=dev)
        self.lps_ws = f32(S * ops.lp_head_workspace_floats(mb, n, e))

    def lp_sweep_forward_backward(self, image: torch.Tensor, label: Optional[torch.Tensor]) -> torch.Tensor:
        """`lp_forward_backward` for the S members: ONE plain image pass, ONE grouped head call (four launches, two for
        eval, whatever S is).  With `label`, `lps_loss` [S] and `lps_grads` [S, stride]; member s's bits are those of
        `lp_forward_backward` with its layer.  Capturable in a HIP graph.  Returns logits [S, B, n_cls], the leading
        S B n_cls floats of `lps_logits` (valid until the next call)."""
        B = self._plain_image_features(image)
        S, train = self.lps_S, label is not None
        e, n = self.cfg.embed, self.cfg.n_cls
        z = self.lps_z.view(-1)[:S * B * e].view(S, B, e)                     # (the call's arrays are dense in B)
        logits = self.lps_logits.view(-1)[:S * B * n].view(S, B, n)
        ops.lp_head_fwd_bwd_grouped(self.img_cls_f[:B], self.lps_params, self.lp_text_f_n, label, self.logit_scale_exp,
                                    z, logits, self.lps_loss if train else None, self.lps_grads if train else None,
                                    self.lps_ws)
        return logits
