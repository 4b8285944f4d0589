"""CoOp and CoCoOp TRAINING on the shared-prefix row layout: `coop_setup(..., shared_prefix=True)`.

The prompt of replica r and class c is [SOS | ctx_r (n_ctx rows) | name . EOT] ("end", generic context; CoOp: one replica,
CoCoOp: one per image with ctx + bias[r]) under CLIP's plain causal mask, so the first P = 1 + n_ctx rows read only
themselves and are, through every text block, the same for all classes of a replica.  The dense path
(engine_coop.py) computes them once per class anyway: R * n_cls * Lmax rows forward and backward.  Here they are kept once
per replica -- the layout of rpo_text_attn_fwd_prefix (engine_cocoop_eval.py, section 9p):

    prefix row (r, p)    at r * P + p                            position p of every sequence of replica r
    suffix row (r, c, s) at R * P + (r * n_cls + c) * S + s      position P + s of sequence (r, c),  S = Lmax - P

R * (P + n_cls * S) rows.  LayerNorm and the GEMMs are row-wise and run over the one row set unchanged; only attention
knows about the sharing.  In the backward, rpo_text_attn_bwd_prefix sums the prefix keys' dK / dV over the classes where
the sharing is, in every block; LayerNorm backward and the dX GEMMs are linear in the incoming gradient for fixed
activations, so the dX of a shared row is the sum of its dense copies' dX and d loss / d ctx_r is simply dX at prefix rows
1 .. P - 1 of replica r: no rpo_reduce_groups over the classes at the end.  The EOT rows are always suffix rows.

`PrefixTrainEngineMixin` is mixed into rpo_amd.engine.Engine; `_coop_text_forward` / `_coop_text_backward` hand over to it
when the engine was set up with `shared_prefix=True`, so everything around them (side stream, head, meta-net, the ctx /
bias sums, the eval branch, `classifier`) is the dense path's own code.
"""
from __future__ import annotations

import torch

from . import ops
from .engine_coop import shared_eot_rows, shared_fill, shared_split
from .engine_text import SCALE


class PrefixTrainEngineMixin:
    def _coop_prefix_setup(self, n_ctx: int, replicas: int) -> None:
        """What the shared layout adds to coop_setup's buffers (already sized to its row count): the frozen rows every
        pass starts from, the EOT rows for every replica count, and the attention backward's workspace."""
        cfg, dev = self.cfg, self.dev
        n, L = cfg.n_cls, self.Lmax
        P = self.coop_P = 1 + n_ctx
        S = self.coop_S = L - P
        self.c_x_sos, self.c_x_suffix = shared_split(self.text_x_frozen, n, L, P)
        self.c_eot_shared = [None] + [torch.as_tensor(shared_eot_rows(R, P, S, self.len_np), device=dev)
                                      for R in range(1, replicas + 1)]
        self.c_attn_ws = torch.empty(max(1, ops.text_attn_bwd_prefix_workspace_floats(replicas, n, P, cfg.heads_t)),
                                     dtype=torch.float32, device=dev)

    def _coop_prefix_forward(self, train: bool, R: int = 1) -> None:
        """`_coop_text_forward` on the shared rows: prefix rows [SOS + pos[0] | c_shift[r] + pos[1:P]] per replica, the
        frozen embedded positions >= P behind them, `_coop_blocks_forward` with rpo_text_attn_fwd_prefix."""
        n, H, P, S = self.cfg.n_cls, self.cfg.heads_t, self.coop_P, self.coop_S
        Rf = R * (P + n * S)
        shared_fill(self.cx[0][:Rf], R, P, self.c_x_sos, self.c_shift[:R], self.text_pos, self.c_x_suffix)
        self._coop_blocks_forward(train, Rf, R * n, self.c_eot_shared[R], lambda q, k, v, out: ops.text_attn_fwd_prefix(
            q, k, v, out, self.len_i32, R, n, P, S, H, SCALE))

    def _coop_prefix_backward(self, R: int = 1) -> None:
        """`_coop_blocks_backward` over the shared rows with rpo_text_attn_bwd_prefix; c_dshift[r] = dX at prefix rows
        1 .. P - 1 of replica r (already summed over the classes)."""
        n, dt, H, P, S = self.cfg.n_cls, self.cfg.d_t, self.cfg.heads_t, self.coop_P, self.coop_S
        dxa = self._coop_blocks_backward(
            R * (P + n * S), R * n, self.c_eot_shared[R], lambda q, k, v, da, dq, dk, dv: ops.text_attn_bwd_prefix(
                q, k, v, da, dq, dk, dv, self.len_i32, R, n, P, S, H, SCALE, workspace=self.c_attn_ws))
        self.c_dshift[:R].copy_(dxa[:R * P].view(R, P, dt)[:, 1:])
