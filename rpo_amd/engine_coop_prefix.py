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

import numpy as np
import torch

from . import ops
from ._lib import EPI_BIAS, EPI_BIAS_QGELU, EPI_BIAS_RESID, EPI_NONE, EPI_QGELU_BWD
from .engine_coop import SCALE, SPLIT_FC, SPLIT_Q


class PrefixTrainEngineMixin:
    def _coop_prefix_setup(self, n_ctx: int, replicas: int) -> None:
        """What the shared layout adds to coop_setup's buffers (already sized to its row count): the frozen rows every
        pass starts from, the EOT rows for every replica count, and the attention backward's workspace."""
        cfg, dev = self.cfg, self.dev
        n, L, dt = cfg.n_cls, self.Lmax, cfg.d_t
        P = self.coop_P = 1 + n_ctx
        S = self.coop_S = L - P
        x = self.text_x_frozen.view(n, L, dt)
        self.c_x_sos = x[0, 0].clone()                                     # SOS embedding + pos[0]: the same for every class
        self.c_x_suffix = x[:, P:].reshape(n * S, dt).contiguous()         # token + positional rows of the positions >= P
        # EOT row of every (replica, class) of a pass over R replicas: the prefix block in front grows with R
        off = np.arange(n, dtype=np.int64) * S + (self.len_np.astype(np.int64) - 1 - P)
        assert int(off.min()) >= 0 and int((self.len_np - P).max()) <= S
        self.c_eot_shared = [None] + [
            torch.as_tensor((R * P + np.arange(R, dtype=np.int64)[:, None] * (n * S) + off[None, :]).reshape(-1), device=dev)
            for R in range(1, replicas + 1)]
        self.c_attn_ws = torch.empty(max(1, ops.text_attn_bwd_prefix_workspace_floats(replicas, n, P, cfg.heads_t)),
                                     dtype=torch.float32, device=dev)

    def _coop_prefix_forward(self, train: bool, R: int = 1) -> None:
        """`_coop_text_forward` on the shared rows: prefix rows [SOS + pos[0] | c_shift[r] + pos[1:P]] per replica, the
        frozen embedded positions >= P behind them, the blocks as in `_cocoop_prefix_pass` with every block's inputs kept
        when training."""
        cfg = self.cfg
        n, dt, H, P, S = cfg.n_cls, cfg.d_t, cfg.heads_t, self.coop_P, self.coop_S
        nv = R * n
        Rf = R * (P + n * S)
        x0 = self.cx[0][:Rf]
        xp = x0[:R * P].view(R, P, dt)
        xp[:, 0] = self.c_x_sos
        torch.add(self.c_shift[:R], self.text_pos[1:P], out=xp[:, 1:])
        x0[R * P:].view(R, n * S, dt).copy_(self.c_x_suffix.unsqueeze(0).expand(R, -1, -1))
        ch, catt, cg, ln = self.ch[:Rf], self.catt[:Rf], self.cg[:Rf], self.len_i32
        for l, blk in enumerate(self.txt):
            x, xm, qkv = self.cx[l][:Rf], self.cxm[l][:Rf], self.cqkv[l][:Rf]
            ops.layernorm_fwd(x, blk.ln1_w, blk.ln1_b, ch)
            ops.gemm_nt(ch, blk.w_in, qkv, EPI_BIAS, bias=blk.b_in)
            ops.text_attn_fwd_prefix(qkv[:, :dt], qkv[:, dt:2 * dt], qkv[:, 2 * dt:], catt, ln, R, n, P, S, H, SCALE)
            ops.gemm_nt(catt, blk.w_out, xm, EPI_BIAS_RESID, bias=blk.b_out, resid=x)
            ops.layernorm_fwd(xm, blk.ln2_w, blk.ln2_b, ch)
            ops.gemm_nt(ch, blk.w_fc, cg, EPI_BIAS_QGELU, bias=blk.b_fc, aux=self.cu[l][:Rf] if train else None,
                        aux_row0=0 if train else Rf)
            ops.gemm_nt(cg, blk.w_proj, self.cx[l + 1][:Rf], EPI_BIAS_RESID, bias=blk.b_proj, resid=xm)
        torch.index_select(self.cx[-1], 0, self.c_eot_shared[R], out=self.c_x_eot[:nv])      # feature at the EOT token
        ops.layernorm_fwd(self.c_x_eot[:nv], self.ln_final[0], self.ln_final[1], self.c_y_eot[:nv])
        ops.gemm_nt(self.c_y_eot[:nv], self.text_proj_t, self.c_text_f[:nv], EPI_NONE)

    def _coop_prefix_backward(self, R: int = 1) -> None:
        """`_coop_text_backward`'s chain over the shared rows with rpo_text_attn_bwd_prefix in place of the dense attention
        backward; c_dshift[r] = dX at prefix rows 1 .. P - 1 of replica r (already summed over the classes)."""
        cfg = self.cfg
        n, dt, H, P, S = cfg.n_cls, cfg.d_t, cfg.heads_t, self.coop_P, self.coop_S
        nv = R * n
        Rf = R * (P + n * S)
        f32m = self.act == torch.float32
        dxa, dxb, dxc, dy = self.c_dxa[:Rf], self.c_dxb[:Rf], self.c_dxc[:Rf], self.c_dy[:, :Rf]
        du, da, dq, ln = self.c_du[:Rf], self.c_da[:Rf], self.c_dqkv[:Rf], self.len_i32
        ops.gemm_nt(self.c_d_text_f[:nv] if f32m else self.c_d_text_f_a[:nv], self.text_proj, self.c_dy_eot[:nv], EPI_NONE)
        ops.layernorm_bwd(self.c_dy_eot[:nv], self.c_x_eot[:nv], self.ln_final[0], None, self.c_dx_eot[:nv])
        dxa.zero_()
        dxa.index_copy_(0, self.c_eot_shared[R], self.c_dx_eot[:nv])
        if not f32m:
            ops.convert(dxa, dxc)
        for l in reversed(range(len(self.txt))):
            blk, qkv = self.txt[l], self.cqkv[l][:Rf]
            ops.gemm_nt(dxa if f32m else dxc, blk.w_proj_t, du, EPI_QGELU_BWD, aux=self.cu[l][:Rf])
            ops.gemm_nt(du, blk.w_fc_t, dy[:SPLIT_FC], EPI_NONE, split_k=SPLIT_FC)
            ops.layernorm_bwd(dy[:SPLIT_FC], self.cxm[l][:Rf], blk.ln2_w, dxa, dxb, None if f32m else dxc)
            ops.gemm_nt(dxb if f32m else dxc, blk.w_out_t, da, EPI_NONE)
            ops.text_attn_bwd_prefix(qkv[:, :dt], qkv[:, dt:2 * dt], qkv[:, 2 * dt:], da, dq[:, :dt], dq[:, dt:2 * dt],
                                     dq[:, 2 * dt:], ln, R, n, P, S, H, SCALE, workspace=self.c_attn_ws)
            ops.gemm_nt(dq, self.c_w_in_t[l], dy[:SPLIT_Q], EPI_NONE, split_k=SPLIT_Q)
            ops.layernorm_bwd(dy[:SPLIT_Q], self.cx[l][:Rf], blk.ln1_w, dxb, dxa, None if f32m else dxc)
        self.c_dshift[:R].copy_(dxa[:R * P].view(R, P, dt)[:, 1:])
