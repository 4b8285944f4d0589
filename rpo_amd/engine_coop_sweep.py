"""Several CoOp runs ("members") with their own n_ctx on ONE shared image pass (rpo_amd/coop_sweep.py).
Mixed into rpo_amd.engine.Engine, whose plain image tower, dense / shared-prefix text rows (engine_coop.py,
engine_coop_prefix.py) and grouped head these methods use.

For CoOp, as for the linear probe, the image feature depends on nothing that is trained: S members on the same batch need
one plain image pass.  What a member owns is a context: row s of `cs_params` [S, set_stride], its first n_s * d_t floats (a
standalone ``CoOp(n_ctx=n_s)``'s flat `coop_params`), with `cs_grads` and the optimiser state in the same layout.  For the
text pass a member is a replica of `coop_setup`: the class set runs once per member with that member's context.  The engine
is built with the prompts of n_max placeholders; a member with fewer has its class-name tokens delta = n_max - n_s positions
earlier and sequences delta shorter -- rpo_amd/csrc/coop_sets.hip builds those rows and reduces their gradients for all
members in one launch each, and the attention and the EOT tail take per-(member, class) lengths as they are.  On the
shared-prefix layout (every member at n_max only) the existing prefix path with R = S serves as it is.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .engine_text import SCALE

MAX_MEMBERS = 256                   # the replicas a text pass takes


def sweep_row_layout(n_max: int, d: int) -> Tuple[int, int]:
    """(row length, set_stride) of a member's row: n_max * d floats, rounded up to 4 floats so that every row starts on the
    16-byte grid.  Pure host arithmetic."""
    length = int(n_max) * int(d)
    return length, (length + 3) // 4 * 4


def sweep_used(n_ctx_members: Sequence[int], d: int) -> np.ndarray:
    """The optimiser's `used` table int32 [S, 2]: member s updates the first n_s * d floats of its row (segment 0) and
    nothing of segment 1 (there is none)."""
    return np.array([[int(n) * int(d), 0] for n in n_ctx_members], dtype=np.int32)


def member_lengths(lengths, n_max: int, n_ctx_members: Sequence[int]) -> np.ndarray:
    """int64 [S, n_cls]: the prompt lengths (SOS .. EOT) of every member -- those of the n_max prompts minus the
    placeholders the member does not have."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(1, -1)
    delta = int(n_max) - np.asarray(n_ctx_members, dtype=np.int64).reshape(-1, 1)
    return lengths - delta


def member_eot_rows(lengths, n_max: int, n_ctx_members: Sequence[int], L: int) -> np.ndarray:
    """int64 [S * n_cls]: the EOT row of every (member, class) in the dense member-major layout of L positions."""
    ml = member_lengths(lengths, n_max, n_ctx_members)
    S, n = ml.shape
    return ((np.arange(S * n, dtype=np.int64) * int(L)).reshape(S, n) + ml - 1).reshape(-1)


class CoopSweepEngineMixin:
    cs_S = 0                            # S of `coop_sweep_setup`, 0 before it

    def coop_sweep_setup(self, S: int, n_ctx_members: Sequence[int], shared_prefix: bool = False,
                         batch: Optional[int] = None) -> None:
        """Buffers of the step of S CoOp members on one batch of up to `batch` images (default: max_batch): `coop_setup`
        for n_max = max(n_ctx_members) and S replicas, the members' `cs_params` / `cs_grads` / `cs_moms` [S, set_stride],
        their lengths and EOT rows, and the grouped head's inputs, outputs and workspace for S groups of `batch` images."""
        cfg, dev = self.cfg, self.dev
        e, dt, n, L = cfg.embed, cfg.d_t, cfg.n_cls, self.Lmax
        nc = [int(v) for v in n_ctx_members]
        if S < 1 or S > MAX_MEMBERS or len(nc) != S:
            raise ValueError(f"coop_sweep_setup: S = {S} with {len(nc)} n_ctx values: 1 <= S <= {MAX_MEMBERS}, one n_ctx each")
        if S > self.max_batch:
            raise ValueError(f"coop_sweep_setup: S = {S} members, the engine was built with max_batch = {self.max_batch} "
                             "(coop_setup takes at most max_batch replicas: build it with max_batch >= S)")
        n_max = max(nc)
        if min(nc) < 1:
            raise ValueError(f"coop_sweep_setup: n_ctx of the members {nc}: every member needs at least one context vector")
        if shared_prefix and any(v != n_max for v in nc):
            raise ValueError(f"coop_sweep_setup: shared_prefix=True with members of different n_ctx {nc}: the prefix length "
                             "P = 1 + n_ctx is per pass")
        Bc = self.max_batch if batch is None else int(batch)
        assert 1 <= Bc <= self.max_batch
        self.coop_setup(n_max, replicas=S, shared_prefix=shared_prefix)
        length, stride = sweep_row_layout(n_max, dt)
        self.cs_S, self.cs_B, self.cs_n_max, self.cs_n_ctx, self.cs_len_row, self.cs_stride = S, Bc, n_max, nc, length, stride
        z = lambda: torch.zeros(S, stride, dtype=torch.float32, device=dev)
        self.cs_params, self.cs_grads, self.cs_moms = z(), z(), z()
        self.cs_nctx = torch.tensor(nc, dtype=torch.int32).to(dev)
        ml = member_lengths(self.len_np, n_max, nc)
        self.cs_len = torch.as_tensor(ml.reshape(-1).astype(np.int32)).to(dev)
        self.cs_eot = torch.as_tensor(member_eot_rows(self.len_np, n_max, nc, L)).to(dev)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        self.cs_loss = torch.zeros(S, dtype=torch.float32, device=dev)
        self.cs_img_f, self.cs_d_img_f = f32(S * Bc, e), f32(S * Bc, e)
        self.cs_label = torch.zeros(S * Bc, dtype=torch.int64, device=dev)
        self.cs_logits = f32(S * Bc, n)
        self.cs_head_ws = f32(S * ops.head_workspace_floats(Bc, n, 1, e))

    def coop_sweep_member_ctx(self, s: int, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Member s's context [n_s, d_t] as a view of its row of `buf` (default `cs_params`)."""
        if not 0 <= s < self.cs_S:
            raise IndexError(f"member {s} of {self.cs_S}")
        ns, dt = self.cs_n_ctx[s], self.cfg.d_t
        return (self.cs_params if buf is None else buf)[s, :ns * dt].view(ns, dt)

    def _coop_sweep_text_forward(self, train: bool) -> None:
        """cs_params -> c_text_f[:S * n_cls]: the text pass over the S members as replicas."""
        cfg = self.cfg
        S, n, L, dt, H, n_max = self.cs_S, cfg.n_cls, self.Lmax, cfg.d_t, cfg.heads_t, self.cs_n_max
        if self.coop_shared:
            self.c_shift[:S].view(S, n_max * dt).copy_(self.cs_params[:, :n_max * dt])
            return self._coop_text_forward(train, S)
        nv = S * n
        Rf = nv * L
        ops.coop_fill_sets(self.text_tok, self.text_pos, self.cs_params, self.cs_nctx, self.cx[0][:Rf], n, L, n_max)
        ln = self.cs_len
        self._coop_blocks_forward(train, Rf, nv, self.cs_eot, lambda q, k, v, out: ops.text_attn_fwd(
            q, k, v, out, ln, nv, L, L, H, causal=True, scale=SCALE))

    def _coop_sweep_text_backward(self) -> None:
        """c_d_text_f[:S * n_cls] -> the first n_max * d_t floats of every row of cs_grads."""
        cfg = self.cfg
        S, n, L, dt, H, n_max = self.cs_S, cfg.n_cls, self.Lmax, cfg.d_t, cfg.heads_t, self.cs_n_max
        if self.coop_shared:
            self._coop_text_backward(S)
            self.cs_grads[:, :n_max * dt].copy_(self.c_dshift[:S].view(S, n_max * dt))
            return
        nv = S * n
        Rf = nv * L
        ln = self.cs_len
        dxa = self._coop_blocks_backward(Rf, nv, self.cs_eot, lambda q, k, v, da, dq, dk, dv: ops.text_attn_bwd_dense(
            q, k, v, da, dq, dk, dv, ln, nv, L, H, SCALE))
        ops.coop_ctx_grad_sets(dxa, self.cs_grads, self.cs_nctx, n, L, n_max)

    @torch.no_grad()
    def coop_sweep_text_features(self) -> torch.Tensor:
        """The members' text features [S, n_cls, e] (un-normalised, the engine's buffer): one eval text pass."""
        self._coop_sweep_text_forward(False)
        return self.c_text_f[:self.cs_S * self.cfg.n_cls].view(self.cs_S, self.cfg.n_cls, self.cfg.embed)

    def coop_sweep_forward_backward(self, image: torch.Tensor, label: Optional[torch.Tensor]) -> torch.Tensor:
        """`coop_forward_backward` for S members on ONE batch: the text forward over S replicas on the side stream under
        the one plain image pass (RPO_COOP_SERIAL=1: one stream), the B image features broadcast to [S * B, e], one grouped
        head call with S groups of B images; with `label` one text backward over S replicas and the members' context
        gradients -> `cs_grads` [S, set_stride] and `cs_loss` [S].  Launches do not grow with S.  Capturable in a HIP graph.
        Returns logits [S, B, n_cls] (the engine's buffer)."""
        cfg = self.cfg
        S, e, n = self.cs_S, cfg.embed, cfg.n_cls
        assert S > 0, "coop_sweep_setup first"
        train = label is not None
        if os.environ.get("RPO_COOP_SERIAL") == "1":
            self._coop_sweep_text_forward(train)
            B = self._plain_image_features(image)
        else:
            main = torch.cuda.current_stream()
            self.side.wait_stream(main)
            with torch.cuda.stream(self.side):
                self._coop_sweep_text_forward(train)
            B = self._plain_image_features(image)
            main.wait_stream(self.side)
        assert B <= self.cs_B, f"coop_sweep_forward_backward takes up to {self.cs_B} images (coop_sweep_setup's batch)"
        R = S * B
        ops.broadcast_rows(self.img_cls_f[:B], self.cs_img_f[:R], S)
        if train:
            self.cs_label[:R].view(S, B).copy_(label.view(1, B).expand(S, B))
        extra = {} if (not train or self.act == torch.float32) else dict(d_text_f_act=self.c_d_text_f_a[:S * n])
        ops.head_fwd_bwd_grouped(self.cs_img_f[:R].view(R, 1, e), self.c_text_f[:S * n].view(S * n, 1, e),
                                 self.cs_label[:R] if train else None, self.logit_scale_exp, self.cs_logits[:R],
                                 self.cs_loss if train else None, self.cs_d_img_f[:R].view(R, 1, e) if train else None,
                                 self.c_d_text_f[:S * n].view(S * n, 1, e) if train else None, self.cs_head_ws, S, **extra)
        if train:
            self._coop_sweep_text_backward()
        return self.cs_logits[:R].view(S, B, n)
