"""Several CoCoOp runs ("members") in one step (rpo_amd/coop_multi.py).  Mixed into
rpo_amd.engine.Engine, whose plain image tower, dense / shared-prefix text rows (engine_coop.py, engine_coop_prefix.py) and
grouped head these methods use.

For CoCoOp a replica of `coop_setup` is an image of the batch: the class set runs once per replica with that replica's own
context `c_shift[r]`, forward and backward.  Nothing in that pass knows whose image a replica is, so S members of b images
are S * b replicas, member-major (image i of member s is replica s * b + i).  What a member owns is a meta-net and a
context: row s of `cm_params` [S, set_stride] = [ctx | w1 | b1 | w2 | b2], a standalone run's flat `coop_params`, with
`cm_grads` and the optimiser state in the same layout.  The four launches that know about members are
rpo_amd/csrc/cocoop_sets.hip's; the head is rpo_head_fwd_bwd_grouped with S * b groups of one image.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from . import ops

MAX_REPLICAS = 256                  # S * b: the replicas rpo_metanet_fwd's LDS limit allows a pass


def cocoop_row_layout(n_ctx: int, e: int, h: int, d: int) -> Tuple[int, Dict[str, int], int]:
    """(row length, offsets, set_stride) of a member's row [ctx (n_ctx d) | w1 (h e) | b1 (h) | w2 (d h) | b2 (d)] -- the
    order of `coop_setup`'s flat `coop_params`.  set_stride: the row length rounded up to 4 floats, so that every row
    starts on the 16-byte grid.  Pure host arithmetic (include/rpo_amd.h, rpo_metanet_fwd_sets)."""
    sizes = (("ctx", n_ctx * d), ("w1", h * e), ("b1", h), ("w2", d * h), ("b2", d))
    offs, at = {}, 0
    for name, n in sizes:
        offs[name] = at
        at += n
    return at, offs, (at + 3) // 4 * 4


class CocoopMultiEngineMixin:
    cm_S = 0                            # S of `cocoop_multi_setup`, 0 before it

    def cocoop_multi_setup(self, S: int, b: int, n_ctx: int, shared_prefix: bool = False) -> None:
        """Buffers of the step of S CoCoOp members with b images each: `coop_setup` for S * b replicas (the row buffers of
        the text pass, dense or shared-prefix, and the standalone `coop_params` that `select_member` fills), the members'
        `cm_params` / `cm_grads` / `cm_moms` [S, set_stride] and the grouped head's workspace."""
        cfg, dev = self.cfg, self.dev
        e, dt, n = cfg.embed, cfg.d_t, cfg.n_cls
        if S < 1 or b < 1:
            raise ValueError(f"cocoop_multi_setup: S = {S}, b = {b}: both must be >= 1")
        if S * b > self.max_batch:
            raise ValueError(f"cocoop_multi_setup: S * b = {S * b} images per step, the engine was built with max_batch = "
                             f"{self.max_batch} (build it with max_batch >= S * b)")
        if S > 1024 or S * b > MAX_REPLICAS:
            raise ValueError(f"cocoop_multi_setup: S = {S}, S * b = {S * b}: at most 1024 members and {MAX_REPLICAS} replicas")
        h = e // 16                                                          # vis_dim // 16 (trainers/cocoop.py:94)
        self.coop_setup(n_ctx, replicas=S * b, meta_hidden=h, shared_prefix=shared_prefix)
        length, offs, stride = cocoop_row_layout(n_ctx, e, h, dt)
        assert length == self.coop_params.numel()
        self.cm_S, self.cm_b, self.cm_len, self.cm_stride, self.cm_offs = S, b, length, stride, offs
        z = lambda: torch.zeros(S, stride, dtype=torch.float32, device=dev)
        self.cm_params, self.cm_grads, self.cm_moms = z(), z(), z()
        self.cm_loss = torch.zeros(S, dtype=torch.float32, device=dev)
        self.cm_head_ws = torch.empty(S * b * ops.head_workspace_floats(1, n, 1, e), dtype=torch.float32, device=dev)

    def cocoop_member_views(self, s: int, buf: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Member s's five tensors as views of its row of `buf` (default `cm_params`): ctx [n_ctx, d], w1 [h, e], b1 [h],
        w2 [d, h], b2 [d]."""
        cfg, o = self.cfg, self.cm_offs
        e, dt, h, nc = cfg.embed, cfg.d_t, self.coop_hidden, self.coop_n_ctx
        row = (self.cm_params if buf is None else buf)[s]
        shapes = dict(ctx=(nc, dt), w1=(h, e), b1=(h,), w2=(dt, h), b2=(dt,))
        return {k: row[o[k]:o[k] + math.prod(sh)].view(*sh) for k, sh in shapes.items()}

    def cocoop_multi_forward_backward(self, image: torch.Tensor, label: Optional[torch.Tensor]) -> torch.Tensor:
        """`cocoop_forward_backward` for S members: image [S * b, 3, R, R] and label [S * b] member-major.  One plain image
        pass, the members' meta-nets and shifted contexts in one launch each, one text pass over S * b replicas, one grouped
        head call; with `label` one text backward, the members' gradient tail and meta-net backward in one launch each ->
        `cm_grads` [S, set_stride] and `cm_loss` [S] (each member's mean over its own b images).  Capturable in a HIP
        graph.  Returns logits [S * b, n_cls] (the engine's buffer)."""
        cfg = self.cfg
        S, b, nc = self.cm_S, self.cm_b, self.coop_n_ctx
        e, n = cfg.embed, cfg.n_cls
        R = S * b
        train = label is not None
        B = self._plain_image_features(image)
        assert S > 0 and B == R, f"cocoop_multi_forward_backward takes S * b = {R} images, member-major"
        ops.metanet_fwd_sets(self.img_cls_f[:R], self.cm_params, nc, self.c_fn[:R], self.c_hid[:R], self.c_bias[:R], b)
        ops.cocoop_shift_sets(self.cm_params, self.c_bias[:R], self.c_shift[:R], b)
        self._coop_text_forward(train, R)
        # every image has its own text features (trainers/cocoop.py:183-188): S * b heads of one image each, one call
        extra = {} if (not train or self.act == torch.float32) else dict(d_text_f_act=self.c_d_text_f_a[:R * n])
        ops.head_fwd_bwd_grouped(self.img_cls_f[:R].view(R, 1, e), self.c_text_f[:R * n].view(R * n, 1, e), label,
                                 self.logit_scale_exp, self.logits[:R], self.c_loss_b[:R] if train else None,
                                 self.c_d_img_f[:R].view(R, 1, e) if train else None,
                                 self.c_d_text_f[:R * n].view(R * n, 1, e) if train else None, self.cm_head_ws, R, **extra)
        if train:
            self._coop_text_backward(R)
            ops.cocoop_grad_tail_sets(self.c_dshift[:R], self.c_loss_b[:R], self.cm_grads, self.c_dbias[:R], self.cm_loss, b)
            ops.metanet_bwd_sets(self.c_dbias[:R], self.c_fn[:R], self.c_hid[:R], self.cm_params, self.cm_grads, nc, b)
        return self.logits[:R]

    def select_member(self, s: int) -> None:
        """Member s's row into the standalone `coop_params` (one device copy): `cocoop_forward_backward`, the conditional
        class sets and everything else that reads `coop_ctx` / `meta` then evaluate member s."""
        if not 0 <= s < self.cm_S:
            raise IndexError(f"member {s} of {self.cm_S}")
        self.coop_params.copy_(self.cm_params[s, :self.cm_len])
