"""Several RPO runs ("members": seeds of one recipe) in one step on the shared frozen towers.  Mixed into
rpo_amd.engine.Engine, whose packed weights, K / V cache, image-tower workspace and streams these methods use.

Nothing reads a prompt, so the frozen image rows, the text K / V cache and every weight are the
same for any number of prompt sets: S runs of batch B are, for the image tower, ONE batch of S * B images whose prompt
rows come from S `img_prompt` tensors (image b belongs to member b // B), and for the text tower S * n_cls virtual
classes that all read the one cache of the n_cls real classes.  The towers' kernels treat every image and every class
independently; the seams are the embedding, the text attention's cache lookup, the head and the gradient sums, which the
engine's own methods take from the grouped entry points while `_multi` is set (include/rpo_amd.h, "ABI 8 additions").

Layout: `m_params` / `m_grads` / `m_mom` are [S, K*d_t + K*d_v] fp32 -- row s is member s's flat [text | img] vector,
exactly a standalone engine's `params` -- so one `rpo_sgd_step` over the flat buffer steps every member, and a member's
row can be copied into `params` to run the single-run eval path with its prompts.  The image workspace is the engine's
own (it must have been built with max_batch >= S * B: the GEMM plans and row-unit hints are then those of
M = S * B * (N + K)); the text tower's per-step buffers, sized for S * n_cls * K rows, exist only after `multi_setup`.
"""
from __future__ import annotations

import contextlib
import os

import torch

from . import ops

SCALE = 0.125                       # 1 / sqrt(head_dim = 64)

# the text tower's per-step buffers (Engine._alloc) that the multi-run step replaces by its own, S times as many rows
_TEXT_BUFS = ("xt", "xtm", "ht", "qt", "att_t", "gt", "ut", "y_final", "text_f", "d_text_f", "d_text_f_a", "ln_stats_t",
              "dy_t", "dxa_t", "dxb_t", "dxc_t", "du_t", "da_t", "dq_t")


class MultiEngineMixin:
    _multi = None                       # S while a multi-run step is being enqueued (`_multi_mode`), else None
    multi_S = 0                         # S of `multi_setup`, 0 before it

    m_k_used = None                     # int32 [S] on the device: the members' own K (`multi_setup(..., member_K=)`), or None

    def multi_setup(self, S: int, B: int, member_K=None) -> None:
        """Buffers of the multi-run step for S members of batch B.  Allocates nothing the single-run engine uses and
        changes none of its buffers.  `member_K`: per member, how many of the engine's K prompt pairs it uses (DESIGN.md
        section 9i) -- the heads then average over the member's own K_s (rpo_head_fwd_bwd_grouped_k) and the rows
        i >= K_s ("inert") start at zero, get zero gradients and ride along through the towers: a member with K_s < K
        costs what a K member costs.  Without it everything is as it was."""
        from .engine import SPLIT_FC, SPLIT_Q
        cfg, dev, act = self.cfg, self.dev, self.act
        self._refuse_rn("multi_setup")
        if S < 1 or B < 1:
            raise ValueError(f"multi_setup: S = {S}, B = {B}: both must be >= 1")
        if S * B > self.max_batch:
            raise ValueError(f"multi_setup: S * B = {S * B} images per step, the engine was built with max_batch = "
                             f"{self.max_batch} (build it with max_batch >= S * B: the image tower's plans are chosen for it)")
        K, dv, dt, e, n, Lt = cfg.K, cfg.d_v, cfg.d_t, cfg.embed, cfg.n_cls, cfg.layers_t
        if member_K is not None:
            member_K = [int(k) for k in member_K]
            if len(member_K) != S or any(not 1 <= k <= K for k in member_K):
                raise ValueError(f"multi_setup: member_K = {member_K} for S = {S} members of an engine with K = {K}: one "
                                 "value in [1, K] per member")
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        a = lambda *s: torch.empty(*s, dtype=act, device=dev)
        au = f32 if os.environ.get("RPO_AUX_F32") == "1" else a
        Rt = S * n * K
        m = dict(Rt=Rt)
        m["xt"] = [f32(Rt, dt) for _ in range(Lt + 1)]
        m["xtm"] = [f32(Rt, dt) for _ in range(Lt)]
        m["ht"] = a(Rt, dt)
        m["qt"] = [a(Rt, dt) for _ in range(Lt)]
        m["att_t"] = a(Rt, dt)
        m["gt"] = a(Rt, 4 * dt)
        m["ut"] = [au(Rt, 4 * dt) for _ in range(Lt)]
        m["y_final"] = a(Rt, dt)
        m["text_f"] = f32(Rt, e)
        m["d_text_f"] = f32(Rt, e)
        m["d_text_f_a"] = a(Rt, e)
        m["ln_stats_t"] = f32(Rt, dt // 64, 2)
        m["dy_t"] = f32(max(SPLIT_FC, SPLIT_Q, 4), Rt, dt)
        m["dxa_t"], m["dxb_t"] = f32(Rt, dt), f32(Rt, dt)
        m["dxc_t"] = a(Rt, dt)
        m["du_t"] = a(Rt, 4 * dt)
        m["da_t"], m["dq_t"] = a(Rt, dt), a(Rt, dt)
        m["_text_fc_units"] = self._text_fc_units_for(Rt)
        assert set(_TEXT_BUFS) <= set(m)
        self._multi_bufs = m
        self.multi_S, self.multi_B = S, B
        nt, ni = K * dt, K * dv
        self.m_params = f32(S, nt + ni)
        self.multi_K = member_K
        self.m_k_used = None
        if member_K is not None:
            self.m_params.zero_()                                    # (inert rows: finite whatever the caller sets later)
            self.m_k_used = torch.tensor(member_K, dtype=torch.int32, device=dev)
        self.m_grads = torch.zeros(S, nt + ni, dtype=torch.float32, device=dev)
        self.m_mom = torch.zeros(S, nt + ni, dtype=torch.float32, device=dev)
        # member s's prompts / gradients: column blocks of its row (sets strided by nt + ni floats)
        self.m_text_prompt = self.m_params[:, :nt].unflatten(1, (K, dt))
        self.m_img_prompt = self.m_params[:, nt:].unflatten(1, (K, dv))
        self.m_g_text = self.m_grads[:, :nt].unflatten(1, (K, dt))
        self.m_g_img = self.m_grads[:, nt:].unflatten(1, (K, dv))
        self.m_logits = f32(S * B, n)
        self.m_loss = f32(S)
        self.m_head_ws = f32(S * ops.head_workspace_floats(B, n, K, e))

    def _text_fc_units_for(self, Rt_: int) -> dict:
        """The row-unit hint of the text tower's c_fc at Rt_ prompt rows (Engine.__init__ says why and when), or {}."""
        tn = (4 * self.cfg.d_t) // 256
        u = next((u for u in range(288, 224, -1) if Rt_ % u == 0 and ((Rt_ // u) * tn) % 256 == 0), 0)
        return (dict(row_units=(u, 0, Rt_)) if (u and Rt_ >= 2048 and self.act != torch.float32
                                                and os.environ.get("RPO_NO_TEXT_UNITS") != "1") else {})

    # ---- the seams: what Engine's own methods call instead of the single-run entry points while `_multi` is set
    def _m_text_embed(self, n: int) -> None:
        ops.broadcast_rows_sets(self.m_text_prompt, self.xt[0], n)

    def _m_text_attn(self, l: int, da, dq) -> None:
        """Text attention of block l for the S * n_cls virtual classes on the one cache: forward (da None) or backward."""
        cfg, kv, dt = self.cfg, self.kv_t[l], self.cfg.d_t
        nv, n = self._multi * cfg.n_cls, cfg.n_cls
        if da is None:
            ops.text_attn_fwd_shared(self.qt[l], kv[:, :dt], kv[:, dt:], self.att_t, self.len_i32, nv, n, cfg.K, self.Lmax,
                                     cfg.heads_t, SCALE)
        else:
            ops.text_attn_bwd_shared(self.qt[l], kv[:, :dt], kv[:, dt:], da, dq, self.len_i32, nv, n, cfg.K, self.Lmax,
                                     cfg.heads_t, SCALE)

    def _m_img_embed(self, B: int, R: int, rows) -> None:
        cfg = self.cfg
        ops.img_embed_norm_grouped(self.x_pre[:R], self.cls, self.pos, self.m_img_prompt, self.ln_pre[0], self.ln_pre[1],
                                   self.x[0][:R], self.vis[0].ln1_w, self.vis[0].ln1_b, self.h[:R], B, cfg.n_frozen, cfg.K,
                                   B // self._multi, rows=rows)

    def _m_img_reduce(self, B: int) -> None:
        ops.reduce_groups_sets(self.dxb_v[:B * self.cfg.K], self.m_g_img, B // self._multi)

    def _m_text_reduce(self, dx, n: int) -> None:
        ops.reduce_groups_sets(dx, self.m_g_text, n)

    def multi_hbm_bytes(self) -> int:
        """Bytes `multi_setup` added."""
        tot = 0
        for v in list(self._multi_bufs.values()) + [self.m_params, self.m_grads, self.m_mom, self.m_logits, self.m_loss,
                                                    self.m_head_ws]:
            for t in (v if isinstance(v, list) else [v]):
                if isinstance(t, torch.Tensor):
                    tot += t.numel() * t.element_size()
        return tot

    @contextlib.contextmanager
    def _multi_mode(self):
        """While enqueueing a multi-run step: the text tower's buffer names point at the S-fold buffers and the seams take
        the grouped entry points.  Restored on exit, so everything else (eval, a single-run step) sees the engine as it
        was built."""
        if not self.multi_S:
            raise RuntimeError("multi_setup(S, B) has not been called on this engine")
        saved = {k: getattr(self, k) for k in self._multi_bufs}
        self.__dict__.update(self._multi_bufs)
        self._multi = self.multi_S
        try:
            yield
        finally:
            self._multi = None
            self.__dict__.update(saved)

    def multi_head(self, label) -> None:
        """The S heads in the launches of one: member s pairs its own B images with its own text features."""
        S, B, K, e, n = self.multi_S, self.multi_B, self.cfg.K, self.cfg.embed, self.cfg.n_cls
        mb = self._multi_bufs
        act = {} if self.act == torch.float32 else dict(d_img_f_act=self.d_img_f_a[:S * B * K], d_text_f_act=mb["d_text_f_a"])
        train = label is not None
        ops.head_fwd_bwd_grouped(self.img_f[:S * B * K].view(S * B, K, e), mb["text_f"].view(S * n, K, e), label,
                                 self.logit_scale_exp, self.m_logits, self.m_loss if train else None,
                                 self.d_img_f[:S * B * K].view(S * B, K, e) if train else None,
                                 mb["d_text_f"].view(S * n, K, e) if train else None, self.m_head_ws, S,
                                 k_used=self.m_k_used, **(act if train else {}))

    def multi_forward_backward(self, image: torch.Tensor, label: torch.Tensor) -> None:
        """Enqueue loss + both prompt gradients of every member: image [S*B, 3, H, W] and label [S*B], member-major.
        Results land in m_loss [S], m_logits [S*B, n_cls], m_grads [S, text | img].  Capturable in a HIP graph.  Same
        launch structure as `forward_backward`: text tower on the side stream, image tower on the current one."""
        S, B = self.multi_S, self.multi_B
        assert image.shape[0] == S * B, f"the multi-run step takes S * B = {S * B} images, member-major"
        assert label.dtype == torch.int64 and label.shape == (S * B,) and label.is_contiguous()
        self._check(image)
        self.text_f_version = -1
        main = torch.cuda.current_stream()
        with self._multi_mode():
            self.side.wait_stream(main)
            with torch.cuda.stream(self.side):
                self._text_forward(train=True)
            self._image_forward(image, train=True)
            main.wait_stream(self.side)
            self.multi_head(label)
            self.side.wait_stream(main)
            with torch.cuda.stream(self.side):
                self._text_backward()
            self._image_backward(S * B)
            main.wait_stream(self.side)

    def multi_load_member(self, s: int) -> None:
        """Member s's prompts into the single-run parameters: the single-run eval path then runs with them."""
        self.params.copy_(self.m_params[s])
        self.params_version += 1
