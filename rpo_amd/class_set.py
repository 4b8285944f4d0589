"""Class sets: the text side of an engine for classes it was NOT built with.

The reference evaluates a trained model on other classes by starting a new process that rebuilds CLIP around the new
class names and loads the checkpoint (`--eval-only --model-dir --load-epoch`: scripts/rpo/base2new_test.sh with SUB=new,
scripts/rpo/xd_test.sh).  Here nothing reads a prompt, so the image pass does not depend on the
class set at all, a class set's frozen text K / V depends on its tokens alone, and its K prompt rows per class are the
text tower's prompt-row pass on that K / V: a `ClassSet` is a second, small text-side state next to an engine whose
image side -- packed weights, workspace, plans -- stays as it is.

    new = trainer.class_set(new_tokens)                      # int ids [n', 77], any n' >= 1
    res = trainer.test(new_split, classes=new)               # evaluator and confusion matrix sized by n'
    b2n = base_to_new(trainer, base_split, new_split, new)   # {"base", "new", "H"} (rpo_amd/evaluator.py)

A class set belongs to the engine that made it; everything it allocates (frozen rows, K / V, features, logits, head
workspace, captured graphs) hangs on the object and dies with it.  `ClassSetEngineMixin` is mixed into
rpo_amd.engine.Engine.
"""
from __future__ import annotations

import contextlib
import dataclasses
from typing import List, Optional

import numpy as np
import torch

from . import ops
from .engine_coop import coop_layout_of


class ClassSet:
    """The text-side state of one class set on one engine.  Built by `Engine.class_set`; the RPO and plain-tower halves
    are filled on first use (an RPO engine never pays for EOT features, a zero-shot engine never for K / V)."""

    def __init__(self, engine, tokens, chunk: Optional[int] = None):
        cfg = engine.cfg
        tokens = np.asarray(tokens)
        if tokens.ndim != 2 or tokens.shape[1] != cfg.context or tokens.shape[0] < 1:
            raise ValueError(f"class_set: tokens must be [n, {cfg.context}] prompt ids with n >= 1, got {tuple(tokens.shape)}")
        if not np.issubdtype(tokens.dtype, np.integer):
            raise TypeError(f"class_set: tokens must be integer prompt ids, got {tokens.dtype}")
        tokens = tokens.astype(np.int64, copy=False)
        vocab = engine._tok_emb_host.shape[0]
        if int(tokens.min()) < 0 or int(tokens.max()) >= vocab:
            raise ValueError(f"class_set: token id outside the vocabulary [0, {vocab})")
        chunk = engine.TEXT_CHUNK if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError("class_set: chunk is classes per pass, >= 1")
        self.engine, self.tokens, self.chunk = engine, tokens, chunk
        self.n = int(tokens.shape[0])
        self.len_np = tokens.argmax(-1) + 1             # EOT has the highest id (trainers/rpo.py:137)
        self.Lmax = int(self.len_np.max())
        dev = engine.dev
        with torch.cuda.device(dev):
            self.len_i32 = torch.tensor(self.len_np, dtype=torch.int32, device=dev)
            self.ids = torch.from_numpy(np.ascontiguousarray(tokens.astype(np.int32))).to(dev)        # [n, context]
            # the frozen rows, make_prompts (trainers/rpo.py:135-136): tok_emb[ids] + pos for the positions < Lmax
            self.x_frozen = self._embed(self.ids, None)
            self.logits = torch.empty(engine.max_batch, self.n, dtype=torch.float32, device=dev)
            self.head_ws = torch.empty(ops.head_workspace_floats(engine.max_batch, self.n, cfg.K, cfg.embed),
                                       dtype=torch.float32, device=dev)
        self.kv_t: Optional[List[torch.Tensor]] = None  # RPO: per layer [n * Lmax, 2 d_t] (k | v)
        self.text_f: Optional[torch.Tensor] = None      # RPO: [n * K, e]
        self.text_f_version = -1                        # prompts version `text_f` belongs to (engine.params_version)
        self.plain_f: Optional[torch.Tensor] = None     # plain towers: EOT features [n, e]
        self._plain_key = None
        self.plain_fixed = False                        # plain_f was given (a prompt ensemble): no context applies
        self.graphs = {}                                # captured eval graphs, keyed per batch size (and K / V source)
        self._shared = None                             # logits / head workspace of the shared prompt-row path

    def _embed(self, ids: torch.Tensor, ctx: Optional[torch.Tensor]) -> torch.Tensor:
        eng = self.engine
        table, pos = eng._text_tables()
        x = torch.empty(self.n * self.Lmax, eng.cfg.d_t, dtype=torch.float32, device=eng.dev)
        return ops.text_embed(ids, table, pos, x, self.Lmax, ctx=ctx)

    def hbm_bytes(self) -> int:
        """Device bytes this object holds (the static inputs of its captured graphs included)."""
        tot, seen = 0, set()

        def walk(v):
            nonlocal tot
            if isinstance(v, torch.Tensor):
                if v.is_cuda and v.untyped_storage().data_ptr() not in seen:
                    seen.add(v.untyped_storage().data_ptr())
                    tot += v.untyped_storage().nbytes()
            elif isinstance(v, (list, tuple)):
                for t in v:
                    walk(t)
            elif isinstance(v, dict):
                for t in v.values():
                    walk(t)
        for k, v in vars(self).items():
            if k != "engine":
                walk(v)
        return tot

    def shared_buffers(self, S: int, B: int):
        """(logits [S * B, n], head workspace, text_f [S * n * K, e]) of the shared prompt-row path for S prompt sets and
        chunks of up to B images; grows, never shrinks."""
        eng, cfg = self.engine, self.engine.cfg
        sh = self._shared
        if sh is None or S > sh["S"] or B > sh["B"]:
            S, B = max(S, sh["S"] if sh else 0), max(B, sh["B"] if sh else 0)
            f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=eng.dev)
            sh = self._shared = dict(S=S, B=B, gen=(sh["gen"] + 1 if sh else 0), logits=f32(S * B, self.n),
                                     head_ws=f32(S * ops.head_workspace_floats(B, self.n, cfg.K, cfg.embed)),
                                     text_f=f32(S * self.n * cfg.K, cfg.embed))
        return sh


class ClassSetEngineMixin:
    _plain_ctx = None                   # the context `set_context` applied last (class sets follow it), or None
    ctx_version = 0                     # bumped by `set_context`

    def class_set(self, tokens, chunk: Optional[int] = None) -> ClassSet:
        """A `ClassSet` of int ids [n', context] for this engine: any n' >= 1, unrelated to cfg.n_cls.  `chunk` classes
        run per text pass (default TEXT_CHUNK), which bounds the workspace of the frozen-token pass and of the prompt-row
        pass; each class's rows depend on that class alone."""
        if getattr(self, "coop_csc", False):
            raise NotImplementedError("class_set: class-specific contexts (CSC) hold one context per TRAINED class; they "
                                      "mean nothing for another class")
        if getattr(self, "coop_hidden", 0):
            raise NotImplementedError("class_set: CoCoOp's per-image text tower is sized for the classes the engine was "
                                      "built with and its text features depend on the image, so no cached [n', e] "
                                      "matrix can serve it; use conditional_class_set(tokens), the per-image "
                                      "shared-prefix pass (rpo_amd/engine_cocoop_eval.py)")
        return ClassSet(self, tokens, chunk)

    def _cs_check(self, cs) -> ClassSet:
        if not isinstance(cs, ClassSet):
            raise TypeError(f"classes: a ClassSet made by this engine's class_set(tokens), not {type(cs).__name__}")
        if cs.engine is not self:
            raise ValueError("classes: this ClassSet belongs to another engine (its K / V and features were computed with "
                             "that engine's weights and sized for its batch)")
        return cs

    # ------------------------------------------------------------------ RPO: frozen K / V once, prompt rows per version
    def _cs_build_kv(self, cs: ClassSet) -> None:
        cfg = self.cfg
        if int(cs.len_np.max()) + cfg.K > cfg.context:
            raise ValueError(f"len_c + K must fit the context (rpo.py:176): the longest prompt of this class set has "
                             f"{int(cs.len_np.max())} tokens, K = {cfg.K}, context = {cfg.context}")
        L, dt = cs.Lmax, cfg.d_t
        kv = [torch.empty(cs.n * L, 2 * dt, dtype=self.act, device=self.dev) for _ in range(cfg.layers_t)]
        for c0 in range(0, cs.n, cs.chunk):
            c1 = min(cs.n, c0 + cs.chunk)
            x = cs.x_frozen[c0 * L:c1 * L].clone()
            self._text_blocks_plain(x, cs.len_i32[c0:c1], c1 - c0, L, [t[c0 * L:c1 * L] for t in kv])
        cs.kv_t = kv

    @contextlib.contextmanager
    def _class_set_mode(self, cs: ClassSet, c0: int, c1: int, bufs: dict, out: torch.Tensor):
        """While the prompt-row pass of classes [c0, c1) of `cs` is enqueued: the names `_text_forward_` reads -- the class
        count, lengths, K / V cache, per-step buffers, result -- point at the class set's, in the manner of `_multi_mode`.
        The tile hints are derived for THIS row count: the c_fc row units by the engine's own rule, the text tower's
        geometry codes (chosen for the engine's Rt rows) only where the row count is the engine's."""
        assert self._multi is None, "a class set's text pass cannot run inside a multi-run step"
        K, L = self.cfg.K, cs.Lmax
        nc = c1 - c0
        rows = nc * K
        own = rows == self.cfg.n_cls * K
        swap = dict(cfg=dataclasses.replace(self.cfg, n_cls=nc), Rt=rows, len_i32=cs.len_i32[c0:c1], Lmax=L,
                    kv_t=[t[c0 * L:c1 * L] for t in cs.kv_t], text_f=out[c0 * K:c1 * K],
                    _text_fc_units=self._text_fc_units_for(rows), _text_tiles=self._text_tiles if own else {})
        for k, v in bufs.items():
            swap[k] = [t[:rows] for t in v] if isinstance(v, list) else v[:rows]
        saved = {k: getattr(self, k) for k in swap}
        saved_ws = self._ws_cfg
        self.__dict__.update(swap)
        self._ws_cfg = self._ws_text_cfg if own else 0
        try:
            yield
        finally:
            self._ws_cfg = saved_ws
            self.__dict__.update(saved)

    def class_text_features(self, cs: ClassSet, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """text_f [n' * K, e] of the CURRENT prompts for the class set: the engine's own `_text_forward_` on the set's
        frozen K / V, `chunk` classes per pass.  Without `out` the set's own buffer, recomputed only when the prompts'
        version moved (as `forward_eval` does for the built-in classes); with `out`, always computed, into it."""
        self._cs_check(cs)
        self._refuse_rn("class_text_features")
        cfg = self.cfg
        K, dt, e, Lt = cfg.K, cfg.d_t, cfg.embed, cfg.layers_t
        if cs.kv_t is None:
            self._cs_build_kv(cs)
        if out is None:
            if cs.text_f is None:
                cs.text_f = torch.empty(cs.n * K, e, dtype=torch.float32, device=self.dev)
            if cs.text_f_version == self.params_version:
                return cs.text_f
            out = cs.text_f
            cs.text_f_version = self.params_version
        assert tuple(out.shape) == (cs.n * K, e) and out.is_contiguous() and out.dtype == torch.float32
        R = min(cs.chunk, cs.n) * K
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
        a = lambda *s: torch.empty(*s, dtype=self.act, device=self.dev)
        bufs = dict(xt=[f32(R, dt) for _ in range(Lt + 1)], xtm=[f32(R, dt) for _ in range(Lt)], ht=a(R, dt),
                    qt=[a(R, dt) for _ in range(Lt)], att_t=a(R, dt), gt=a(R, 4 * dt), y_final=a(R, dt),
                    ln_stats_t=f32(R, dt // 64, 2))
        for c0 in range(0, cs.n, cs.chunk):
            c1 = min(cs.n, c0 + cs.chunk)
            with self._class_set_mode(cs, c0, c1, bufs, out):
                self._text_forward_(train=False)
        return out

    # ------------------------------------------------------------------ plain towers: EOT features
    def class_plain_features(self, cs: ClassSet, ctx: Optional[torch.Tensor] = None, position: str = "end",
                             version: Optional[int] = None) -> torch.Tensor:
        """EOT features [n', e] (un-normalised, as `CLIP.encode_text`) of the class set under the plain causal tower.
        `ctx` [n_ctx, d_t] on the device: a generic CoOp context, put where `coop_layout`'s rule puts it for each
        class-token `position`, through the negative ids of rpo_text_embed.  Cached: with `version` while the caller's
        version stands, else while `ctx` holds the values it held (one small device comparison)."""
        self._cs_check(cs)
        if cs.plain_fixed:
            return cs.plain_f
        key = cs._plain_key
        if cs.plain_f is not None and key is not None and key[0] == position:
            if version is not None and key[1] == version:
                return cs.plain_f
            if version is None and key[1] is None and ((ctx is None and key[2] is None) or (
                    ctx is not None and key[2] is not None and key[2].shape == ctx.shape and torch.equal(key[2], ctx))):
                return cs.plain_f
        L = cs.Lmax
        if ctx is None:
            x_all = cs.x_frozen
        else:
            if ctx.dim() != 2 or ctx.shape[1] != self.cfg.d_t:
                raise NotImplementedError("class_set: only a generic context [n_ctx, d_t] can be applied to another class "
                                          "set; class-specific contexts (CSC) hold one context per trained class")
            n_ctx = int(ctx.shape[0])
            if 1 + n_ctx >= L:
                raise ValueError(f"class_set: a context of {n_ctx} vectors needs prompts of more than {1 + n_ctx} tokens "
                                 f"('X X .. name.' with n_ctx placeholders); the longest of this class set has {L}")
            src, ctx_pos = coop_layout_of(cs.len_np, n_ctx, position, L)
            ids = np.take_along_axis(cs.tokens[:, :L], np.maximum(src, 0), 1).astype(np.int32)
            # context vector j of every class: id -1 - j at the position the layout gives it
            np.put_along_axis(ids, ctx_pos, (-1 - np.arange(n_ctx, dtype=np.int32))[None, :], 1)
            ctx = ctx.to(dtype=torch.float32).contiguous()
            x_all = cs._embed(torch.from_numpy(np.ascontiguousarray(ids)).to(self.dev), ctx)
        out = torch.empty(cs.n, self.cfg.embed, dtype=torch.float32, device=self.dev)
        for c0 in range(0, cs.n, cs.chunk):
            c1 = min(cs.n, c0 + cs.chunk)
            x = x_all[c0 * L:c1 * L].clone()
            self._text_blocks_plain(x, cs.len_i32[c0:c1], c1 - c0, L)
            self._text_eot_features(x, cs.len_i32[c0:c1], c1 - c0, L, out[c0:c1])
        cs.plain_f = out
        cs._plain_key = (position, version, None if (ctx is None or version is not None) else ctx.clone())
        return out

    def _cs_plain_current(self, cs: ClassSet) -> torch.Tensor:
        """The class set's features under whatever `set_context` applied last (generic context, class token at the end)."""
        return self.class_plain_features(cs, self._plain_ctx, "end", version=self.ctx_version)

    # ------------------------------------------------------------------ the eval forwards
    def _cs_eval_body(self, image: torch.Tensor, B: int, cs: ClassSet) -> None:
        self._image_forward(image, train=False)
        K, e = self.cfg.K, self.cfg.embed
        ops.head_fwd_bwd(self.img_f[:B * K].view(B, K, e), cs.text_f.view(cs.n, K, e), None, self.logit_scale_exp,
                         cs.logits[:B], None, None, None, cs.head_ws)

    def _cs_forward_eval(self, image: torch.Tensor, cs: ClassSet, use_graph: bool) -> torch.Tensor:
        """`forward_eval` against a class set: the image side is the engine's own; the head reads the set's features and
        writes the set's logits.  Graphs are keyed per (batch size, class set): they live on the class set."""
        self._cs_check(cs)
        self._refuse_rn("forward_eval")
        B = self._check(image)
        self.class_text_features(cs)
        if not use_graph:
            self._cs_eval_body(image, B, cs)
            return cs.logits[:B]
        entry = cs.graphs.get(("eval", B))
        if entry is None:
            static = torch.empty_like(image)
            static.copy_(image)
            self._cs_eval_body(static, B, cs)           # eager warm-up: sets kernel attributes (not capturable)
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._cs_eval_body(static, B, cs)
            entry = cs.graphs[("eval", B)] = (g, static)
        g, static = entry
        if static.data_ptr() != image.data_ptr():
            static.copy_(image, non_blocking=True)
        g.replay()
        return cs.logits[:B]

    def _cs_forward_plain(self, image: torch.Tensor, cs: ClassSet, text_f: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`forward_plain` against a class set (`text_f`: the caller's features for it, e.g. CoOp's under its current
        context; default: under `set_context`'s)."""
        self._cs_check(cs)
        e = self.cfg.embed
        if text_f is None:
            text_f = self._cs_plain_current(cs)
        if self.img_cls_f is None:
            self.img_cls_f = torch.empty(self.max_batch, e, dtype=torch.float32, device=self.dev)
        B = self._plain_image_features(image)
        ops.head_fwd_bwd(self.img_cls_f[:B].view(B, 1, e), text_f.view(cs.n, 1, e), None, self.logit_scale_exp,
                         cs.logits[:B], None, None, None, cs.head_ws)
        return cs.logits[:B]

    def _cs_lp_forward(self, image: torch.Tensor, cs: ClassSet) -> torch.Tensor:
        """The linear probe against a class set: lp_layer on the image feature, then the set's normalised features."""
        self._cs_check(cs)
        f = self._cs_plain_current(cs)
        if getattr(cs, "lp_f_n", None) is None or cs._lp_src is not f:
            cs.lp_f_n = (f / f.norm(dim=-1, keepdim=True)).contiguous()               # as `_lp_text_features` (:81)
            cs._lp_src = f
            cs.lp_ws = torch.empty(ops.lp_head_workspace_floats(self.max_batch, cs.n, self.cfg.embed), dtype=torch.float32,
                                   device=self.dev)
        B = self._plain_image_features(image)
        ops.lp_head_fwd_bwd(self.img_cls_f[:B], self.lp_w, self.lp_b, cs.lp_f_n, None, self.logit_scale_exp, self.lp_z[:B],
                            cs.logits[:B], None, None, None, cs.lp_ws)
        return cs.logits[:B]
