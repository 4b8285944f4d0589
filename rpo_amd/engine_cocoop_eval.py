"""CoCoOp on other class sets: the shared-prefix inference pass.

CoCoOp's text features depend on the image (the meta-net shifts the context per image, trainers/cocoop.py:141-143), so a
class set cannot be a cached [n', e] matrix: it is a per-image text pass.  The prompt of image b and class c is
[SOS | ctx + bias[b] | name . EOT] (:123-161, always the "end" layout) under CLIP's plain causal mask, so the first
P = 1 + n_ctx rows read only themselves and are, through every block, THE SAME for all classes of an image.  They are
computed once per image: a pass over Bc images and nc classes runs Bc * (P + nc * S) rows (S = Lmax - P) instead of the
dense path's Bc * nc * Lmax.  Only attention knows about the sharing (rpo_text_attn_fwd_prefix); LayerNorm and the GEMMs
are row-wise and run over the one contiguous row set unchanged.

    ccs = trainer.conditional_class_set(new_tokens)          # int ids [n', 77] of the "X X .. name." prompts
    logits = trainer.model_inference(image, classes=ccs)     # [B, n'], the CURRENT ctx and meta-net
    res = trainer.test(new_split, classes=ccs)
    b2n = base_to_new(trainer, base_split, new_split, ccs)

Forward only; the training step (Engine.cocoop_forward_backward) is not touched.  `ConditionalEvalEngineMixin` is mixed
into rpo_amd.engine.Engine.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops
from .class_set import ClassSet
from .engine_coop import shared_eot_rows, shared_fill, shared_split
from .engine_text import SCALE

MAX_IMAGES_PER_PASS = 256           # rpo_metanet_fwd keeps B * h floats in 48 KB of LDS; the grouped head takes <= 1024 groups


class ConditionalClassSet(ClassSet):
    """The token side of a class set for CoCoOp: lengths, the embedded rows of the positions >= P (tok_emb[ids] + pos,
    rpo_text_embed, once) and the workspace of the shared-prefix pass.  Nothing that depends on ctx or the meta-net is
    kept between calls.  Built by `Engine.conditional_class_set`."""

    # rows of one pass (prefix + suffix rows of its images): bounds the workspace to ROW_BUDGET rows of [fp32 x 2 | act x 9]
    # d_t-wide buffers, 0.22 GB at d_t = 512 in the 16-bit modes
    ROW_BUDGET = 16384

    @staticmethod
    def plan(tokens, n_ctx: int, images_per_pass: Optional[int], budget: int, vocab: Optional[int] = None) -> Optional[dict]:
        """The geometry of the pass for these prompt ids -- P, S, Lmax, images and classes per pass -- or a ValueError
        where the prompts cannot be CoCoOp's or the pass cannot be laid out.  Pure host arithmetic.  None where `tokens`
        is not an integer [n >= 1, context] matrix of ids below `vocab` at all: ClassSet's constructor says what is wrong
        with it."""
        t = np.asarray(tokens)
        if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1 or not np.issubdtype(t.dtype, np.integer):
            return None
        if vocab is not None and (int(t.min()) < 0 or int(t.max()) >= vocab):
            return None
        lens = t.argmax(-1) + 1                         # EOT has the highest id
        n, Lmax, P = int(t.shape[0]), int(lens.max()), 1 + int(n_ctx)
        if int(lens.min()) < P + 3:
            raise ValueError(f"conditional_class_set: every prompt must be 'X X .. name.' with {n_ctx} placeholders, i.e. at "
                             f"least {P + 3} tokens (SOS, {n_ctx} X, a name token, '.', EOT); the shortest has "
                             f"{int(lens.min())}")
        if Lmax > 80:
            raise ValueError(f"conditional_class_set: the longest prompt has {Lmax} tokens, rpo_text_attn_fwd_prefix "
                             "takes 80")
        S = Lmax - P
        per_image = P + n * S
        if images_per_pass is None:
            images_per_pass = max(1, min(MAX_IMAGES_PER_PASS, budget // per_image))
        images_per_pass = int(images_per_pass)
        if not 1 <= images_per_pass <= MAX_IMAGES_PER_PASS:
            raise ValueError(f"conditional_class_set: images_per_pass must be 1 .. {MAX_IMAGES_PER_PASS}, got {images_per_pass}")
        if budget < P + S:
            raise ValueError(f"conditional_class_set: a row budget of {budget} does not hold one class ({P + S} rows)")
        # classes per pass: all of them, unless the images of a pass would then exceed the row budget
        classes_per_pass = n if images_per_pass * per_image <= budget else \
            max(1, min(n, (budget // images_per_pass - P) // S))
        return dict(P=P, S=S, Lmax=Lmax, images_per_pass=images_per_pass, classes_per_pass=classes_per_pass)

    def __init__(self, engine, tokens, n_ctx: int, images_per_pass: Optional[int] = None, row_budget: Optional[int] = None):
        # what needs no device comes first: ClassSet's own checks refuse a wrong shape / dtype / id, these the lengths
        plan = self.plan(tokens, n_ctx, images_per_pass, self.ROW_BUDGET if row_budget is None else int(row_budget),
                         engine._tok_emb_host.shape[0])
        super().__init__(engine, tokens)
        assert plan is not None and plan["Lmax"] == self.Lmax
        P = self.P = plan["P"]
        self.S, self.images_per_pass, self.classes_per_pass = plan["S"], plan["images_per_pass"], plan["classes_per_pass"]
        self.x_sos, self.x_suffix = shared_split(self.x_frozen, self.n, self.Lmax, P)
        self.x_frozen = None
        self._ws = None                                                     # per-pass buffers, sized on first use
        self._out = None                                                    # per-call buffers (image features, logits)
        self._eot = {}

    def rows_per_pass(self, images: Optional[int] = None, classes: Optional[int] = None) -> int:
        Bc = self.images_per_pass if images is None else images
        nc = self.classes_per_pass if classes is None else classes
        return Bc * (self.P + nc * self.S)

    def out_buffers(self, B: int) -> dict:
        """(img_f [B, e], logits [B, n]) of a call over B images; grows, never shrinks."""
        eng = self.engine
        if self._out is None or self._out["B"] < B:
            f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=eng.dev)
            self._out = dict(B=B, img_f=f32(B, eng.cfg.embed), logits=f32(B, self.n))
        return self._out

    def pass_buffers(self, Bc: int) -> dict:
        """The workspace of a pass over up to Bc images and `classes_per_pass` classes; grows, never shrinks."""
        eng, cfg = self.engine, self.engine.cfg
        if self._ws is None or self._ws["Bc"] < Bc:
            dt, e, h, nc = cfg.d_t, cfg.embed, eng.coop_hidden, self.classes_per_pass
            R = self.rows_per_pass(Bc)
            f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=eng.dev)
            a = lambda *s: torch.empty(*s, dtype=eng.act, device=eng.dev)
            self._ws = dict(Bc=Bc, x=f32(R, dt), xm=f32(R, dt), h=a(R, dt), qkv=a(R, 3 * dt), att=a(R, dt), g=a(R, 4 * dt),
                            fn=f32(Bc, e), hid=f32(Bc, h), bias=f32(Bc, dt), shift=f32(Bc, self.P - 1, dt),
                            x_eot=f32(Bc * nc, dt), y_eot=a(Bc * nc, dt), f_chunk=f32(Bc * nc, e),
                            text_f=f32(Bc * self.n, e),
                            head_ws=f32(Bc * ops.head_workspace_floats(1, self.n, 1, e)))
        return self._ws

    def eot_rows(self, Bc: int, c0: int, c1: int) -> torch.Tensor:
        """The EOT row of every (image, class) of a pass over Bc images and classes [c0, c1): always a suffix row."""
        key = (Bc, c0, c1)
        if key not in self._eot:
            self._eot[key] = torch.as_tensor(shared_eot_rows(Bc, self.P, self.S, self.len_np[c0:c1]), device=self.engine.dev)
        return self._eot[key]


class ConditionalEvalEngineMixin:
    def conditional_class_set(self, tokens, images_per_pass: Optional[int] = None,
                              row_budget: Optional[int] = None) -> ConditionalClassSet:
        """A `ConditionalClassSet` of int ids [n', context] ("X X .. name." prompts with this engine's n_ctx placeholders)
        for a CoCoOp engine: any n' >= 1.  A pass takes `images_per_pass` images (default: what `row_budget` rows hold,
        ConditionalClassSet.ROW_BUDGET) and all classes -- or chunks of them where that many images exceed the budget."""
        if not getattr(self, "coop_hidden", 0):
            raise NotImplementedError("conditional_class_set is CoCoOp's (an engine set up with a meta-net); the other "
                                      "trainers take class_set(tokens)")
        return ConditionalClassSet(self, tokens, self.coop_n_ctx, images_per_pass, row_budget)

    def _cocoop_prefix_pass(self, ccs: ConditionalClassSet, img_f: torch.Tensor, logits: torch.Tensor) -> None:
        """logits [Bc, n'] of Bc images (raw features img_f [Bc, e]) against the class set: meta-net, the text blocks over
        Bc * (P + nc * S) rows per class chunk, EOT features, one grouped head launch."""
        cfg = self.cfg
        e, H, n, P, S, Lt = cfg.embed, cfg.heads_t, ccs.n, ccs.P, ccs.S, len(self.txt)
        Bc = img_f.shape[0]
        ws = ccs.pass_buffers(Bc)
        w1, b1, w2, b2 = self.meta
        bias, shift = ws["bias"][:Bc], ws["shift"][:Bc]
        ops.metanet_fwd(img_f, w1, b1, w2, b2, ws["fn"][:Bc], ws["hid"][:Bc], bias)
        torch.add(self.coop_ctx.unsqueeze(0), bias.unsqueeze(1), out=shift)                  # ctx + bias (:141-143)
        _, pos = self._text_tables()
        text_f = ws["text_f"][:Bc * n].view(Bc, n, e)
        for c0 in range(0, n, ccs.classes_per_pass):
            c1 = min(n, c0 + ccs.classes_per_pass)
            nc = c1 - c0
            R = Bc * (P + nc * S)
            x, xm, h, qkv, att, g = (ws[k][:R] for k in ("x", "xm", "h", "qkv", "att", "g"))
            shared_fill(x, Bc, P, ccs.x_sos, shift, pos, ccs.x_suffix[c0 * S:c1 * S])
            ln = ccs.len_i32[c0:c1]
            attn = lambda q, k, v, out: ops.text_attn_fwd_prefix(q, k, v, out, ln, Bc, nc, P, S, H, SCALE)
            self._text_blocks([x] * (Lt + 1), [xm] * Lt, [qkv] * Lt, h, att, g, attn)
            f = ws["text_f"][:Bc * n] if nc == n else ws["f_chunk"][:Bc * nc]
            self._text_eot_tail(x, ccs.eot_rows(Bc, c0, c1), ws["x_eot"][:Bc * nc], ws["y_eot"][:Bc * nc], f)
            if nc != n:
                text_f[:, c0:c1].copy_(f.view(Bc, nc, e))
        # every image has its own text features: Bc independent heads of one image each, in one launch
        ops.head_fwd_bwd_grouped(img_f.view(Bc, 1, e), ws["text_f"][:Bc * n].view(Bc * n, 1, e), None, self.logit_scale_exp,
                                 logits, None, None, None, ws["head_ws"], Bc)

    def cocoop_class_logits(self, image: torch.Tensor, ccs: ConditionalClassSet) -> torch.Tensor:
        """logits [B, n'] of any number of images against a conditional class set, under the CURRENT ctx and meta-net: the
        plain image tower in chunks of max_batch, then the text side `images_per_pass` images at a time.  Returns the
        set's own buffer, valid until the next call with it."""
        self._cs_check(ccs)
        if not isinstance(ccs, ConditionalClassSet):
            raise TypeError("classes: CoCoOp takes the ConditionalClassSet made by conditional_class_set(tokens)")
        assert self.coop_hidden > 0 and image.dim() == 4
        B = image.shape[0]
        out = ccs.out_buffers(B)
        img_f, logits = out["img_f"][:B], out["logits"][:B]
        for b0 in range(0, B, self.max_batch):
            nb = self._plain_image_features(image[b0:b0 + self.max_batch])
            img_f[b0:b0 + nb].copy_(self.img_cls_f[:nb])
        for i0 in range(0, B, ccs.images_per_pass):
            i1 = min(B, i0 + ccs.images_per_pass)
            self._cocoop_prefix_pass(ccs, img_f[i0:i1], logits[i0:i1])
        return logits
