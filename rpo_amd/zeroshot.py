"""Zero-shot CLIP inference on the HIP engine: the host-side mirror of `trainers/zsclip.py` (ZeroshotCLIP.build_model /
model_inference, :31-63) and of the unmasked towers the sibling trainers call (`trainers/coop.py:196-208`).

    logits = exp(logit_scale) * normalise(encode_image(image)) @ normalise(encode_text(prompts)).T

Nothing is trained here.  The class-name prompts are tokenised by the caller (the BPE tokenizer is out of scope; the
Oxford-Pets base prompts are bundled as ids); their text features are computed once, as the reference does (:48-53).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .config import RPOConfig
from .custom_clip import config_from_state_dict
from .engine import Engine, make_engine
from .loop import EvalMixin
from . import ops, synth


class ZeroshotCLIP(EvalMixin):
    def __init__(self, state_dict: Dict[str, np.ndarray], tokens: Optional[np.ndarray] = None,
                 device: str | torch.device = "cuda:0", act_dtype: torch.dtype = torch.float16, max_batch: int = 100,
                 cfg: Optional[RPOConfig] = None):
        """state_dict: CLIP weights under the reference's key names (numpy); tokens: int64 [n_cls, 77] prompt ids
        (default: the bundled Oxford-Pets base prompts); max_batch: the reference's test batch is 100
        (configs/trainers/RPO/main_K24.yaml:5)."""
        if tokens is None:
            tokens = synth.oxford_pets_base_tokens()
        tokens = np.asarray(tokens, dtype=np.int64)
        if cfg is None:
            cfg = config_from_state_dict(state_dict, 1, tokens.shape[0])     # one (unused) prompt row per image
        self.cfg = cfg
        self.engine = make_engine(cfg, state_dict, tokens, torch.device(device), act_dtype, max_batch)
        self.device = self.engine.dev
        with torch.cuda.device(self.engine.dev):
            self.engine.cache_text_kv()                                       # text features: once (zsclip.py:48-53)

    def set_context(self, ctx) -> None:
        """Evaluate CoOp-style learned context vectors (trainers/coop.py:117-134: generic context [n_ctx, d_t], class
        token at the end): `tokens` must then be the ids of the reference's "X X .. name." prompts.  Clears a classifier
        given through `set_text_features`."""
        with torch.cuda.device(self.engine.dev):
            self.engine.set_plain_text_features(None)
            self.engine.set_context(ctx)
            self.engine.cache_text_kv()

    @torch.no_grad()
    def encode_text(self, tokens: np.ndarray, chunk: Optional[int] = None) -> torch.Tensor:
        """`CLIP.encode_text` of any prompts: tokens int64 [P, 77] -> [P, e] fp32 on the device, un-normalised
        (Engine.encode_text; P is independent of n_cls, the model's own text features are untouched)."""
        return self.engine.encode_text(tokens, chunk)

    def set_text_features(self, features) -> None:
        """The classifier of `model_inference` / `test` becomes `features` [n_cls, e] (normalised or not: the head
        normalises) instead of the text features of the prompts the model was built with.  It stays through later
        `cache_text_kv` calls; `set_text_features(None)` or `set_context` drops it."""
        with torch.cuda.device(self.engine.dev):
            self.engine.set_plain_text_features(features)

    @torch.no_grad()
    def model_inference(self, image: torch.Tensor, classes=None) -> torch.Tensor:
        """trainers/zsclip.py:58-63 -> logits [B, n_cls] (fp32, on the device); `classes`: a `ClassSet`
        (`class_set(tokens)`) -- logits [B, n'] against it."""
        eng = self.engine
        with torch.cuda.device(eng.dev):
            image = image.to(device=eng.dev, dtype=torch.float32).contiguous()
            return eng.forward_plain(image, classes=classes).clone()

    __call__ = model_inference

    def _eval_logits(self, image: torch.Tensor, classes=None) -> torch.Tensor:
        """`model_inference` on a device batch without the clone (loop.EvalMixin.test)."""
        return self.engine.forward_plain(image, classes=classes)

    @torch.no_grad()
    def classifier(self, classes=None):
        """The text features `forward_plain` classifies with (the prompts', `set_text_features`', or a `ClassSet`'s) as
        the cosine classifier of rpo_features_classify (trainers/zsclip.py:58-63)."""
        eng = self.engine
        with torch.cuda.device(eng.dev):
            cls = eng.plain_text_features() if classes is None else eng._cs_plain_current(eng._cs_check(classes))
        return cls, None, True, True, eng.logit_scale_exp


class ZeroshotCLIP2(ZeroshotCLIP):
    """Prompt ensembling (trainers/zsclip.py:63-99): the class names under T templates; the classifier is the normalised
    mean over the templates of each template's normalised text features.  The caller tokenises (template strings are
    the caller's: the reference takes 7 of `IMAGENET_TEMPLATES_SELECT` plus the dataset's own)."""
    def __init__(self, state_dict: Dict[str, np.ndarray], tokens: np.ndarray, device: str | torch.device = "cuda:0",
                 act_dtype: torch.dtype = torch.float16, max_batch: int = 100, cfg: Optional[RPOConfig] = None,
                 chunk: Optional[int] = None):
        """tokens: int64 [T, n_cls, 77], template-major, in the order the reference sums them (zsclip.py:89-94); the
        engine is built on tokens[0].  chunk: prompts per text pass (Engine.encode_text)."""
        tokens = np.asarray(tokens)
        if tokens.ndim != 3:
            raise ValueError(f"ZeroshotCLIP2: tokens must be [T, n_cls, 77] (one block of class prompts per template), "
                             f"got {tokens.ndim} dimension(s)")
        if tokens.shape[2] != 77 or tokens.shape[0] < 1 or tokens.shape[1] < 1:
            raise ValueError(f"ZeroshotCLIP2: tokens must be [T, n_cls, 77] with CLIP's context of 77 ids, "
                             f"got {tuple(tokens.shape)}")
        tokens = tokens.astype(np.int64, copy=False)
        super().__init__(state_dict, tokens[0], device, act_dtype, max_batch, cfg)
        T, n, _ = tokens.shape
        self.n_templates = T
        self._template_tokens, self._template_chunk = tokens, chunk             # (held by reference: test_templates)
        self._template_features = None
        with torch.cuda.device(self.engine.dev):
            feats = self.engine.encode_text(tokens.reshape(T * n, 77), chunk)         # [T * n, e], stays on the device
            acc = torch.empty(n, self.cfg.embed, dtype=torch.float32, device=self.device)
            ops.text_ensemble_accumulate(feats, n, acc, first=True)                   # sum_t f_t / |f_t|, ascending t
            self.text_features = ops.text_ensemble_finish(acc, T)                      # normalise(mean)
            self.set_text_features(self.text_features)

    def set_context(self, ctx) -> None:
        raise NotImplementedError("ZeroshotCLIP2.set_context: a learned context belongs to one template, the ensemble has T")

    @torch.no_grad()
    def test_templates(self, image_set, features=None, verbose: bool = False, per_class_result: bool = False):
        """The accuracy of EVERY template next to the ensemble's, from one launch on cached image features: T + 1
        evaluator dicts -- template t's own classifier (its text features, as a `ZeroshotCLIP` built on that template
        classifies), and the ensemble last (`test(image_set)`'s).  `features`: an `ImageFeatures` of this engine and set
        (default: built here, one image pass).  The per-template text features are computed on the first call and kept."""
        from .features import ImageFeatures, classify_many
        if features is None:
            features = ImageFeatures.build(self, image_set)
        features.check(self.engine, image_set)
        T, n, e = self.n_templates, self.cfg.n_cls, self.cfg.embed
        with torch.cuda.device(self.engine.dev):
            if self._template_features is None:
                self._template_features = self.engine.encode_text(self._template_tokens.reshape(T * n, 77),
                                                                  self._template_chunk).view(T, n, e)
            cls = torch.cat([self._template_features, self.text_features.view(1, n, e)], 0)
            return classify_many(features, cls, None, True, True, self.engine.logit_scale_exp, verbose=verbose,
                                 per_class_result=per_class_result)

    @torch.no_grad()
    def class_set(self, tokens, chunk: Optional[int] = None):
        """tokens [T, n', 77], template-major: the class set's classifier is the ensemble over ITS T templates (the
        existing rpo_text_ensemble_* kernels on `encode_text`'s features); [n', 77]: one template."""
        tokens = np.asarray(tokens)
        if tokens.ndim == 2:
            tokens = tokens[None]
        if tokens.ndim != 3 or tokens.shape[2] != self.cfg.context or tokens.shape[0] < 1 or tokens.shape[1] < 1:
            raise ValueError(f"ZeroshotCLIP2.class_set: tokens must be [T, n, {self.cfg.context}] (one block of class "
                             f"prompts per template), got {tuple(tokens.shape)}")
        with torch.cuda.device(self.engine.dev):
            cs = self.engine.class_set(tokens[0], chunk)
            T, n, _ = tokens.shape
            feats = self.engine.encode_text(tokens.reshape(T * n, tokens.shape[2]), chunk)
            acc = torch.empty(n, self.cfg.embed, dtype=torch.float32, device=self.device)
            ops.text_ensemble_accumulate(feats, n, acc, first=True)
            cs.plain_f, cs.plain_fixed = ops.text_ensemble_finish(acc, T), True
        return cs
