"""``ImageFeatures``: the plain image tower's features of a resident image set, computed once, and their classification
by any number of classifiers in one launch.

For the trainers on the plain towers -- `ZeroshotCLIP`, `ZeroshotCLIP2`, `CoOp`, `LP`, on ViT or ResNet -- the image
feature `encode_image(image)` depends on nothing they train: CoOp trains the context, LP trains `lp_layer`, and both sit
BEHIND the feature.  So for a set that is evaluated again and again (the validation set after every epoch, one test set
for several trained models, every template of a prompt ensemble) the image pass needs to run once; what is left per
evaluation is a classifier [C, e] over [n, e] features -- 2 KB per image at e = 512 -- which `rpo_features_classify`
(rpo_amd/csrc/classify.hip) runs for S classifiers at once, head and evaluator fused, writing integers only.

    F   = ImageFeatures.build(trainer, val_set)                     # one image pass
    trainer.train(train_set, val_set=val_set, val_features=F)       # no validation image pass in any epoch
    res = trainer.test(val_set, features=F)                         # the evaluator's dict, one launch, one read-back
    all = classify_many(F, cls)                                     # cls [S, C, e]: S dicts from one launch

CoCoOp's text features depend on the image and RPO's image rows on its prompts (its cache is `FrozenImageKV`): both
refuse `features=`.
"""
from __future__ import annotations

import zlib
from typing import Dict, List, Optional

import numpy as np
import torch

from . import ops
from .evaluator import Classification

MAX_CLASSIFIERS = 1024                     # rpo_features_classify's S per launch (include/rpo_amd.h)


def weights_checksum(state_dict: Dict[str, np.ndarray]) -> str:
    """A fingerprint of a CLIP state dict that costs nothing next to packing it: names, shapes and up to 4096 evenly
    spaced elements of every tensor.  It tells two checkpoints apart, not two tensors that differ in one element."""
    h = 0
    for k in sorted(state_dict):
        a = np.asarray(state_dict[k])
        h = zlib.crc32(f"{k}{tuple(a.shape)}{a.dtype}".encode(), h)
        flat = a.reshape(-1)
        step = max(1, flat.size // 4096)
        h = zlib.crc32(np.ascontiguousarray(flat[::step]).view(np.uint8).data, h)
    return f"{h:08x}"


def lp_compose(text_f_n: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, scale: float):
    """The linear probe as ONE affine classifier on the image feature f (trainers/linear_prob.py:85-95):
        logits = scale (f W^T + b) T^T = scale f (T W)^T + scale T b
    -> (M = T W [C, e], c = scale T b [C]), formed in float64 and rounded once to fp32; `scale` multiplies M's part in
    the kernel (norms off).  Pure: any device, no engine."""
    T = text_f_n.to(torch.float64)
    M = T @ weight.to(torch.float64)
    c = (T @ bias.to(torch.float64)) * float(scale)
    return M.to(torch.float32).contiguous(), c.to(torch.float32).contiguous()


class ImageFeatures:
    def __init__(self, meta: dict, feat: torch.Tensor, labels_dev: torch.Tensor, labels: List[int], device: torch.device):
        self.meta, self.feat, self.labels_dev, self.labels, self.device = meta, feat, labels_dev, labels, device

    def __len__(self) -> int:
        return self.feat.shape[0]

    @staticmethod
    def bytes_needed(cfg, n_images: int) -> int:
        """n * e fp32: 2048 bytes per image at e = 512."""
        return int(n_images) * cfg.embed * 4

    @staticmethod
    def _meta(cfg, act_dtype: torch.dtype, weights: str, n_images: int) -> dict:
        return dict(config=cfg.name, act_dtype=act_dtype, weights=weights, image_size=cfg.image_size, embed=cfg.embed,
                    n_images=int(n_images))

    @classmethod
    def build(cls, trainer_or_engine, image_set, batch_size: int = 100, budget_bytes: Optional[int] = None) -> "ImageFeatures":
        """Runs the eval transform (resize + centre crop) and the engine's plain image pass (`Engine.encode_image`) chunk
        by chunk -- chunks of min(batch_size, engine.max_batch), the last one ragged, as `EvalMixin.test` -- and keeps
        [n, e] fp32 on the device with the set's labels.  Over `budget_bytes`: ValueError naming both byte counts, before
        anything but the engine's configuration is read."""
        from .loop import EvalMixin
        engine = trainer_or_engine.engine if isinstance(trainer_or_engine, EvalMixin) else trainer_or_engine
        cfg, act = engine.cfg, engine.act
        n = len(image_set)
        need = cls.bytes_needed(cfg, n)
        if budget_bytes is not None and need > budget_bytes:
            raise ValueError(f"ImageFeatures.build: the features of {n} images need {need} bytes, the budget is "
                             f"{int(budget_bytes)} bytes")
        if n < 1:
            raise ValueError("ImageFeatures.build: the image set is empty")
        from .input_pipeline import DeviceTransform, InputConfig
        dev = engine.dev
        chunk = max(1, min(batch_size, engine.max_batch))
        with torch.cuda.device(dev), torch.no_grad():
            feat = torch.empty(n, cfg.embed, dtype=torch.float32, device=dev)
            tf = DeviceTransform(InputConfig(SIZE=(cfg.image_size, cfg.image_size)), False, dev, chunk, max_image_bytes=16)
            buf = torch.zeros(chunk, 3, cfg.image_size, cfg.image_size, dtype=torch.float32, device=dev)
            for b0 in range(0, n, chunk):
                B = min(chunk, n - b0)
                image = tf.from_set(image_set, range(b0, b0 + B), out=buf[:B])
                feat[b0:b0 + B].copy_(engine.encode_image(image))
            labels_dev = image_set.labels_dev.to(dev).clone()
        return cls(cls._meta(cfg, act, engine.weights_id, n), feat, labels_dev, list(image_set.labels), dev)

    def nbytes(self) -> int:
        return self.feat.numel() * self.feat.element_size()

    def check(self, engine, image_set=None) -> None:
        """Refuses an engine or a set these features were not built for, by name."""
        n = self.meta["n_images"] if image_set is None else len(image_set)
        want = self._meta(engine.cfg, engine.act, engine.weights_id, n)
        bad = [f"{k}: features {self.meta[k]}, asked {want[k]}" for k in want if self.meta[k] != want[k]]
        if not bad and self.device != engine.dev:
            bad = [f"device: features {self.device}, engine {engine.dev}"]
        if not bad and image_set is not None and list(image_set.labels) != self.labels:
            bad = ["labels: the set's labels are not the ones the features were built with"]
        if bad:
            raise ValueError("ImageFeatures do not match this engine / image set (" + "; ".join(bad) + "): build them "
                             "with ImageFeatures.build(trainer, image_set) for this model and set")


@torch.no_grad()
def classify_many(features: ImageFeatures, cls: torch.Tensor, bias: Optional[torch.Tensor] = None, norm_feat: bool = True,
                  norm_cls: bool = True, scale: float = 1.0, verbose: bool = False, per_class_result: bool = False,
                  pred_out: Optional[torch.Tensor] = None) -> List[dict]:
    """S classifiers cls [S, C, e] (bias [S, C] or None) over the cached features: ONE rpo_features_classify launch per
    1024 classifiers and one read-back -> per classifier the dict `test()` returns (+ "confusion_matrix").  The flags
    and `scale` are the kernel's: logits = scale (/ |f|) (/ |cls|) <f, cls> + bias.  `pred_out`: int32 [S, n] on the
    device, receives the predictions."""
    dev = features.device
    cls = torch.as_tensor(cls, dtype=torch.float32, device=dev)
    if cls.dim() != 3 or cls.shape[2] != features.feat.shape[1] or cls.shape[0] < 1 or cls.shape[1] < 1:
        raise ValueError(f"classify_many: cls must be [S, C, {features.feat.shape[1]}], got {tuple(cls.shape)}")
    cls = cls.contiguous()
    S, C, _ = cls.shape
    if bias is not None:
        bias = torch.as_tensor(bias, dtype=torch.float32, device=dev).contiguous()
        if tuple(bias.shape) != (S, C):
            raise ValueError(f"classify_many: bias must be [{S}, {C}], got {tuple(bias.shape)}")
    n = len(features)
    with torch.cuda.device(dev):
        counts = torch.zeros(S, 2, dtype=torch.int64, device=dev)
        cmat = torch.zeros(S, C * C, dtype=torch.int32, device=dev)
        for s0 in range(0, S, MAX_CLASSIFIERS):
            s1 = min(S, s0 + MAX_CLASSIFIERS)
            ops.features_classify(features.feat, cls[s0:s1], None if bias is None else bias[s0:s1], features.labels_dev,
                                  scale, norm_feat, norm_cls, counts[s0:s1], cmat[s0:s1],
                                  None if pred_out is None else pred_out[s0:s1])
        counts_h, cmat_h = counts.cpu().numpy(), cmat.cpu().numpy()             # the one read-back
    out = []
    for s in range(S):
        ev = Classification(C, per_class_result)
        ev.process_counts(counts_h[s], cmat_h[s])
        res = ev.evaluate(verbose=verbose)
        res["confusion_matrix"] = ev.cmat.copy()
        out.append(res)
    assert all(r["total"] == n for r in out)
    return out
