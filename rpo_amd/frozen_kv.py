"""``FrozenImageKV``: the per-block K / V of a resident image set's frozen rows, computed once.

A frozen image row's whole way through the image tower depends on the image alone -- not on the prompts, on K or on the
class set -- so for a set that is evaluated again and again (the validation set after every
epoch, the test set for every member of an `RPOMulti`) the frozen pass needs to run once: its K / V columns,
`qkv[l][:B*N, d_v:]` after any image forward, are copied into `[n * N, 2 d_v]` per block (as `cache_text_kv` keeps the
text tower's), and every later evaluation is the prompt-row pass alone (rpo_amd/engine_prompt_rows.py).  The cache
stays valid across training steps; it is tied to the backbone, the storage mode, the image size and the set.
"""
from __future__ import annotations

from typing import Optional

import torch

from .config import refuse_long_grid
from .engine_prompt_rows import PromptKV


def _esz(act_dtype: torch.dtype) -> int:
    return 4 if act_dtype == torch.float32 else 2


class FrozenImageKV:
    def __init__(self, meta: dict, layers: list, device: torch.device):
        self.meta, self.layers, self.device = meta, layers, device
        dv = meta["d_v"]
        first = torch.zeros(1, dtype=torch.int32, device=device)
        # (k, v) per block as column halves of the cache rows: leading dimension 2 d_v
        self.kv = PromptKV([(t[:, :dv], t[:, dv:]) for t in layers], meta["n_images"], first)

    @staticmethod
    def bytes_needed(cfg, n_images: int, act_dtype: torch.dtype = torch.bfloat16) -> int:
        """n * N * 2 d_v * element size * layers_v: 7 262 208 bytes per image for ViT-B/16 in 16-bit."""
        return int(n_images) * cfg.n_frozen * 2 * cfg.d_v * _esz(act_dtype) * cfg.layers_v

    @staticmethod
    def _meta(cfg, act_dtype: torch.dtype, n_images: int) -> dict:
        return dict(d_v=cfg.d_v, n_frozen=cfg.n_frozen, layers_v=cfg.layers_v, act_dtype=act_dtype,
                    image_size=cfg.image_size, n_images=int(n_images))

    @classmethod
    def build(cls, engine, image_set, batch_size: int = 100, budget_bytes: Optional[int] = None) -> "FrozenImageKV":
        """Runs the eval transform (resize + centre crop) and the existing frozen pass chunk by chunk (chunks of
        min(batch_size, engine.max_batch), the last one ragged -- `EvalMixin.test`'s) and keeps every block's K / V.
        Over `budget_bytes`: ValueError naming both byte counts, before anything is allocated."""
        cfg, act = engine.cfg, engine.act
        refuse_long_grid(cfg, "FrozenImageKV.build")
        n = len(image_set)
        need = cls.bytes_needed(cfg, n, act)
        if budget_bytes is not None and need > budget_bytes:
            raise ValueError(f"FrozenImageKV.build: the frozen K / V of {n} images need {need} bytes, the budget is "
                             f"{int(budget_bytes)} bytes")
        engine._refuse_rn("FrozenImageKV.build")
        from .input_pipeline import DeviceTransform, InputConfig
        dev, N, dv = engine.dev, cfg.n_frozen, cfg.d_v
        chunk = max(1, min(batch_size, engine.max_batch))
        with torch.cuda.device(dev), torch.no_grad():
            layers = [torch.empty(n * N, 2 * dv, dtype=act, device=dev) for _ in range(cfg.layers_v)]
            tf = DeviceTransform(InputConfig(SIZE=(cfg.image_size, cfg.image_size)), False, dev, chunk, max_image_bytes=16)
            buf = torch.zeros(chunk, 3, cfg.image_size, cfg.image_size, dtype=torch.float32, device=dev)
            for b0 in range(0, n, chunk):
                B = min(chunk, n - b0)
                image = tf.from_set(image_set, range(b0, b0 + B), out=buf[:B])
                engine.frozen_pass(image)
                for l, t in enumerate(layers):
                    t[b0 * N:(b0 + B) * N].copy_(engine.qkv[l][:B * N, dv:])
        return cls(cls._meta(cfg, act, n), layers, dev)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.layers)

    def check(self, engine, image_set) -> None:
        """Refuses an engine or a set this cache was not built for."""
        want = self._meta(engine.cfg, engine.act, len(image_set))
        bad = [f"{k}: cache {self.meta[k]}, asked {want[k]}" for k in want if self.meta[k] != want[k]]
        if not bad and self.device != engine.dev:
            bad = [f"device: cache {self.device}, engine {engine.dev}"]
        if bad:
            raise ValueError("FrozenImageKV does not match this engine / image set (" + "; ".join(bad) + "): build it "
                             "with FrozenImageKV.build(engine, image_set) for this trainer and set")
