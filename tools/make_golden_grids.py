#!/usr/bin/env python3
"""Both ends of the ViT patch-grid range pinned by the reference's OWN code: ViT-B/32 (7 x 7 grid, 50 frozen tokens,
patch rows of 3072) and ViT-L/14 at 336 px (24 x 24 grid, 577 frozen tokens -- the image tower's attention walks the
keys in chunks there, csrc/attn_image.hip).

The reference's modules are imported, never copied: `CLIP` / `CustomCLIP` of trainers/rpo.py through
tools/make_golden_vitl14_ref.py's `build` (which supplies the four dimension literals of trainers/rpo.py from outside,
the `1 + 14 * 14 + K` of the visual mask among them -- rebuilt from the model's own grid), `CLIP.forward` and
trainers/coop.py's `CustomCLIP` as tools/make_golden_plainclip.py runs them.  Inputs come from rpo_amd.synth (seeded
weights, images, labels, the Oxford-Pets token ids): a file holds outputs plus `weights_crc`.

Writes into tests/golden/ (depth 2 + 2 everywhere):
  ref_vitl14_336_d2_k24_b2.npz           RPO CustomCLIP, ViT-L/14 widths at 336 px, K 24, batch 2: eval logits, loss, both
                                         prompt gradients, the prompt rows after every block (keys of ref_vitl14_d2_k24_b2)
  ref_vitb32_d2_k24_b3.npz               RPO CustomCLIP at patch 32, K 24, batch 3: logits, loss, both gradients
  ref_plainclip_vitl14_336_d2_b2.npz     CLIP.forward logits and both feature sets
  ref_plainclip_vitb32_d2_b3.npz         the same at patch 32
  ref_coop_vitb32_d2_b3_ctx16.npz        trainers/coop.py CustomCLIP + cross-entropy + backward (keys of ref_coop_d2_b2_ctx16)
and their entries into tests/golden/manifest_grids.json.  About a minute on a CPU.
"""
from __future__ import annotations

import json
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg  # noqa: E402
import make_golden_vitl14_ref as mvr  # noqa: E402
from rpo_amd import synth  # noqa: E402
from rpo_amd.config import OXFORD_PETS_BASE_CLASSES, vit_b32, vit_l14_336  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
TEXT_ROW_CLASSES = 3          # classes whose text prompt rows are kept (3: the file stays under 1 MiB; the 224-px one keeps 4)


def _save(tag: str, rec: dict, manifest: dict, **entry) -> None:
    path = os.path.join(OUT, f"ref_{tag}.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size <= 1 << 20, f"{path}: {size} bytes"
    manifest[tag] = dict(source="reference", bytes=size, **entry)
    print(tag, manifest[tag], flush=True)


def rpo_case(CLIP, ref_rpo, tag: str, cfg, B: int, rows: bool, manifest: dict) -> None:
    t0 = time.time()
    toks = synth.oxford_pets_base_tokens()
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
    model = mvr.build(CLIP, ref_rpo, cfg, sd)
    assert np.array_equal(model.text_tokenized.numpy(), toks)
    assert tuple(model.visual_mask.shape) == (cfg.seq_v, cfg.seq_v)
    tp, ip = synth.prompts(cfg, sd, seed=7)
    mg.set_prompts(model, tp, ip)
    image = torch.from_numpy(synth.images(cfg, B))
    label = torch.from_numpy(synth.labels(cfg, B))
    rec = {}
    if rows:
        img_rows, text_rows, handles = mg.hook_prompt_rows(model, cfg.K, model.len_prompts)
    logits, loss, gt, gi = mg.ref_train_eval(model, image, label)
    if rows:
        for h in handles:
            h.remove()
        rec["img_rows"] = torch.stack(img_rows[-cfg.layers_v:]).numpy()       # the train pass (hooks fired twice)
        rec["text_rows"] = torch.stack(text_rows[-cfg.layers_t:]).numpy()[:, :TEXT_ROW_CLASSES]
    rec.update(logits=logits.numpy(), loss=np.float32(loss.item()), g_text=gt.numpy(), g_img=gi.numpy(),
               label=label.numpy(), weights_crc=np.bytes_(synth.state_dict_checksum(sd)))
    _save(tag, rec, manifest, how="trainers/rpo.py CustomCLIP, dimension literals supplied by "
          "tools/make_golden_vitl14_ref.py build()", model=cfg.name, image_size=cfg.image_size, patch=cfg.patch,
          n_frozen=cfg.n_frozen, depth=cfg.layers_v, K=cfg.K, B=B, loss=float(loss), seconds=round(time.time() - t0, 1))


def _plain_clip(CLIP, cfg, sd):
    model = CLIP(cfg.embed, cfg.image_size, cfg.layers_v, cfg.d_v, cfg.patch, cfg.context, cfg.vocab, cfg.d_t,
                 cfg.heads_t, cfg.layers_t).float()
    res = model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model


def plain_case(CLIP, tag: str, cfg, B: int, manifest: dict) -> None:
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    model = _plain_clip(CLIP, cfg, sd).eval()
    image = torch.from_numpy(synth.images(cfg, B))
    text = torch.from_numpy(synth.oxford_pets_base_tokens())
    with torch.no_grad():
        logits, _ = model(image, text)
        img_f, txt_f = model.encode_image(image), model.encode_text(text)
    _save(tag, dict(logits=logits.numpy(), image_features=img_f.numpy(), text_features=txt_f.numpy(),
                    weights_crc=np.bytes_(synth.state_dict_checksum(sd))), manifest,
          how="clip/model.py CLIP.forward", model=cfg.name, image_size=cfg.image_size, patch=cfg.patch,
          n_frozen=cfg.n_frozen, depth=cfg.layers_v, B=B)


def coop_case(CLIP, tag: str, cfg, B: int, n_ctx: int, manifest: dict) -> None:
    import trainers.coop as ref_coop                  # (same stubs as trainers/rpo.py: make_golden._reference)
    ns = types.SimpleNamespace
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    clip_model = _plain_clip(CLIP, cfg, sd)
    rcfg = ns(TRAINER=ns(COOP=ns(N_CTX=n_ctx, CTX_INIT="", CSC=False, CLASS_TOKEN_POSITION="end", PREC="fp32")),
              INPUT=ns(SIZE=(cfg.image_size, cfg.image_size)))
    model = ref_coop.CustomCLIP(rcfg, list(OXFORD_PETS_BASE_CLASSES), clip_model)
    for name, p in model.named_parameters():
        p.requires_grad_("prompt_learner" in name)             # trainers/coop.py:228-230
    ctx = (np.random.default_rng(11).standard_normal((n_ctx, cfg.d_t)) * 0.02).astype(np.float32)
    assert tuple(model.prompt_learner.ctx.shape) == ctx.shape
    model.prompt_learner.ctx.data = torch.from_numpy(ctx.copy())
    image = torch.from_numpy(synth.images(cfg, B))
    label = torch.from_numpy(synth.labels(cfg, B))
    logits = model(image)
    loss = F.cross_entropy(logits, label)                     # trainers/coop.py:268-269
    loss.backward()
    _save(tag, dict(logits=logits.detach().numpy(), loss=np.float32(loss.item()), ctx=ctx,
                    ctx_grad=model.prompt_learner.ctx.grad.numpy(), label=label.numpy(),
                    tokenized_prompts=model.tokenized_prompts.numpy().astype(np.int64),
                    weights_crc=np.bytes_(synth.state_dict_checksum(sd))), manifest,
          how="trainers/coop.py CustomCLIP + F.cross_entropy + backward", model=cfg.name, image_size=cfg.image_size,
          patch=cfg.patch, n_frozen=cfg.n_frozen, depth=cfg.layers_v, B=B, n_ctx=n_ctx, loss=float(loss))


def main() -> None:
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    _, CLIP, ref_rpo = mg._reference()
    only = set(sys.argv[1:])
    want = lambda tag: not only or tag in only
    manifest = {}
    d2 = dict(layers_v=2, layers_t=2)
    try:
        if want("vitl14_336_d2_k24_b2"):
            rpo_case(CLIP, ref_rpo, "vitl14_336_d2_k24_b2", vit_l14_336(K=24, **d2), 2, True, manifest)
        if want("vitb32_d2_k24_b3"):
            rpo_case(CLIP, ref_rpo, "vitb32_d2_k24_b3", vit_b32(K=24, **d2), 3, False, manifest)
    finally:
        ref_rpo.torch = torch
    if want("plainclip_vitl14_336_d2_b2"):
        plain_case(CLIP, "plainclip_vitl14_336_d2_b2", vit_l14_336(K=1, **d2), 2, manifest)
    if want("plainclip_vitb32_d2_b3"):
        plain_case(CLIP, "plainclip_vitb32_d2_b3", vit_b32(K=1, **d2), 3, manifest)
    if want("coop_vitb32_d2_b3_ctx16"):
        coop_case(CLIP, "coop_vitb32_d2_b3_ctx16", vit_b32(K=1, **d2), 3, 16, manifest)
    mp = os.path.join(OUT, "manifest_grids.json")
    man = json.load(open(mp)) if os.path.exists(mp) else {"cases": {}}
    man["cases"].update(manifest)
    json.dump(man, open(mp, "w"), indent=1)


if __name__ == "__main__":
    main()
