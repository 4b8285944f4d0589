#!/usr/bin/env python3
"""Golden vectors for class sets (rpo_amd/class_set.py) from the real reference: what its `--eval-only` processes
compute when they rebuild CLIP around ANOTHER set of class names -- the 18 Oxford-Pets "new" classes, as
`subsample_classes` splits the 37 (datasets/oxford_pets.py) -- on the `d2_k8_b3` workload of tests/helpers.py (its
synthetic weights, prompts and images).  Writes, under tests/golden/:

  ref_classset_rpo.npz          trainers/rpo.py CustomCLIP's eval logits [3, 18] with the workload's prompts
  ref_classset_coop_end.npz     trainers/coop.py CustomCLIP logits, n_ctx 4, class token at the end, a given context
  ref_classset_coop_middle.npz  the same with the class token in the middle
  ref_classset_zeroshot.npz     clip/model.py CLIP.forward logits (zero-shot)
  ref_classset_lp.npz           trainers/linear_prob.py CustomCLIP logits with a random non-identity lp_layer (re-created
                                from its seed by tests/lp_fixtures.c1_init: a dense 512 x 512 matrix is 1 MB)
  manifest_classsets.json       provenance (generator, torch, byte counts)

Each file holds the token ids it used (the reference's tokenizer; the BPE tokenizer is out of scope on the other side).
Runs in the build container only (imports the reference through make_golden._reference); no test runs it.  The .npz
members carry a fixed timestamp: the files regenerate bit for bit."""
import io
import json
import os
import sys
import types
import zipfile
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from make_golden import _reference, build_reference_model, set_prompts, REPO     # noqa: E402  (nothing copied)
from rpo_amd import synth                         # noqa: E402
from rpo_amd.config import PROMPT_TEMPLATE, vit_b16  # noqa: E402
from lp_fixtures import c1_init                   # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
ns = types.SimpleNamespace
NEW_CLASSES = ("leonberger", "maine_coon", "miniature_pinscher", "newfoundland", "persian", "pomeranian", "pug", "ragdoll",
               "russian_blue", "saint_bernard", "samoyed", "scottish_terrier", "shiba_inu", "siamese", "sphynx",
               "staffordshire_bull_terrier", "wheaten_terrier", "yorkshire_terrier")
DEPTH, K, B, N_CTX = 2, 8, 3, 4                   # tests/helpers.py CASES["d2_k8_b3"]


def savez_fixed(path, **arrays):
    """np.savez_compressed with every member stamped 1980-01-01 (numpy stamps the wall clock: no two runs alike)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=6)


def clip_of(CLIP, cfg, sd):
    m = CLIP(cfg.embed, cfg.image_size, cfg.layers_v, cfg.d_v, cfg.patch, cfg.context, cfg.vocab, cfg.d_t, cfg.heads_t,
             cfg.layers_t).float()
    res = m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m


def main():
    torch.manual_seed(0)
    ref_clip, CLIP, ref_rpo = _reference()
    import trainers.coop as ref_coop              # noqa: E402
    import trainers.linear_prob as ref_lp         # noqa: E402
    cfg = vit_b16(layers_v=DEPTH, layers_t=DEPTH, K=K)
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    crc = np.bytes_(synth.state_dict_checksum(sd))
    image = torch.from_numpy(synth.images(cfg, B))
    names = np.array(NEW_CLASSES, dtype=np.str_)
    files = {}

    def write(name, **arrays):
        path = os.path.join(GOLD, name)
        savez_fixed(path, classnames=names, weights_crc=crc, **arrays)
        files[name] = dict(source="reference", model=cfg.name, depth=DEPTH, B=B, n_cls=len(NEW_CLASSES),
                           bytes=os.path.getsize(path))
        print(name, "|logits|max", float(np.abs(arrays["logits"]).max()), files[name]["bytes"], "bytes", flush=True)

    # ---- RPO: trainers/rpo.py CustomCLIP rebuilt around the new class names, the workload's prompts
    model = build_reference_model(CLIP, ref_rpo, cfg, sd, NEW_CLASSES)
    tp, ip = synth.prompts(cfg, sd, seed=7)
    set_prompts(model, tp, ip)
    model.prompt_learner.eval()
    with torch.no_grad():
        logits = model(image)
    toks = model.text_tokenized.numpy().astype(np.int64)
    texts = [PROMPT_TEMPLATE.replace("_", c) for c in NEW_CLASSES]
    assert np.array_equal(toks, torch.cat([ref_clip.tokenize(t) for t in texts]).numpy())
    write("ref_classset_rpo.npz", tokens=toks, logits=logits.numpy(), K=np.int64(K), prompt_seed=np.int64(7))
    del model

    # ---- zero-shot: CLIP.forward on the same token ids
    clip_model = clip_of(CLIP, cfg, sd).eval()
    with torch.no_grad():
        zl, _ = clip_model(image, torch.from_numpy(toks))
    write("ref_classset_zeroshot.npz", tokens=toks, logits=zl.numpy())

    # ---- CoOp: generic context of n_ctx 4, class token at the end / in the middle
    ctx = (np.random.default_rng(11).standard_normal((N_CTX, cfg.d_t)) * 0.02).astype(np.float32)
    for position in ("end", "middle"):
        rcfg = ns(TRAINER=ns(COOP=ns(N_CTX=N_CTX, CTX_INIT="", CSC=False, CLASS_TOKEN_POSITION=position, PREC="fp32")),
                  INPUT=ns(SIZE=(cfg.image_size, cfg.image_size)))
        model = ref_coop.CustomCLIP(rcfg, list(NEW_CLASSES), clip_of(CLIP, cfg, sd))
        model.prompt_learner.ctx.data = torch.from_numpy(ctx.copy())
        with torch.no_grad():
            cl = model(image)
        write(f"ref_classset_coop_{position}.npz", tokens=model.tokenized_prompts.numpy().astype(np.int64),
              logits=cl.numpy(), ctx=ctx, n_ctx=np.int64(N_CTX), class_token_position=np.str_(position),
              name_lens=np.asarray(model.prompt_learner.name_lens, dtype=np.int64))
        del model

    # ---- LP: lp_layer = the seeded non-identity (W, b) of tests/lp_fixtures.c1_init
    rcfg = ns(TRAINER=ns(LP=ns(PROMPT="A photo of a {cls_name}", PREC="fp32")))
    model = ref_lp.CustomCLIP(rcfg, list(NEW_CLASSES), clip_of(CLIP, cfg, sd))
    w, b = c1_init(cfg.embed)
    model.lp_layer.weight.data = torch.from_numpy(w.copy())
    model.lp_layer.bias.data = torch.from_numpy(b.copy())
    with torch.no_grad():
        ll = model(image)
    write("ref_classset_lp.npz", tokens=ref_clip.tokenize(model.prompts).numpy().astype(np.int64), logits=ll.numpy(),
          text_features=model.text_features.numpy(), lp_bias=b, lp_w_crc32=np.int64(zlib.crc32(w.tobytes())))

    with open(os.path.join(GOLD, "manifest_classsets.json"), "w") as f:
        json.dump(dict(generator="tools/make_golden_classsets.py", torch=torch.__version__, numpy=np.__version__,
                       files=files), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
