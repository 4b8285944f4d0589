#!/usr/bin/env python3
"""Golden vectors of prompt ensembling from the real reference: `trainers.zsclip.ZeroshotCLIP2.build_model` and
`model_inference` (trainers/zsclip.py:55-99) run as they stand on this repo's synthetic weights, the 19 Oxford-Pets base
class names and the reference's own tokenizer and template lists.  Writes tests/golden/ref_zsclip2_*.npz and
tests/golden/manifest_zsclip2.json.  Runs in the build container only (needs the reference); no test runs it.

The trainer object is made with object.__new__ (its Dassl base class is a stub), given cfg / dm / device by hand, and
`load_clip_to_cpu` of trainers.zsclip -- which would download -- is replaced by a function that returns the synthetic
model.  `build_model` extends the class attribute `templates` in place (`self.templates += [...]`, :83), so the list is
restored between cases.  The template strings are stored in the fixtures as data and stated nowhere in this repository's
code.  The .npz members carry a fixed timestamp: the files regenerate bit for bit."""
import io, json, os, sys, types, zipfile
import numpy as np, torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _reference, REPO          # noqa: E402  (stubs the absent dassl / yacs imports, nothing copied)
from rpo_amd import synth                         # noqa: E402
from rpo_amd.config import OXFORD_PETS_BASE_CLASSES, rn_clip, vit_b16  # noqa: E402

ref_clip, CLIP, _ = _reference()
import trainers.zsclip as zsclip                  # noqa: E402
GOLD = os.path.join(REPO, "tests", "golden")
ns = types.SimpleNamespace
TEMPLATES0 = list(zsclip.ZeroshotCLIP2.templates)


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


def vit_case():
    cfg = vit_b16(layers_v=2, layers_t=2, K=1)
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    model = CLIP(cfg.embed, cfg.image_size, cfg.layers_v, cfg.d_v, cfg.patch, cfg.context, cfg.vocab, cfg.d_t,
                 cfg.heads_t, cfg.layers_t)
    return cfg, sd, model


def rn_case():
    cfg = rn_clip((1, 1, 1, 1), 64, 1024, layers_t=2)
    sd = synth.rn_clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    model = CLIP(cfg.embed, cfg.image_size, tuple(cfg.rn_layers), cfg.rn_width, None, cfg.context, cfg.vocab, cfg.d_t,
                 cfg.heads_t, cfg.layers_t)
    return cfg, sd, model


manifest = {"generator": "tools/make_golden_zsclip2.py", "torch": torch.__version__, "numpy": np.__version__, "files": {}}
for tag, make, dataset, B in (("d2_b3", vit_case, "OxfordPets", 3), ("rn_mini_b3", rn_case, "OxfordPets", 3),
                              ("d2_b3_imagenet", vit_case, "ImageNet", 3)):
    zsclip.ZeroshotCLIP2.templates = list(TEMPLATES0)
    cfg, sd, model = make()
    model = model.float().eval()
    res = model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    zsclip.load_clip_to_cpu = lambda _cfg, _m=model: _m           # the original downloads
    t = object.__new__(zsclip.ZeroshotCLIP2)
    t.cfg = ns(MODEL=ns(BACKBONE=ns(NAME=cfg.name)), DATASET=ns(NAME=dataset))
    t.dm = ns(dataset=ns(classnames=list(OXFORD_PETS_BASE_CLASSES)))
    t.device = "cpu"
    image = torch.from_numpy(synth.images(cfg, B))
    with torch.no_grad():
        t.build_model()
        logits = t.model_inference(image)
        img_f = model.encode_image(image)
        templates = list(t.templates)
        tokens = torch.stack([torch.cat([ref_clip.tokenize(s.format(c.replace("_", " "))) for c in OXFORD_PETS_BASE_CLASSES])
                              for s in templates]).to(torch.int64)
        per_t = torch.stack([model.encode_text(tokens[i]) for i in range(len(templates))])
    T = len(templates)
    assert T == (7 if dataset == "ImageNet" else 8) and tuple(tokens.shape) == (T, len(OXFORD_PETS_BASE_CLASSES), 77)
    name = f"ref_zsclip2_{tag}.npz"
    savez_fixed(os.path.join(GOLD, name), tokens=tokens.numpy(), templates=np.array(templates, dtype=np.str_),
                per_template_features=per_t.numpy(), text_features=t.text_features.numpy(), logits=logits.numpy(),
                image_features=img_f.numpy(), weights_crc=np.bytes_(synth.state_dict_checksum(sd)))
    single = 100.0 * torch.nn.functional.normalize(img_f, dim=-1) @ torch.nn.functional.normalize(per_t[-1], dim=-1).t()
    manifest["files"][name] = dict(source="reference", model=cfg.name, layers_t=cfg.layers_t, dataset=dataset, T=T, B=B,
                                   bytes=os.path.getsize(os.path.join(GOLD, name)))
    print(name, "T", T, "|logits|max", float(logits.abs().max()), "vs last template alone",
          float((logits - single).abs().max()), manifest["files"][name]["bytes"], "bytes")
zsclip.ZeroshotCLIP2.templates = list(TEMPLATES0)

with open(os.path.join(GOLD, "manifest_zsclip2.json"), "w") as f:
    json.dump(manifest, f, indent=1)
    f.write("\n")
