#!/usr/bin/env python3
"""Golden vectors of CLIP with a ResNet image tower (clip/model.py:10-152, ModifiedResNet) from the real reference:
`clip.model.CLIP.forward` (what trainers/zsclip.py:58-63 runs) and CoOp's CustomCLIP + F.cross_entropy + backward
(trainers/coop.py:196-208, :266-270) on the weights of `synth.rn_clip_state_dict`, loaded with strict=True into the
reference's CLIP(..., vision_layers=<tuple>, ...).  Outputs only (no weights) go to tests/golden/ref_rn_*.npz, each with
the `weights_crc` of its state dict; tests/golden/manifest_rn.json records versions and byte counts.  Runs in the build
container only (needs the reference)."""
import json, os, sys, types
import numpy as np, torch
import torch.nn.functional as F
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _reference, REPO          # noqa: E402  (stubs the absent dassl / yacs imports, nothing copied)
from rpo_amd import synth                         # noqa: E402
from rpo_amd.config import OXFORD_PETS_BASE_CLASSES, rn_clip  # noqa: E402

ref_clip, CLIP, _ = _reference()
import trainers.coop as ref_coop                  # noqa: E402
GOLD = os.path.join(REPO, "tests", "golden")
toks = synth.oxford_pets_base_tokens()
ns = types.SimpleNamespace
# tag -> config: a reduced RN (one block per stage, text depth 2), RN50, RN101 (CLIP's text tower: 512 wide, 12 layers)
CFGS = {"mini": rn_clip((1, 1, 1, 1), 64, 1024, layers_t=2), "rn50": rn_clip(), "rn101": rn_clip((3, 4, 23, 3), 64, 512)}


def reference_clip(cfg, sd):
    model = CLIP(cfg.embed, cfg.image_size, tuple(cfg.rn_layers), cfg.rn_width, None, cfg.context, cfg.vocab, cfg.d_t,
                 cfg.heads_t, cfg.layers_t).float().eval()
    res = model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model


manifest_path = os.path.join(GOLD, "manifest_rn.json")
manifest = {"generator": "tools/make_golden_rn.py", "torch": torch.__version__, "numpy": np.__version__, "files": {}}
sds = {}
for tag, B in (("mini", 3), ("rn50", 4), ("rn101", 2)):
    cfg = CFGS[tag]
    sd = sds[tag] = synth.rn_clip_state_dict(cfg, seed=0)
    model = reference_clip(cfg, sd)
    image = torch.from_numpy(synth.images(cfg, B))
    text = torch.from_numpy(toks)
    with torch.no_grad():
        logits, _ = model(image, text)
        img_f, txt_f = model.encode_image(image), model.encode_text(text)
    name = f"ref_rn_plainclip_{tag}_b{B}.npz"
    np.savez_compressed(os.path.join(GOLD, name), logits=logits.numpy(), image_features=img_f.numpy(),
                        text_features=txt_f.numpy(), weights_crc=np.bytes_(synth.state_dict_checksum(sd)))
    manifest["files"][name] = dict(source="reference", model=cfg.name, layers=list(cfg.rn_layers), layers_t=cfg.layers_t,
                                   B=B, bytes=os.path.getsize(os.path.join(GOLD, name)))
    print(name, "|logits|max", float(logits.abs().max()), manifest["files"][name]["bytes"], "bytes")

# CoOp (generic context, class token at the end: configs/trainers/CoOp/rn50.yaml's defaults): logits, loss, d loss / d ctx
for tag, B, n_ctx in (("mini", 3, 4), ("mini", 3, 16)):
    cfg, sd = CFGS[tag], sds[tag]
    clip_model = reference_clip(cfg, sd)
    rcfg = ns(TRAINER=ns(COOP=ns(N_CTX=n_ctx, CTX_INIT="", CSC=False, CLASS_TOKEN_POSITION="end", PREC="fp32")),
              INPUT=ns(SIZE=(cfg.image_size, cfg.image_size)))
    model = ref_coop.CustomCLIP(rcfg, list(OXFORD_PETS_BASE_CLASSES), clip_model)
    for pname, p in model.named_parameters():
        p.requires_grad_("prompt_learner" in pname)              # trainers/coop.py:228-230
    ctx = (np.random.default_rng(11).standard_normal((n_ctx, cfg.d_t)) * 0.02).astype(np.float32)
    model.prompt_learner.ctx.data = torch.from_numpy(ctx.copy())
    image = torch.from_numpy(synth.images(cfg, B))
    label = torch.from_numpy(synth.labels(cfg, B))
    logits = model(image)
    loss = F.cross_entropy(logits, label)
    loss.backward()
    name = f"ref_rn_coop_{tag}_b{B}_ctx{n_ctx}.npz"
    np.savez_compressed(os.path.join(GOLD, name), logits=logits.detach().numpy(), loss=np.float32(loss.item()), ctx=ctx,
                        ctx_grad=model.prompt_learner.ctx.grad.numpy(), label=label.numpy(),
                        tokenized_prompts=model.tokenized_prompts.numpy().astype(np.int64),
                        weights_crc=np.bytes_(synth.state_dict_checksum(sd)))
    manifest["files"][name] = dict(source="reference", model=cfg.name, B=B, n_ctx=n_ctx,
                                   bytes=os.path.getsize(os.path.join(GOLD, name)))
    print(name, "loss", float(loss), manifest["files"][name]["bytes"], "bytes")

# CoOp on RN50 at configs/trainers/CoOp/rn50.yaml's train batch 32, n_ctx 16: logits, loss and ctx.grad of the first
# batch, then the context after each of 3 steps of torch.optim.SGD at rn50.yaml's LR 0.002 with the momentum / weight
# decay of the repo's OptimConfig defaults (0.9 / 5e-4); batch s uses images seed 70 + s, labels seed 80 + s
from rpo_amd.trainer import OptimConfig  # noqa: E402
cfg, sd, B, n_ctx = CFGS["rn50"], sds["rn50"], 32, 16
clip_model = reference_clip(cfg, sd)
rcfg = ns(TRAINER=ns(COOP=ns(N_CTX=n_ctx, CTX_INIT="", CSC=False, CLASS_TOKEN_POSITION="end", PREC="fp32")),
          INPUT=ns(SIZE=(cfg.image_size, cfg.image_size)))
model = ref_coop.CustomCLIP(rcfg, list(OXFORD_PETS_BASE_CLASSES), clip_model)
for pname, p in model.named_parameters():
    p.requires_grad_("prompt_learner" in pname)
ctx = (np.random.default_rng(11).standard_normal((n_ctx, cfg.d_t)) * 0.02).astype(np.float32)
model.prompt_learner.ctx.data = torch.from_numpy(ctx.copy())
oc = OptimConfig()
opt = torch.optim.SGD([model.prompt_learner.ctx], lr=0.002, momentum=oc.momentum, weight_decay=oc.weight_decay)
out, traj, losses = {}, [], []
for step in range(3):
    image = torch.from_numpy(synth.images(cfg, B, seed=70 + step))
    label = torch.from_numpy(synth.labels(cfg, B, seed=80 + step))
    opt.zero_grad()
    logits = model(image)
    loss = F.cross_entropy(logits, label)
    loss.backward()
    if step == 0:
        out = dict(logits=logits.detach().numpy(), loss=np.float32(loss.item()), label=label.numpy(),
                   ctx_grad=model.prompt_learner.ctx.grad.numpy().copy())
    opt.step()
    losses.append(float(loss))
    traj.append(model.prompt_learner.ctx.detach().numpy().copy())
name = "ref_rn_coop_rn50_b32_ctx16.npz"
np.savez_compressed(os.path.join(GOLD, name), ctx=ctx, traj_ctx=np.stack(traj), traj_loss=np.asarray(losses, np.float32),
                    lr=np.float32(0.002), momentum=np.float32(oc.momentum), weight_decay=np.float32(oc.weight_decay),
                    tokenized_prompts=model.tokenized_prompts.numpy().astype(np.int64),
                    weights_crc=np.bytes_(synth.state_dict_checksum(sd)), **out)
manifest["files"][name] = dict(source="reference", model=cfg.name, B=B, n_ctx=n_ctx, sgd_steps=3,
                               bytes=os.path.getsize(os.path.join(GOLD, name)))
print(name, "losses", losses, manifest["files"][name]["bytes"], "bytes")

with open(manifest_path, "w") as f:
    json.dump(manifest, f, indent=1)
    f.write("\n")
