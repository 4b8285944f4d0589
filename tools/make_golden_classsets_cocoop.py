#!/usr/bin/env python3
"""Golden vector for CoCoOp's conditional class sets (rpo_amd/engine_cocoop_eval.py) from the real
reference: `trainers/cocoop.py`'s CustomCLIP rebuilt around the 18 Oxford-Pets "new" classes (as `subsample_classes`
splits the 37, datasets/oxford_pets.py) on the `d2_k8_b3` workload of tests/helpers.py, with a GIVEN context (n_ctx 4)
and a seeded meta-net, prompt learner in eval() mode.  Writes, under tests/golden/:

  ref_classset_cocoop.npz           tokens [18, 77], ctx, the four meta-net tensors, logits [3, 18], the weights' CRC
  manifest_classsets_cocoop.json    provenance (generator, torch, byte counts)

The meta-net's b1 is moved off the ReLU kink unit by unit, as `_sibling_case` of tests/test_gpu_model.py does: a 16-bit
image tower moves the pre-activations by a fraction of a percent of their spread, and a unit that flips between the
reference and the device would move every logit of that image.  Runs in the build container only (imports the reference
through make_golden._reference, copies nothing); no test runs it.  The .npz members carry a fixed timestamp."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from make_golden import _reference, REPO          # noqa: E402  (nothing copied)
from make_golden_classsets import B, DEPTH, K, N_CTX, NEW_CLASSES, clip_of, savez_fixed     # noqa: E402
from rpo_amd import synth                         # noqa: E402
from rpo_amd.config import vit_b16                # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
ns = types.SimpleNamespace
NAME = "ref_classset_cocoop.npz"


def main():
    torch.manual_seed(0)
    _, CLIP, _ = _reference()
    import trainers.cocoop as ref_cocoop          # noqa: E402
    cfg = vit_b16(layers_v=DEPTH, layers_t=DEPTH, K=K)
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    image = torch.from_numpy(synth.images(cfg, B))
    rcfg = ns(TRAINER=ns(COCOOP=ns(N_CTX=N_CTX, CTX_INIT="", PREC="fp32")), INPUT=ns(SIZE=(cfg.image_size, cfg.image_size)))
    model = ref_cocoop.CustomCLIP(rcfg, list(NEW_CLASSES), clip_of(CLIP, cfg, sd))
    e, h, dt = cfg.embed, cfg.embed // 16, cfg.d_t
    rng = np.random.default_rng(41)
    u = lambda shape, fan: rng.uniform(-fan ** -0.5, fan ** -0.5, shape).astype(np.float32)    # nn.Linear's default ranges
    vals = dict(ctx=(rng.standard_normal((N_CTX, dt)) * 0.02).astype(np.float32),
                w1=u((h, e), e), b1=u((h,), e), w2=u((dt, h), h), b2=u((dt,), h))
    with torch.no_grad():
        imf = model.image_encoder(image)
    a = (imf / imf.norm(dim=-1, keepdim=True)).double().numpy() @ vals["w1"].T.astype(np.float64)
    margin = 0.03 * float(np.abs(a).max())
    for j in range(h):
        shift = next(k * margin for k in sorted(range(-B - 1, B + 2), key=abs)
                     if np.abs(a[:, j] + vals["b1"][j] + k * margin).min() >= margin)
        vals["b1"][j] += np.float32(shift)
    pre = a + vals["b1"].astype(np.float64)
    assert np.abs(pre).min() >= 0.99 * margin and (pre < 0).any() and (pre > 0).any()
    pl = model.prompt_learner
    pl.ctx.data = torch.from_numpy(vals["ctx"].copy())
    pl.meta_net.linear1.weight.data = torch.from_numpy(vals["w1"].copy())
    pl.meta_net.linear1.bias.data = torch.from_numpy(vals["b1"].copy())
    pl.meta_net.linear2.weight.data = torch.from_numpy(vals["w2"].copy())
    pl.meta_net.linear2.bias.data = torch.from_numpy(vals["b2"].copy())
    model.eval()
    with torch.no_grad():
        logits = model(image)
    assert tuple(logits.shape) == (B, len(NEW_CLASSES))
    path = os.path.join(GOLD, NAME)
    savez_fixed(path, classnames=np.array(NEW_CLASSES, dtype=np.str_), weights_crc=np.bytes_(synth.state_dict_checksum(sd)),
                tokens=model.tokenized_prompts.numpy().astype(np.int64), logits=logits.numpy(), n_ctx=np.int64(N_CTX),
                relu_margin=np.float64(margin), **vals)
    files = {NAME: dict(source="reference", model=cfg.name, depth=DEPTH, B=B, n_cls=len(NEW_CLASSES),
                        bytes=os.path.getsize(path))}
    print(NAME, "|logits|max", float(np.abs(logits.numpy()).max()), files[NAME]["bytes"], "bytes", flush=True)
    with open(os.path.join(GOLD, "manifest_classsets_cocoop.json"), "w") as f:
        json.dump(dict(generator="tools/make_golden_classsets_cocoop.py", torch=torch.__version__, numpy=np.__version__,
                       files=files), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
