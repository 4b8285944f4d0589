#!/usr/bin/env python3
"""Golden vectors of the linear probe from the REAL reference (`trainers/linear_prob.py`: CustomCLIP :61-95 on the synthetic
CLIP weights of rpo_amd/synth.py, + F.cross_entropy + backward + torch.optim.SGD), for rpo_amd/lp.py.  Writes, under
tests/golden/:

  ref_lp_d2_b3.npz     depth 2, B = 3, the 19 Oxford-Pets base classes; two (W, b) cases: c0 = the reference's identity
                       init (saturated softmax), c1 = W = 0.01 eye + N(0, 1e-3), b = N(0, 1e-2) (logits O(1-10)).  Per case:
                       eval logits, loss, the gradients, and a 4-step SGD trajectory (lr 5e-4, momentum 0.9, wd 5e-4) on
                       four seeded batches: per-step losses and gradient factors, final b, rows 0-7 and the diagonal of
                       the final W.
  ref_lp_full_b32.npz  full ViT-B/16, B = 32, identity init: logits, loss, gradients.
  ref_lp_ckpt.npz      the reference's lp_layer after one SGD step from the identity: the layout of the dict its run saved
                       (keys, optimizer param groups, scheduler state), the step's gradient factors, rows 0-7 and the
                       diagonal of W and of its momentum, and the eval logits of the layer.
  manifest_lp.json     provenance (generator, torch, byte counts).

Size: a dense 512 x 512 fp32 matrix is 1 MB, so no fixture holds one (tests/lp_fixtures.py).  lp_layer.weight.grad =
dz^T . image_features has rank B: it is stored as its two factors -- `dz` (the gradient of lp_layer's output, captured
with retain_grad) and the image features -- and W after SGD steps as the per-step factors, from which
tests/lp_fixtures.sgd_replay rebuilds it; both reconstructions are checked here against the reference's own dense tensors
before anything is written, and tests/lp_fixtures.write_reference_checkpoint rebuilds the reference's checkpoint file.
W0 of case c1 is re-created from its seed by whoever reads it (its CRC32 is stored).  The token ids of the
"A photo of a {cls_name}" prompts are stored too (the tokenizer is out of scope on the other side).  Runs in the build
container only (imports the reference through make_golden._reference)."""
import json
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from make_golden import _reference, REPO          # noqa: E402  (stubs the absent dassl / yacs imports, nothing copied)
from rpo_amd import synth                         # noqa: E402
from rpo_amd.config import OXFORD_PETS_BASE_CLASSES, vit_b16  # noqa: E402
from lp_fixtures import c1_init, grads, sgd_replay, write_reference_checkpoint  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
SGD = (5e-4, 0.9, 5e-4)                           # the ctxv1 yaml's LR; Dassl's momentum / weight decay
TRAJ_SEEDS = [(1234 + 10 * s, 4321 + 10 * s) for s in range(4)]      # (images, labels) seeds of the four steps
SAMPLE_ROWS = 8                                   # dense rows of a reference W stored for a direct comparison


def build(ref_lp, CLIP, cfg, sd):
    clip_model = CLIP(cfg.embed, cfg.image_size, cfg.layers_v, cfg.d_v, cfg.patch, cfg.context, cfg.vocab, cfg.d_t,
                      cfg.heads_t, cfg.layers_t).float()                 # PREC fp32: clip_model.float() (:117-119)
    clip_model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    rcfg = types.SimpleNamespace(TRAINER=types.SimpleNamespace(LP=types.SimpleNamespace(PROMPT="A photo of a {cls_name}",
                                                                                         PREC="fp32")))
    model = ref_lp.CustomCLIP(rcfg, list(OXFORD_PETS_BASE_CLASSES), clip_model)
    for name, p in model.named_parameters():                             # :128-134
        p.requires_grad_("lp_layer" in name)
    return model


def fwd_bwd(model, image, label):
    """loss, dz, x of one training forward + backward (gradients left in lp_layer's .grad); the factors are checked
    against the reference's dense weight.grad / bias.grad."""
    feats = {}

    def hook(mod, inp, out):
        feats["x"] = inp[0].detach().clone()
        out.retain_grad()
        feats["z"] = out
    h = model.lp_layer.register_forward_hook(hook)
    lp = model.lp_layer
    lp.weight.grad = lp.bias.grad = None
    loss = torch.nn.functional.cross_entropy(model(image), label)
    loss.backward()
    h.remove()
    dz, x = feats["z"].grad.detach().clone(), feats["x"]
    gw, gb = grads(dz.numpy(), x.numpy())
    err = float(np.abs(gw - lp.weight.grad.numpy()).max() / max(float(lp.weight.grad.abs().max()), 1e-30))
    errb = float(np.abs(gb - lp.bias.grad.numpy()).max() / max(float(lp.bias.grad.abs().max()), 1e-30))
    assert err <= 1e-5 and errb <= 1e-5, f"dz^T x differs from weight.grad by {err:.2e}, sum dz from bias.grad by {errb:.2e}"
    return loss.detach(), dz, x


def train_eval(model, image, label):
    """(eval logits, loss, dz, weight.grad, bias.grad, image features) of one forward / backward."""
    with torch.no_grad():
        logits = model(image).clone()
    loss, dz, x = fwd_bwd(model, image, label)
    lp = model.lp_layer
    return logits, loss, dz, lp.weight.grad.clone(), lp.bias.grad.clone(), x


def dense_sample(w: np.ndarray) -> dict:
    return dict(rows=np.ascontiguousarray(w[:SAMPLE_ROWS]), diag=np.ascontiguousarray(np.diag(w)))


def check_replay(got: np.ndarray, want: np.ndarray, what: str) -> None:
    want = np.asarray(want, np.float64)
    err = float(np.abs(np.asarray(got, np.float64) - want).max()) / max(1.0, float(np.abs(want).max()))
    assert err <= 1e-6, f"{what}: the SGD replay over the stored factors is {err:.2e} off the reference (relative to max(1, |x|))"


def main():
    torch.manual_seed(0)
    ref_clip, CLIP, _ = _reference()
    import trainers.linear_prob as ref_lp         # noqa: E402
    os.makedirs(GOLD, exist_ok=True)
    manifest = {}
    lr, mom, wd = SGD

    # ---- depth 2, B = 3: two (W, b) cases, gradients and a 4-step trajectory
    cfg = vit_b16(layers_v=2, layers_t=2, K=1)
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    model = build(ref_lp, CLIP, cfg, sd)
    B, e = 3, cfg.embed
    image = torch.from_numpy(synth.images(cfg, B))
    label = torch.from_numpy(synth.labels(cfg, B))
    toks = ref_clip.tokenize(model.prompts).numpy().astype(np.int64)
    rec = dict(tokenized_prompts=toks, text_features=model.text_features.numpy(), label=label.numpy(),
               sgd_hparams=np.asarray(SGD, dtype=np.float64), traj_seeds=np.asarray(TRAJ_SEEDS, dtype=np.int64),
               c1_seed=np.int64(2024), weights_crc=np.bytes_(synth.state_dict_checksum(sd)))
    w1, b1 = c1_init(e)
    rec["c1_w0_crc32"] = np.int64(zlib.crc32(w1.tobytes()))
    for case, (w0, b0) in enumerate(((np.eye(e, dtype=np.float32), np.zeros(e, np.float32)), (w1, b1))):
        lp = model.lp_layer
        lp.weight.data = torch.from_numpy(w0.copy())
        lp.bias.data = torch.from_numpy(b0.copy())
        logits, loss, dz, gw, gb, x = train_eval(model, image, label)
        p = f"c{case}_"
        rec.update({p + "logits": logits.numpy(), p + "loss": np.float32(loss.item()), p + "dz": dz.numpy(),
                    p + "g_bias": gb.numpy(), p + "b0": b0})
        rec["image_features"] = x.numpy()
        opt = torch.optim.SGD(lp.parameters(), lr=lr, momentum=mom, weight_decay=wd)
        losses, dzs, xs = [], [], []
        for si, li in TRAJ_SEEDS:
            im = torch.from_numpy(synth.images(cfg, B, seed=si))
            lb = torch.from_numpy(synth.labels(cfg, B, seed=li))
            l_, dz_k, x_k = fwd_bwd(model, im, lb)
            opt.step()
            losses.append(l_.item())
            dzs.append(dz_k.numpy())
            xs.append(x_k.numpy())
        w_fin, b_fin = lp.weight.detach().numpy().copy(), lp.bias.detach().numpy().copy()
        rw, rb, _, _ = sgd_replay(w0, b0, dzs, xs, lr, mom, wd)
        check_replay(rw, w_fin, f"case {case} W")
        check_replay(rb, b_fin, f"case {case} b")
        smp = dense_sample(w_fin)
        rec.update({p + "traj_losses": np.asarray(losses, dtype=np.float32), p + "traj_dz": np.stack(dzs),
                    p + "traj_x": np.stack(xs), p + "b_final": b_fin, p + "w_final_rows": smp["rows"],
                    p + "w_final_diag": smp["diag"]})
        print(f"d2_b3 case {case}: loss {loss.item():.4f} |logits|max {float(logits.abs().max()):.2f} "
              f"|g_w|max {float(gw.abs().max()):.3e} traj {np.round(losses, 4).tolist()}", flush=True)
    path = os.path.join(GOLD, "ref_lp_d2_b3.npz")
    np.savez_compressed(path, **rec)
    manifest["ref_lp_d2_b3.npz"] = dict(source="reference", model="ViT-B/16", depth=2, B=B, bytes=os.path.getsize(path))

    # ---- the checkpoint: identity init, one SGD step on the first trajectory batch, Dassl's dict
    lp = model.lp_layer
    lp.weight.data = torch.eye(e)
    lp.bias.data = torch.zeros(e)
    opt = torch.optim.SGD(lp.parameters(), lr=lr, momentum=mom, weight_decay=wd)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=30)
    si, li = TRAJ_SEEDS[0]
    _, dz, x = fwd_bwd(model, torch.from_numpy(synth.images(cfg, B, seed=si)), torch.from_numpy(synth.labels(cfg, B, seed=li)))
    opt.step()
    sched.step()
    ck = {"state_dict": lp.state_dict(), "epoch": 1, "optimizer": opt.state_dict(), "scheduler": sched.state_dict(),
          "val_result": None}
    layout = dict(keys=list(ck), epoch=ck["epoch"], val_result=ck["val_result"],
                  param_groups=ck["optimizer"]["param_groups"], scheduler=ck["scheduler"],
                  state_keys={str(i): sorted(v) for i, v in ck["optimizer"]["state"].items()})
    with torch.no_grad():
        ck_logits = model(image).numpy()
    mw = ck["optimizer"]["state"][0]["momentum_buffer"].numpy()
    mb = ck["optimizer"]["state"][1]["momentum_buffer"].numpy()
    rw, rb, rmw, rmb = sgd_replay(np.eye(e), np.zeros(e), [dz.numpy()], [x.numpy()], lr, mom, wd)
    for got, want, what in ((rw, lp.weight, "W"), (rb, lp.bias, "b"), (rmw, mw, "momentum W"), (rmb, mb, "momentum b")):
        check_replay(got, torch.as_tensor(want).detach().numpy(), f"checkpoint {what}")
    path = os.path.join(GOLD, "ref_lp_ckpt.npz")
    sw, smw = dense_sample(lp.weight.detach().numpy()), dense_sample(mw)
    np.savez_compressed(path, layout=np.bytes_(json.dumps(layout)), dz=dz.numpy(), x=x.numpy(),
                        sgd_hparams=np.asarray(SGD, dtype=np.float64), w_rows=sw["rows"], w_diag=sw["diag"],
                        mom_w_rows=smw["rows"], mom_w_diag=smw["diag"], bias=lp.bias.detach().numpy(), mom_b=mb,
                        logits=ck_logits, image_seed=np.int64(1234), B=np.int64(B))
    # the rebuilt file gives the reference's logits
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        rebuilt = torch.load(write_reference_checkpoint(path, tmp), weights_only=True)
    lp.load_state_dict(rebuilt["state_dict"])
    with torch.no_grad():
        err = float(np.abs(model(image).numpy() - ck_logits).max())
    assert err <= 1e-4 * max(1.0, float(np.abs(ck_logits).max())), f"rebuilt checkpoint: logits {err:.2e} off"
    manifest["ref_lp_ckpt.npz"] = dict(source="reference", bytes=os.path.getsize(path))
    print("ckpt: |logits|max", float(np.abs(ck_logits).max()), "rebuilt file logits err", err, flush=True)
    del model

    # ---- full ViT-B/16, B = 32, identity init
    cfg = vit_b16(K=1)
    sd = synth.clip_state_dict(cfg, seed=0)
    model = build(ref_lp, CLIP, cfg, sd)
    B = 32
    image = torch.from_numpy(synth.images(cfg, B))
    label = torch.from_numpy(synth.labels(cfg, B))
    logits, loss, dz, gw, gb, x = train_eval(model, image, label)
    path = os.path.join(GOLD, "ref_lp_full_b32.npz")
    np.savez_compressed(path, tokenized_prompts=ref_clip.tokenize(model.prompts).numpy().astype(np.int64),
                        text_features=model.text_features.numpy(), image_features=x.numpy(), label=label.numpy(),
                        logits=logits.numpy(), loss=np.float32(loss.item()), dz=dz.numpy(), g_bias=gb.numpy(),
                        weights_crc=np.bytes_(synth.state_dict_checksum(sd)))
    manifest["ref_lp_full_b32.npz"] = dict(source="reference", model="ViT-B/16", depth=12, B=B, bytes=os.path.getsize(path))
    print(f"full_b32: loss {loss.item():.4f} |logits|max {float(logits.abs().max()):.2f}", flush=True)

    with open(os.path.join(GOLD, "manifest_lp.json"), "w") as f:
        json.dump(dict(generator="tools/make_golden_lp.py", torch=torch.__version__, numpy=np.__version__, files=manifest),
                  f, indent=1)


if __name__ == "__main__":
    main()
