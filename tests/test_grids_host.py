"""Both ends of the ViT patch-grid range on the host: ViT-B/32 (7 x 7 grid) and ViT-L/14 at 336 px (24 x 24 grid, 577
frozen tokens).  The oracle against the reference's own outputs (tools/make_golden_grids.py) at the tolerances
tests/test_oracle_golden.py holds it to for the depth-2 ViT-L/14 fixture, the two configs, and the paths that refuse
above the 288-token limit of rpo_attn_prompt_fwd where they are set up."""
import json
import os
import types

import numpy as np
import pytest
import torch

from oracle import rpo_oracle
from rpo_amd import synth
from rpo_amd.config import vit_b32, vit_l14_336

from helpers import GOLDEN

D2 = dict(layers_v=2, layers_t=2)
GRIDS = {"vitl14_336": (vit_l14_336, 2), "vitb32": (vit_b32, 3)}       # tag -> (config, batch of its fixtures)


def gold(name):
    return dict(np.load(os.path.join(GOLDEN, f"ref_{name}.npz")))


def test_configs_of_both_grids():
    b, l = vit_b32(), vit_l14_336()
    assert (b.n_frozen, b.patch_dim, b.grid, b.d_v, b.name) == (50, 3072, 7, 768, "ViT-B/32")
    assert (l.n_frozen, l.patch_dim, l.grid, l.d_v, l.name) == (577, 588, 24, 1024, "ViT-L/14@336px")
    assert (l.layers_v, l.d_t, l.embed, l.heads_v) == (24, 768, 768, 16) and vit_l14_336(K=4).seq_v == 581


@pytest.mark.parametrize("make", [vit_b32, vit_l14_336])
def test_config_from_state_dict_round_trips(make):
    from rpo_amd.custom_clip import config_from_state_dict
    cfg = make(K=24, **D2)
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=[0, 49407])
    assert config_from_state_dict(sd, cfg.K, cfg.n_cls) == cfg


def test_manifest_grids_matches_the_committed_fixtures():
    man = json.load(open(os.path.join(GOLDEN, "manifest_grids.json")))["cases"]
    assert sorted(man) == sorted(["vitl14_336_d2_k24_b2", "vitb32_d2_k24_b3", "plainclip_vitl14_336_d2_b2",
                                  "plainclip_vitb32_d2_b3", "coop_vitb32_d2_b3_ctx16"])
    for tag, rec in man.items():
        size = os.path.getsize(os.path.join(GOLDEN, f"ref_{tag}.npz"))
        assert size == rec["bytes"] and size <= 1 << 20, tag


@pytest.mark.parametrize("tag,name", [("vitl14_336", "vitl14_336_d2_k24_b2"), ("vitb32", "vitb32_d2_k24_b3")])
def test_rpo_oracle_matches_reference_at_both_grids(tag, name):
    """trainers/rpo.py's own CustomCLIP (forward and autograd) at the grid, through the outside-supplied literals: eval
    logits, loss, both prompt gradients and -- 336 px -- the prompt rows after every block of both towers."""
    make, B = GRIDS[tag]
    g = gold(name)
    cfg = make(K=24, **D2)
    toks = synth.oxford_pets_base_tokens()
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
    assert synth.state_dict_checksum(sd) == g["weights_crc"].item().decode()
    tp, ip = synth.prompts(cfg, sd, seed=7)
    m = rpo_oracle.OracleRPO(sd, toks, cfg.K, cfg.patch)
    m.set_prompts(tp, ip)
    image, label = synth.images(cfg, B), synth.labels(cfg, B)
    assert image.shape[-1] == cfg.image_size and np.array_equal(label, g["label"])
    if "img_rows" in g:
        with torch.no_grad():
            _, trows = m.text_tower(m.text_prompt, return_rows=True)
            _, irows = m.image_tower(torch.from_numpy(image), m.img_prompt, return_rows=True)
        nc = g["text_rows"].shape[1]
        np.testing.assert_allclose(torch.stack(trows).numpy()[:, :nc], g["text_rows"], atol=3e-5)
        np.testing.assert_allclose(torch.stack(irows).numpy(), g["img_rows"], atol=3e-5)
    out, gt, gi = m.loss_and_grads(image, label)
    np.testing.assert_allclose(out.logits.detach().numpy(), g["logits"], atol=3e-5, rtol=0)
    assert abs(float(out.loss) - float(g["loss"])) < 2e-5
    for mine, ref in ((gt.numpy(), g["g_text"]), (gi.numpy(), g["g_img"])):
        assert np.abs(mine - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("tag,name", [("vitl14_336", "plainclip_vitl14_336_d2_b2"), ("vitb32", "plainclip_vitb32_d2_b3")])
def test_plain_clip_oracle_matches_reference_at_both_grids(tag, name):
    make, B = GRIDS[tag]
    g = gold(name)
    cfg = make(K=1, **D2)
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    assert g["weights_crc"].item().decode() == synth.state_dict_checksum(sd)
    logits, img_f, txt_f = rpo_oracle.plain_clip_forward(sd, synth.images(cfg, B), synth.oxford_pets_base_tokens(), cfg.patch)
    np.testing.assert_allclose(logits.numpy(), g["logits"], atol=3e-5, rtol=0)
    assert np.abs(img_f.numpy() - g["image_features"]).max() <= 2e-5 * max(1.0, np.abs(g["image_features"]).max())
    assert np.abs(txt_f.numpy() - g["text_features"]).max() <= 2e-5 * max(1.0, np.abs(g["text_features"]).max())


def test_coop_oracle_matches_reference_at_patch_32():
    g = gold("coop_vitb32_d2_b3_ctx16")
    cfg = vit_b32(K=1, **D2)
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    assert g["weights_crc"].item().decode() == synth.state_dict_checksum(sd)
    assert g["ctx"].shape == (16, cfg.d_t) and sorted(g) == sorted(gold("coop_d2_b2_ctx16"))
    logits, loss, grad = rpo_oracle.coop_loss_and_grad(sd, synth.images(cfg, 3), g["tokenized_prompts"], g["ctx"], g["label"],
                                                       cfg.patch)
    np.testing.assert_allclose(logits.numpy(), g["logits"], atol=3e-5, rtol=0)
    assert abs(float(loss) - float(g["loss"])) < 2e-5
    assert np.abs(grad.numpy() - g["ctx_grad"]).max() <= 2e-5 * max(1.0, np.abs(g["ctx_grad"]).max())


def test_the_336px_fixture_has_the_keys_of_the_224px_one():
    assert sorted(gold("vitl14_336_d2_k24_b2")) == sorted(gold("vitl14_d2_k24_b2"))


# ---- what stops at the 288-token limit of rpo_attn_prompt_fwd refuses where it is set up ---------------------------
def test_shared_frozen_row_paths_refuse_above_288_tokens_before_any_device_work(monkeypatch):
    from rpo_amd import engine, loop, multi, sweep, trainer
    from rpo_amd.engine_prompt_rows import PromptRowsEngineMixin
    from rpo_amd.frozen_kv import FrozenImageKV
    touched = []
    monkeypatch.setattr(engine, "make_engine", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(torch.cuda, "device", lambda *a, **k: touched.append(2))
    cfg = vit_l14_336(K=24, **D2)
    msg = "577 frozen tokens.*288-token limit of rpo_attn_prompt_fwd"

    class Eng(PromptRowsEngineMixin):
        act, max_batch = torch.bfloat16, 4

        def __init__(self, cfg):
            self.cfg = cfg

        def _refuse_rn(self, what):
            pass

    images = [np.zeros((8, 8, 3), np.uint8)] * 3
    with pytest.raises(NotImplementedError, match=msg):
        Eng(cfg).prompt_rows_setup(2, 4)
    with pytest.raises(NotImplementedError, match=msg):
        FrozenImageKV.build(Eng(cfg), images)

    def bare(cls):
        t = object.__new__(cls)
        t.cfg, t.engine = cfg, Eng(cfg)
        return t

    with pytest.raises(NotImplementedError, match=msg):
        bare(trainer.RPO).test(images, frozen=object())
    with pytest.raises(NotImplementedError, match=msg):
        bare(trainer.RPO).train(images, max_epoch=1, val_set=images, val_frozen=object())
    with pytest.raises(NotImplementedError, match=msg):
        bare(multi.RPOMulti).test_all(images)
    with pytest.raises(NotImplementedError, match=msg):
        bare(sweep.RPOSweep).test(images)
    assert not touched, "a refusal came after device work"
    # up to 288 tokens nothing is refused here
    from rpo_amd.config import refuse_long_grid, vit_b16, vit_l14
    for ok in (vit_b32(), vit_b16(), vit_l14(), cfg.with_(image_size=224)):
        refuse_long_grid(ok, "x")
    with pytest.raises(NotImplementedError, match="1025 frozen tokens"):
        refuse_long_grid(cfg.with_(image_size=448), "x")
