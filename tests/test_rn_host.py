"""Host-side logic of the CLIP ResNet tower: config inference from a state dict, the BatchNorm fold, the FLOP count and
the reference-pinned fixtures (tests/golden/ref_rn_*.npz, tools/make_golden_rn.py).  No GPU needed."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

from rpo_amd import synth  # noqa: E402
from rpo_amd.config import flops_rn_image, rn_clip, rn_plan, vit_b16, vit_l14  # noqa: E402
from rpo_amd.custom_clip import config_from_state_dict  # noqa: E402

RN = {"RN50": ((3, 4, 6, 3), 64, 1024, 224, 512), "RN101": ((3, 4, 23, 3), 64, 512, 224, 512),
      "RN50x4": ((4, 6, 10, 6), 80, 640, 288, 640)}


def _shape_dict(layers, width, embed, res, d_t):
    """Key names and shapes of a CLIP RN state dict as clip/model.py:94-152 builds it (values are never read)."""
    z = lambda *s: np.empty(s, dtype=np.float32)
    sd = {"text_projection": z(d_t, embed), "positional_embedding": z(77, d_t), "token_embedding.weight": z(49408, d_t),
          "ln_final.weight": z(d_t), "logit_scale": z()}
    for l in range(12):
        sd[f"transformer.resblocks.{l}.ln_1.weight"] = z(d_t)
    sd["visual.conv1.weight"] = z(width // 2, 3, 3, 3)
    inpl = width
    for s, n in enumerate(layers):
        p = width * (1 << s)
        for i in range(n):
            sd[f"visual.layer{s + 1}.{i}.conv1.weight"] = z(p, inpl, 1, 1)
            sd[f"visual.layer{s + 1}.{i}.bn1.weight"] = z(p)
            inpl = 4 * p
    sd["visual.attnpool.positional_embedding"] = z((res // 32) ** 2 + 1, width * 32)
    return sd


@pytest.mark.parametrize("name", sorted(RN))
def test_config_from_rn_state_dict_follows_build_model(name):
    layers, width, embed, res, d_t = RN[name]
    cfg = config_from_state_dict(_shape_dict(layers, width, embed, res, d_t), 1, 19)
    # clip/model.py:412-419 + CLIP.__init__ (:252-259): heads = width * 32 // 64, resolution = 32 x the pool grid
    assert cfg.is_rn and cfg.name == name and cfg.rn_layers == layers and cfg.rn_width == width
    assert (cfg.image_size, cfg.embed, cfg.d_v, cfg.heads_v, cfg.n_frozen) == (res, embed, width * 32, width * 32 // 64,
                                                                           (res // 32) ** 2 + 1)
    assert (cfg.d_t, cfg.layers_t, cfg.context) == (d_t, 12, 77)


def test_vit_configs_unchanged():
    for c in (vit_b16(layers_v=2, layers_t=3, K=5), vit_l14(layers_v=1, layers_t=1)):
        sd = synth.clip_state_dict(c, seed=0, token_rows=[49407])
        got = config_from_state_dict(sd, c.K, c.n_cls)
        assert got == c and not got.is_rn and got.vision == "vit"
    assert (vit_b16().n_frozen, vit_b16().patch_dim) == (197, 768)


def test_bn_fold_matches_eval_batchnorm_of_conv():
    from rpo_amd.engine_rn import fold_bn
    g = torch.Generator().manual_seed(0)
    for cin, cout, k in ((16, 32, 3), (64, 24, 1)):
        x = torch.randn(2, cin, 9, 9, generator=g, dtype=torch.float64)
        w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)
        bn = torch.nn.BatchNorm2d(cout).double().eval()
        bn.weight.data = torch.randn(cout, generator=g, dtype=torch.float64)
        bn.bias.data = torch.randn(cout, generator=g, dtype=torch.float64)
        bn.running_mean.data = torch.randn(cout, generator=g, dtype=torch.float64)
        bn.running_var.data = torch.rand(cout, generator=g, dtype=torch.float64) + 0.1
        with torch.no_grad():
            ref = bn(F.conv2d(x, w, padding=k // 2))
        wf, b = fold_bn(w.numpy(), bn.weight.data.numpy(), bn.bias.data.numpy(), bn.running_mean.numpy(), bn.running_var.numpy())
        assert wf.shape == (cout, k, k, cin)                              # [Cout, kh, kw, Cin]
        got = F.conv2d(x, torch.from_numpy(wf).permute(0, 3, 1, 2), padding=k // 2) + torch.from_numpy(b)[None, :, None, None]
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def _flops_from_table(layers, width, embed, R=224):
    """2 FLOP per MAC from the layer table of clip/model.py (stem, Bottlenecks, attention pool), written out directly."""
    conv = lambda h, cin, cout, k: 2.0 * h * h * cin * cout * k * k
    w, h = width, R // 2
    f = conv(h, 3, w // 2, 3) + conv(h, w // 2, w // 2, 3) + conv(h, w // 2, w, 3)
    h, inpl = h // 2, w
    for s, n in enumerate(layers):
        p = w * 2 ** s
        for i in range(n):
            st = 2 if (s and not i) else 1
            f += conv(h, inpl, p, 1) + conv(h, p, p, 3) + conv(h // st, p, 4 * p, 1)
            if i == 0:
                f += conv(h // st, inpl, 4 * p, 1)
            inpl, h = 4 * p, h // st
    C, T = 32 * w, h * h + 1
    return f + 2.0 * T * C * 2 * C + 2.0 * C * C + 4.0 * T * C + 2.0 * C * embed


def test_flops_rn_image():
    for layers, embed, gf in (((3, 4, 6, 3), 1024, 11.586), ((3, 4, 23, 3), 512, 19.009)):
        cfg = rn_clip(layers, 64, embed)
        assert flops_rn_image(cfg) == pytest.approx(_flops_from_table(layers, 64, embed), rel=1e-12)
        assert flops_rn_image(cfg) / 1e9 == pytest.approx(gf, abs=1e-3)
    assert sum(b["down"] for b in rn_plan(rn_clip())) == 4


def test_manifest_rn_byte_counts():
    man = json.load(open(os.path.join(GOLD, "manifest_rn.json")))
    assert man["generator"] == "tools/make_golden_rn.py" and len(man["files"]) == 6
    for name, ent in man["files"].items():
        assert os.path.getsize(os.path.join(GOLD, name)) == ent["bytes"], name


@pytest.mark.parametrize("tag,cfg", [("mini", rn_clip((1, 1, 1, 1), 64, 1024, layers_t=2)), ("rn50", rn_clip()),
                                     ("rn101", rn_clip((3, 4, 23, 3), 64, 512))])
def test_fixture_weights_crc_matches_synth(tag, cfg):
    sd = synth.rn_clip_state_dict(cfg, seed=0, check=False)
    crc = synth.state_dict_checksum(sd)
    files = [f for f in os.listdir(GOLD) if f.startswith(f"ref_rn_") and f"_{tag}_" in f]
    assert files
    for f in files:
        assert bytes(np.load(os.path.join(GOLD, f))["weights_crc"]).decode() == crc, f


def test_unsupported_resnets_are_named_at_load():
    """RN50x4 / RN50x16 have channel counts (stem 40 / 48, planes 80 / 96) the conv kernels refuse: the engine names them
    at load (rpo_amd.engine_rn.rn_unsupported) instead of failing inside the first forward."""
    from rpo_amd.engine_rn import rn_unsupported
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert rn_unsupported(rn_clip(), dt) is None
        assert rn_unsupported(rn_clip((3, 4, 23, 3), 64, 512), dt) is None
        assert rn_unsupported(rn_clip((4, 6, 10, 6), 80, 640, image_size=288), dt) is not None
        assert rn_unsupported(rn_clip((6, 8, 18, 8), 96, 768, image_size=384), dt) is not None


def test_bn_fold_at_trained_statistics():
    """fold_bn against float64 F.batch_norm(F.conv2d(...)) at a trained BatchNorm's statistics: running_var log-uniform
    in [1e-6, 1e3] plus exact zeros (the fold's gain is then 1 / sqrt(eps) = 316), gammas of both signs plus exact zeros
    (dead channels: W' = 0, b' = beta), means up to +-50.  Every element within 1e-12 of |x| (*) |W'| + |b'|: both sides
    are float64 (unit roundoff 1.1e-16) sums of at most 9 * 64 + 2 terms of that magnitude."""
    from helpers import assert_within
    from rpo_amd.engine_rn import fold_bn
    g = torch.Generator().manual_seed(3)
    u = lambda n: torch.rand(n, generator=g, dtype=torch.float64)
    for cin, cout, k in ((16, 40, 3), (64, 24, 1)):
        x = torch.randn(2, cin, 7, 9, generator=g, dtype=torch.float64)
        w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)
        var = torch.exp(math.log(1e-6) + u(cout) * math.log(1e3 / 1e-6))
        var[::7] = 0.0
        gamma = torch.randn(cout, generator=g, dtype=torch.float64)
        gamma[3::5] = 0.0
        beta = torch.randn(cout, generator=g, dtype=torch.float64)
        mean = (2 * u(cout) - 1) * 50.0
        assert var.min() == 0 and var[var > 0].min() < 1e-4 and var.max() > 10 and (gamma > 0).any() and (gamma < 0).any()
        assert (gamma == 0).any() and mean.abs().max() > 25
        ref = F.batch_norm(F.conv2d(x, w, padding=k // 2), mean, var, gamma, beta, False, 0.0, 1e-5)
        wf, b = fold_bn(w.numpy(), gamma.numpy(), beta.numpy(), mean.numpy(), var.numpy())
        assert wf.shape == (cout, k, k, cin) and wf.dtype == np.float64 and b.dtype == np.float64
        wt, bt = torch.from_numpy(wf).permute(0, 3, 1, 2), torch.from_numpy(b)[None, :, None, None]
        got = F.conv2d(x, wt, padding=k // 2) + bt
        mag = F.conv2d(x.abs(), wt.abs(), padding=k // 2) + bt.abs()
        assert_within(got, ref, 1e-12 * mag, f"fold_bn {cin}->{cout} k{k}")
        dead = gamma == 0
        assert bool((got[:, dead] == beta[dead][None, :, None, None]).all())


def _contract_refuses(layers, width, image_size, f32):
    """The kernel contract (include/rpo_amd.h), written out against ModifiedResNet's layer table (clip/model.py:94-152):
    rpo_conv_stem takes Cout % 8 == 0 up to 128; rpo_conv2d_nhwc Cin % 16 (f32) / % 32 (16-bit) == 0 and Cout % 32 == 0;
    the attention pool at most 256 tokens."""
    ck = 16 if f32 else 32
    stem = width // 2
    bad = stem % 8 != 0 or stem > 128
    convs = [(stem, stem), (stem, width)]
    inpl = width
    for s, n in enumerate(layers):
        p = width * 2 ** s
        for i in range(n):
            convs += [(inpl, p), (p, p), (p, 4 * p)]
            if i == 0:
                convs.append((inpl, 4 * p))                 # the downsample branch (stride > 1 or inplanes != 4 planes)
            inpl = 4 * p
    bad = bad or any(ci % ck or co % 32 for ci, co in convs)
    return bad or (image_size // 32) ** 2 + 1 > 256


@pytest.mark.parametrize("width,layers,image_size", [(64, (3, 4, 6, 3), 224), (80, (4, 6, 10, 6), 288),
                                                     (96, (6, 8, 18, 8), 384), (128, (3, 15, 36, 10), 448),
                                                     (64, (1, 1, 1, 1), 480), (64, (1, 1, 1, 1), 512)])
def test_rn_unsupported_follows_the_kernel_contract(width, layers, image_size):
    from rpo_amd.engine_rn import rn_unsupported
    cfg = rn_clip(layers, width, 1024, image_size=image_size)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        want = _contract_refuses(layers, width, image_size, dt == torch.float32)
        assert (rn_unsupported(cfg, dt) is not None) == want, (width, image_size, dt)
    # widths 64 and 128 run, 80 (stem 40) and 96 (stem 48: Cout % 32) do not; 512 px gives 257 tokens
    assert _contract_refuses(layers, width, image_size, True) == (width in (80, 96) or image_size == 512)
