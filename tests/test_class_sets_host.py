"""Class sets on the host (rpo_amd/class_set.py): the reference fixtures of the 18 Oxford-Pets new
classes (tests/golden/ref_classset_*.npz, tools/make_golden_classsets.py) and their manifest, the oracle on foreign tokens
against them, the pure CoOp layout rule, the harmonic mean, and the C ABI's bookkeeping for rpo_text_embed."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle.rpo_oracle import OracleRPO, coop_loss_and_grad, plain_clip_forward
from rpo_amd import synth
from rpo_amd.config import vit_b16

from helpers import CASES, GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("ref_classset_rpo.npz", "ref_classset_coop_end.npz", "ref_classset_coop_middle.npz", "ref_classset_zeroshot.npz",
         "ref_classset_lp.npz")
NEW_CLASSES = ("leonberger", "maine_coon", "miniature_pinscher", "newfoundland", "persian", "pomeranian", "pug", "ragdoll",
               "russian_blue", "saint_bernard", "samoyed", "scottish_terrier", "shiba_inu", "siamese", "sphynx",
               "staffordshire_bull_terrier", "wheaten_terrier", "yorkshire_terrier")


def gold(name):
    return dict(np.load(os.path.join(GOLDEN, name)))


def workload():
    """The `d2_k8_b3` workload of tests/helpers.py with the token rows every fixture uses."""
    depth, K, B, ls = CASES["d2_k8_b3"]
    cfg = vit_b16(layers_v=depth, layers_t=depth, K=K)
    rows = sorted(set(np.concatenate([gold(f)["tokens"].ravel() for f in FILES]).tolist() + [49407]))
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=rows, logit_scale=float(ls))
    return cfg, sd, synth.images(cfg, B)


def test_manifest_matches_the_committed_fixtures():
    man = json.load(open(os.path.join(GOLDEN, "manifest_classsets.json")))
    assert man["generator"] == "tools/make_golden_classsets.py"
    assert set(man["files"]) == set(FILES)
    for name, rec in man["files"].items():
        path = os.path.join(GOLDEN, name)
        assert os.path.getsize(path) == rec["bytes"], (name, os.path.getsize(path), rec["bytes"])
        assert rec["bytes"] < 64 * 1024 and rec["n_cls"] == 18 and rec["B"] == 3
        g = gold(name)
        assert tuple(g["classnames"].tolist()) == NEW_CLASSES
        assert g["tokens"].shape == (18, 77) and g["tokens"].dtype == np.int64 and g["logits"].shape == (3, 18)
        assert (g["tokens"][:, 0] == 49406).all() and (g["tokens"].max(1) == 49407).all()


def test_fixture_weights_are_the_workloads():
    cfg, sd, _ = workload()
    full = synth.clip_state_dict(cfg, seed=0, logit_scale=float(CASES["d2_k8_b3"][3]))
    crc = synth.state_dict_checksum(full)
    for name in FILES:
        assert bytes(gold(name)["weights_crc"]).decode() == crc, name


def test_oracle_rpo_on_the_new_classes_matches_the_reference():
    cfg, sd, image = workload()
    g = gold("ref_classset_rpo.npz")
    assert int(g["K"]) == cfg.K
    m = OracleRPO(sd, g["tokens"], cfg.K, cfg.patch)
    m.set_prompts(*synth.prompts(cfg, sd, seed=int(g["prompt_seed"])))
    with torch.no_grad():
        logits = m.forward(image).logits
    np.testing.assert_allclose(logits.numpy(), g["logits"], atol=3e-5, rtol=0)


def test_oracle_plain_clip_on_the_new_classes_matches_the_reference():
    cfg, sd, image = workload()
    g = gold("ref_classset_zeroshot.npz")
    with torch.no_grad():
        logits, _, _ = plain_clip_forward(sd, image, g["tokens"], cfg.patch)
    assert np.abs(logits.numpy() - g["logits"]).max() <= 3e-5


@pytest.mark.parametrize("position", ["end", "middle"])
def test_oracle_coop_forward_on_the_new_classes_matches_the_reference(position):
    cfg, sd, image = workload()
    g = gold(f"ref_classset_coop_{position}.npz")
    assert str(g["class_token_position"]) == position and int(g["n_ctx"]) == 4
    logits, _, _ = coop_loss_and_grad(sd, image, g["tokens"], g["ctx"], np.zeros(3, dtype=np.int64), cfg.patch, position)
    assert np.abs(logits.numpy() - g["logits"]).max() <= 3e-5


# ---- the pure layout rule ---------------------------------------------------------------------------------------------------

class _Shell:
    """What `coop_layout` reads of an engine."""
    def __init__(self, tokens, n_cls):
        from rpo_amd.engine_coop import CoopEngineMixin
        self.len_np = tokens.argmax(-1) + 1
        self.Lmax = int(self.len_np.max())
        self.cfg = type("C", (), {"n_cls": n_cls})()
        self.coop_layout = CoopEngineMixin.coop_layout.__get__(self)


@pytest.mark.parametrize("position", ["end", "middle", "front"])
def test_layout_function_equals_coop_layout_on_the_engines_own_lengths(position):
    from rpo_amd.engine_coop import coop_layout_of
    toks = synth.coop_tokens(synth.oxford_pets_base_tokens(), 4)
    sh = _Shell(toks, toks.shape[0])
    src, cp = sh.coop_layout(4, position)
    src2, cp2 = coop_layout_of(sh.len_np, 4, position, sh.Lmax)
    assert np.array_equal(src, src2) and np.array_equal(cp, cp2)
    assert src.shape == (19, sh.Lmax) and cp.shape == (19, 4)
    # against the rule written out: [SOS | ctx | name | . EOT], [SOS | ctx/2 | name | ctx/2 | . EOT], [SOS | name | ctx | . EOT]
    for c in range(19):
        nl = int(sh.len_np[c]) - 4 - 3
        name = list(range(5, 5 + nl))
        want = {"end": [0, -1, -1, -1, -1] + name, "middle": [0, -1, -1] + name + [-1, -1],
                "front": [0] + name + [-1, -1, -1, -1]}[position]
        assert src[c, :5 + nl].tolist() == want
        assert src[c, 5 + nl:].tolist() == list(range(5 + nl, sh.Lmax))
        assert cp[c].tolist() == [p for p, s in enumerate(src[c]) if s < 0]


@pytest.mark.parametrize("position", ["end", "middle", "front"])
@pytest.mark.parametrize("n_ctx", [4, 16])
def test_layout_function_at_a_name_of_one_token_and_at_the_longest_that_fits(position, n_ctx):
    from rpo_amd.engine_coop import coop_layout_of
    longest = 77                                        # SOS + n_ctx + name + '.' + EOT fills the context
    lens = np.array([n_ctx + 4, longest])
    src, cp = coop_layout_of(lens, n_ctx, position)
    assert src.shape == (2, longest)
    for c, L in enumerate(lens):
        nl = int(L) - n_ctx - 3
        row = src[c, :L]
        assert (row < 0).sum() == n_ctx and row[0] == 0 and row[L - 2:].tolist() == [L - 2, L - 1]   # SOS, '.', EOT stay
        assert sorted(row[row >= 0].tolist()) == [0] + list(range(1 + n_ctx, int(L)))             # every token once
        names = row[(row >= 1 + n_ctx) & (row < 1 + n_ctx + nl)]
        assert names.tolist() == list(range(1 + n_ctx, 1 + n_ctx + nl))                          # the name, in order, contiguous
        first = int(np.nonzero(row == 1 + n_ctx)[0][0])
        assert first == {"end": 1 + n_ctx, "middle": 1 + n_ctx // 2, "front": 1}[position]
        assert cp[c].tolist() == sorted(cp[c].tolist()) and (row[cp[c]] == -1).all()
    with pytest.raises(AssertionError):
        coop_layout_of(np.array([n_ctx + 3]), n_ctx, position)                                   # no name token at all


def test_harmonic_mean():
    from rpo_amd.evaluator import harmonic_mean
    assert harmonic_mean(80.0, 60.0) == pytest.approx(2 * 80 * 60 / 140)
    assert harmonic_mean(75.5, 75.5) == pytest.approx(75.5)
    assert harmonic_mean(0.0, 90.0) == 0.0 and harmonic_mean(90.0, 0.0) == 0.0 and harmonic_mean(0.0, 0.0) == 0.0
    assert harmonic_mean(100.0, 50.0) < 75.0                               # below the arithmetic mean
    with pytest.raises(ValueError):
        harmonic_mean(-1.0, 50.0)


def test_base_to_new_is_two_tests_and_their_harmonic_mean():
    from rpo_amd.class_set import ClassSet
    from rpo_amd.evaluator import base_to_new, harmonic_mean
    calls = []

    class T:
        def class_set(self, tokens):
            calls.append(("class_set", tokens))
            return cs

        def test(self, image_set, classes=None, **kw):
            calls.append((image_set, classes, kw))
            return {"accuracy": 80.0 if classes is None else 60.0}

    cs = object.__new__(ClassSet)
    out = base_to_new(T(), "base", "new", cs, verbose=False)
    assert (out["base"], out["new"], out["H"]) == (80.0, 60.0, harmonic_mean(80.0, 60.0))
    assert calls == [("base", None, {"verbose": False}), ("new", cs, {"verbose": False})]
    calls.clear()
    base_to_new(T(), "base", "new", "tokens")
    assert calls[0] == ("class_set", "tokens") and calls[2][1] is cs


# ---- the C ABI --------------------------------------------------------------------------------------------------------------

def test_text_embed_is_declared_exported_and_bound():
    from rpo_amd import _lib, ops
    from rpo_amd.build import build_library
    build_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpo_amd.h")).read(), flags=re.S)
    assert re.search(r"\brpo_text_embed\s*\(", src), "rpo_text_embed is not declared in include/rpo_amd.h"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "rpo_text_embed") and "rpo_text_embed" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["rpo_text_embed"][1]) == 12 and hasattr(ops, "text_embed")
    assert _lib.load().rpo_version() == 8


def test_text_embed_checks_its_arguments_before_anything_is_enqueued():
    """No device is touched: every call below is refused by the argument checks (fake, 16-byte aligned addresses)."""
    from rpo_amd import _lib
    lib = _lib.load()
    p = 1 << 20
    base = dict(ids=p, ld=77, table=p, vocab=100, pos=p, ctx=None, n_ctx=0, out=p, n=3, L=20, d=512, stream=None)
    f = lambda **kw: lib.rpo_text_embed(*{**base, **kw}.values())           # (dict order = the argument order)
    assert f(d=510) == _lib.E_SHAPE and f(d=0) == _lib.E_SHAPE
    assert f(L=78) == _lib.E_SHAPE                                          # L > ld_ids
    assert f(out=p + 4) == _lib.E_ALIGN and f(table=p + 8) == _lib.E_ALIGN and f(pos=p + 4) == _lib.E_ALIGN
    assert f(n_ctx=4, ctx=p + 4) == _lib.E_ALIGN
    assert f(n=0) == _lib.E_BADARG and f(L=0) == _lib.E_BADARG and f(ids=None) == _lib.E_BADARG
    assert f(n_ctx=4, ctx=None) == _lib.E_BADARG and f(vocab=0) == _lib.E_BADARG and f(n_ctx=-1) == _lib.E_BADARG
