"""CoCoOp on other class sets, on the host (rpo_amd/engine_cocoop_eval.py): rpo_text_attn_fwd_prefix
is declared, exported and bound; bad arguments get its own error codes with nothing launched (never-dereferenced host
pointers, as tests/test_multi_host.py); the geometry and the validation of `conditional_class_set` as far as they need no
device; the reference fixture (tests/golden/ref_classset_cocoop.npz, tools/make_golden_classsets_cocoop.py), its manifest,
and the CPU oracle on its tokens.  No GPU needed."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from rpo_amd import synth
from rpo_amd.config import vit_b16

from helpers import CASES, GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rpo_text_attn_fwd_prefix"
FIXTURE = "ref_classset_cocoop.npz"


def gold():
    return dict(np.load(os.path.join(GOLDEN, FIXTURE)))


def test_prefix_attention_is_declared_exported_and_bound():
    from rpo_amd import _lib, ops
    from rpo_amd.build import build_library
    build_library()
    hdr = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(rf"\b{NAME}\s*\(", src), f"{NAME} is not declared in include/rpo_amd.h"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), f"librpo_hip.so does not export {NAME}"
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 15
    assert callable(ops.text_attn_fwd_prefix)
    assert list(inspect.signature(ops.text_attn_fwd_prefix).parameters)[:5] == ["q", "k", "v", "out", "len_i32"]
    # an addition to ABI 8, documented as such; the version does not move
    assert _lib.load().rpo_version() == 8 and "#define RPO_ABI_VERSION 8" in hdr
    assert re.search(r"/\* \(ABI 8 addition\)(?:(?!\*/).)*\*/\s*int rpo_text_attn_fwd_prefix\s*\(", hdr, flags=re.S)


def test_prefix_attention_refuses_bad_arguments_without_launching():
    from rpo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                # 16-byte aligned host memory: never dereferenced
    BAD, SHAPE, ALIGN, DTYPE = _lib.E_BADARG, _lib.E_SHAPE, _lib.E_ALIGN, _lib.E_DTYPE
    base = dict(q=p, k=p, v=p, ld=1536, out=p, ldo=512, dtype=_lib.RPO_BF16, len=p, n_img=3, n_cls=19, P=5, S=6, H=8,
                scale=0.125, stream=None)
    f = lambda **kw: getattr(lib, NAME)(*{**base, **kw}.values())           # (dict order = the argument order)
    for name in ("q", "k", "v", "out", "len"):
        assert f(**{name: None}) == BAD, name
    for name in ("n_img", "n_cls", "P", "S", "H"):
        assert f(**{name: 0}) == BAD and f(**{name: -1}) == BAD, name
    assert f(P=17, S=64) == SHAPE and f(P=1, S=80) == SHAPE and f(P=80, S=1) == SHAPE      # P + S = 81
    assert f(P=2 ** 30, S=2 ** 30) == SHAPE                                             # (the sum is not taken in 32 bits)
    assert f(n_img=2 ** 30, n_cls=2 ** 30) == SHAPE                                     # more workgroups than a grid holds
    assert f(ld=1535) == ALIGN and f(ldo=511) == ALIGN and f(dtype=_lib.RPO_F32, ld=1538, ldo=514) == ALIGN
    assert f(k=p + 4) == ALIGN and f(v=p + 8) == ALIGN
    assert f(dtype=7) == DTYPE and f(dtype=-1) == DTYPE


def test_plan_of_a_pass():
    """P, S, rows per pass and the chunking rule, on the Oxford-Pets base prompts with n_ctx 4 (pure host arithmetic)."""
    from rpo_amd.engine_cocoop_eval import MAX_IMAGES_PER_PASS, ConditionalClassSet as CCS
    toks = synth.coop_tokens(synth.oxford_pets_base_tokens(), 4)
    lens = toks.argmax(-1) + 1
    n, Lmax = toks.shape[0], int(lens.max())
    pl = CCS.plan(toks, 4, None, CCS.ROW_BUDGET)
    assert (pl["P"], pl["S"], pl["Lmax"]) == (5, Lmax - 5, Lmax) and pl["classes_per_pass"] == n
    per_image = 5 + n * (Lmax - 5)
    assert pl["images_per_pass"] == min(MAX_IMAGES_PER_PASS, CCS.ROW_BUDGET // per_image) >= 1
    assert per_image < n * Lmax                                          # fewer rows than the dense pass, always
    # an explicit images_per_pass is kept; the classes are chunked when those images exceed the budget
    pl = CCS.plan(toks, 4, 2, 2 * per_image)
    assert (pl["images_per_pass"], pl["classes_per_pass"]) == (2, n)
    pl = CCS.plan(toks, 4, 2, 2 * per_image - 1)
    assert pl["images_per_pass"] == 2 and 1 <= pl["classes_per_pass"] < n
    assert 2 * (5 + pl["classes_per_pass"] * pl["S"]) <= 2 * per_image - 1 < 2 * (5 + (pl["classes_per_pass"] + 1) * pl["S"])
    pl = CCS.plan(toks, 4, 1, 5 + 3 * (Lmax - 5))                         # one image alone exceeds the budget
    assert (pl["images_per_pass"], pl["classes_per_pass"]) == (1, 3)
    # one image alone over the default budget: one image per pass, classes in chunks
    many = synth.coop_tokens(synth.synthetic_tokens(vit_b16(layers_v=1, layers_t=1, K=1, n_cls=400), [60] * 400, seed=3), 16)
    pl = CCS.plan(many, 16, None, CCS.ROW_BUDGET)
    assert pl["images_per_pass"] == 1 and pl["classes_per_pass"] == (CCS.ROW_BUDGET - 17) // pl["S"] < 400


def test_conditional_class_set_validates_before_any_device_work():
    from rpo_amd.engine_cocoop_eval import ConditionalClassSet as CCS, ConditionalEvalEngineMixin

    class Shell(ConditionalEvalEngineMixin):
        """What the checks read of an engine; `dev` is never reached by a refused call."""
        TEXT_CHUNK = 256
        cfg = type("C", (), {"context": 77, "d_t": 512})()
        _tok_emb_host = np.zeros((49408, 1), dtype=np.float32)
        coop_hidden, coop_n_ctx = 32, 4

        @property
        def dev(self):
            raise AssertionError("a refused call reached the device")

    eng = Shell()
    toks = synth.coop_tokens(synth.oxford_pets_base_tokens(), 4)
    with pytest.raises(ValueError, match="tokens must be"):
        eng.conditional_class_set(toks[:, :76])
    with pytest.raises(ValueError, match="tokens must be"):
        eng.conditional_class_set(toks[:0])
    with pytest.raises(TypeError, match="integer"):
        eng.conditional_class_set(toks.astype(np.float32))
    for bad in (-1, 49408):
        t = toks.copy()
        t[3, 2] = bad
        with pytest.raises(ValueError, match="outside the vocabulary"):
            eng.conditional_class_set(t)
    short = toks.copy()
    short[2] = 0
    short[2, 0], short[2, 1:6], short[2, 6] = 49406, 343, 49407          # SOS, 4 X, '.', EOT: no name token (7 < 8)
    with pytest.raises(ValueError, match="at least 8 tokens"):
        eng.conditional_class_set(short)
    # Lmax <= 80 is the kernel's limit; CLIP's context of 77 keeps real prompts below it
    wide = np.zeros((2, 90), dtype=np.int64)
    wide[:, 0], wide[:, 1:84], wide[:, 84] = 49406, 343, 49407
    with pytest.raises(ValueError, match="takes 80"):
        CCS.plan(wide, 4, None, CCS.ROW_BUDGET)
    for ipp in (0, -1, 257):
        with pytest.raises(ValueError, match="images_per_pass"):
            eng.conditional_class_set(toks, images_per_pass=ipp)
    with pytest.raises(ValueError, match="row budget"):
        eng.conditional_class_set(toks, row_budget=10)
    # the other trainers' engines have no meta-net: refused by name
    plain = Shell()
    plain.coop_hidden = 0
    with pytest.raises(NotImplementedError, match="CoCoOp"):
        plain.conditional_class_set(toks)


def test_manifest_matches_the_committed_fixture():
    man = json.load(open(os.path.join(GOLDEN, "manifest_classsets_cocoop.json")))
    assert man["generator"] == "tools/make_golden_classsets_cocoop.py" and set(man["files"]) == {FIXTURE}
    rec = man["files"][FIXTURE]
    path = os.path.join(GOLDEN, FIXTURE)
    assert os.path.getsize(path) == rec["bytes"], (os.path.getsize(path), rec["bytes"])
    assert rec["bytes"] < 256 * 1024 and rec["n_cls"] == 18 and rec["B"] == 3
    g = gold()
    assert g["tokens"].shape == (18, 77) and g["tokens"].dtype == np.int64 and g["logits"].shape == (3, 18)
    assert (g["tokens"][:, 0] == 49406).all() and (g["tokens"].max(1) == 49407).all() and int(g["n_ctx"]) == 4
    assert g["ctx"].shape == (4, 512) and g["w1"].shape == (32, 512) and g["b1"].shape == (32,)
    assert g["w2"].shape == (512, 32) and g["b2"].shape == (512,)
    # the same token ids as CoOp's fixture of the same 18 classes (one tokenizer, one "X X X X name." template)
    coop = dict(np.load(os.path.join(GOLDEN, "ref_classset_coop_end.npz")))
    assert np.array_equal(g["tokens"], coop["tokens"]) and tuple(g["classnames"].tolist()) == tuple(coop["classnames"].tolist())


def test_oracle_cocoop_on_the_new_classes_matches_the_reference():
    """The CPU oracle (what the GPU tests of the dense path are held to) on the fixture's tokens, ctx and meta-net: the
    reference's logits within 3e-5, and the fixture's weights are the workload's."""
    from oracle.rpo_oracle import cocoop_loss_and_grads
    depth, K, B, ls = CASES["d2_k8_b3"]
    cfg = vit_b16(layers_v=depth, layers_t=depth, K=K)
    g = gold()
    full = synth.clip_state_dict(cfg, seed=0, logit_scale=float(ls))
    assert bytes(g["weights_crc"]).decode() == synth.state_dict_checksum(full)
    meta = {k: g[k] for k in ("w1", "b1", "w2", "b2")}
    logits, _, _ = cocoop_loss_and_grads(full, synth.images(cfg, B), g["tokens"], g["ctx"], meta, np.zeros(B, dtype=np.int64),
                                         cfg.patch)
    assert np.abs(logits.detach().numpy() - g["logits"]).max() <= 3e-5
