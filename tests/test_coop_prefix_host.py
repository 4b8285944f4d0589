"""CoOp / CoCoOp training on the shared-prefix layout, on the host (rpo_amd/engine_coop_prefix.py):
rpo_text_attn_bwd_prefix and its workspace query are declared, exported and bound; bad arguments get their own error codes
with nothing launched (never-dereferenced host pointers, as tests/test_cocoop_classset_host.py); `shared_prefix=True`
refuses class-specific contexts and the other class-token positions before an engine is made; the row arithmetic of the
layout.  No GPU needed."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from rpo_amd import synth
from rpo_amd.config import vit_b16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rpo_text_attn_bwd_prefix"
WS_NAME = "rpo_text_attn_bwd_prefix_workspace_floats"


def test_prefix_backward_is_declared_exported_and_bound():
    from rpo_amd import _lib, ops
    from rpo_amd.build import build_library
    build_library()
    hdr = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in (NAME, WS_NAME):
        assert re.search(rf"\b{name}\s*\(", src), f"{name} is not declared in include/rpo_amd.h"
        assert hasattr(lib, name), f"librpo_hip.so does not export {name}"
        assert name in _lib.SIGNATURES
    # the version script exports the rpo_ names and nothing else
    emap = open(os.path.join(ROOT, "rpo_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*rpo_\*;", emap) and re.search(r"local:\s*\*;", emap)
    assert len(_lib.SIGNATURES[NAME][1]) == 20 and len(_lib.SIGNATURES[WS_NAME][1]) == 4
    assert callable(ops.text_attn_bwd_prefix) and callable(ops.text_attn_bwd_prefix_workspace_floats)
    assert list(inspect.signature(ops.text_attn_bwd_prefix).parameters)[:8] == ["q", "k", "v", "d_out", "dq", "dk", "dv",
                                                                                 "len_i32"]
    # additions to ABI 8, documented as such; the version does not move
    assert _lib.load().rpo_version() == 8 and "#define RPO_ABI_VERSION 8" in hdr
    assert re.search(rf"/\* \(ABI 8 addition\)(?:(?!\*/).)*\*/\s*int {NAME}\s*\(", hdr, flags=re.S)
    assert re.search(rf"/\* \(ABI 8 addition\)(?:(?!\*/).)*\*/\s*int64_t {WS_NAME}\s*\(", hdr, flags=re.S)


def test_workspace_size_is_slots_of_prefix_partials():
    """One [dk | dv][P][64] fp32 partial per (image, head, class group) plus one for the prefix's own part; the grouping is
    a function of n_cls and H alone, so the size is linear in n_img (an image's slots do not depend on the others)."""
    from rpo_amd import _lib
    ws = getattr(_lib.load(), WS_NAME)
    for n_img, n_cls, P, H in [(1, 1, 2, 1), (1, 19, 17, 8), (3, 5, 5, 8), (1, 1000, 17, 8), (2, 397, 5, 12)]:
        n = ws(n_img, n_cls, P, H)
        per = 2 * P * 64 * H
        assert n > 0 and n % (n_img * per) == 0
        slots = n // (n_img * per)
        assert 2 <= slots <= n_cls + 1                       # at least one class group and the self part
        assert n == n_img * ws(1, n_cls, P, H)
    assert ws(1, 1000, 17, 8) * 4 <= 17 * 2 ** 20            # no more than groups of 4 would take at ImageNet's class count
    for bad in [(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-1, 1, 1, 1)]:
        assert ws(*bad) == 0


def test_prefix_backward_refuses_bad_arguments_without_launching():
    from rpo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                # 16-byte aligned host memory: never dereferenced
    BAD, SHAPE, ALIGN, DTYPE = _lib.E_BADARG, _lib.E_SHAPE, _lib.E_ALIGN, _lib.E_DTYPE
    base = dict(q=p, k=p, v=p, ld=1536, d_out=p, lddo=512, dq=p, dk=p, dv=p, ldd=1536, dtype=_lib.RPO_BF16, len=p, n_img=3,
                n_cls=19, P=5, S=6, H=8, scale=0.125, workspace=p, stream=None)
    f = lambda **kw: getattr(lib, NAME)(*{**base, **kw}.values())           # (dict order = the argument order)
    for name in ("q", "k", "v", "d_out", "dq", "dk", "dv", "len", "workspace"):
        assert f(**{name: None}) == BAD, name
    for name in ("n_img", "n_cls", "P", "S", "H"):
        assert f(**{name: 0}) == BAD and f(**{name: -1}) == BAD, name
    assert f(P=17, S=64) == SHAPE and f(P=1, S=80) == SHAPE and f(P=80, S=1) == SHAPE      # P + S = 81
    assert f(P=2 ** 30, S=2 ** 30) == SHAPE                                             # (the sum is not taken in 32 bits)
    assert f(n_img=2 ** 30, n_cls=2 ** 30) == SHAPE                                     # more workgroups than a grid holds
    assert f(n_img=2 ** 30, H=2 ** 10) == SHAPE
    assert f(ld=1535) == ALIGN and f(lddo=511) == ALIGN and f(ldd=1535) == ALIGN
    assert f(dtype=_lib.RPO_F32, ld=1538) == ALIGN and f(dtype=_lib.RPO_F32, lddo=514) == ALIGN
    assert f(k=p + 4) == ALIGN and f(v=p + 8) == ALIGN and f(workspace=p + 4) == ALIGN
    assert f(dtype=7) == DTYPE and f(dtype=-1) == DTYPE


@pytest.mark.parametrize("kw,word", [(dict(csc=True), "csc"), (dict(class_token_position="middle"), "class_token_position"),
                                     (dict(class_token_position="front"), "class_token_position")],
                         ids=["csc", "middle", "front"])
def test_shared_prefix_refuses_what_shares_no_rows_before_an_engine_is_made(monkeypatch, kw, word):
    from rpo_amd import coop, engine
    touched = []
    monkeypatch.setattr(engine, "make_engine", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(coop, "make_engine", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(torch.cuda, "device", lambda *a, **k: touched.append(2))
    cfg = vit_b16(layers_v=1, layers_t=1, K=1)
    toks = synth.coop_tokens(synth.oxford_pets_base_tokens(), 4)
    sd = {"token_embedding.weight": np.zeros((1, cfg.d_t), dtype=np.float32)}
    for make in (lambda: coop.CoOpCustomCLIP(sd, toks, 4, cfg=cfg, shared_prefix=True, **kw),
                 lambda: coop.CoOp(sd, toks, 4, cfg=cfg, shared_prefix=True, **kw)):
        with pytest.raises(ValueError, match=rf"shared_prefix=True.*{word}"):
            make()
    assert not touched, "a refused constructor reached the engine or the device"
    # the engine's own entry point refuses too, before it reads anything of the engine
    from rpo_amd.engine_coop import CoopEngineMixin
    with pytest.raises(ValueError, match="shared_prefix=True"):
        CoopEngineMixin.coop_setup(object(), 4, shared_prefix=True, **kw)


def test_shared_prefix_is_off_by_default_everywhere():
    from rpo_amd import coop
    from rpo_amd.engine_coop import CoopEngineMixin
    for fn in (coop.CoOpCustomCLIP.__init__, coop.CoOp.__init__, coop.CoCoOpCustomCLIP.__init__, coop.CoCoOp.__init__,
               CoopEngineMixin.coop_setup):
        par = inspect.signature(fn).parameters
        assert "shared_prefix" in par and par["shared_prefix"].default is False, fn.__qualname__


def test_row_counts_of_the_shared_layout():
    """R * (P + n_cls * S) rows against the dense R * n_cls * Lmax; the issue's two arithmetic examples."""
    from rpo_amd.engine_coop import shared_rows
    for R, n, lens, n_ctx in [(1, 1000, [41] * 1000, 16), (1, 5, [20, 41, 33, 27, 22], 16), (3, 7, [8, 11, 29, 9, 10, 12, 8], 4),
                              (1, 1, [5], 1), (4, 100, [8 + (7 * c) % 18 for c in range(100)], 4)]:
        Lmax, P = max(lens), 1 + n_ctx
        S = Lmax - P
        got = shared_rows(R, n, Lmax, n_ctx)
        assert got == R * P + R * n * S
        # the last suffix row of the layout (rpo_text_attn_fwd_prefix's) is the last row
        assert R * P + ((R - 1) * n + n - 1) * S + S - 1 == got - 1
        assert got < R * n * Lmax or n == 1
        assert R * n * Lmax - got == R * (n - 1) * P           # every class but one gives up its copy of the prefix
    assert shared_rows(1, 1000, 41, 16) == 24017 and 1000 * 41 == 41000
    toks = synth.coop_tokens(synth.oxford_pets_base_tokens(), 16)
    lens = toks.argmax(-1) + 1
    n, Lmax = toks.shape[0], int(lens.max())
    assert n == 19 and int(lens.min()) >= 17 + 3
    assert 1.9 <= n * Lmax / shared_rows(1, n, Lmax, 16) <= 2.3   # "about 2.1" at the Oxford-Pets base prompts
