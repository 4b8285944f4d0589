"""Host-side checks of the shared-frozen-pass evaluation (rpo_amd/frozen_kv.py, rpo_amd/engine_prompt_rows.py,
rpo_attn_prompt_fwd): the cache's size is arithmetic on the configuration, the budget refusal comes before anything is
allocated, the entry point is an ABI 8 addition that is declared, exported and bound and refuses bad arguments with nothing
launched, the new modules do not import the oracle, and trainers without frozen rows refuse `val_frozen`.  No GPU needed."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bytes_needed_is_arithmetic_on_the_configuration():
    from rpo_amd.config import vit_b16
    from rpo_amd.frozen_kv import FrozenImageKV
    cfg = vit_b16()
    assert (cfg.n_frozen, cfg.d_v, cfg.layers_v) == (197, 768, 12)
    for n in (1, 9, 1000):
        assert FrozenImageKV.bytes_needed(cfg, n, torch.bfloat16) == 7_262_208 * n
        assert FrozenImageKV.bytes_needed(cfg, n, torch.float16) == 7_262_208 * n
        assert FrozenImageKV.bytes_needed(cfg, n, torch.float32) == 2 * 7_262_208 * n
    shallow = vit_b16(layers_v=2, layers_t=2)
    assert FrozenImageKV.bytes_needed(shallow, 9, torch.bfloat16) == 9 * 197 * 2 * 768 * 2 * 2


def test_budget_refusal_names_both_byte_counts_before_any_allocation():
    from rpo_amd.config import vit_b16
    from rpo_amd.frozen_kv import FrozenImageKV
    cfg = vit_b16()

    class Untouchable:
        """An engine stub: reading anything but the configuration and the storage type is an error."""
        def __init__(self):
            self.cfg, self.act = cfg, torch.bfloat16

        def __getattr__(self, name):
            raise AssertionError(f"build() touched engine.{name} before refusing the budget")

    with pytest.raises(ValueError) as e:
        FrozenImageKV.build(Untouchable(), [None] * 1000, budget_bytes=1 << 30)
    assert str(7_262_208 * 1000) in str(e.value) and str(1 << 30) in str(e.value)


def test_attn_prompt_fwd_is_an_abi8_addition_declared_exported_and_bound():
    from rpo_amd import _lib, ops
    from rpo_amd.build import build_library
    build_library()
    hdr = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\brpo_attn_prompt_fwd\s*\(", src), "rpo_attn_prompt_fwd is not declared in include/rpo_amd.h"
    comment = [c for c in re.findall(r"/\*.*?\*/", hdr, flags=re.S) if "(ABI 8 addition)" in c and "prompt sets" in c]
    decl = hdr.index("int rpo_attn_prompt_fwd(")
    assert any(0 < decl - (hdr.index(c) + len(c)) < 4 for c in comment), "not marked (ABI 8 addition) at its declaration"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "rpo_attn_prompt_fwd") and "rpo_attn_prompt_fwd" in _lib.SIGNATURES
    assert callable(ops.attn_prompt_fwd)
    assert _lib.load().rpo_version() == 8 and "#define RPO_ABI_VERSION 8" in hdr


def test_attn_prompt_fwd_refuses_bad_arguments_without_launching():
    from rpo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                # 16-byte aligned host memory: never dereferenced
    BAD, SHAPE, ALIGN, DTYPE = _lib.E_BADARG, _lib.E_SHAPE, _lib.E_ALIGN, _lib.E_DTYPE
    call = lambda q=p, ldq=768, ldkv=2304, out=p, ldo=768, dtype=_lib.RPO_BF16, B=4, H=12, N=197, Kp=24, sets=3, first=None: \
        lib.rpo_attn_prompt_fwd(q, ldq, p, p, ldkv, out, ldo, dtype, B, H, N, Kp, sets, first, 0.125, None)
    assert call(q=None) == BAD and call(out=None) == BAD
    assert call(B=0) == BAD and call(Kp=0) == BAD and call(sets=0) == BAD and call(N=0) == BAD
    assert call(N=289) == SHAPE
    assert call(dtype=7) == DTYPE
    assert call(ldkv=2303) == ALIGN and call(ldq=771) == ALIGN and call(ldo=770) == ALIGN
    assert call(q=p + 2) == ALIGN and call(first=p + 2) == ALIGN


def test_the_new_modules_do_not_import_the_oracle():
    for name in ("frozen_kv.py", "engine_prompt_rows.py"):
        text = open(os.path.join(ROOT, "rpo_amd", name)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), name
        assert "oracle." not in text and "import oracle" not in text, name


def test_trainers_without_frozen_rows_refuse_val_frozen():
    from rpo_amd.loop import LoopMixin
    from rpo_amd.trainer import RPO

    class Other(LoopMixin):
        optim_cfg = types.SimpleNamespace(max_epoch=1)
        epoch = 0

        def run_epoch(self, *a, **k):
            raise AssertionError("the refusal comes before the first epoch")

    with pytest.raises(NotImplementedError, match="val_frozen"):
        Other().train(None, max_epoch=1, val_set=object(), val_frozen=object())
    assert RPO._takes_frozen and not LoopMixin._takes_frozen
