"""Host-side checks of the shared-batch sweep (rpo_amd/shared_sweep.py, rpo_amd/engine_prompt_train.py, rpo_attn_prompt_bwd;
DESIGN.md section 9u): the entry point is an ABI 8 addition that is declared, exported and bound and refuses bad arguments with
nothing launched; the byte count of the step's buffers is arithmetic on the configuration; every refusal of the trainer
fires by name before a device is touched; the new modules leave the pinned ones alone.  No GPU needed."""
import ctypes
import dataclasses
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rpo_attn_prompt_bwd"


def test_attn_prompt_bwd_is_an_abi8_addition_declared_exported_and_bound():
    from rpo_amd import _lib, ops
    from rpo_amd.build import build_library
    build_library()
    hdr = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(rf"\b{NAME}\s*\(", src), f"{NAME} is not declared in include/rpo_amd.h"
    comment = [c for c in re.findall(r"/\*.*?\*/", hdr, flags=re.S) if "(ABI 8 addition)" in c and "backward twin" in c]
    decl = hdr.index(f"int {NAME}(")
    assert any(0 < decl - (hdr.index(c) + len(c)) < 4 for c in comment), "not marked (ABI 8 addition) at its declaration"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, NAME), f"librpo_hip.so does not export {NAME}"
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 18
    assert callable(ops.attn_prompt_bwd)
    assert _lib.load().rpo_version() == 8 and "#define RPO_ABI_VERSION 8" in hdr


def test_attn_prompt_bwd_refuses_bad_arguments_without_launching():
    from rpo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                # 16-byte aligned host memory: never dereferenced
    BAD, SHAPE, ALIGN, DTYPE = _lib.E_BADARG, _lib.E_SHAPE, _lib.E_ALIGN, _lib.E_DTYPE
    call = lambda q=p, ldq=768, k=p, v=p, ldkv=2304, da=p, ldda=768, dq=p, lddq=768, dtype=_lib.RPO_BF16, B=4, H=12, N=197, \
        Kp=24, sets=3, first=None: lib.rpo_attn_prompt_bwd(q, ldq, k, v, ldkv, da, ldda, dq, lddq, dtype, B, H, N, Kp, sets,
                                                           first, 0.125, None)
    assert call(q=None) == BAD and call(k=None) == BAD and call(v=None) == BAD and call(da=None) == BAD and call(dq=None) == BAD
    assert call(B=0) == BAD and call(H=0) == BAD and call(Kp=0) == BAD and call(sets=0) == BAD and call(N=0) == BAD
    assert call(N=289) == SHAPE and call(N=289, dtype=_lib.RPO_F32) == SHAPE
    assert call(sets=(1 << 24) // 24 + 1) == SHAPE              # sets * Kp above 2^24, the forward's limit
    assert call(sets=1 << 20, Kp=16, B=1 << 8) == SHAPE         # sets * Kp * B above INT32_MAX
    assert call(dtype=7) == DTYPE
    assert call(ldkv=2303) == ALIGN and call(ldq=771) == ALIGN and call(ldda=771) == ALIGN and call(lddq=770) == ALIGN
    assert call(q=p + 2) == ALIGN and call(da=p + 2) == ALIGN and call(k=p + 4) == ALIGN and call(v=p + 8) == ALIGN
    assert call(dq=p + 2) == ALIGN and call(first=p + 2) == ALIGN


def test_prompt_train_bytes_is_arithmetic_on_the_configuration():
    from rpo_amd.config import vit_b16
    from rpo_amd.engine_prompt_train import DY_SLABS, prompt_train_bytes
    cfg = vit_b16(K=24)
    assert (cfg.d_v, cfg.embed, cfg.layers_v, DY_SLABS) == (768, 512, 12, 4)
    # 16-bit modes, per row: 12 blocks x (x 3072 + xm 3072 + q 1536 + u 6144 = 13 824) = 165 888 B of per-block saves, + the
    # last boundary and the ln_pre input (6 144), the forward's temporaries (12 896), the head gradients (3 072), the chain's
    # workspaces (29 184)
    per_row = 165_888 + 6_144 + 12_896 + 3_072 + 29_184
    for S, B in ((1, 1), (3, 4), (8, 32)):
        assert prompt_train_bytes(cfg, S, B, torch.bfloat16) == S * B * 24 * per_row
        assert prompt_train_bytes(cfg, S, B, torch.float16) == S * B * 24 * per_row
        assert prompt_train_bytes(cfg, S, B, torch.float32) == S * B * 24 * 331_872
    assert prompt_train_bytes(cfg, 8, 32) == 1_334_378_496
    assert prompt_train_bytes(cfg, 1, 1, torch.bfloat16, aux_f32=True) - prompt_train_bytes(cfg, 1, 1) == 24 * 12 * 6144
    # pure: the configuration's four sizes and nothing else are read
    stub = types.SimpleNamespace(K=5, d_v=128, embed=64, layers_v=2)
    per_block = 4 * 128 * 2 + 2 * 128 + 2 * 512
    want = 3 * 2 * 5 * (2 * per_block + 8 * 128 + (2 * 128 + 16 + 2 * 128 + 2 * 512 + 2 * 128 + 4 * 64) + 6 * 64
                        + (8 * 128 + 2 * 128 + 2 * 512 + 4 * 128 + 16 * 128))
    assert prompt_train_bytes(stub, 3, 2, torch.float16) == want


def test_every_refusal_of_the_shared_sweep_fires_before_a_device_is_touched(monkeypatch):
    from rpo_amd import engine, shared_sweep
    from rpo_amd.config import rn_clip, vit_l14_336
    from rpo_amd.trainer import OptimConfig
    touched = []
    monkeypatch.setattr(engine, "make_engine", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(torch.cuda, "device", lambda *a, **k: touched.append(2))
    from rpo_amd.config import vit_b16
    cfg = vit_b16(layers_v=1, layers_t=1, K=8)
    T = shared_sweep.RPOSharedSweep
    mk = lambda **kw: [dict(seed=1, K=8, optim=OptimConfig()), dict(dict(seed=2, K=4, optim=OptimConfig(lr=0.02)), **kw)]
    with pytest.raises(NotImplementedError, match="RPOSharedSweep needs a ViT image tower.*ResNet"):
        T(rn_clip((1, 1, 1, 1), 64, 1024, K=4), {}, members=mk())
    with pytest.raises(NotImplementedError, match="RPOSharedSweep: world_size > 1"):
        T(cfg, {}, members=mk(), world_size=2)
    with pytest.raises(NotImplementedError, match="RPOSharedSweep: .*577 frozen tokens.*288-token limit"):
        T(vit_l14_336(K=8, layers_v=1, layers_t=1), {}, members=mk())
    with pytest.raises(ValueError, match="max_epoch"):
        T(cfg, {}, members=mk(optim=OptimConfig(max_epoch=30)))
    with pytest.raises(ValueError, match="batch size"):
        T(cfg, {}, members=mk(batch_size=8), batch_size=4)
    with pytest.raises(ValueError, match="storage mode"):
        T(cfg, {}, members=mk(act_dtype=torch.float16), act_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="CLIP / class set / backbone"):
        T(cfg, {}, members=mk(cfg=dataclasses.replace(cfg, n_cls=37)))
    with pytest.raises(ValueError, match="K = 0"):
        T(cfg, {}, members=mk(K=0))
    with pytest.raises(ValueError, match="exactly one of seed= or prompts="):
        T(cfg, {}, members=mk(seed=None))
    with pytest.raises(ValueError, match="members"):
        T(cfg, {}, members=[])
    assert not touched


def test_the_shared_sweep_is_a_sweep_with_one_batch_and_lives_in_new_modules():
    import inspect
    from rpo_amd import engine, engine_prompt_train, shared_sweep, sweep
    T = shared_sweep.RPOSharedSweep
    assert issubclass(T, sweep.RPOSweep) and T.__module__ == "rpo_amd.shared_sweep"
    assert list(inspect.signature(T.__init__).parameters) == list(inspect.signature(sweep.RPOSweep.__init__).parameters)
    for name in ("skipped_steps", "test", "test_all", "model_inference", "save_model", "load_model", "update_lr"):
        assert getattr(T, name) is getattr(sweep.RPOSweep, name), f"{name} is not inherited unchanged"
    assert list(inspect.signature(T.run_epoch).parameters)[:3] == ["self", "image_set", "generator"]
    assert issubclass(engine.Engine, engine_prompt_train.PromptTrainEngineMixin)
    for name in ("prompt_train_setup", "shared_forward_backward", "prompt_train_hbm_bytes"):
        assert callable(getattr(engine.Engine, name))
    assert not hasattr(sweep, "RPOSharedSweep")                  # (the pinned modules gained no public name)
    for name in ("shared_sweep.py", "engine_prompt_train.py"):
        text = open(os.path.join(ROOT, "rpo_amd", name)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M) and "import oracle" not in text, name


def test_the_shared_step_refuses_an_engine_without_its_buffers_and_a_per_member_batch():
    from rpo_amd.engine_prompt_train import PromptTrainEngineMixin
    from rpo_amd.shared_sweep import RPOSharedSweep
    eng = object.__new__(type("E", (PromptTrainEngineMixin,), {}))
    with pytest.raises(RuntimeError, match="prompt_train_setup"):
        eng.shared_forward_backward(None, None)
    tr = object.__new__(RPOSharedSweep)
    with pytest.raises(ValueError, match="ONE batch"):
        tr.parse_batch_train([{"img": np.zeros(1), "label": [0]}] * 3)
    with pytest.raises(ValueError, match="ONE image set and ONE generator"):
        tr.run_epoch([None, None])
