"""Host-side checks of the cached image features (rpo_amd/features.py, rpo_features_classify): the entry point is an ABI 8
addition that is declared, exported and bound and refuses bad arguments with nothing launched; the budget refusal comes
before the engine is touched; CoCoOp and the RPO trainers refuse `features=` by name before any device work; the linear
probe's composition into one affine classifier matches float64; the module does not import the oracle.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_features_classify_is_an_abi8_addition_declared_exported_and_bound():
    from rpo_amd import _lib, ops
    from rpo_amd.build import SOURCES, build_library
    build_library()
    hdr = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\brpo_features_classify\s*\(", src), "rpo_features_classify is not declared in include/rpo_amd.h"
    comment = [c for c in re.findall(r"/\*.*?\*/", hdr, flags=re.S) if "(ABI 8 addition)" in c and "CACHED image features" in c]
    decl = hdr.index("int rpo_features_classify(")
    assert any(0 < decl - (hdr.index(c) + len(c)) < 4 for c in comment), "not marked (ABI 8 addition) at its declaration"
    for cite in ("trainers/zsclip.py:58-63", "trainers/coop.py:196-208", "trainers/linear_prob.py:85-95"):
        assert any(cite in c for c in comment), f"the declaration's comment does not cite {cite}"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "rpo_features_classify") and "rpo_features_classify" in _lib.SIGNATURES
    assert callable(ops.features_classify)
    assert "classify.hip" in SOURCES
    assert "classify.hip" in open(os.path.join(ROOT, "tools", "build_debug.sh")).read()
    assert _lib.load().rpo_version() == 8 and "#define RPO_ABI_VERSION 8" in hdr


def test_features_classify_refuses_bad_arguments_without_launching():
    from rpo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                # 16-byte aligned host memory: never dereferenced
    BAD, SHAPE, ALIGN = _lib.E_BADARG, _lib.E_SHAPE, _lib.E_ALIGN

    def call(feat=p, ldf=512, cls=p, bias=None, label=p, counts=p, n=100, C=19, e=512, S=1):
        return lib.rpo_features_classify(feat, ldf, cls, bias, label, 100.0, 1, 1, counts, None, None, None, n, C, e, S, None)
    assert call(feat=None) == BAD and call(cls=None) == BAD and call(label=None) == BAD and call(counts=None) == BAD
    assert call(e=48, ldf=48) == SHAPE and call(e=1056, ldf=1056) == SHAPE and call(e=0) == SHAPE
    assert call(C=0) == SHAPE and call(C=65537) == SHAPE
    assert call(S=0) == SHAPE and call(S=1025) == SHAPE
    assert call(n=0) == SHAPE
    assert call(ldf=511) == SHAPE
    assert call(feat=p + 4) == ALIGN and call(cls=p + 8) == ALIGN and call(counts=p + 4) == ALIGN


def test_budget_refusal_comes_before_the_engine_is_touched():
    from rpo_amd.config import vit_b16
    from rpo_amd.features import ImageFeatures
    cfg = vit_b16()
    assert ImageFeatures.bytes_needed(cfg, 1) == 2048 and ImageFeatures.bytes_needed(cfg, 50_000) == 102_400_000

    class Untouchable:
        """An engine stub: reading anything but the configuration and the storage type is an error."""
        def __init__(self):
            self.cfg, self.act = cfg, torch.bfloat16

        def __getattr__(self, name):
            raise AssertionError(f"build() touched engine.{name} before refusing the budget")

    with pytest.raises(ValueError) as e:
        ImageFeatures.build(Untouchable(), [None] * 1000, budget_bytes=1 << 20)
    assert str(2048 * 1000) in str(e.value) and str(1 << 20) in str(e.value)


def test_trainers_whose_features_depend_on_what_they_train_refuse_by_name():
    """`object.__new__`: no engine, no device -- the refusal reads nothing of the trainer."""
    from rpo_amd.coop import CoCoOp, CoOp
    from rpo_amd.lp import LP
    from rpo_amd.multi import RPOMulti
    from rpo_amd.sweep import RPOSweep
    from rpo_amd.trainer import RPO
    from rpo_amd.zeroshot import ZeroshotCLIP
    coco = object.__new__(CoCoOp)
    with pytest.raises(NotImplementedError, match=r"CoCoOp.*text features depend on the image"):
        coco.test(None, features=object())
    with pytest.raises(NotImplementedError, match=r"CoCoOp.*text features depend on the image"):
        coco.train(None, max_epoch=1, val_set=object(), val_features=object())
    with pytest.raises(NotImplementedError, match=r"CoCoOp.*text features depend on the image"):
        coco.classifier()
    for klass, calls in ((RPO, ("test",)), (RPOMulti, ("test", "test_all")), (RPOSweep, ("test", "test_all"))):
        t = object.__new__(klass)
        for name in calls:
            with pytest.raises(NotImplementedError, match=rf"{klass.__name__}.*FrozenImageKV"):
                getattr(t, name)(None, features=object())
    with pytest.raises(NotImplementedError, match=r"RPO.*FrozenImageKV"):
        object.__new__(RPO).train(None, max_epoch=1, val_set=object(), val_features=object())
    for klass in (CoOp, LP, ZeroshotCLIP):
        assert klass._features_why_not is None
    # val_frozen keeps refusing for the plain-tower trainers exactly as before
    for klass in (CoOp, LP):
        t = object.__new__(klass)
        t.optim_cfg = type("O", (), {"max_epoch": 1})()
        with pytest.raises(NotImplementedError, match="val_frozen"):
            t.train(None, max_epoch=1, val_set=object(), val_frozen=object())


@pytest.mark.parametrize("C,e,seed", [(19, 64, 0), (37, 512, 1)])
def test_lp_composition_matches_float64(C, e, seed):
    """scale (f W^T + b) T^T against scale <f, M> + c with the fp32 (M, c) of lp_compose: the only roundings are those of
    M and c, 2^-24 relative each, so 1e-6 of the largest logit holds with room."""
    from rpo_amd.features import lp_compose
    g = torch.Generator().manual_seed(seed)
    T = torch.randn(C, e, generator=g)
    T = T / T.norm(dim=-1, keepdim=True)
    W = torch.eye(e) + 0.05 * torch.randn(e, e, generator=g)
    b = 0.1 * torch.randn(e, generator=g)
    f = torch.randn(23, e, generator=g)
    scale = 100.0
    M, c = lp_compose(T, W, b, scale)
    assert M.dtype == torch.float32 and c.dtype == torch.float32 and M.shape == (C, e) and c.shape == (C,)
    f64, T64, W64, b64 = f.double(), T.double(), W.double(), b.double()
    ref = scale * (f64 @ W64.t() + b64) @ T64.t()
    got = scale * (f64 @ M.double().t()) + c.double()
    assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


def test_weights_checksum_tells_checkpoints_apart():
    import numpy as np
    from rpo_amd.features import weights_checksum
    a = {"visual.proj": np.arange(12, dtype=np.float32).reshape(3, 4), "logit_scale": np.float32(4.6)}
    b = {k: np.array(v, copy=True) for k, v in a.items()}
    assert weights_checksum(a) == weights_checksum(b)
    b["visual.proj"][1, 1] += 1
    assert weights_checksum(a) != weights_checksum(b)


def test_features_module_does_not_import_the_oracle():
    text = open(os.path.join(ROOT, "rpo_amd", "features.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M)
    assert "oracle." not in text and "import oracle" not in text
