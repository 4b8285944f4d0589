"""Host-side checks of the logistic probe (rpo_amd/logreg.py, rpo_amd/csrc/logreg.hip): the three
entry points are ABI 8 additions that are declared, exported and bound; the workspace size; every refused argument gets its
own code with nothing launched; every refusal of the Python layer comes before a device is touched; `shots_mask` against a
literal.  No GPU needed."""
import ctypes
import fnmatch
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rpo_logreg_workspace_floats", "rpo_logreg_loss_grad_sets", "rpo_logreg_step_sets")


def test_entry_points_are_abi8_additions_declared_exported_and_bound():
    from rpo_amd import _lib, ops
    from rpo_amd.build import SOURCES, build_library
    build_library()
    hdr = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    vs = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "rpo_amd", "csrc", "exports.map")).read(), flags=re.S)
    globs = re.findall(r"[A-Za-z_*?][\w*?]*(?=\s*;)", vs.split("global:")[1].split("local:")[0])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} is not declared in include/rpo_amd.h"
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), f"exports.map does not list {name}"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    comment = [c for c in re.findall(r"/\*.*?\*/", hdr, flags=re.S) if "(ABI 8 addition)" in c and "logistic" in c]
    decl = hdr.index("int64_t rpo_logreg_workspace_floats(")
    assert any(0 < decl - (hdr.index(c) + len(c)) < 4 for c in comment), "not marked (ABI 8 addition) at its declaration"
    assert len(_lib.SIGNATURES[NAMES[0]][1]) == 4 and len(_lib.SIGNATURES[NAMES[1]][1]) == 19
    assert len(_lib.SIGNATURES[NAMES[2]][1]) == 13
    assert callable(ops.logreg_loss_grad_sets) and callable(ops.logreg_step_sets)
    assert "logreg.hip" in SOURCES
    assert "logreg.hip" in open(os.path.join(ROOT, "tools", "build_debug.sh")).read()
    assert _lib.load().rpo_version() == 8 and "#define RPO_ABI_VERSION 8" in hdr


def test_workspace_is_zero_for_non_positive_arguments_and_monotone():
    from rpo_amd import _lib
    ws = _lib.load().rpo_logreg_workspace_floats
    base = (100, 19, 512, 3)
    assert ws(*base) > 0
    # the residuals, one chunk of gradient partials, the bias / loss partials, the penalty and the row scales all fit
    n, C, e, S = base
    assert ws(*base) >= S * n * C + S * C * e + S * C + S * ((n + 31) // 32) + S + S * n
    for k in range(4):
        for bad in (0, -1):
            a = list(base)
            a[k] = bad
            assert ws(*a) == 0
        prev = 0
        for v in (1, 2, 31, 32, 33, 64, 1000, 1024, 1025, 4096):
            a = list(base)
            a[k] = v if k != 2 else 32 * v
            now = ws(*a)
            assert now >= prev and now > 0, (k, v)
            prev = now
        a, b = list(base), list(base)
        b[k] = 2 * b[k]
        assert ws(*b) > ws(*a)
    assert ws(16000, 1000, 512, 8) > 2 ** 27                      # (past int32 bytes: the size is an int64)


def test_refused_arguments_get_their_codes_without_a_device():
    from rpo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                # 16-byte aligned host memory: never dereferenced
    BAD, SHAPE, ALIGN = _lib.E_BADARG, _lib.E_SHAPE, _lib.E_ALIGN

    def call(feat=p, ldf=512, label=p, weight=None, omega=p, l2=p, params=p, stride=19 * 512 + 20, done=None, grads=p, loss=p,
             n=100, C=19, e=512, S=1, ws=p):
        return lib.rpo_logreg_loss_grad_sets(feat, ldf, label, weight, omega, l2, params, stride, done, 0, 1, grads, loss, n,
                                             C, e, S, ws, None)
    for name in ("feat", "label", "omega", "l2", "params", "grads", "loss", "ws"):
        assert call(**{name: None}) == BAD, name
    assert call(ldf=0) == BAD and call(stride=0) == BAD and call(stride=-4) == BAD
    assert call(e=48, ldf=48) == SHAPE and call(e=1056, ldf=1056) == SHAPE and call(e=0) == SHAPE
    assert call(C=0) == SHAPE and call(C=1025, stride=1025 * 513 + 3) == SHAPE
    assert call(S=0) == SHAPE and call(S=1025) == SHAPE
    assert call(n=0) == SHAPE and call(ldf=511) == SHAPE
    assert call(stride=19 * 512 + 16) == SHAPE                    # (the bias does not fit)
    assert call(feat=p + 4) == ALIGN and call(params=p + 8) == ALIGN and call(ws=p + 4) == ALIGN and call(grads=p + 4) == ALIGN
    assert call(stride=19 * 512 + 21) == ALIGN and call(omega=p + 4) == ALIGN

    def step(x=p, y=p, g=p, stride=64, count=63, t=p, L=p, tol=p, done=p, iters=p, ginf=p, S=1):
        return lib.rpo_logreg_step_sets(x, y, g, stride, count, t, L, tol, done, iters, ginf, S, None)
    for name in ("x", "y", "g", "t", "L", "tol", "done", "iters", "ginf"):
        assert step(**{name: None}) == BAD, name
    assert step(stride=0) == BAD
    assert step(S=0) == SHAPE and step(S=1025) == SHAPE and step(count=0) == SHAPE and step(count=65) == SHAPE


def _stub(n=6, e=32, labels=(0, 1, 2, 0, 1, 2), device="cuda:0"):
    """An `ImageFeatures` whose tensors live on the host while it claims a device: a refusal that came after any device
    work would fail on this machine (no device), and the device refusal itself is the last one."""
    from rpo_amd.features import ImageFeatures
    feat = torch.zeros(n, e)
    return ImageFeatures({"n_images": n}, feat, torch.tensor(labels), list(labels), torch.device(device))


def test_python_refusals_come_before_any_device_work(monkeypatch):
    from rpo_amd import logreg, ops
    from rpo_amd.logreg import LogisticProbe

    def forbidden(*a, **k):
        raise AssertionError("a refusal came after device work")
    for name in ("logreg_loss_grad_sets", "logreg_step_sets", "logreg_workspace_floats", "_stream"):
        monkeypatch.setattr(ops, name, forbidden)
    monkeypatch.setattr(torch.cuda, "current_stream", forbidden)
    monkeypatch.setattr(torch.cuda, "device", forbidden)
    monkeypatch.setattr(logreg.ImageFeatures, "build", forbidden)
    F = _stub()
    with pytest.raises(ValueError, match=r"n_cls must be 1 \.\. 1024, got 1025"):
        LogisticProbe(F, 1025, [1.0])
    with pytest.raises(ValueError, match=r"n_cls must be 1 \.\. 1024, got 1025"):
        LogisticProbe.from_set(object(), type("Set", (), {"labels": [0, 1]})(), n_cls=1025)
    for bad in ([0.0], [1.0, -1e-3], [float("nan")], []):
        with pytest.raises(ValueError, match=r"l2"):
            LogisticProbe(F, 3, bad)
    with pytest.raises(ValueError, match=r"sample_weight must be \[2, 6\]"):
        LogisticProbe(F, 3, [1.0, 0.1], sample_weight=torch.ones(6))
    with pytest.raises(ValueError, match=r"sample_weight must be \[2, 6\]"):
        LogisticProbe(F, 3, [1.0, 0.1], sample_weight=torch.ones(2, 5))
    w = torch.ones(2, 6)
    w[1, 3] = -0.5
    with pytest.raises(ValueError, match=r"negative"):
        LogisticProbe(F, 3, [1.0, 0.1], sample_weight=w)
    w = torch.ones(2, 6)
    w[1] = 0
    with pytest.raises(ValueError, match=r"member\(s\) \[1\] sum to 0"):
        LogisticProbe(F, 3, [1.0, 0.1], sample_weight=w)
    with pytest.raises(ValueError, match=r"2 label\(s\) outside \[0, 2\), the first is 2"):
        LogisticProbe(F, 2, [1.0])
    with pytest.raises(ValueError, match=r"outside \[0, 3\), the first is -1"):
        LogisticProbe(_stub(labels=(0, 1, 2, -1, 1, 2)), 3, [1.0])
    with pytest.raises(ValueError, match=r"another device"):
        LogisticProbe(F, 3, [1.0])                               # host tensors under a device's name: the last refusal
    probe = object.__new__(LogisticProbe)
    probe.device, probe.e = torch.device("cuda:0"), 32
    with pytest.raises(ValueError, match=r"test: the features are on another device"):
        probe.test(_stub(device="cuda:1"))
    with pytest.raises(ValueError, match=r"test: the features are on another device"):
        probe.select(_stub(device="cuda:1"))


def test_shots_mask_against_a_literal():
    from rpo_amd.logreg import shots_mask
    labels = [0, 1, 0, 2, 1, 0, 2, 2, 0, 1]                     # class 0 x 4, 1 x 3, 2 x 3
    lab = torch.tensor(labels)
    g = torch.Generator().manual_seed(5)
    m = shots_mask(labels, (1, 2, 4), g)
    assert m.dtype == torch.float32 and tuple(m.shape) == (3, 10) and set(m.unique().tolist()) <= {0.0, 1.0}
    for row, k in zip(m, (1, 2, 4)):
        for c, have in ((0, 4), (1, 3), (2, 3)):
            assert int(row[lab == c].sum()) == min(k, have), (k, c)
    assert bool((m[0] <= m[1]).all()) and bool((m[1] <= m[2]).all())          # nested: one permutation for every k
    # the rule, restated: first k of each class along the permutation the generator gives
    perm = torch.randperm(10, generator=torch.Generator().manual_seed(5)).tolist()
    want = torch.zeros(10)
    for c in range(3):
        want[[i for i in perm if labels[i] == c][:2]] = 1.0
    assert torch.equal(m[1], want)
    assert torch.equal(shots_mask(labels, (1, 2, 4), torch.Generator().manual_seed(5)), m)      # same seed, same table
    assert torch.equal(shots_mask(lab, (1, 2, 4), torch.Generator().manual_seed(5)), m)          # a tensor of labels
    others = [shots_mask(labels, (1, 2, 4), torch.Generator().manual_seed(s)) for s in (6, 7, 8, 9)]
    assert any(not torch.equal(o, m) for o in others)
    with pytest.raises(ValueError, match="shots"):
        shots_mask(labels, (0,), g)


def test_logreg_module_does_not_import_the_oracle():
    text = open(os.path.join(ROOT, "rpo_amd", "logreg.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M)
