"""Host-side checks of prompt ensembling (rpo_amd/csrc/ensemble.hip, rpo_amd.zeroshot.ZeroshotCLIP2): the C ABI entry
points, the arguments refused before anything is launched, the fixtures' provenance record, and the fixtures' own
consistency (the reference's ensemble and logits recomputed from its stored per-template features in float64).
No GPU needed."""
import ctypes
import fnmatch
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ("rpo_text_ensemble_accumulate", "rpo_text_ensemble_finish")
CASES = {"d2_b3": (8, 512), "rn_mini_b3": (8, 1024), "d2_b3_imagenet": (7, 512)}      # tag -> (T, embed)


def test_ensemble_entry_points_are_declared_exported_and_bound():
    from rpo_amd import _lib
    from rpo_amd.build import SOURCES, build_library
    assert "ensemble.hip" in SOURCES
    build_library()
    header = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"#define\s+RPO_ABI_VERSION\s+8\b", header)
    # the version script exports by pattern: every global pattern is listed, the new names must match one of them
    vs = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "rpo_amd", "csrc", "exports.map")).read(), flags=re.S)
    globs = [g.strip() for g in re.search(r"global:(.*?)local:", vs, flags=re.S).group(1).split(";") if g.strip()]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} is not declared in include/rpo_amd.h"
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), f"exports.map does not list {name}"
        assert hasattr(lib, name), f"librpo_hip.so does not export {name}"
        assert name in _lib.SIGNATURES
    assert _lib.load().rpo_version() == 8


def test_ensemble_refuses_bad_arguments_without_launching():
    from rpo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    acc, fin = lib.rpo_text_ensemble_accumulate, lib.rpo_text_ensemble_finish
    #        feat  ld    T  stride n_cls e     acc  first
    bad = [(None, 512, 8, 19, 19, 512, p, 1),            # null feat
           (p, 512, 8, 19, 19, 512, None, 1),            # null acc
           (p, 512, 8, 19, 19, 0, p, 1),                 # e < 1
           (p, 1028, 8, 19, 19, 1025, p, 1),             # e > 1024
           (p, 511, 8, 19, 19, 512, p, 1),               # ld < e
           (p, 512, 0, 19, 19, 512, p, 1),               # T < 1
           (p, 512, 8, 19, 0, 512, p, 1),                # n_cls < 1
           (p, 512, 8, 18, 19, 512, p, 1)]               # blocks of n_cls rows that overlap
    for a in bad:
        assert acc(*a, None) == _lib.E_BADARG, a
    #        acc  n_cls e   T_total out
    for a in ((None, 19, 512, 8, p), (p, 19, 512, 8, None), (p, 0, 512, 8, p), (p, 19, 0, 8, p), (p, 19, 1025, 8, p),
              (p, 19, 512, 0, p)):
        assert fin(*a, None) == _lib.E_BADARG, a
    assert all(v == 0.0 for v in buf)


def test_manifest_zsclip2_matches_the_committed_fixtures():
    man = json.load(open(os.path.join(GOLD, "manifest_zsclip2.json")))
    assert man["generator"] == "tools/make_golden_zsclip2.py"
    assert set(man["files"]) == {f"ref_zsclip2_{tag}.npz" for tag in CASES}
    for name, rec in man["files"].items():
        path = os.path.join(GOLD, name)
        assert os.path.getsize(path) == rec["bytes"], (name, os.path.getsize(path), rec["bytes"])
        assert rec["bytes"] < 1024 * 1024
        assert rec["T"] == CASES[name[len("ref_zsclip2_"):-len(".npz")]][0]


@pytest.mark.parametrize("tag", sorted(CASES))
def test_fixture_ensemble_and_logits_follow_from_its_per_template_features(tag):
    """trainers/zsclip.py:88-96 and :55-60 restated in float64 on the fixture's own per-template features: the stored
    ensemble to 1e-6 (measured 2.6e-8), the stored logits to 1e-4."""
    T, e = CASES[tag]
    g = np.load(os.path.join(GOLD, f"ref_zsclip2_{tag}.npz"))
    n = g["tokens"].shape[1]
    assert g["tokens"].shape == (T, n, 77) and g["tokens"].dtype == np.int64 and g["templates"].shape == (T,)
    assert g["per_template_features"].shape == (T, n, e) and g["text_features"].shape == (n, e)
    assert all("{}" in str(s) for s in g["templates"])
    f = g["per_template_features"].astype(np.float64)
    mean = (f / np.linalg.norm(f, axis=-1, keepdims=True)).sum(0) / T
    ens = mean / np.linalg.norm(mean, axis=-1, keepdims=True)
    err = np.abs(ens - g["text_features"]).max()
    print(f"[{tag}] float64 ensemble vs the reference's: {err:.2e}")
    assert err <= 1e-6
    img = g["image_features"].astype(np.float64)
    scale = float(np.exp(np.float32(np.log(100.0))))               # exp(logit_scale) of the synthetic weights
    logits = scale * (img / np.linalg.norm(img, axis=-1, keepdims=True)) @ g["text_features"].astype(np.float64).T
    lerr = np.abs(logits - g["logits"]).max()
    print(f"[{tag}] float64 logits vs the reference's: {lerr:.2e}")
    assert lerr <= 1e-4


@pytest.mark.parametrize("shape", [(19, 77), (2, 8, 19, 77), (8, 19, 76), (8, 19, 78)])
def test_zeroshotclip2_rejects_tokens_of_the_wrong_shape(shape):
    from rpo_amd.zeroshot import ZeroshotCLIP2
    with pytest.raises(ValueError, match=r"\[T, n_cls, 77\]"):
        ZeroshotCLIP2({}, np.zeros(shape, dtype=np.int64))
