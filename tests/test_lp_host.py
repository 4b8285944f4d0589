"""Host-side checks of the linear-probe trainer (rpo_amd/lp.py, csrc/lp_head.hip): the C ABI entry points, the fixtures'
provenance record, the checkpoint layout against the reference's own file, and the arguments refused before any device
is touched.  No GPU needed."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_lp_head_is_declared_exported_and_bound():
    from rpo_amd import _lib
    from rpo_amd.build import SOURCES, build_library
    assert "lp_head.hip" in SOURCES
    build_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpo_amd.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rpo_lp_head_workspace_floats", "rpo_lp_head_fwd_bwd"):
        assert re.search(rf"\b{name}\s*\(", src), f"{name} is not declared in include/rpo_amd.h"
        assert hasattr(lib, name), f"librpo_hip.so does not export {name}"
        assert name in _lib.SIGNATURES
    assert _lib.load().rpo_version() == 8
    # workspace: dz [B, e] + row max / sum-exp partials per 32-class tile
    assert _lib.load().rpo_lp_head_workspace_floats(32, 1000, 512) == 32 * 512 + 2 * 32 * 32


def test_lp_head_refuses_unsupported_shapes_without_launching():
    from rpo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    for B, C, e in ((0, 19, 512), (129, 19, 512), (3, 19, 520), (3, 19, 2048), (3, 0, 512), (3, 19, 16)):
        rc = lib.rpo_lp_head_fwd_bwd(p, p, p, p, None, 100.0, p, p, None, None, None, B, C, e, p, None)
        assert rc == _lib.E_SHAPE, (B, C, e, rc)
    # training call without the gradient pointers
    assert lib.rpo_lp_head_fwd_bwd(p, p, p, p, p, 100.0, p, p, None, None, None, 3, 19, 512, p, None) == _lib.E_BADARG


def test_manifest_lp_matches_the_committed_fixtures():
    man = json.load(open(os.path.join(GOLD, "manifest_lp.json")))
    assert man["generator"] == "tools/make_golden_lp.py"
    names = set(man["files"])
    assert {"ref_lp_d2_b3.npz", "ref_lp_full_b32.npz", "ref_lp_ckpt.npz"} <= names
    total = 0
    for name, rec in man["files"].items():
        path = os.path.join(GOLD, name)
        assert os.path.exists(path), path
        assert os.path.getsize(path) == rec["bytes"], (name, os.path.getsize(path), rec["bytes"])
        total += rec["bytes"]
    assert total < 1e6
    for name in names:                          # no dense e x e matrix in a fixture (tests/lp_fixtures.py)
        assert man["files"][name]["bytes"] < 512 * 1024, name


def test_default_optim_is_the_ctxv1_yaml():
    from rpo_amd.lp import LP_PROMPT, lp_optim_config
    from rpo_amd.trainer import lr_at_epoch
    oc = lp_optim_config()
    # configs/trainers/LP/vit_b16_c4_ep10_batch1_ctxv1.yaml + Dassl's SGD defaults
    assert (oc.lr, oc.max_epoch, oc.lr_scheduler, oc.warmup_epoch, oc.warmup_type, oc.warmup_cons_lr) == \
        (5e-4, 30, "cosine", 1, "constant", 1e-5)
    assert (oc.momentum, oc.weight_decay) == (0.9, 5e-4)
    assert lr_at_epoch(oc, 0) == 1e-5 and lr_at_epoch(oc, 1) == 5e-4
    assert LP_PROMPT.format(cls_name="abyssinian") == "A photo of a abyssinian"


def test_fp16_precision_is_refused_before_any_device_work(monkeypatch):
    from rpo_amd import lp
    touched = []
    monkeypatch.setattr(lp, "make_engine", lambda *a, **k: touched.append(1))
    with pytest.raises(ValueError, match="dtype error"):
        lp.LP({}, np.zeros((19, 77), np.int64), prec="fp16")
    with pytest.raises(ValueError, match="prec must be"):
        lp.LP({}, np.zeros((19, 77), np.int64), prec="bf16")
    assert not touched


def _fake_trainer(steps: int):
    """An LP trainer object without an engine: enough for checkpoint_dict (the host side of save_model)."""
    from rpo_amd import lp, optim
    e = 512
    eng = type("E", (), {})()
    eng.lp_params = torch.arange(e * e + e, dtype=torch.float32) * 1e-6
    eng.lp_w, eng.lp_b = eng.lp_params[:e * e].view(e, e), eng.lp_params[e * e:]
    eng.lp_moms = torch.linspace(-1, 1, e * e + e)
    model = lp.LPCustomCLIP.__new__(lp.LPCustomCLIP)
    model.engine = eng
    tr = lp.LP.__new__(lp.LP)
    tr.model, tr.engine, tr.optim_cfg = model, eng, lp.lp_optim_config()
    tr.epoch, tr.lr, tr._steps = 1, 5e-4, steps
    tr._opt = optim.make_optimizer([tr.optim_cfg], e * e + e, e * e + e, 0, "cpu", s0=eng.lp_moms)
    return tr


def test_checkpoint_round_trips_and_matches_the_reference_layout(tmp_path):
    from rpo_amd.lp import LP_MODEL_NAME
    from rpo_amd.trainer import load_checkpoint_file, write_checkpoint
    from lp_fixtures import write_reference_checkpoint
    tr = _fake_trainer(steps=3)
    ck = tr.checkpoint_dict()
    path = write_checkpoint(str(tmp_path), ck, ck["epoch"], is_best=True, name=LP_MODEL_NAME)
    assert path == os.path.join(str(tmp_path), "lp_layer", "model.pth.tar-1")
    assert os.path.exists(os.path.join(str(tmp_path), "lp_layer", "model-best.pth.tar"))
    back = load_checkpoint_file(path)                   # the restricted loader
    assert torch.equal(back["state_dict"]["weight"], tr.engine.lp_w) and torch.equal(back["state_dict"]["bias"], tr.engine.lp_b)
    m = back["optimizer"]["state"]
    assert torch.equal(torch.cat([m[0]["momentum_buffer"].reshape(-1), m[1]["momentum_buffer"].reshape(-1)]), tr.engine.lp_moms)
    # ... and the reference's own file (Dassl's dict after one torch.optim.SGD step on lp_layer, rebuilt from its fixture)
    ref = load_checkpoint_file(write_reference_checkpoint(os.path.join(GOLD, "ref_lp_ckpt.npz"), str(tmp_path / "ref")))
    assert set(ref) <= set(back), set(ref) - set(back)
    assert list(ref["state_dict"]) == list(back["state_dict"]) == ["weight", "bias"]
    for k in ("weight", "bias"):
        assert ref["state_dict"][k].shape == back["state_dict"][k].shape
    rg, bg = ref["optimizer"]["param_groups"][0], back["optimizer"]["param_groups"][0]
    assert rg["params"] == bg["params"] == [0, 1]
    for key in ("lr", "momentum", "weight_decay", "dampening", "nesterov"):
        assert key in bg
    assert (rg["momentum"], rg["weight_decay"]) == (bg["momentum"], bg["weight_decay"])
    for i, k in enumerate(("weight", "bias")):
        assert ref["optimizer"]["state"][i]["momentum_buffer"].shape == m[i]["momentum_buffer"].shape == \
            ref["state_dict"][k].shape
    # no step yet: no momentum state, as torch.optim.SGD
    assert _fake_trainer(steps=0).checkpoint_dict()["optimizer"]["state"] == {}


def test_write_checkpoint_default_directory_is_unchanged(tmp_path):
    from rpo_amd.trainer import write_checkpoint
    path = write_checkpoint(str(tmp_path), {"state_dict": {}, "epoch": 2}, 2)
    assert path == os.path.join(str(tmp_path), "prompt_learner", "model.pth.tar-2")


def test_lp_module_imports_neither_oracle_nor_experiments():
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "rpo_amd", "lp.py")).read())
    tree2 = ast.parse(open(os.path.join(ROOT, "rpo_amd", "engine_lp.py")).read())
    mods = []
    for t in (tree, tree2):
        for node in ast.walk(t):
            if isinstance(node, ast.Import):
                mods += [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                mods.append(("." * node.level) + (node.module or ""))
    assert not any(m.split(".")[0] == "oracle" or m.lstrip(".").startswith("experimental") for m in mods), mods


def test_reference_checkpoint_rebuild_matches_the_stored_dense_samples(tmp_path):
    """The checkpoint rebuilt from the step's gradient factors agrees with the dense rows, diagonal and bias of the
    reference's W and momentum that the fixture keeps, and carries the layout recorded from the reference's dict."""
    import json
    from lp_fixtures import write_reference_checkpoint
    from rpo_amd.trainer import load_checkpoint_file
    npz = os.path.join(GOLD, "ref_lp_ckpt.npz")
    g = np.load(npz)
    ck = load_checkpoint_file(write_reference_checkpoint(npz, str(tmp_path)))
    w, mw = ck["state_dict"]["weight"].numpy(), ck["optimizer"]["state"][0]["momentum_buffer"].numpy()
    n = g["w_rows"].shape[0]
    for got, want in ((w[:n], g["w_rows"]), (np.diag(w), g["w_diag"]), (mw[:n], g["mom_w_rows"]),
                      (np.diag(mw), g["mom_w_diag"]), (ck["state_dict"]["bias"].numpy(), g["bias"]),
                      (ck["optimizer"]["state"][1]["momentum_buffer"].numpy(), g["mom_b"])):
        assert np.abs(got - want).max() <= 1e-6 * max(1.0, float(np.abs(want).max()))
    layout = json.loads(bytes(g["layout"]).decode())
    assert list(ck) == layout["keys"] and ck["epoch"] == layout["epoch"] == 1
    assert ck["optimizer"]["param_groups"] == layout["param_groups"] and ck["scheduler"] == layout["scheduler"]
    assert sorted(ck["optimizer"]["state"][0]) == layout["state_keys"]["0"] == ["momentum_buffer"]
