"""Host-side checks of the sweep trainer (rpo_amd/sweep.py) and its two C ABI additions,
rpo_head_fwd_bwd_grouped_k and rpo_sgd_step_sets: declared, exported and bound; bad arguments get the calls' own error
codes with nothing launched; what members may not differ in is refused by name before a device is touched; the gather /
scatter between a member's row and a standalone run's flat vector; a member's checkpoint is a standalone RPO(K = K_s)'s file
in both directions; seeded members draw RPO's prompts at their own K; the learning-rate table.  No GPU needed."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rpo_head_fwd_bwd_grouped_k", "rpo_sgd_step_sets")


def _cfg(K=8, depth=1):
    from rpo_amd.config import vit_b16
    return vit_b16(layers_v=depth, layers_t=depth, K=K)


def test_sweep_entry_points_are_declared_exported_and_bound():
    from rpo_amd import _lib, ops
    from rpo_amd.build import build_library
    build_library()
    hdr = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), f"{name} is not declared in include/rpo_amd.h"
        assert hasattr(lib, name), f"librpo_hip.so does not export {name}"
        assert name in _lib.SIGNATURES
    assert callable(ops.sgd_step_sets)
    import inspect
    assert "k_used" in inspect.signature(ops.head_fwd_bwd_grouped).parameters
    # additions to ABI 8, documented as such; the version does not move
    assert _lib.load().rpo_version() == 8 and "#define RPO_ABI_VERSION 8" in hdr
    assert hdr.count("(ABI 8 addition") >= 6


def test_sweep_entry_points_refuse_bad_arguments_without_launching():
    from rpo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                # 16-byte aligned host memory: never dereferenced
    BAD, SHAPE, DTYPE = _lib.E_BADARG, _lib.E_SHAPE, _lib.E_DTYPE
    head = lambda S=3, B=4, C=19, K=24, e=512, k=p, label=p, loss=p, act=None, dt=_lib.RPO_F32: lib.rpo_head_fwd_bwd_grouped_k(
        p, p, label, 100.0, p, loss, p, p, act, act, dt, S, B, C, K, e, k, p, None)
    assert head(k=None) == BAD                                  # callers without per-group K have their own entry point
    assert head(S=0) == BAD and head(S=-1) == BAD and head(B=0) == BAD and head(K=0) == BAD and head(loss=None) == BAD
    assert head(e=2048) == SHAPE and head(e=1025) == SHAPE and head(S=1025) == SHAPE
    assert head(act=p, dt=_lib.RPO_F32) == DTYPE
    sgd = lambda sets=3, stride=1024, hyper=p, seg0=256, seg1=384, pp=p, found=None: lib.rpo_sgd_step_sets(
        pp, p, p, stride, sets, hyper, None, seg0, seg1, 1, found, None)
    assert sgd(hyper=None) == BAD and sgd(pp=None) == BAD
    assert sgd(sets=0) == BAD and sgd(sets=-2) == BAD and sgd(seg0=0, seg1=0) == BAD and sgd(seg0=-1) == BAD
    assert sgd(stride=256 + 384 - 1) == SHAPE and sgd(stride=256 + 384 - 1, found=p) == SHAPE
    assert sgd(sets=65536) == SHAPE


def test_what_members_may_not_differ_in_is_refused_by_name_before_any_device_work(monkeypatch):
    from rpo_amd import engine, sweep
    from rpo_amd.config import rn_clip
    from rpo_amd.trainer import OptimConfig
    touched = []
    monkeypatch.setattr(engine, "make_engine", lambda *a, **k: touched.append(1))
    cfg = _cfg()
    mk = lambda **kw: [dict(seed=1, K=8, optim=OptimConfig()), dict(dict(seed=2, K=4, optim=OptimConfig(lr=0.02)), **kw)]
    with pytest.raises(ValueError, match="max_epoch"):
        sweep.RPOSweep(cfg, {}, members=mk(optim=OptimConfig(max_epoch=30)))
    with pytest.raises(ValueError, match="batch size"):
        sweep.RPOSweep(cfg, {}, members=mk(batch_size=8), batch_size=4)
    with pytest.raises(ValueError, match="storage mode"):
        sweep.RPOSweep(cfg, {}, members=mk(act_dtype=torch.float16), act_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="CLIP / class set / backbone"):
        sweep.RPOSweep(cfg, {}, members=mk(cfg=dataclasses.replace(cfg, n_cls=37)))
    with pytest.raises(NotImplementedError, match="ResNet"):
        sweep.RPOSweep(rn_clip((1, 1, 1, 1), 64, 1024, K=4), {}, members=mk())
    with pytest.raises(NotImplementedError, match="world_size"):
        sweep.RPOSweep(cfg, {}, members=mk(), world_size=2)
    with pytest.raises(ValueError, match="K = 0"):
        sweep.RPOSweep(cfg, {}, members=mk(K=0))
    with pytest.raises(ValueError, match="exactly one of seed= or prompts="):
        sweep.RPOSweep(cfg, {}, members=mk(prompts=(np.zeros((4, cfg.d_t)), np.zeros((4, cfg.d_v)))))        # both
    with pytest.raises(ValueError, match="exactly one of seed= or prompts="):
        sweep.RPOSweep(cfg, {}, members=mk(seed=None))                                                        # neither
    with pytest.raises(ValueError, match="members"):
        sweep.RPOSweep(cfg, {}, members=[])
    assert not touched


def test_gather_scatter_between_a_member_row_and_a_standalone_flat_vector():
    from rpo_amd.sweep import flat_to_member_row, member_row_to_flat, used_table
    K, Ks, dt, dv = 8, 3, 512, 768
    row = torch.arange(K * (dt + dv), dtype=torch.float32) + 1.0
    flat = member_row_to_flat(row, K, Ks, dt, dv)
    tp, ip = row[:K * dt].reshape(K, dt), row[K * dt:].reshape(K, dv)
    assert torch.equal(flat, torch.cat([tp[:Ks].reshape(-1), ip[:Ks].reshape(-1)]))          # the standalone file's flat order
    back = flat_to_member_row(flat, K, Ks, dt, dv)
    bt, bi = back[:K * dt].reshape(K, dt), back[K * dt:].reshape(K, dv)
    assert torch.equal(bt[:Ks], tp[:Ks]) and torch.equal(bi[:Ks], ip[:Ks])
    assert not bt[Ks:].any() and not bi[Ks:].any()                                           # inert columns zero
    assert torch.equal(member_row_to_flat(back, K, Ks, dt, dv), flat)
    assert torch.equal(member_row_to_flat(row, K, K, dt, dv), row) and torch.equal(flat_to_member_row(row, K, K, dt, dv), row)
    with pytest.raises(ValueError):
        flat_to_member_row(flat[:-1], K, Ks, dt, dv)
    assert used_table([8, 3], dt, dv).tolist() == [[8 * dt, 8 * dv], [3 * dt, 3 * dv]]
    assert used_table([8, 3], dt, dv).dtype == torch.int32


def _stand_in(cfg, member_K, optims):
    """An RPOSweep without an engine: the checkpoint code paths on stand-in buffers (as tests/test_multi_host.py)."""
    from rpo_amd import optim, sweep
    from rpo_amd.trainer import lr_at_epoch
    S, n = len(member_K), cfg.K * (cfg.d_t + cfg.d_v)
    tr = sweep.RPOSweep.__new__(sweep.RPOSweep)
    tr.cfg, tr.n_runs, tr.member_K, tr.optim_cfgs = cfg, S, list(member_K), list(optims)
    tr.member_cfgs = [dataclasses.replace(cfg, K=k) for k in member_K]
    tr.epoch, tr._steps = 2, 5
    tr.lr = [lr_at_epoch(oc, 2) for oc in optims]
    tr.engine = type("E", (), {})()
    tr.engine.m_params, tr.engine.m_mom = torch.zeros(S, n), torch.zeros(S, n)
    tr._opt = optim.make_optimizer(optims, n, cfg.K * cfg.d_t, cfg.K * cfg.d_v, "cpu", s0=tr.engine.m_mom,
                                   used=sweep.used_table(member_K, cfg.d_t, cfg.d_v))
    tr._opt.set_epoch(2)
    return tr


def test_member_checkpoint_is_a_standalone_rpo_file_of_its_own_K_in_both_directions(tmp_path):
    from rpo_amd import optim
    from rpo_amd.sweep import flat_to_member_row, member_row_to_flat
    from rpo_amd.trainer import RPO, OptimConfig, checkpoint_dict, load_checkpoint_file, lr_at_epoch, write_checkpoint
    cfg = _cfg(K=8)
    K, dt, dv = cfg.K, cfg.d_t, cfg.d_v
    member_K = [8, 3]
    optims = [OptimConfig(lr=0.01), OptimConfig(lr=0.02, momentum=0.8, weight_decay=1e-4)]
    tr = _stand_in(cfg, member_K, optims)
    g = torch.Generator().manual_seed(3)
    for s, k in enumerate(member_K):
        tr.engine.m_params[s] = flat_to_member_row(torch.randn(k * (dt + dv), generator=g), K, k, dt, dv)
        tr.engine.m_mom[s] = flat_to_member_row(torch.randn(k * (dt + dv), generator=g), K, k, dt, dv)
    dirs = [str(tmp_path / f"m{s}") for s in range(2)]
    paths = tr.save_model(dirs, is_best=True)
    assert paths[1] == os.path.join(dirs[1], "prompt_learner", "model.pth.tar-2")
    for s, k in enumerate(member_K):
        ck = load_checkpoint_file(paths[s])
        assert tuple(ck["state_dict"]["text_prompt"].shape) == (k, dt) and tuple(ck["state_dict"]["img_prompt"].shape) == (k, dv)
        mb = [ck["optimizer"]["state"][i]["momentum_buffer"] for i in (0, 1)]
        assert tuple(mb[0].shape) == (k, dt) and tuple(mb[1].shape) == (k, dv) and sum(m.numel() for m in mb) == k * (dt + dv)
        grp = ck["optimizer"]["param_groups"][0]
        assert grp["lr"] == lr_at_epoch(optims[s], 2) and grp["momentum"] == optims[s].momentum
        assert grp["weight_decay"] == optims[s].weight_decay and grp["initial_lr"] == optims[s].lr
        assert ck["epoch"] == 2 and ck["steps"] == 5
        # ---- through a standalone RPO(K = K_s)'s own reader
        kcfg = dataclasses.replace(cfg, K=k)

        class PL(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.text_prompt = torch.nn.Parameter(torch.zeros(kcfg.K, dt))
                self.img_prompt = torch.nn.Parameter(torch.zeros(kcfg.K, dv))

        solo = RPO.__new__(RPO)
        solo.model = type("M", (), {})()
        solo.model.prompt_learner = PL()
        solo.engine = type("E", (), {})()
        solo.engine.mom, solo.engine.params_version = torch.zeros(k * (dt + dv)), 0
        solo.optim_cfg, solo._graph = optims[s], None
        solo._opt = optim.make_optimizer([optims[s]], k * (dt + dv), k * (dt + dv), 0, "cpu", s0=solo.engine.mom)
        solo.load_model(dirs[s])
        want_p, want_m = member_row_to_flat(tr.engine.m_params[s], K, k, dt, dv), member_row_to_flat(tr.engine.m_mom[s], K, k, dt, dv)
        got_p = torch.cat([solo.model.prompt_learner.text_prompt.detach().reshape(-1),
                           solo.model.prompt_learner.img_prompt.detach().reshape(-1)])
        assert torch.equal(got_p, want_p) and torch.equal(solo.engine.mom, want_m)
        assert solo.epoch == 2 and solo._steps == 5 and solo.lr == lr_at_epoch(optims[s], 2)
        # the same keys and layout as the dict RPO.save_model builds
        want = checkpoint_dict(solo.model.prompt_learner.state_dict(), 2, want_m, optims[s], lr_at_epoch(optims[s], 2), 5, k * dt)
        assert list(ck) == list(want) and ck["optimizer"]["param_groups"] == want["optimizer"]["param_groups"]
    # ---- standalone files -> members
    solo_dirs, want_rows = [], []
    for s, k in enumerate(member_K):
        p, m = torch.randn(k * (dt + dv), generator=g), torch.randn(k * (dt + dv), generator=g)
        d = str(tmp_path / f"solo{s}")
        write_checkpoint(d, checkpoint_dict({"text_prompt": p[:k * dt].reshape(k, dt), "img_prompt": p[k * dt:].reshape(k, dv)},
                                            3, m, optims[s], 0.01, 7, k * dt), 3)
        solo_dirs.append(d)
        want_rows.append((flat_to_member_row(p, K, k, dt, dv), flat_to_member_row(m, K, k, dt, dv)))
    tr.load_model(solo_dirs, epoch=3)
    for s in range(2):
        assert torch.equal(tr.engine.m_params[s], want_rows[s][0]) and torch.equal(tr.engine.m_mom[s], want_rows[s][1])
    assert not tr.engine.m_params[1, 3 * dt:K * dt].any() and not tr.engine.m_mom[1, K * dt + 3 * dv:].any()
    assert tr.epoch == 3 and tr._steps == 7 and tr.lr == [lr_at_epoch(oc, 3) for oc in optims]
    assert tr._opt.epoch == 3 and torch.equal(tr._opt.hyper, optim.sgd_hyper_table(optims, 3))   # the table holds epoch 3's rates
    # a file of another K is refused by name; so are files of different epochs
    with pytest.raises(ValueError, match="this trainer has K = 8"):
        tr.load_model([solo_dirs[1], solo_dirs[1]], epoch=3)
    write_checkpoint(solo_dirs[1], checkpoint_dict({"text_prompt": torch.zeros(3, dt), "img_prompt": torch.zeros(3, dv)}, 4,
                                                   None, optims[1], 0.01, 0, 3 * dt), 3)
    with pytest.raises(ValueError, match="one loop runs all members"):
        tr.load_model(solo_dirs, epoch=3)


@pytest.mark.parametrize("second", ["sgd", "adam"])
def test_a_mix_of_files_with_and_without_optimiser_state_is_refused(tmp_path, second):
    """One first-step flag (plain SGD) / one loop (table-driven) covers every member: member 0's file has momentum, member 1's
    was written before its first step.  The wording is the trainer's own per optimiser family."""
    from rpo_amd.trainer import OptimConfig, checkpoint_dict, write_checkpoint
    cfg = _cfg(K=8)
    dt, dv = cfg.d_t, cfg.d_v
    optims = [OptimConfig(lr=0.01), OptimConfig(lr=0.02) if second == "sgd" else OptimConfig(name="adam", lr=1e-3)]
    tr = _stand_in(cfg, [8, 3], optims)
    dirs = []
    for s, k in enumerate([8, 3]):
        mom, steps = (torch.ones(k * (dt + dv)), 7) if s == 0 else (None, 0)
        ck = checkpoint_dict({"text_prompt": torch.zeros(k, dt), "img_prompt": torch.zeros(k, dv)}, 3, mom, optims[0], 0.01, steps, k * dt)
        write_checkpoint(str(tmp_path / f"m{s}"), ck, 3)
        dirs.append(str(tmp_path / f"m{s}"))
    want = ("RPOSweep.load_model: some checkpoints carry momentum and some do not (one first-step flag covers every member)"
            if second == "sgd" else "RPOSweep.load_model: some checkpoints carry optimiser state and some do not")
    with pytest.raises(ValueError) as err:
        tr.load_model(dirs, epoch=3)
    assert str(err.value) == want and tr.epoch == 2 and tr._steps == 5


def test_seeded_members_draw_rpo_initial_prompts_at_their_own_K():
    from rpo_amd import synth
    from rpo_amd.custom_clip import init_prompts
    from rpo_amd.sweep import sweep_prompts
    cfg = _cfg(K=4)
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    given = (np.full((3, cfg.d_t), 0.5, np.float32), np.full((3, cfg.d_v), -0.5, np.float32))
    members = [dict(seed=5, K=4), dict(prompts=given, K=3), dict(seed=6, K=2)]
    got = sweep_prompts(sd, members, cfg.d_t, cfg.d_v)
    for m, (tp, ip) in zip(members, got):
        assert tp.shape == (m["K"], cfg.d_t) and ip.shape == (m["K"], cfg.d_v)
        if "seed" in m:
            torch.manual_seed(m["seed"])
            wt, wi = init_prompts(sd, m["K"], cfg.d_t, cfg.d_v)
            assert np.array_equal(tp, wt) and np.array_equal(ip, wi)
    assert np.array_equal(got[1][0], given[0]) and np.array_equal(got[1][1], given[1])


def test_lr_table_follows_each_members_own_schedule():
    from rpo_amd.optim import sgd_hyper_table as hyper_table
    from rpo_amd.trainer import OptimConfig, lr_at_epoch
    ocs = [OptimConfig(lr=0.01, warmup_epoch=1, weight_decay=5e-4, momentum=0.9, max_epoch=4),
           OptimConfig(lr=0.035, warmup_epoch=2, warmup_cons_lr=3e-5, weight_decay=1e-3, momentum=0.8, max_epoch=4)]
    seen = set()
    for epoch in range(4):
        t = hyper_table(ocs, epoch)
        assert t.dtype == torch.float32 and tuple(t.shape) == (2, 4)
        for s, oc in enumerate(ocs):
            want = np.array([lr_at_epoch(oc, epoch), oc.momentum, oc.weight_decay, 1.0]).astype(np.float32)
            assert np.array_equal(t[s].numpy().view(np.uint32), want.view(np.uint32)), f"epoch {epoch} member {s}"
        seen.add(tuple(t[:, 0].tolist()))
    assert len(seen) == 4 and hyper_table(ocs, 1)[0, 0] != hyper_table(ocs, 1)[1, 0]
    assert hyper_table(ocs, 0, grad_scale=0.5)[:, 3].tolist() == [0.5, 0.5]


def test_sweep_imports_neither_oracle_nor_experiments():
    import ast
    mods = []
    for node in ast.walk(ast.parse(open(os.path.join(ROOT, "rpo_amd", "sweep.py")).read())):
        if isinstance(node, ast.Import):
            mods += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            mods.append(("." * node.level) + (node.module or ""))
    assert mods and not any(m.split(".")[0] == "oracle" or m.lstrip(".").startswith("experimental") for m in mods), mods
