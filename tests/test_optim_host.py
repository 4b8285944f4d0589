"""Host-side checks of the optimisers and schedules beyond SGD + cosine (rpo_amd/optim.py, rpo_amd/trainer.py:OptimConfig /
lr_at_epoch): the schedules against torch's own schedulers, the linear warm-up formula, the refusals,
the unchanged defaults, the new entry point's declaration / export / binding / argument checks, and torch.optim's
state-dict layout in both directions.  No GPU needed."""
import copy
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_EPOCH = 9


def _torch_schedule(sched: str, stepsize, gamma: float, lr: float, n: int):
    """lr in force during epochs 0 .. n - 1 of the torch scheduler the name stands for, driven on a dummy optimiser."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    if sched == "single_step":
        size = stepsize[-1] if stepsize[-1] > 0 else MAX_EPOCH
        s = torch.optim.lr_scheduler.StepLR(opt, step_size=size, gamma=gamma)
    elif sched == "multi_step":
        s = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=list(stepsize), gamma=gamma)
    else:
        s = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=MAX_EPOCH)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        s.step()
    return out


SCHEDULES = [("single_step", (-1,)), ("single_step", (3,)), ("single_step", (2, 5)), ("multi_step", (2, 5)), ("cosine", (-1,))]
WARMUPS = [("none", 0), ("constant", 1), ("constant", 3), ("linear", 1), ("linear", 3)]


@pytest.mark.parametrize("sched,stepsize", SCHEDULES)
@pytest.mark.parametrize("wtype,wep", WARMUPS)
def test_lr_at_epoch_is_the_torch_scheduler_behind_the_warm_up(sched, stepsize, wtype, wep):
    from rpo_amd.trainer import OptimConfig, lr_at_epoch
    lr, gamma = 0.0123, 0.3
    oc = OptimConfig(lr=lr, max_epoch=MAX_EPOCH, lr_scheduler=sched, stepsize=stepsize, gamma=gamma, warmup_epoch=wep,
                     warmup_type=wtype, warmup_cons_lr=2e-5, warmup_min_lr=3e-5)
    want = _torch_schedule(sched, stepsize, gamma, lr, MAX_EPOCH + 1)
    for e in range(MAX_EPOCH + 1):
        got = lr_at_epoch(oc, e)
        if e < wep:                                         # the warm-up wrapper does not step its successor
            if wtype == "constant":
                assert got == 2e-5
            else:                                           # Dassl's LinearWarmupScheduler, as remembered
                assert got == (3e-5 if e == 0 else lr * e / wep)
        else:
            w = want[e - wep]
            assert abs(got - w) <= 1e-12 * abs(w), (e, got, w)


def test_existing_cosine_and_constant_values_are_unchanged():
    import math
    from rpo_amd.trainer import OptimConfig, lr_at_epoch
    oc = OptimConfig()                                      # main_K24.yaml: cosine, one constant warm-up epoch
    assert lr_at_epoch(oc, 0) == 1e-5
    for e in range(1, 16):
        assert lr_at_epoch(oc, e) == 0.5 * 0.01 * (1.0 + math.cos(math.pi * (e - 1) / 15))
    oc = OptimConfig(lr=0.02, lr_scheduler="constant", warmup_epoch=2)
    assert [lr_at_epoch(oc, e) for e in range(5)] == [1e-5, 1e-5, 0.02, 0.02, 0.02]
    oc = OptimConfig(lr=0.02, lr_scheduler="constant", warmup_epoch=0)
    assert [lr_at_epoch(oc, e) for e in range(3)] == [0.02] * 3


def test_default_config_is_todays_on_the_old_fields_and_has_the_new_defaults():
    from rpo_amd.trainer import OptimConfig
    from rpo_amd.optim import is_plain_sgd
    oc = OptimConfig()
    old = dict(lr=0.01, max_epoch=15, lr_scheduler="cosine", warmup_epoch=1, warmup_type="constant", warmup_cons_lr=1e-5,
               momentum=0.9, weight_decay=5e-4)
    new = dict(name="sgd", sgd_dampening=0.0, sgd_nesterov=False, rmsprop_alpha=0.99, adam_beta1=0.9, adam_beta2=0.999,
               stepsize=(-1,), gamma=0.1, warmup_min_lr=1e-5)
    assert dataclasses.asdict(oc) == {**old, **new}
    assert [f.name for f in dataclasses.fields(oc)][:len(old)] == list(old)          # positional construction still means the same
    assert is_plain_sgd(oc) and is_plain_sgd(OptimConfig(lr=0.1, momentum=0.0))
    assert not is_plain_sgd(OptimConfig(sgd_nesterov=True)) and not is_plain_sgd(OptimConfig(sgd_dampening=0.1))
    assert not is_plain_sgd(OptimConfig(name="adam"))


def test_refusals(monkeypatch):
    from rpo_amd import engine, optim, sweep
    from rpo_amd.config import vit_b16
    from rpo_amd.trainer import OptimConfig
    with pytest.raises(ValueError, match="Dassl ships its own RAdam"):
        optim.validate(OptimConfig(name="radam"))
    with pytest.raises(ValueError, match="foo"):
        optim.validate(OptimConfig(name="foo"))
    with pytest.raises(ValueError, match="gamma"):
        optim.validate(OptimConfig(gamma=-0.1))
    with pytest.raises(ValueError, match="Nesterov"):
        optim.validate(OptimConfig(sgd_nesterov=True, momentum=0.0))
    for name in optim.KINDS:
        optim.validate(OptimConfig(name=name))
    # at construction of a trainer, before a device is touched
    touched = []
    monkeypatch.setattr(engine, "make_engine", lambda *a, **k: touched.append(1))
    cfg = vit_b16(layers_v=1, layers_t=1, K=4)
    for bad in (OptimConfig(name="radam"), OptimConfig(name="foo"), OptimConfig(gamma=-1.0)):
        with pytest.raises(ValueError):
            sweep.RPOSweep(cfg, {}, members=[dict(seed=1, K=4, optim=bad)])
    assert not touched


def test_entry_point_is_declared_exported_bound_and_refuses_bad_arguments():
    from rpo_amd import _lib, ops
    from rpo_amd.build import SOURCES, build_library
    assert "optim.hip" in SOURCES
    build_library()
    hdr = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\brpo_optim_step_sets\s*\(", src) and "rpo_optim_step_sets" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "rpo_optim_step_sets") and callable(ops.optim_step_sets)
    assert _lib.load().rpo_version() == 8 and "#define RPO_ABI_VERSION 8" in hdr
    comment = [c for c in re.findall(r"/\*.*?\*/", hdr, flags=re.S) if "(ABI 8 addition)" in c and "trainers/rpo.py:274" in c]
    assert comment and all(f"RPO_OPT_{k.upper()} = {v}" in hdr for k, v in __import__("rpo_amd.optim").optim.KINDS.items())
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                # host memory: never dereferenced, nothing is launched
    BAD, SHAPE = _lib.E_BADARG, _lib.E_SHAPE
    call = lambda pp=p, g=p, s0=p, s1=p, s2=None, stride=1024, sets=3, kind=p, hyper=p, step=p, seg0=256, seg1=384, needs=0, \
        found=None: lib.rpo_optim_step_sets(pp, g, s0, s1, s2, stride, sets, kind, hyper, step, None, seg0, seg1, needs, found, None)
    for kw in (dict(pp=None), dict(g=None), dict(s0=None), dict(s1=None), dict(kind=None), dict(hyper=None), dict(step=None),
               dict(sets=0), dict(sets=-2), dict(seg0=0, seg1=0), dict(seg0=-1), dict(seg1=-1), dict(needs=1)):
        assert call(**kw) == BAD, kw
    assert call(stride=256 + 384 - 1) == SHAPE and call(stride=256 + 384 - 1, found=p) == SHAPE
    assert call(sets=65536) == SHAPE and call(sets=65536, s2=p, needs=1) == SHAPE


SHAPES = [(4, 8), (3, 5)]                                    # text_prompt [K, d_t], img_prompt [K, d_v] of a tiny trainer


def _torch_optimizer(oc, params):
    kw = dict(lr=oc.lr, weight_decay=oc.weight_decay)
    if oc.name == "sgd":
        return torch.optim.SGD(params, momentum=oc.momentum, dampening=oc.sgd_dampening, nesterov=oc.sgd_nesterov, **kw)
    if oc.name == "rmsprop":
        return torch.optim.RMSprop(params, momentum=oc.momentum, alpha=oc.rmsprop_alpha, **kw)
    cls = torch.optim.AdamW if oc.name == "adamw" else torch.optim.Adam
    return cls(params, betas=(oc.adam_beta1, oc.adam_beta2), amsgrad=oc.name == "amsgrad", **kw)


@pytest.mark.parametrize("kw", [dict(name="sgd", sgd_nesterov=True), dict(name="sgd", sgd_dampening=0.3), dict(name="adam"),
                                dict(name="adamw"), dict(name="amsgrad"), dict(name="rmsprop"),
                                dict(name="rmsprop", momentum=0.0)], ids=lambda kw: "-".join(f"{v}" for v in kw.values()))
def test_state_dict_loads_into_torch_and_round_trips_bit_for_bit(kw):
    from rpo_amd import optim
    from rpo_amd.trainer import OptimConfig
    oc = OptimConfig(lr=0.003, weight_decay=1e-3, **kw)
    n = sum(int(np.prod(s)) for s in SHAPES)
    g = torch.Generator().manual_seed(5)
    names = optim.state_names(oc)
    rows = [torch.randn(n, generator=g).abs() for _ in names]            # made-up rows
    sd = optim.torch_state_dict(oc, 0.0021, rows, 7, SHAPES)
    # ---- torch's own object accepts it and holds exactly these tensors
    params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
    opt = _torch_optimizer(oc, params)
    ref = _torch_optimizer(oc, [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES])
    for q in ref.param_groups[0]["params"]:
        q.grad = torch.ones_like(q)
    ref.step()
    want = ref.state_dict()
    assert set(sd["param_groups"][0]) - {"initial_lr"} == set(want["param_groups"][0])
    assert all(list(sd["state"][i]) == list(want["state"][i]) for i in range(len(SHAPES))), "torch's keys, in torch's order"
    opt.load_state_dict(copy.deepcopy(sd))           # (torch keeps the tensors it is given: the step below writes them)
    back = opt.state_dict()
    assert back["param_groups"][0]["lr"] == 0.0021 and back["param_groups"][0]["params"] == [0, 1]
    off = 0
    for i, s in enumerate(SHAPES):
        m = int(np.prod(s))
        st = back["state"][i]
        if oc.name != "sgd":
            assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 7.0
        for nm, row in zip(names, rows):
            if nm == "momentum_buffer" and oc.name == "rmsprop" and oc.momentum == 0:
                assert nm not in st
                continue
            assert st[nm].dtype == torch.float32 and tuple(st[nm].shape) == s
            assert torch.equal(st[nm].reshape(-1).view(torch.int32), row[off:off + m].view(torch.int32))
        off += m
    for q in params:                                         # and torch can step from it
        q.grad = torch.ones_like(q)
    opt.step()
    # ---- and back into rows
    got = optim.rows_from_state_dict(oc, sd, SHAPES)
    assert got is not None and got[1] == (1 if oc.name == "sgd" else 7)
    for nm, a, b in zip(names, got[0], rows):
        if nm == "momentum_buffer" and oc.name == "rmsprop" and oc.momentum == 0:
            assert not a.any()
        else:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # a file of another kind or of other shapes carries no matching state; nor does one without state
    other = OptimConfig(name="rmsprop" if oc.name != "rmsprop" else "adam")
    assert optim.rows_from_state_dict(other, sd, SHAPES) is None
    assert optim.rows_from_state_dict(oc, sd, [(4, 8), (3, 6)]) is None
    assert optim.rows_from_state_dict(oc, optim.torch_state_dict(oc, 0.1, rows, 0, SHAPES), SHAPES) is None
    assert optim.torch_state_dict(oc, 0.1, rows, 0, SHAPES)["state"] == {}


def test_hyper_table_carries_the_betas_to_double_precision():
    from rpo_amd import optim
    from rpo_amd.trainer import OptimConfig, lr_at_epoch
    ocs = [OptimConfig(name="sgd", sgd_nesterov=True, lr=0.01), OptimConfig(name="adam", lr=1e-3, weight_decay=0.0),
           OptimConfig(name="rmsprop", lr=2e-3, momentum=0.5), OptimConfig(name="sgd", sgd_dampening=0.3)]
    t = optim.hyper_table(ocs, 2, grad_scale=0.5)
    assert t.dtype == torch.float32 and tuple(t.shape) == (4, 8) and optim.kind_table(ocs).tolist() == [0, 1, 4, 0]
    for s, oc in enumerate(ocs):
        assert t[s, 0] == np.float32(lr_at_epoch(oc, 2)) and t[s, 1] == 0.5 and t[s, 2] == np.float32(oc.weight_decay)
    assert t[0, 6] == 1.0 and t[3, 6] == 0.0 and t[0, 3] == np.float32(0.9) and t[0, 4] == 0.0
    assert abs((float(t[1, 3]) + float(t[1, 6])) - 0.9) < 1e-15 and abs((float(t[1, 4]) + float(t[1, 7])) - 0.999) < 1e-15
    assert abs((float(t[2, 4]) + float(t[2, 7])) - 0.99) < 1e-15 and t[2, 3] == 0.5 and t[2, 5] == np.float32(1e-8)
    assert abs((float(t[3, 4]) + float(t[3, 7])) - 0.3) < 1e-15


# ------------------------------------------------------------------------------ the plain-SGD optimiser: what it launches
def _recorders(monkeypatch):
    from rpo_amd import ops
    calls = []
    for fn in ("sgd_step", "sgd_step_guarded", "sgd_step_sets"):
        monkeypatch.setattr(ops, fn, lambda *a, _fn=fn, **k: calls.append((_fn, a, k)))
    monkeypatch.setattr(ops, "optim_step_sets", lambda *a, **k: pytest.fail("the table-driven kernel from PlainSGD"))
    return calls


def _is(a: torch.Tensor, b: torch.Tensor) -> bool:
    """The same memory seen the same way: what a kernel launch would get."""
    return a.data_ptr() == b.data_ptr() and tuple(a.shape) == tuple(b.shape) and a.stride() == b.stride() and a.dtype == b.dtype


def test_plain_sgd_issues_the_launches_the_trainers_issued(monkeypatch):
    """`PlainSGD` calls the ops function the trainers called, with their arguments and slices: rpo_sgd_step over the whole
    flat buffer [text 8 | img 16] or one half, rpo_sgd_step_guarded with a found_inf, the rate of the epoch as a kernel
    argument (and as the graph key); with `used`, rpo_sgd_step_sets on a device table [S, 4] and a constant graph key."""
    from rpo_amd import optim
    from rpo_amd.trainer import OptimConfig, lr_at_epoch
    calls = _recorders(monkeypatch)
    oc = OptimConfig(lr=0.01, momentum=0.8, weight_decay=1e-3, max_epoch=3)
    nt, n = 8, 24
    p, g, m = torch.arange(n, dtype=torch.float32), torch.ones(n), torch.zeros(n)
    opt = optim.make_optimizer([oc], n, n, 0, "cpu", s0=m, grad_scale=0.25)
    assert type(opt) is optim.PlainSGD and opt.splittable and not opt.table_driven
    lr0, lr1 = lr_at_epoch(oc, 0), lr_at_epoch(oc, 1)
    assert lr0 != lr1 and opt.graph_key() == lr0
    # ---- the whole buffer: the first step, then a later one
    opt.step(p, g, None, first_step=True)
    opt.step(p, g, first_step=False)
    for (fn, a, k), first in zip(calls, (True, False)):
        assert fn == "sgd_step" and _is(a[0], p) and _is(a[1], g) and _is(a[2], m)
        assert a[3:] == (lr0, 0.8, 1e-3, 0.25) and k == {"first_step": first}
    # ---- each half (RPO's early text): [0, nt) and [nt, n) of all three buffers
    del calls[:]
    opt.step(p, g, first_step=False, part=slice(0, nt))
    opt.step(p, g, first_step=False, part=slice(nt, None))
    for (fn, a, k), sl in zip(calls, (slice(0, nt), slice(nt, None))):
        assert fn == "sgd_step" and _is(a[0], p[sl]) and _is(a[1], g[sl]) and _is(a[2], m[sl]) and a[0].numel() in (nt, n - nt)
        assert a[3:] == (lr0, 0.8, 1e-3, 0.25) and k == {"first_step": False}
    # ---- guarded: a found_inf selects rpo_sgd_step_guarded (never with a part)
    del calls[:]
    found = torch.zeros(2, dtype=torch.int32)
    opt.step(p, g, found, first_step=True)
    (fn, a, k), = calls
    assert fn == "sgd_step_guarded" and _is(a[0], p) and _is(a[1], g) and _is(a[2], m) and a[3:] == (lr0, 0.8, 1e-3, 0.25)
    assert set(k) == {"first_step", "found_inf"} and k["first_step"] is True and k["found_inf"] is found
    with pytest.raises(AssertionError):
        opt.step(p, g, found, part=slice(0, nt))
    # ---- a new epoch: the rate of the next launch and the graph key change; the same epoch again changes nothing
    del calls[:]
    opt.set_epoch(1)
    opt.set_epoch(1)
    opt.step(p, g, first_step=False)
    assert calls[0][1][3] == lr1 and opt.graph_key() == lr1 and opt.epoch == 1
    # ---- a [S, n] buffer with one shared config (RPOMulti): one launch over the flat view, grad_scale 1
    del calls[:]
    P, G, M = p.view(2, 12), g.view(2, 12), torch.zeros(2, 12)
    multi = optim.make_optimizer([oc], n, n, 0, "cpu", s0=M)
    multi.step(P, G, None, first_step=True)
    (fn, a, k), = calls
    assert fn == "sgd_step" and _is(a[0], P.view(-1)) and _is(a[1], G.view(-1)) and _is(a[2], M.view(-1))
    assert a[3:] == (lr0, 0.8, 1e-3, 1.0) and k == {"first_step": True}
    # ---- the sets form: 2 sets with their own configs, `used` shorter than the segments
    del calls[:]
    ocs = [oc, OptimConfig(lr=0.02, momentum=0.9, weight_decay=5e-4, max_epoch=3, warmup_epoch=2)]
    used = torch.tensor([[3, 5], [4, 8]], dtype=torch.int32)
    sets = optim.make_optimizer(ocs, 12, 4, 8, "cpu", s0=M, used=used)
    assert type(sets) is optim.PlainSGD and not sets.splittable and not sets.table_driven and sets.graph_key() == 0
    found2 = torch.zeros(2, 2, dtype=torch.int32)
    sets.step(P, G, None, first_step=True)
    sets.step(P, G, found2, first_step=False)
    for (fn, a, k), fi, first in zip(calls, (None, found2), (True, False)):
        assert fn == "sgd_step_sets" and _is(a[0], P) and _is(a[1], G) and _is(a[2], M) and a[3] is sets.hyper and a[4:] == (4, 8)
        assert set(k) == {"first_step", "used", "found_inf"} and k["first_step"] is first and k["used"] is used and k["found_inf"] is fi
    assert torch.equal(sets.hyper, optim.sgd_hyper_table(ocs, 0)) and tuple(sets.hyper.shape) == (2, 4)
    table = sets.hyper
    for epoch in (1, 2, 7):                             # (7: past the schedule's end, the formula still gives a rate)
        sets.set_epoch(epoch)
        assert sets.hyper is table and torch.equal(table, optim.sgd_hyper_table(ocs, epoch)) and sets.graph_key() == 0
    assert not torch.equal(optim.sgd_hyper_table(ocs, 1), optim.sgd_hyper_table(ocs, 2))
    with pytest.raises(AssertionError):
        sets.step(P, G, None, part=slice(0, 4))
    # ---- one member that is not plain SGD: the table-driven optimiser for all of them
    assert not optim.is_plain_sgd(OptimConfig(sgd_nesterov=True)) and not optim.is_plain_sgd(OptimConfig(name="adam"))


@pytest.mark.parametrize("steps", [0, 3])
def test_plain_sgd_state_dict_is_torch_optim_sgds_layout_and_loads_back(steps):
    """The `optimizer` entry of a plain-SGD trainer, key order included, against the literal dict (the layout the LP and
    host-logic tests pin against the reference's file); `load_state_dict` restores the momentum row from it."""
    from rpo_amd import optim
    from rpo_amd.trainer import OptimConfig
    oc = OptimConfig(lr=0.01, momentum=0.8, weight_decay=1e-3)
    shapes = [(2, 4), (2, 8)]
    m = torch.arange(24, dtype=torch.float32) * 0.5 - 3.0
    opt = optim.make_optimizer([oc], 24, 24, 0, "cpu", s0=m.clone())
    got = opt.state_dict(shapes, lr=0.004, steps=steps)
    state = {} if steps == 0 else {0: {"momentum_buffer": m[:8].reshape(2, 4)}, 1: {"momentum_buffer": m[8:].reshape(2, 8)}}
    want = {"state": state,
            "param_groups": [{"lr": 0.004, "momentum": 0.8, "dampening": 0, "weight_decay": 1e-3, "nesterov": False,
                              "maximize": False, "foreach": None, "differentiable": False, "fused": None, "initial_lr": 0.01,
                              "params": [0, 1]}]}
    assert list(got) == list(want) and list(got["state"]) == list(want["state"])
    (gg,), (wg,) = got["param_groups"], want["param_groups"]
    assert list(gg.items()) == list(wg.items()) and all(type(gg[k]) is type(wg[k]) for k in wg)
    for i in want["state"]:
        assert list(got["state"][i]) == ["momentum_buffer"]
        a, b = got["state"][i]["momentum_buffer"], want["state"][i]["momentum_buffer"]
        assert a.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b)
        assert a.data_ptr() != opt.s0.data_ptr()                      # a copy, not a view of the live buffer
    if steps:                                                         # torch.optim.SGD itself takes it
        params = [torch.nn.Parameter(torch.zeros(sh)) for sh in shapes]
        topt = torch.optim.SGD(params, lr=0.1, momentum=0.9)
        topt.load_state_dict(got)
        assert torch.equal(topt.state[params[1]]["momentum_buffer"], m[8:].reshape(2, 8))
    # ---- and back: a fresh optimiser's momentum row
    fresh_m = torch.zeros(24)
    fresh = optim.make_optimizer([oc], 24, 24, 0, "cpu", s0=fresh_m)
    assert fresh.load_state_dict(want, shapes, steps=steps) is (steps > 0)
    assert torch.equal(fresh_m, m if steps else torch.zeros(24))
    assert not fresh.load_state_dict(want, [(2, 4), (4, 4)]) and not fresh.load_state_dict(None, shapes)
    assert optim.state_shapes(oc, want) == ([] if steps == 0 else shapes)
