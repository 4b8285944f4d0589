"""Host-side checks of the linear-probe sweep (rpo_amd/lp_sweep.py) and its C ABI addition
rpo_lp_head_fwd_bwd_grouped: declared, exported and bound; bad arguments get the call's own error codes with nothing
launched; what the sweep does not do is refused by name before a device is touched; the members' optimiser tables are
optim.hyper_table / kind_table of their configs; a member's checkpoint is a standalone LP's file in both directions.
No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rpo_lp_head_fwd_bwd_grouped"


def _cfg(depth=1):
    from rpo_amd.config import vit_b16
    return vit_b16(layers_v=depth, layers_t=depth, K=1)


def test_grouped_lp_head_is_declared_exported_and_bound():
    import inspect
    import rpo_amd
    from rpo_amd import _lib, ops
    from rpo_amd.build import build_library
    build_library()
    hdr = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(rf"\b{NAME}\s*\(", src), f"{NAME} is not declared in include/rpo_amd.h"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), f"librpo_hip.so does not export {NAME}"
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int32 or restype is ctypes.c_int
    decl = src[src.index(f"int {NAME}("):]
    decl = decl[:decl.index(";")]
    assert len(argtypes) == decl.count(",") + 1 == 16, "the ctypes signature has the header's parameter count"
    assert argtypes[2] is ctypes.c_int64 and "int64_t set_stride" in decl
    assert list(inspect.signature(ops.lp_head_fwd_bwd_grouped).parameters)[:3] == ["img_f", "params", "text_f_n"]
    # an addition to ABI 8, documented as such; the version does not move
    assert _lib.load().rpo_version() == 8 and "#define RPO_ABI_VERSION 8" in hdr
    comment = hdr[:hdr.index(f"int {NAME}(")].rsplit("/*", 1)[1]
    assert comment.lstrip().startswith("(ABI 8 addition)")
    from rpo_amd.lp_sweep import LPSweep
    assert rpo_amd.LPSweep is LPSweep and "LPSweep" in rpo_amd.__all__


def test_grouped_lp_head_refuses_bad_arguments_without_launching():
    from rpo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                  # 16-byte aligned host memory: never dereferenced
    BAD, SHAPE, ALIGN = _lib.E_BADARG, _lib.E_SHAPE, _lib.E_ALIGN
    e = 64
    call = lambda S=3, B=4, C=19, e=e, stride=e * e + e, img=p, params=p, t=p, label=p, z=p, logits=p, loss=p, grads=p, ws=p: \
        lib.rpo_lp_head_fwd_bwd_grouped(img, params, stride, t, label, 100.0, z, logits, loss, grads, S, B, C, e, ws, None)
    for kw in (dict(img=None), dict(params=None), dict(t=None), dict(z=None), dict(logits=None), dict(ws=None),
               dict(loss=None), dict(grads=None)):
        assert call(**kw) == BAD, kw
    for kw in (dict(S=0), dict(S=-1), dict(S=1025), dict(stride=e * e + e - 4), dict(B=0), dict(B=129), dict(C=0),
               dict(C=32769), dict(e=16), dict(e=48), dict(e=1056, stride=1056 * 1057)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(stride=e * e + e + 2), dict(params=p + 4), dict(img=p + 8), dict(z=p + 4), dict(t=p + 12)):
        assert call(**kw) == ALIGN, kw
    # eval needs neither loss nor grads; its other refusals are the same
    assert call(label=None, loss=None, grads=None, S=0) == SHAPE and call(label=None, loss=None, grads=None, z=None) == BAD


def _members(**second):
    from rpo_amd.trainer import OptimConfig
    return [dict(optim=OptimConfig(lr=5e-4, max_epoch=4)), dict(dict(optim=OptimConfig(name="adam", lr=1e-3, max_epoch=4)), **second)]


class _Set:
    """The few things an evaluation reads of an image set before it touches the device."""
    def __init__(self, labels):
        self.labels = list(labels)

    def __len__(self):
        return len(self.labels)

    def check_labels(self, n_cls):
        assert all(0 <= v < n_cls for v in self.labels)


def _stand_in(cfg, optims, e=None):
    """An LPSweep without an engine: the refusals of the evaluation and the checkpoint code on stand-in buffers."""
    from rpo_amd import lp_sweep
    from rpo_amd.trainer import lr_at_epoch
    import dataclasses
    e = e or cfg.embed
    cfg = dataclasses.replace(cfg, embed=e, d_t=e)                # (a narrow layer keeps the stand-in's rows small)
    S, stride = len(optims), e * e + e
    tr = lp_sweep.LPSweep.__new__(lp_sweep.LPSweep)
    tr.cfg, tr.n_runs, tr.optim_cfgs, tr.amp, tr._found_inf, tr._graph = cfg, S, list(optims), False, None, None
    tr.epoch, tr._steps = 2, 5
    tr.lr = [lr_at_epoch(oc, 2) for oc in optims]
    eng = tr.engine = type("E", (), {})()
    eng.cfg, eng.act, eng.weights_id, eng.dev = cfg, torch.float32, "0badc0de", torch.device("cpu")
    eng.lps_params, eng.lps_moms = torch.zeros(S, stride), torch.zeros(S, stride)
    eng.lps_w, eng.lps_b = eng.lps_params[:, :e * e].view(S, e, e), eng.lps_params[:, e * e:]
    tr.device = eng.dev
    tr._opt = lp_sweep.member_optimizer(optims, stride, "cpu", eng.lps_moms)
    tr._opt.set_epoch(2)
    return tr


def test_what_the_sweep_does_not_do_is_refused_by_name_before_any_device_work(monkeypatch):
    from rpo_amd import engine, lp_sweep
    from rpo_amd.config import rn_clip
    from rpo_amd.features import ImageFeatures
    from rpo_amd.trainer import OptimConfig
    touched = []
    monkeypatch.setattr(engine, "make_engine", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(torch.cuda, "device", lambda *a, **k: touched.append(2))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cfg, toks = _cfg(), np.zeros((19, 77), np.int64)
    with pytest.raises(NotImplementedError, match="LPSweep: world_size > 1"):
        lp_sweep.LPSweep({}, toks, members=_members(), cfg=cfg, world_size=2)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="LPSweep: world_size > 1"):
        lp_sweep.LPSweep({}, toks, members=_members(), cfg=cfg)
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(NotImplementedError, match="LPSweep on a ResNet"):
        lp_sweep.LPSweep({}, toks, members=_members(), cfg=rn_clip((1, 1, 1, 1), 64, 1024))
    with pytest.raises(ValueError, match="PREC fp16 is not supported"):
        lp_sweep.LPSweep({}, toks, members=_members(), cfg=cfg, prec="fp16")
    with pytest.raises(ValueError, match="LPSweep: no members"):
        lp_sweep.LPSweep({}, toks, members=[], cfg=cfg)
    with pytest.raises(ValueError, match=r"LPSweep: the members differ in max_epoch \(\[4, 30\]\)"):
        lp_sweep.LPSweep({}, toks, members=_members(optim=OptimConfig(max_epoch=30)), cfg=cfg)
    with pytest.raises(ValueError, match="radam"):                                   # optim.py's own refusals hold per member
        lp_sweep.LPSweep({}, toks, members=_members(optim=OptimConfig(name="radam", max_epoch=4)), cfg=cfg)
    with pytest.raises(ValueError, match="member 1's weight / bias"):
        lp_sweep.LPSweep({}, toks, members=_members(weight=np.eye(8, dtype=np.float32)), cfg=cfg)
    # ---- evaluation: class sets, and features of another engine or set
    tr = _stand_in(cfg, [m["optim"] for m in _members()], e=32)
    ds = _Set([0, 1, 2, 18])
    want = "LPSweep.*classes=.*load the member's checkpoint into an LP"
    for call in (lambda: tr.test_all(ds, classes=object()), lambda: tr.test(ds, member=1, classes=object()),
                 lambda: tr.model_inference(torch.zeros(1, 3, 8, 8), classes=object()), lambda: tr.class_set(toks)):
        with pytest.raises(NotImplementedError, match=want):
            call()
    eng = tr.engine
    cfg = tr.cfg
    meta = ImageFeatures._meta(cfg, eng.act, eng.weights_id, 4)
    feat = lambda **kw: ImageFeatures(dict(meta, **kw.pop("meta", {})), torch.zeros(4, cfg.embed), torch.tensor(ds.labels),
                                      kw.pop("labels", list(ds.labels)), torch.device("cpu"))
    with pytest.raises(ValueError, match="weights: features deadbeef, asked 0badc0de"):
        tr.test_all(ds, features=feat(meta=dict(weights="deadbeef")))
    with pytest.raises(ValueError, match="act_dtype"):
        tr.test(ds, member=0, features=feat(meta=dict(act_dtype=torch.bfloat16)))
    with pytest.raises(ValueError, match="n_images: features 4, asked 3"):
        tr.test_all(_Set([0, 1, 2]), features=feat())
    with pytest.raises(ValueError, match="labels"):
        tr.test_all(ds, features=feat(labels=[0, 1, 2, 17]))
    with pytest.raises(ValueError, match="n_images"):
        tr.train(ds, val_set=_Set([0, 1, 2]), val_features=feat())
    with pytest.raises(ValueError, match="pass both"):
        tr.train(ds, val_features=feat())
    with pytest.raises(IndexError, match="member 2 of 2"):
        tr.test(ds, member=2)
    assert not touched


@pytest.mark.parametrize("kinds", [("sgd", "sgd"), ("sgd", "nesterov", "adam", "amsgrad", "rmsprop", "adamw")])
def test_member_tables_are_the_optimisers_own(kinds):
    """The members' device tables equal optim.hyper_table / kind_table (all plain SGD: sgd_hyper_table) of the configs at
    every epoch, so the rates a member sees are its standalone run's; nothing about them is a kernel argument."""
    from rpo_amd import optim
    from rpo_amd.lp_sweep import member_optimizer
    from rpo_amd.trainer import OptimConfig
    mk = {"sgd": lambda i: OptimConfig(lr=5e-4 * (i + 1), weight_decay=1e-4 * i, max_epoch=3, warmup_epoch=1),
          "nesterov": lambda i: OptimConfig(lr=2e-3, momentum=0.8, sgd_nesterov=True, max_epoch=3),
          "adam": lambda i: OptimConfig(name="adam", lr=1e-3, adam_beta2=0.99, max_epoch=3, lr_scheduler="single_step", stepsize=(1,)),
          "amsgrad": lambda i: OptimConfig(name="amsgrad", lr=3e-4, max_epoch=3),
          "rmsprop": lambda i: OptimConfig(name="rmsprop", lr=1e-4, momentum=0.5, max_epoch=3),
          "adamw": lambda i: OptimConfig(name="adamw", lr=1e-3, weight_decay=0.01, max_epoch=3)}
    ocs = [mk[k](i) for i, k in enumerate(kinds)]
    e = 32
    stride = e * e + e
    s0 = torch.zeros(len(ocs), stride)
    opt = member_optimizer(ocs, stride, "cpu", s0)
    bits = lambda t: t.contiguous().view(torch.int32)
    assert opt.graph_key() == 0 and opt.S == len(ocs) and (opt.seg0, opt.seg1, opt.stride) == (stride, 0, stride)
    assert opt.used.tolist() == [[stride, 0]] * len(ocs) and opt.s0.data_ptr() == s0.data_ptr()
    for epoch in range(4):
        opt.set_epoch(epoch)
        if all(optim.is_plain_sgd(oc) for oc in ocs):
            assert isinstance(opt, optim.PlainSGD) and torch.equal(bits(opt.hyper), bits(optim.sgd_hyper_table(ocs, epoch)))
        else:
            assert opt.table_driven and torch.equal(opt.kind, optim.kind_table(ocs))
            assert torch.equal(bits(opt.hyper), bits(optim.hyper_table(ocs, epoch)))
            assert opt.needs_s2 == ("amsgrad" in kinds)


def test_member_checkpoint_is_a_standalone_lp_file_in_both_directions(tmp_path):
    from rpo_amd import optim
    from rpo_amd.lp import LP, LP_MODEL_NAME
    from rpo_amd.trainer import OptimConfig, load_checkpoint_file, lr_at_epoch
    cfg, e = _cfg(), 32
    stride = e * e + e
    optims = [OptimConfig(lr=5e-4, max_epoch=4), OptimConfig(lr=2e-3, weight_decay=1e-4, sgd_nesterov=True, max_epoch=4),
              OptimConfig(name="adam", lr=1e-3, max_epoch=4)]
    tr = _stand_in(cfg, optims, e=e)
    g = torch.Generator().manual_seed(3)
    tr.engine.lps_params.copy_(torch.randn(3, stride, generator=g))
    for row in tr._opt._state():
        if row is not None:
            row.copy_(torch.randn(3, stride, generator=g).abs())
    tr._opt.counter.fill_(5)
    dirs = [str(tmp_path / f"m{s}") for s in range(3)]
    paths = tr.save_model(dirs, is_best=True, val_results=[1.0, 2.0, 3.0])
    assert paths[1] == os.path.join(dirs[1], LP_MODEL_NAME, "model.pth.tar-2")

    def solo_lp(oc):
        solo = LP.__new__(LP)
        solo.model = type("M", (), {})()
        p = torch.zeros(stride)
        solo.engine = type("E", (), {})()
        solo.engine.lp_params, solo.engine.lp_moms = p, torch.zeros(stride)
        solo.model.named_parameters = lambda: iter([("weight", p[:e * e].view(e, e)), ("bias", p[e * e:])])
        solo.model.state_dict = lambda: {n: t.clone() for n, t in solo.model.named_parameters()}
        solo.optim_cfg, solo._graph, solo.epoch, solo._steps, solo.lr = oc, None, 0, 0, lr_at_epoch(oc, 0)
        solo._opt = optim.make_optimizer([oc], stride, stride, 0, "cpu", s0=solo.engine.lp_moms)
        return solo

    for s, oc in enumerate(optims):
        ck = load_checkpoint_file(paths[s])
        solo = solo_lp(oc)
        assert solo.resume_model(dirs[s]) == 2                                   # model-best, through LP's own reader
        assert torch.equal(solo.engine.lp_params, tr.engine.lps_params[s]), s
        for a, b in zip(solo._opt._state(), tr._opt._state()[:len(optim.state_names(oc))]):
            assert torch.equal(a.view(-1), b[s]), s
        assert solo._steps == 5 and solo.lr == lr_at_epoch(oc, 2) and ck["val_result"] == float(s + 1)
        # the same keys, layout and values as the dict LP.checkpoint_dict builds in that state
        want, got = solo.checkpoint_dict(val_result=float(s + 1)), tr.checkpoint_dict(s, val_result=float(s + 1))
        assert list(got) == list(want) == list(ck) and got["optimizer"]["param_groups"] == want["optimizer"]["param_groups"]
        assert got["epoch"] == want["epoch"] == 2 and got["steps"] == want["steps"] == 5 and got["scheduler"] == want["scheduler"]
        for i in (0, 1):
            assert list(got["optimizer"]["state"][i]) == list(want["optimizer"]["state"][i])
            for k, v in got["optimizer"]["state"][i].items():
                assert torch.equal(torch.as_tensor(v), torch.as_tensor(want["optimizer"]["state"][i][k])), (s, i, k)
        for k in ("weight", "bias"):
            assert torch.equal(got["state_dict"][k], want["state_dict"][k])
    # ---- standalone files -> members
    solo_dirs, rows = [], []
    for s, oc in enumerate(optims):
        solo = solo_lp(oc)
        solo.engine.lp_params.copy_(torch.randn(stride, generator=g))
        for row in solo._opt._state():
            if row is not None:
                row.copy_(torch.randn(1, stride, generator=g).abs().view(row.shape))
        if solo._opt.table_driven:
            solo._opt.counter.fill_(7)
        solo.epoch, solo._steps, solo.lr = 3, 7, lr_at_epoch(oc, 3)
        solo.save_model(str(tmp_path / f"solo{s}"))
        solo_dirs.append(str(tmp_path / f"solo{s}"))
        rows.append((solo.engine.lp_params.clone(), [r.clone().view(-1) for r in solo._opt._state()[:len(optim.state_names(oc))]]))
    tr.load_model(solo_dirs, epoch=3)
    for s, oc in enumerate(optims):
        assert torch.equal(tr.engine.lps_params[s], rows[s][0])
        for a, b in zip(rows[s][1], tr._opt._state()):
            assert torch.equal(a, b[s]), s
    assert tr.epoch == 3 and tr._steps == 7 and tr.lr == [lr_at_epoch(oc, 3) for oc in optims]
    assert tr._opt.epoch == 3 and tr._opt.steps() == [7, 7, 7]
    # files of different epochs are refused, and nothing is half-applied
    from rpo_amd.trainer import write_checkpoint
    ck = load_checkpoint_file(os.path.join(solo_dirs[1], LP_MODEL_NAME, "model.pth.tar-3"))
    write_checkpoint(solo_dirs[1], dict(ck, epoch=4), 3, False, name=LP_MODEL_NAME)
    before = tr.engine.lps_params.clone()
    with pytest.raises(ValueError, match=r"epochs \[3, 4, 3\]; one loop runs all members"):
        tr.load_model(solo_dirs, epoch=3)
    assert torch.equal(tr.engine.lps_params, before) and tr.epoch == 3
