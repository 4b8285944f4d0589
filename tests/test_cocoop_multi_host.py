"""Host-side checks of CoCoOpMulti (rpo_amd/coop_multi.py) and its four C ABI additions
(rpo_amd/csrc/cocoop_sets.hip): declared, exported and bound; bad arguments get the calls' own error codes with nothing
launched; what the trainer does not do is refused by name before a device is touched; the defaults of the signatures it
builds on are what they were; the members' row layout is a standalone run's flat buffer.  No GPU needed."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rpo_metanet_fwd_sets": 13, "rpo_cocoop_shift_sets": 9, "rpo_cocoop_grad_tail_sets": 11, "rpo_metanet_bwd_sets": 13}


def _cfg(depth=1):
    from rpo_amd.config import vit_b16
    return vit_b16(layers_v=depth, layers_t=depth, K=1)


def test_the_four_entry_points_are_declared_exported_and_bound():
    import rpo_amd
    from rpo_amd import _lib, ops
    from rpo_amd.build import SOURCES, build_library
    build_library()
    assert "cocoop_sets.hip" in SOURCES
    hdr = open(os.path.join(ROOT, "include", "rpo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in NAMES.items():
        assert re.search(rf"\bint {name}\s*\(", src), f"{name} is not declared in include/rpo_amd.h"
        assert hasattr(lib, name), f"librpo_hip.so does not export {name}"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int32 or restype is ctypes.c_int
        decl = src[src.index(f"int {name}("):]
        decl = decl[:decl.index(";")]
        assert len(argtypes) == decl.count(",") + 1 == n_args, f"{name}: the ctypes signature has the header's parameter count"
        assert "int64_t set_stride" in decl and argtypes[[a.strip().split()[-1] for a in decl.split(",")].index("set_stride")] \
            is ctypes.c_int64
        assert hasattr(ops, name[len("rpo_"):])
    # additions to ABI 8, documented as such; the version does not move
    assert _lib.load().rpo_version() == 8 and "#define RPO_ABI_VERSION 8" in hdr
    comment = hdr[:hdr.index("int rpo_metanet_fwd_sets(")].rsplit("/*", 1)[1]
    assert comment.lstrip().startswith("(ABI 8 additions)")
    # the tail's signature is the issue's: no width of the meta-net enters it
    decl = src[src.index("int rpo_cocoop_grad_tail_sets("):]
    assert [a.strip().split()[-1].lstrip("*") for a in decl[decl.index("(") + 1:decl.index(")")].split(",")] == \
        ["d_shift", "loss_img", "grads", "set_stride", "d_bias", "loss", "S", "b", "n_ctx", "d", "stream"]
    from rpo_amd.coop_multi import CoCoOpMulti
    assert rpo_amd.CoCoOpMulti is CoCoOpMulti and "CoCoOpMulti" in rpo_amd.__all__
    from rpo_amd.engine import Engine
    from rpo_amd.engine_cocoop_multi import CocoopMultiEngineMixin
    assert issubclass(Engine, CocoopMultiEngineMixin)


def test_the_four_entry_points_refuse_bad_arguments_without_launching():
    """Every call here is refused, and a refusal returns before the launch: the pointers are host memory that no kernel
    could read.  A call that passes every check is never made."""
    from rpo_amd import _lib
    from rpo_amd.engine_cocoop_multi import cocoop_row_layout
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                  # 16-byte aligned host memory: never dereferenced
    BAD, SHAPE, ALIGN = _lib.E_BADARG, _lib.E_SHAPE, _lib.E_ALIGN
    e, h, d, nc = 64, 4, 32, 4
    row = cocoop_row_layout(nc, e, h, d)[0]
    assert row % 4 == 0
    fwd = lambda S=3, b=2, e=e, h=h, d=d, nc=nc, stride=row, img=p, params=p, fn=p, hid=p, bias=p: \
        lib.rpo_metanet_fwd_sets(img, params, stride, nc, fn, hid, bias, S, b, e, h, d, None)
    bwd = lambda S=3, b=2, e=e, h=h, d=d, nc=nc, stride=row, dbias=p, fn=p, hid=p, params=p, grads=p: \
        lib.rpo_metanet_bwd_sets(dbias, fn, hid, params, grads, stride, nc, S, b, e, h, d, None)
    shift = lambda S=3, b=2, d=d, nc=nc, stride=row, params=p, bias=p, out=p: \
        lib.rpo_cocoop_shift_sets(params, stride, bias, out, S, b, nc, d, None)
    tail = lambda S=3, b=2, d=d, nc=nc, stride=row, dshift=p, loss_img=p, grads=p, dbias=p, loss=p: \
        lib.rpo_cocoop_grad_tail_sets(dshift, loss_img, grads, stride, dbias, loss, S, b, nc, d, None)
    ptrs = {fwd: ("img", "params", "fn", "hid", "bias"), bwd: ("dbias", "fn", "hid", "params", "grads"),
            shift: ("params", "bias", "out"), tail: ("dshift", "loss_img", "grads", "dbias", "loss")}
    for call, names in ptrs.items():
        for k in names:
            assert call(**{k: None}) == BAD, k
        for kw in (dict(nc=0), dict(d=0), dict(d=-1)):
            assert call(**kw) == BAD, kw
        for kw in (dict(S=0), dict(S=-1), dict(S=1025), dict(b=0), dict(b=-3)):
            assert call(**kw) == SHAPE, kw
        for kw in (dict(stride=row + 2), dict(stride=row + 1)):
            assert call(**kw) == ALIGN, kw
    for call in (fwd, bwd):
        assert call(e=0) == BAD and call(h=0) == BAD
        assert call(stride=row - 4) == SHAPE, "set_stride below the row length"
        assert call(params=p + 4) == ALIGN
    assert bwd(grads=p + 8) == ALIGN and tail(grads=p + 4) == ALIGN and shift(params=p + 4) == ALIGN
    for call in (shift, tail):                                    # the context-only calls touch the ctx part of a row
        assert call(stride=nc * d - 4) == SHAPE
    # the LDS limits of rpo_metanet_fwd / rpo_metanet_bwd with B = b: (e + h) * 4 and b * h * 4 bytes in 48 KB
    big_e = 12288 - h + 4
    assert fwd(e=big_e, stride=cocoop_row_layout(nc, big_e, h, d)[0]) == SHAPE
    big_b = 12288 // h + 1
    assert bwd(b=big_b, S=1) == SHAPE and fwd(b=big_b, S=1, params=None) == BAD


def _members():
    from rpo_amd.trainer import OptimConfig
    return [dict(seed=1), dict(seed=2, optim=OptimConfig(name="adam", lr=1e-3, max_epoch=10))]


def test_what_the_trainer_does_not_do_is_refused_by_name_before_any_device_work(monkeypatch):
    from rpo_amd import coop_multi, engine
    from rpo_amd.config import rn_clip
    from rpo_amd.trainer import OptimConfig
    touched = []
    monkeypatch.setattr(engine, "make_engine", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(torch.cuda, "device", lambda *a, **k: touched.append(2))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cfg, toks = _cfg(), np.zeros((19, 77), np.int64)
    M = coop_multi.CoCoOpMulti
    with pytest.raises(NotImplementedError, match="CoCoOpMulti: world_size > 1"):
        M({}, toks, _members(), cfg=cfg, world_size=2)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="CoCoOpMulti: world_size > 1"):
        M({}, toks, _members(), cfg=cfg)
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(NotImplementedError, match="CoCoOpMulti on a ResNet"):
        M({}, toks, _members(), cfg=rn_clip((1, 1, 1, 1), 64, 1024))
    with pytest.raises(ValueError, match="CoCoOpMulti: no members"):
        M({}, toks, [], cfg=cfg)
    with pytest.raises(ValueError, match="radam"):
        M({}, toks, [dict(seed=1), dict(seed=2, optim=OptimConfig(name="radam", max_epoch=10))], cfg=cfg)
    with pytest.raises(ValueError, match=r"S \* b = 129 \* 2 = 258 images per step.*256 replicas"):
        M({}, toks, [dict(seed=s) for s in range(129)], batch_size=2, cfg=cfg)
    with pytest.raises(ValueError, match=r"S \* b = 257 \* 1 = 257"):
        M({}, toks, [dict(seed=s) for s in range(257)], cfg=cfg)
    ctx, meta = np.zeros((4, 512), np.float32), {}
    with pytest.raises(ValueError, match="member 1 must have exactly one of seed=.*it has both"):
        M({}, toks, [dict(seed=1), dict(seed=2, ctx=ctx, meta=meta)], cfg=cfg)
    with pytest.raises(ValueError, match="member 0 must have exactly one of seed=.*it has neither"):
        M({}, toks, [dict(optim=OptimConfig(max_epoch=10)), dict(seed=2)], cfg=cfg)
    with pytest.raises(ValueError, match="member 1 gives its tensors: both ctx"):
        M({}, toks, [dict(seed=1), dict(ctx=ctx)], cfg=cfg)
    with pytest.raises(ValueError, match=r"the members differ in max_epoch \(\[10, 30\]\)"):
        M({}, toks, [dict(seed=1), dict(seed=2, optim=OptimConfig(max_epoch=30))], cfg=cfg)
    assert not touched, "a refused constructor reached the engine or the device"


def test_existing_signatures_keep_their_defaults():
    """CoCoOpMulti is built on these; none of them gained, lost or changed a parameter."""
    from rpo_amd import coop, multi, optim
    from rpo_amd.engine_coop import CoopEngineMixin
    from rpo_amd.engine_cocoop_eval import ConditionalEvalEngineMixin
    sig = lambda fn: str(inspect.signature(fn))
    assert sig(CoopEngineMixin.coop_setup) == ("(self, n_ctx: 'int', replicas: 'int' = 1, meta_hidden: 'int' = 0, csc: 'bool' = "
                                               "False, class_token_position: 'str' = 'end', shared_prefix: 'bool' = False) -> "
                                               "'None'")
    assert sig(CoopEngineMixin.cocoop_forward_backward) == \
        "(self, image: 'torch.Tensor', label: 'Optional[torch.Tensor]') -> 'torch.Tensor'"
    assert sig(CoopEngineMixin._coop_text_forward) == "(self, train: 'bool', R: 'int' = 1) -> 'None'"
    assert sig(CoopEngineMixin._coop_text_backward) == "(self, R: 'int' = 1) -> 'None'"
    assert sig(ConditionalEvalEngineMixin.conditional_class_set) == \
        ("(self, tokens, images_per_pass: 'Optional[int]' = None, row_budget: 'Optional[int]' = None) -> "
         "'ConditionalClassSet'")
    par = inspect.signature(coop.CoCoOp.__init__).parameters
    assert [(k, v.default) for k, v in par.items() if k in ("n_ctx", "batch_size", "num_batches", "use_graph", "amp",
                                                            "shared_prefix", "act_dtype")] == \
        [("n_ctx", 4), ("act_dtype", torch.float16), ("batch_size", 1), ("num_batches", 1), ("use_graph", False), ("amp", False),
         ("shared_prefix", False)]
    par = inspect.signature(coop.CoCoOpCustomCLIP.__init__).parameters
    assert par["max_batch"].default == 1 and par["shared_prefix"].default is False and par["meta"].default is None
    assert sig(optim.make_optimizer) == ("(optims: 'Sequence', set_stride: 'int', seg0: 'int', seg1: 'int', device, s0: "
                                         "'Optional[torch.Tensor]' = None, used: 'Optional[torch.Tensor]' = None, "
                                         "grad_scale: 'float' = 1.0)")
    # (the members' epoch loop moved into a mixin both multi-run trainers share; RPOMulti's refusals keep their wording)
    assert sig(multi.member_batches) == ("(set_sizes: 'Sequence[int]', batch_size: 'int', generators: "
                                         "'Sequence[Optional[torch.Generator]]', who: 'str' = 'RPOMulti') -> 'List[list]'")
    assert multi.RPOMulti.run_epoch is multi.MemberLoopMixin.run_epoch and multi.RPOMulti._loop_name == "RPOMulti"
    with pytest.raises(ValueError, match=r"^RPOMulti\.run_epoch: the members' sets have \[8, 4\] images"):
        multi.member_batches([8, 4], 4, [None, None])
    # the new trainer's own defaults: the reference's recipe (n_ctx 4, batch 1), nothing opted into
    par = inspect.signature(coop.CoCoOp.__init__).parameters
    new = inspect.signature(__import__("rpo_amd.coop_multi", fromlist=["x"]).CoCoOpMulti.__init__).parameters
    for k in ("n_ctx", "batch_size", "num_batches", "use_graph", "amp", "shared_prefix", "act_dtype", "cfg"):
        assert new[k].default == par[k].default, k


@pytest.mark.parametrize("e,h,d,n_ctx,floats", [(512, 32, 512, 4, 35360), (768, 48, 768, 4, 77616)],
                         ids=["ViT-B/16", "ViT-L/14-text-widths"])
def test_row_layout_is_a_standalone_runs_flat_buffer(e, h, d, n_ctx, floats):
    from rpo_amd.engine_cocoop_multi import cocoop_row_layout
    length, offs, stride = cocoop_row_layout(n_ctx, e, h, d)
    assert length == floats == n_ctx * d + h * e + h + d * h + d
    assert offs == {"ctx": 0, "w1": n_ctx * d, "b1": n_ctx * d + h * e, "w2": n_ctx * d + h * e + h,
                    "b2": n_ctx * d + h * e + h + d * h}
    assert stride == floats and stride % 4 == 0                  # both rows end on the 16-byte grid: no padding
    # ... and coop_setup's `sizes` order, which is what `select_member` copies a row into
    sizes = [n_ctx * d] + [h * e, h, d * h, d]
    assert list(offs.values()) == list(np.cumsum([0] + sizes)[:-1])


def test_row_stride_is_padded_to_the_16_byte_grid():
    from rpo_amd.engine_cocoop_multi import cocoop_row_layout
    length, offs, stride = cocoop_row_layout(3, 50, 3, 7)          # 21 + 150 + 3 + 21 + 7 = 202
    assert length == 202 and stride == 204 and offs["b2"] == 195


def test_member_start_and_check_members():
    """A seeded member draws what CoCoOpCustomCLIP draws under torch.manual_seed(seed), in its order; given tensors are
    laid out in the row order; ctx_init replaces the context draw and leaves the meta-net's."""
    from rpo_amd.coop_multi import check_members, member_start
    cfg = _cfg()
    e, dt, h = cfg.embed, cfg.d_t, cfg.embed // 16
    row = member_start(dict(seed=5), cfg, 19, 4, None)
    torch.manual_seed(5)
    ctx = torch.empty(4, dt).normal_(std=0.02)
    l1, l2 = torch.nn.Linear(e, h), torch.nn.Linear(h, dt)
    want = torch.cat([t.detach().reshape(-1) for t in (ctx, l1.weight, l1.bias, l2.weight, l2.bias)]).numpy()
    assert row.dtype == np.float32 and np.array_equal(row, want)
    emb = np.random.default_rng(0).standard_normal((40, dt)).astype(np.float32)
    ids = np.array([3, 7, 7, 1])
    row2 = member_start(dict(seed=5, ctx_init=ids), cfg, 19, 4, emb)
    torch.manual_seed(5)
    l1, l2 = torch.nn.Linear(e, h), torch.nn.Linear(h, dt)
    assert np.array_equal(row2[:4 * dt], emb[ids].reshape(-1)) and np.array_equal(row2[4 * dt:4 * dt + h * e],
                                                                                   l1.weight.detach().numpy().reshape(-1))
    meta = dict(w1=np.ones((h, e)), b1=np.zeros(h), w2=np.full((dt, h), 2.0), b2=np.full(dt, 3.0))
    row3 = member_start(dict(ctx=np.full((4, dt), 5.0), meta=meta), cfg, 19, 4, None)
    assert row3[0] == 5 and row3[4 * dt] == 1 and row3[4 * dt + h * e] == 0 and row3[4 * dt + h * e + h] == 2 and row3[-1] == 3
    with pytest.raises(ValueError, match=r"ctx has shape \(3, 512\)"):
        member_start(dict(ctx=np.zeros((3, dt)), meta=meta), cfg, 19, 4, None)
    with pytest.raises(ValueError, match="unknown keys"):
        check_members([dict(seed=1, lr=0.1)])
    with pytest.raises(ValueError, match="ctx_init initialises a seeded member"):
        check_members([dict(ctx=np.zeros((4, dt)), meta=meta, ctx_init=ids)])
