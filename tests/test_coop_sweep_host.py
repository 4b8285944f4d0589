"""Host-side checks of CoOpSweep (rpo_amd/coop_sweep.py) and its two C ABI additions
(rpo_amd/csrc/coop_sets.hip): declared, exported and bound; bad arguments get the calls' own error codes with nothing
launched; what the trainer does not do is refused by name before an engine is made; the members' tokens, lengths, EOT rows,
row stride and `used` table are arithmetic on the host.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rpo_coop_fill_sets": 12, "rpo_coop_ctx_grad_sets": 10}


def _cfg(depth=1):
    from rpo_amd.config import vit_b16
    return vit_b16(layers_v=depth, layers_t=depth, K=1)


def test_the_two_entry_points_are_declared_exported_and_bound():
    import rpo_amd
    from rpo_amd import _lib, ops
    from rpo_amd.build import SOURCES, build_library
    build_library()
    assert "coop_sets.hip" in SOURCES
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
        names = [a.strip().split()[-1].lstrip("*") for a in decl[decl.index("(") + 1:decl.index(")")].split(",")]
        assert "int64_t set_stride" in decl and argtypes[names.index("set_stride")] is ctypes.c_int64
        assert names[-6:] == ["S", "n_cls", "L", "n_max", "d", "stream"] and "n_ctx_members" in names
        assert hasattr(ops, name[len("rpo_"):])
    # additions to ABI 8, documented as such; the version does not move
    assert _lib.load().rpo_version() == 8 and "#define RPO_ABI_VERSION 8" in hdr
    comment = hdr[:hdr.index("int rpo_coop_fill_sets(")].rsplit("/*", 1)[1]
    assert comment.lstrip().startswith("(ABI 8 additions)")
    from rpo_amd.coop_sweep import CoOpSweep
    assert rpo_amd.CoOpSweep is CoOpSweep and "CoOpSweep" in rpo_amd.__all__
    from rpo_amd.engine import Engine
    from rpo_amd.engine_coop_sweep import CoopSweepEngineMixin
    assert issubclass(Engine, CoopSweepEngineMixin)


def test_the_two_entry_points_refuse_bad_arguments_without_launching():
    """Every call here is refused, and a refusal returns before the launch: the pointers are host memory that no kernel
    could read.  A call that passes every check is never made."""
    from rpo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                  # 16-byte aligned host memory: never dereferenced
    BAD, SHAPE, ALIGN = _lib.E_BADARG, _lib.E_SHAPE, _lib.E_ALIGN
    d, n_max, n_cls, L = 32, 4, 7, 12
    row = n_max * d
    fill = lambda S=3, n_cls=n_cls, L=L, n_max=n_max, d=d, stride=row, tok=p, pos=p, params=p, nc=p, x0=p: \
        lib.rpo_coop_fill_sets(tok, pos, params, stride, nc, x0, S, n_cls, L, n_max, d, None)
    grad = lambda S=3, n_cls=n_cls, L=L, n_max=n_max, d=d, stride=row, dx=p, grads=p, nc=p: \
        lib.rpo_coop_ctx_grad_sets(dx, grads, stride, nc, S, n_cls, L, n_max, d, None)
    ptrs = {fill: ("tok", "pos", "params", "nc", "x0"), grad: ("dx", "grads", "nc")}
    for call, names in ptrs.items():
        for k in names:
            assert call(**{k: None}) == BAD, k
        for kw in (dict(n_cls=0), dict(L=0), dict(d=0), dict(d=-4)):
            assert call(**kw) == BAD, kw
        for kw in (dict(S=0), dict(S=-1), dict(S=1025), dict(n_max=0), dict(n_max=-2), dict(n_max=L, stride=L * d),
                   dict(stride=row - 4), dict(stride=0), dict(S=1024, n_cls=70000, L=77)):
            assert call(**kw) == SHAPE, kw
        for kw in (dict(stride=row + 2), dict(stride=row + 1)):
            assert call(**kw) == ALIGN, kw
    assert fill(d=30, stride=4 * 30) == SHAPE, "the fill moves float4s"
    for k in ("tok", "pos", "params", "x0"):
        assert fill(**{k: p + 4}) == ALIGN, k
    assert grad(grads=p + 8) == ALIGN


def _tokens(lengths, n_ctx, seed=5):
    from rpo_amd import synth
    base = synth.synthetic_tokens(_cfg(), lengths, seed=seed)
    return base, synth.coop_tokens(base, n_ctx)


@pytest.mark.parametrize("n_max", [4, 16])
def test_member_tokens_are_coop_tokens_of_the_shorter_context(n_max):
    from rpo_amd import synth
    from rpo_amd.coop_sweep import member_tokens
    from rpo_amd.engine_coop_sweep import member_eot_rows, member_lengths
    lengths = [4, 25, 3, 11, 18, 7, 29]                           # SOS .. EOT of the bare names: ragged
    base, toks = _tokens(lengths, n_max)
    ln = synth.len_prompts(toks)
    assert list(ln) == [v + n_max for v in lengths]
    L = int(ln.max())
    members = [1, 2, n_max]
    for n_s in members:
        got = member_tokens(toks, n_max, n_s)
        assert got.dtype == np.int64 and np.array_equal(got, synth.coop_tokens(base, n_s)), n_s
        assert np.array_equal(synth.len_prompts(got), ln - (n_max - n_s))
    assert member_tokens(toks, n_max, n_max) is not toks
    for bad in (0, n_max + 1, -1):
        with pytest.raises(ValueError, match=f"must be in 1 .. {n_max}"):
            member_tokens(toks, n_max, bad)
    ml = member_lengths(ln, n_max, members)
    assert ml.shape == (3, 7) and np.array_equal(ml, np.stack([synth.len_prompts(member_tokens(toks, n_max, n)) for n in members]))
    eot = member_eot_rows(ln, n_max, members, L)
    assert eot.dtype == np.int64 and eot.shape == (21,)
    for s, n_s in enumerate(members):
        mt = member_tokens(toks, n_max, n_s)
        for c in range(7):
            row = int(eot[s * 7 + c])
            assert row // L == s * 7 + c and mt[c, row % L] == synth.EOT_TOKEN == mt[c].max()


@pytest.mark.parametrize("d,n_max,members,stride", [(512, 4, (4, 1, 2), 2048), (768, 16, (16, 4), 12288), (6, 3, (3, 1), 20)])
def test_row_stride_and_used_table(d, n_max, members, stride):
    from rpo_amd.engine_coop_sweep import sweep_row_layout, sweep_used
    length, st = sweep_row_layout(n_max, d)
    assert length == n_max * d and st == stride and st % 4 == 0 and 0 <= st - length < 4
    used = sweep_used(members, d)
    assert used.dtype == np.int32 and used.tolist() == [[n * d, 0] for n in members]
    assert int(used[:, 0].max()) <= length


def _members():
    from rpo_amd.trainer import OptimConfig
    return [dict(seed=1), dict(seed=2, n_ctx=2, optim=OptimConfig(name="adam", lr=1e-3, max_epoch=50))]


def test_what_the_trainer_does_not_do_is_refused_by_name_before_an_engine_is_made(monkeypatch):
    from rpo_amd import coop_sweep, engine
    from rpo_amd.trainer import OptimConfig
    touched = []
    monkeypatch.setattr(engine, "make_engine", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(torch.cuda, "device", lambda *a, **k: touched.append(2))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cfg, toks = _cfg(), np.zeros((19, 77), np.int64)
    M = coop_sweep.CoOpSweep
    kw = dict(n_ctx=4, cfg=cfg)
    with pytest.raises(NotImplementedError, match="CoOpSweep: world_size > 1"):
        M({}, toks, _members(), world_size=2, **kw)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="CoOpSweep: world_size > 1"):
        M({}, toks, _members(), **kw)
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="generic context at the front of the name only"):
        M({}, toks, _members(), csc=True, **kw)
    with pytest.raises(ValueError, match="member 1 asks for csc=True.*generic context at the front of the name only"):
        M({}, toks, [dict(seed=1), dict(seed=2, csc=True)], **kw)
    for pos in ("middle", "front"):
        with pytest.raises(ValueError, match=f"class_token_position='{pos}'.*generic context at the front of the name only"):
            M({}, toks, _members(), class_token_position=pos, **kw)
        with pytest.raises(ValueError, match="member 0 asks for.*generic context at the front of the name only"):
            M({}, toks, [dict(seed=1, class_token_position=pos)], **kw)
    with pytest.raises(ValueError, match=r"shared_prefix=True with members of different n_ctx \[4, 2\]: the prefix length P"):
        M({}, toks, _members(), shared_prefix=True, **kw)
    with pytest.raises(NotImplementedError, match="load the member's checkpoint into a CoOp"):
        M({}, toks, _members(), classes=object(), **kw)
    with pytest.raises(NotImplementedError, match="load the member's checkpoint into a CoOp"):
        M({}, toks, _members(), class_set=object(), **kw)
    with pytest.raises(ValueError, match="CoOpSweep: no members"):
        M({}, toks, [], **kw)
    with pytest.raises(ValueError, match="CoOpSweep: 257 members.*at most 256 replicas"):
        M({}, toks, [dict(seed=s) for s in range(257)], **kw)
    ctx = np.zeros((4, 512), np.float32)
    with pytest.raises(ValueError, match="member 1 must have exactly one of seed=.*it has both"):
        M({}, toks, [dict(seed=1), dict(seed=2, ctx=ctx)], **kw)
    with pytest.raises(ValueError, match="member 0 must have exactly one of seed=.*it has neither"):
        M({}, toks, [dict(optim=OptimConfig(max_epoch=50)), dict(seed=2)], **kw)
    with pytest.raises(ValueError, match="ctx_init initialises a seeded member"):
        M({}, toks, [dict(ctx=ctx, ctx_init=np.array([1, 2, 3, 4]))], **kw)
    for bad in (0, 5):
        with pytest.raises(ValueError, match=rf"member 1 has n_ctx = {bad}; a member's n_ctx must be in 1 \.\. 4"):
            M({}, toks, [dict(seed=1), dict(seed=2, n_ctx=bad)], **kw)
    with pytest.raises(ValueError, match="unknown keys"):
        M({}, toks, [dict(seed=1, lr=0.1)], **kw)
    with pytest.raises(ValueError, match="radam"):
        M({}, toks, [dict(seed=1), dict(seed=2, optim=OptimConfig(name="radam", max_epoch=50))], **kw)
    with pytest.raises(ValueError, match=r"the members differ in max_epoch \(\[50, 30\]\)"):
        M({}, toks, [dict(seed=1), dict(seed=2, optim=OptimConfig(max_epoch=30))], **kw)
    assert not touched, "a refused constructor reached the engine or the device"
    # the trainer's own methods refuse other class sets by name, too (no engine needed to say so)
    tr = object.__new__(M)
    for call in (lambda: tr.class_set(toks), lambda: tr.model_inference(None, 0, classes=object()),
                 lambda: tr.test(None, 0, classes=object()), lambda: tr.test_all(None, classes=object())):
        with pytest.raises(NotImplementedError, match="load the member's checkpoint into a CoOp"):
            call()
    assert M._reports_acc is False


def test_a_seeded_member_draws_what_the_standalone_trainer_draws():
    from rpo_amd.coop import _init_ctx
    from rpo_amd.coop_sweep import check_members, member_start
    cfg = _cfg()
    ms = check_members([dict(seed=5), dict(seed=5, n_ctx=2), dict(seed=9, n_ctx=3, ctx_init=np.array([3, 7, 1]))], 4)
    assert [m["n_ctx"] for m in ms] == [4, 2, 3]
    emb = np.random.default_rng(0).standard_normal((40, cfg.d_t)).astype(np.float32)
    for m, n_s in zip(ms[:2], (4, 2)):
        got = member_start(m, cfg, 19, emb)
        torch.manual_seed(5)
        want = _init_ctx(cfg, 19, n_s, False, None, None, emb)
        assert got.shape == (n_s, cfg.d_t) and got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(member_start(ms[2], cfg, 19, emb), emb[[3, 7, 1]])
    with pytest.raises(ValueError, match=r"ctx has shape \(3, 512\), its n_ctx = 2"):
        member_start(check_members([dict(ctx=np.zeros((3, 512)), n_ctx=2)], 4)[0], cfg, 19, emb)
