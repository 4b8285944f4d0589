"""CoOpSweep on the GPU (rpo_amd/coop_sweep.py, rpo_amd/engine_coop_sweep.py, rpo_amd/csrc/coop_sets.hip; DESIGN.md section
9s): the two member kernels against the host's float32 composition and rpo_reduce_groups (bits), then the step of S members
with their own n_ctx against the CPU oracle run on each member alone, a standalone CoOp (bits), itself with one member
replaced, graph replay, torch.optim, and the standalone trainer's checkpoints and evaluation; the same on a ResNet.  Every
test here fails without the feature: there are no `ops.coop_*_sets`, no `coop_sweep_setup` and no `rpo_amd.coop_sweep`."""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import BF16_GRAD_REL, BF16_LOGIT_ATOL, F16_GRAD_REL, F16_LOGIT_ATOL, GOLDEN, TOL_F32
from rpo_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MODES = ["f32", "bf16", "f16"]
N_MAX = 4
MIXED = (4, 1, 2)                   # the members' n_ctx
B = 3
NAN = float("nan")


def bits(t):
    return torch.as_tensor(t).detach().contiguous().view(torch.int32).cpu()


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _relmax(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _rows(S, stride, seed, members=None, d=0):
    """[S + 1, stride] on the device, NaN everywhere (padding, unused tails and the guard row S stay NaN); with `members`,
    member s's first n_s * d floats are N(0, 0.05)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.full((S + 1, stride), NAN)
    for s, n_s in enumerate(members or ()):
        t[s, :n_s * d] = 0.05 * torch.randn(n_s * d, generator=g)
    return t.to(DEV)


# ============================================================================================ 1. the kernels

@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("d", [512, 768])
@pytest.mark.parametrize("members", [(4,), MIXED], ids=["S1", "S3"])
def test_fill_kernel_is_the_hosts_float32_composition(members, d, pad):
    """rpo_coop_fill_sets against numpy float32: one add per element, so array_equal.  The unused tail of a shorter member's
    row, the padding and a guard row are NaN and must not be read; a guard row behind x0 keeps its bits."""
    from rpo_amd import ops
    S, n_cls, L = len(members), 5, 11
    stride = N_MAX * d + pad
    g = torch.Generator().manual_seed(3 * S + d + pad)
    tok, pos = torch.randn(n_cls * L, d, generator=g), torch.randn(L, d, generator=g)
    params_all = _rows(S, stride, seed=17 + S, members=members, d=d)
    before = params_all.clone()
    x0_all = torch.full((S * n_cls * L + 1, d), NAN, device=DEV)
    nc = torch.tensor(members, dtype=torch.int32, device=DEV)
    ops.coop_fill_sets(tok.to(DEV), pos.to(DEV), params_all[:S], nc, x0_all[:-1], n_cls, L, N_MAX)
    torch.cuda.synchronize()
    got = x0_all.cpu().numpy()
    assert np.isnan(got[-1]).all(), "the guard row behind x0 was written"
    assert same(params_all, before)
    tk, ps, pr = tok.numpy().reshape(n_cls, L, d), pos.numpy(), before.cpu().numpy()
    want = np.empty((S, n_cls, L, d), np.float32)
    for s, n_s in enumerate(members):
        delta = N_MAX - n_s
        for p in range(L):
            if p == 0:
                want[s, :, p] = tk[:, 0] + ps[0]
            elif p <= n_s:
                want[s, :, p] = pr[s, (p - 1) * d:p * d] + ps[p]
            elif p + delta < L:
                want[s, :, p] = tk[:, p + delta] + ps[p]
            else:
                want[s, :, p] = ps[p]
    assert np.isfinite(want).all()
    assert np.array_equal(got[:-1].view(np.uint32), want.reshape(-1, d).view(np.uint32))


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("n_cls", [7, 65])
@pytest.mark.parametrize("members", [(4,), MIXED], ids=["S1", "S3"])
def test_gradient_kernel_has_the_bits_of_reduce_groups(members, n_cls, pad):
    """rpo_coop_ctx_grad_sets against rpo_reduce_groups(groups = n_cls, rows = n_s) on the member's gathered rows, in both
    of its regimes (n_cls 7: one thread per element; 65: eight partial sums): array_equal.  The unused tail is exact zeros;
    padding and a guard row keep their NaN bits; dx is not written."""
    from rpo_amd import ops
    S, L, d = len(members), 9, 512
    stride = N_MAX * d + pad
    g = torch.Generator().manual_seed(5 * S + n_cls + pad)
    dx = (torch.randn(S * n_cls * L, d, generator=g) * 10.0 ** torch.randint(-5, 1, (S * n_cls * L, 1), generator=g).float()).to(DEV)
    dx0 = dx.clone()
    grads_all = _rows(S, stride, seed=0)
    g_before = grads_all.clone()
    nc = torch.tensor(members, dtype=torch.int32, device=DEV)
    ops.coop_ctx_grad_sets(dx, grads_all[:S], nc, n_cls, L, N_MAX)
    torch.cuda.synchronize()
    assert same(dx, dx0)
    for s, n_s in enumerate(members):
        rows = dx.view(S, n_cls, L, d)[s, :, 1:1 + n_s].reshape(n_cls * n_s, d).contiguous()
        want = torch.full((n_s, d), NAN, device=DEV)
        ops.reduce_groups(rows, want, n_cls)
        assert bool(torch.isfinite(want).all()) and same(grads_all[s, :n_s * d].view(n_s, d), want), f"member {s}"
        tail = grads_all[s, n_s * d:N_MAX * d]
        assert same(tail, torch.zeros_like(tail)), f"member {s}: the unused tail is not exact zeros"
    mask = torch.ones(S + 1, stride, dtype=torch.bool)
    mask[:S, :N_MAX * d] = False
    assert torch.equal(bits(grads_all)[mask], bits(g_before)[mask]), "the kernel wrote into the padding or the guard row"
    first = grads_all.clone()
    ops.coop_ctx_grad_sets(dx, grads_all[:S], nc, n_cls, L, N_MAX)
    assert same(grads_all, first), "two calls differ"


# ============================================================================================ 2. the step against the oracle
# The world of tests/test_gpu_cocoop_multi.py: 7 classes of ragged lengths (the longest prompt is the engine's Lmax), depth-1
# towers, n_max = 4.  Members with n_ctx (4, 1, 2) on ONE batch of B = 3 images; the oracle runs each member ALONE on that
# member's own tokens (`member_tokens`) and context.  Measured worst case over the members (logits f16 / bf16, gradients
# f16 / bf16): dense 9.20e-3 / 6.9e-2 and 2.1e-3 / 1.5e-2, shared-prefix 9.98e-3 / 7.3e-2 and 2.5e-3 / 1.4e-2, at bounds of 1.0e-2 /
# 0.12 and 6e-3 / 5e-2 -- the f16 logit bound is at the edge of what 16-bit storage gives on this class set, as
# tests/test_gpu_cocoop_classset.py notes for the standalone code.  No bound is widened.
BASE7 = [4 + (7 * c) % 22 for c in range(7)]
WORLD_SEED = 40


def _sibling_bounds(act, o_logits, Lmax):
    """tests/test_gpu_model.py's `_sibling_bounds`, restated: (loss bound, logit bound, gradient bound) of a storage mode."""
    if act == torch.float32:
        return TOL_F32, TOL_F32, TOL_F32
    la, gr = (F16_LOGIT_ATOL, F16_GRAD_REL) if act == torch.float16 else (BF16_LOGIT_ATOL, BF16_GRAD_REL)
    return la, la * max(1.0, float(np.abs(o_logits).max()) / 8.7) * (2 if Lmax > 64 else 1), gr


@functools.lru_cache(maxsize=None)
def _world():
    from rpo_amd.config import vit_b16
    cfg = vit_b16(layers_v=1, layers_t=1, K=1, n_cls=len(BASE7))
    toks = synth.coop_tokens(synth.synthetic_tokens(cfg, BASE7, seed=17 + WORLD_SEED), N_MAX)
    sd = synth.clip_state_dict(cfg, seed=23 + WORLD_SEED, token_rows=np.unique(toks).tolist() + [49407])
    return cfg, sd, toks


@functools.lru_cache(maxsize=None)
def _batch(step=0):
    cfg, _, _ = _world()
    image = synth.images(cfg, B, seed=31 + WORLD_SEED + 1000 * step)
    label = synth.labels(cfg, B, seed=37 + WORLD_SEED + 1000 * step)
    label[0] = cfg.n_cls - 1
    return image, label


def _bt(step=0):
    image, label = _batch(step)
    return {"img": torch.from_numpy(image), "label": torch.from_numpy(label)}


@functools.lru_cache(maxsize=None)
def _ctx(seed, n_s):
    cfg, _, _ = _world()
    rng = np.random.default_rng(29 + WORLD_SEED + 1000 * seed + n_s)
    return (0.02 * rng.standard_normal((n_s, cfg.d_t))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _oracle(seed, n_s):
    """oracle.rpo_oracle.coop_loss_and_grad on this member ALONE: its tokens, its context, the shared batch."""
    from oracle.rpo_oracle import coop_loss_and_grad
    from rpo_amd.coop_sweep import member_tokens
    cfg, sd, toks = _world()
    image, label = _batch()
    logits, loss, g = coop_loss_and_grad(sd, image, member_tokens(toks, N_MAX, n_s), _ctx(seed, n_s), label, cfg.patch)
    return logits.numpy(), float(loss), g.numpy()


def _sweep(mode, n_ctxs=MIXED, seeds=(0, 1, 2), optims=None, **kw):
    from rpo_amd.coop_sweep import CoOpSweep
    cfg, sd, toks = _world()
    members = [dict(ctx=_ctx(sd_, n), n_ctx=n, **({} if optims is None else dict(optim=optims[i])))
               for i, (sd_, n) in enumerate(zip(seeds, n_ctxs))]
    kw.setdefault("num_batches", 10 ** 9)
    return CoOpSweep(sd, toks, members, n_ctx=N_MAX, batch_size=B, act_dtype=DT[mode], cfg=cfg, device=DEV, **kw)


def _check_against_oracle(mode, n_ctxs, shared):
    act, seeds = DT[mode], (0, 1, 2)
    for s, n in zip(seeds, n_ctxs):                                  # the oracle first, on the CPU
        _oracle(s, n)
    tr = _sweep(mode, n_ctxs, seeds, shared_prefix=shared)
    eng = tr.engine
    with torch.cuda.device(eng.dev):
        image, label = tr.parse_batch_train(_bt())
        logits = eng.coop_sweep_forward_backward(image, label).cpu().numpy()
        loss = eng.cs_loss.cpu().numpy()
    assert eng.coop_shared == shared and logits.shape == (3, B, len(BASE7)) and loss.shape == (3,)
    for i, (s, n) in enumerate(zip(seeds, n_ctxs)):
        o_logits, o_loss, o_g = _oracle(s, n)
        lb_loss, lb_logits, gb = _sibling_bounds(act, o_logits, eng.Lmax)
        le, ll = float(np.abs(logits[i] - o_logits).max()), abs(float(loss[i]) - o_loss)
        rel = _relmax(eng.coop_sweep_member_ctx(i, eng.cs_grads).cpu().numpy(), o_g)
        print(f"\n[coop sweep {mode} shared={shared} member {i} n_ctx={n}] logits err {le:.3e} (bound {lb_logits:.3e}, max "
              f"|logit| {np.abs(o_logits).max():.2f}) loss err {ll:.3e} (bound {lb_loss:.3e}) ctx grad rel {rel:.2e} (bound {gb})")
        assert ll <= lb_loss and le <= lb_logits, f"member {i}"
        assert rel <= gb, (i, rel)
        tail = eng.cs_grads[i, n * eng.cfg.d_t:]
        assert not bool(tail.any()), f"member {i}: gradient behind its n_ctx"
    # the members differ (a set whose members agree would prove nothing)
    assert not np.array_equal(logits[0], logits[1]) and not np.array_equal(logits[1], logits[2])


@pytest.mark.parametrize("mode", MODES)
def test_members_with_their_own_n_ctx_against_the_oracle_on_each_member_alone(mode):
    """S = 3 members with n_ctx (4, 1, 2): every member's loss, logits and context gradient against
    oracle.rpo_oracle.coop_loss_and_grad run on that member alone with its own tokens, at `_sibling_bounds`."""
    _check_against_oracle(mode, MIXED, shared=False)


@pytest.mark.parametrize("mode", MODES)
def test_shared_prefix_members_against_the_oracle(mode):
    """Three members of n_ctx 4 on the shared-prefix rows (`shared_prefix=True`), at the same bounds."""
    _check_against_oracle(mode, (4, 4, 4), shared=True)


def test_full_length_rows_are_the_rows_a_standalone_forward_builds():
    """The n_s = n_max member's input rows equal, bit for bit, the rows `_coop_text_forward` of a standalone CoOp with that
    context leaves in cx[0]."""
    from rpo_amd.coop import CoOp
    cfg, sd, toks = _world()
    tr = _sweep("bf16")
    solo = CoOp(sd, toks, N_MAX, None, DEV, torch.bfloat16, batch_size=B, ctx=_ctx(0, 4), cfg=cfg)
    image = torch.from_numpy(_batch()[0])
    tr.model_inference_all(image)
    solo.model_inference(image)
    rows = cfg.n_cls * tr.engine.Lmax
    assert same(tr.engine.cx[0][:rows], solo.engine.cx[0][:rows])
    assert not same(tr.engine.cx[0][rows:2 * rows], solo.engine.cx[0][:rows])


# ============================================================================================ 3. S = 1

def _oc(name="sgd", **kw):
    from rpo_amd.trainer import OptimConfig
    kw.setdefault("lr", 0.002)
    return OptimConfig(name=name, momentum=0.9, weight_decay=5e-4, warmup_epoch=0, lr_scheduler="constant", max_epoch=10, **kw)


@pytest.mark.parametrize("mode,kind,amp", [("bf16", "sgd", False), ("f32", "adam", False), ("bf16", "sgd", True),
                                           ("f32", "sgd", False)])
def test_one_full_length_member_is_a_standalone_coop_bit_for_bit(mode, kind, amp):
    """S = 1, n_s = n_max: the same shapes through the same kernels -- three optimiser steps leave the parameters, the
    optimiser state, every step's gradient and loss bit-identical to a standalone CoOp given the same ctx / OptimConfig."""
    from rpo_amd.coop import CoOp
    cfg, sd, toks = _world()
    oc = _oc(kind)
    solo = CoOp(sd, toks, N_MAX, oc, DEV, DT[mode], batch_size=B, num_batches=10 ** 9, ctx=_ctx(0, 4), cfg=cfg, amp=amp)
    tr = _sweep(mode, (4,), (0,), optims=[oc], amp=amp)
    n = solo.engine.coop_params.numel()
    assert tr.engine.cs_stride == n and same(tr.engine.cs_params[0], solo.engine.coop_params)
    for step in range(3):
        want, got = solo.forward_backward(_bt(step))["loss"], tr.forward_backward(_bt(step))["loss"][0]
        assert np.float32(want).tobytes() == np.float32(got).tobytes(), (step, want, got)
        assert same(tr.engine.cs_logits[:B], solo.engine.logits[:B]), f"step {step}: logits"
        assert same(tr.engine.cs_grads[0], solo.engine.coop_grads), f"step {step}: gradients"
        assert same(tr.engine.cs_params[0], solo.engine.coop_params), f"step {step}: parameters"
    for a, w in zip(tr._opt._state(), solo._opt._state()):
        assert (a is None) == (w is None) and (a is None or same(a[0], w.view(-1))), "optimiser state"
    assert tr.skipped_steps() == [0] and solo.skipped_steps == 0 and tr.checkpoint_dict(0)["steps"] == 3


def test_a_seeded_member_starts_where_the_seeded_standalone_trainer_starts():
    from rpo_amd.coop import CoOp
    from rpo_amd.coop_sweep import CoOpSweep, member_tokens
    cfg, sd, toks = _world()
    ci = np.unique(toks)[1:3]                                            # two ids that have embedding rows
    tr = CoOpSweep(sd, toks, [dict(seed=3), dict(seed=11, n_ctx=2), dict(seed=5, n_ctx=2, ctx_init=ci)], n_ctx=N_MAX,
                   batch_size=B, act_dtype=torch.bfloat16, cfg=cfg, device=DEV)
    for s, (seed, n_s, init) in enumerate(((3, 4, None), (11, 2, None), (5, 2, ci))):
        torch.manual_seed(seed)
        solo = CoOp(sd, member_tokens(toks, N_MAX, n_s), n_s, None, DEV, torch.bfloat16, batch_size=B, cfg=cfg, ctx_init=init)
        assert same(tr.engine.coop_sweep_member_ctx(s).reshape(-1), solo.engine.coop_params), f"seed {seed}"
        assert not bool(tr.engine.cs_params[s, n_s * cfg.d_t:].any())
        del solo


# ============================================================================================ 4. isolation, amp, graphs

def _one_step(tr, step=0):
    loss = tr.forward_backward(_bt(step))["loss"]
    eng = tr.engine
    return loss, eng.cs_logits[:tr.n_runs * B].view(tr.n_runs, B, -1).clone(), eng.cs_grads.clone(), eng.cs_params.clone()


@pytest.mark.parametrize("mode", MODES)
def test_replacing_a_member_leaves_the_others_bit_identical(mode):
    """S = 3: member 1 replaced by another context AND another n_ctx (1 -> 3) -- every output, gradient and updated
    parameter of members 0 and 2 keeps its bits."""
    la, logits_a, ga, pa = _one_step(_sweep(mode, MIXED, (0, 1, 2), optims=[_oc()] * 3))
    lb, logits_b, gb, pb = _one_step(_sweep(mode, (4, 3, 2), (0, 7, 2), optims=[_oc()] * 3))
    assert not same(logits_a[1], logits_b[1]) and not same(pa[1], pb[1])
    for s in (0, 2):
        assert np.float32(la[s]).tobytes() == np.float32(lb[s]).tobytes(), f"member {s}: loss"
        assert same(logits_a[s], logits_b[s]), f"member {s}: logits"
        assert same(ga[s], gb[s]) and same(pa[s], pb[s]), f"member {s}: gradients / parameters"


def test_amp_skips_the_member_whose_gradients_are_not_finite():
    """amp=True, member 1's ctx set to NaN: members 0 and 2 step, bit-identical to the run without the NaN; member 1's row
    and optimiser state keep their bits; skipped_steps() == [0, 1, 0]."""
    clean = _sweep("f16", optims=[_oc()] * 3, amp=True)
    _, _, _, p_clean = _one_step(clean)
    assert clean.skipped_steps() == [0, 0, 0]
    tr = _sweep("f16", optims=[_oc()] * 3, amp=True)
    eng = tr.engine
    eng.coop_sweep_member_ctx(1).fill_(NAN)
    before = eng.cs_params.clone()
    losses, _, grads, after = _one_step(tr)
    assert tr.skipped_steps() == [0, 1, 0]
    assert same(after[1], before[1]), "the skipped member's row changed"
    assert not np.isfinite(losses[1]) and np.isfinite(losses[0]) and np.isfinite(losses[2])
    assert not bool(torch.isfinite(eng.coop_sweep_member_ctx(1, grads)).all())
    for s in (0, 2):
        assert same(after[s], p_clean[s]) and not same(after[s], before[s]), f"member {s}"
    assert not bool(tr._opt._state()[0][1].any()), "a skipped step wrote optimiser state"


@pytest.mark.parametrize("shared", [False, True])
def test_graph_replay_equals_eager_and_is_captured_once(shared):
    """Three steps, every one a new epoch with new rates (warm-up, then the cosine; adam beside sgd): graph replay leaves
    the parameters and optimiser state of eager launches, bit for bit, from ONE capture -- the rates are device data."""
    from rpo_amd.trainer import OptimConfig
    optims = [OptimConfig(lr=0.002, max_epoch=10, warmup_epoch=1, warmup_cons_lr=1e-5),
              OptimConfig(name="adam", lr=1e-3, max_epoch=10, warmup_epoch=1, warmup_cons_lr=1e-4),
              OptimConfig(lr=0.004, max_epoch=10, warmup_epoch=1, warmup_cons_lr=2e-5, momentum=0.8)]
    runs = []
    for use_graph in (False, True):
        tr = _sweep("bf16", (4, 4, 4) if shared else MIXED, optims=optims, use_graph=use_graph, num_batches=1,
                    shared_prefix=shared)
        lrs, losses = [], []
        for step in range(3):
            lrs.append(list(tr.lr))
            losses.append(tr.forward_backward(_bt(step))["loss"])
        assert tr.epoch == 3 and tr.captures == (1 if use_graph else 0)
        assert lrs[0] != lrs[1] != lrs[2] and lrs[0] == [1e-5, 1e-4, 2e-5]
        runs.append((np.asarray(losses, np.float32), tr.engine.cs_params.clone(),
                     [None if r is None else r.clone() for r in tr._opt._state()]))
    (la, pa, sa), (lb, pb, sb_) = runs
    assert np.isfinite(la).all() and la.tobytes() == lb.tobytes(), (la.tolist(), lb.tolist())
    assert same(pa, pb) and all((a is None and w is None) or same(a, w) for a, w in zip(sa, sb_))


# ============================================================================================ 5. mixed optimisers

def _torch_opt(oc, params, lr):
    kw = dict(lr=lr, weight_decay=oc.weight_decay)
    if oc.name == "sgd":
        return torch.optim.SGD(params, momentum=oc.momentum, dampening=oc.sgd_dampening, nesterov=oc.sgd_nesterov, **kw)
    cls = torch.optim.AdamW if oc.name == "adamw" else torch.optim.Adam
    return cls(params, betas=(oc.adam_beta1, oc.adam_beta2), amsgrad=oc.name == "amsgrad", **kw)


def test_mixed_optimisers_follow_torch_on_each_members_own_gradients():
    """sgd + adam + adamw members with n_ctx (4, 1, 2), two steps: each member's context equals torch.optim's rule applied
    to ITS gradients (read back after every step), under the tolerance rule of tests/test_gpu_optim.py, restated: torch runs
    on the CPU in float32 and in float64 on the same fp32 gradients, E_ref = max |x32 - x64|, and the device row must lie
    within max(4 E_ref, 4 * 2^-24 * max |x64|) of the float64 run.  Nothing behind a member's n_ctx moves."""
    optims = [_oc("sgd"), _oc("adam", lr=1e-3), _oc("adamw", lr=1e-3)]
    tr = _sweep("f32", optims=optims)
    eng = tr.engine
    pairs = []
    for s, oc in enumerate(optims):
        p = [torch.nn.Parameter(eng.coop_sweep_member_ctx(s).detach().cpu().to(dt).clone()) for dt in (torch.float32, torch.float64)]
        pairs.append((p, [_torch_opt(oc, [q], oc.lr) for q in p]))
    for step in range(2):
        tr.forward_backward(_bt(step))
        for s, (p, opts) in enumerate(pairs):
            g = eng.coop_sweep_member_ctx(s, eng.cs_grads).cpu()
            for q, o in zip(p, opts):
                q.grad = g.to(q.dtype).clone()
                o.step()
    for s, (p, _) in enumerate(pairs):
        got, x32, x64 = eng.coop_sweep_member_ctx(s).cpu().double(), p[0].detach().double(), p[1].detach()
        e_ref = float((x32 - x64).abs().max())
        bound = max(4.0 * e_ref, 4.0 * 2.0 ** -24 * float(x64.abs().max()))
        err = float((got - x64).abs().max())
        print(f"[coop sweep optim] member {s} ({optims[s].name}): err {err:.3e} E_ref {e_ref:.3e} bound {bound:.3e}")
        assert bool(torch.isfinite(got).all()) and err <= bound, f"member {s} ({optims[s].name}): {err:.3e} > {bound:.3e}"
        assert not bool(eng.cs_params[s, MIXED[s] * eng.cfg.d_t:].any()), f"member {s}: floats behind its n_ctx moved"
    assert tr._opt.table_driven and tr._opt.steps() == [2, 2, 2]


# ============================================================================================ 6. checkpoints, evaluation, epochs

def _decoded(n, seed):
    rng = np.random.default_rng(seed)
    sizes = [(375, 500), (500, 333), (224, 224), (97, 260), (301, 97), (60, 40), (230, 231), (256, 192)]
    return [rng.integers(0, 256, (*sizes[i % len(sizes)], 3), dtype=np.uint8) for i in range(n)]


def _solo(s, optims, mode="bf16", **kw):
    from rpo_amd.coop import CoOp
    from rpo_amd.coop_sweep import member_tokens
    cfg, sd, toks = _world()
    n_s = MIXED[s]
    return CoOp(sd, member_tokens(toks, N_MAX, n_s), n_s, optims[s], DEV, DT[mode], batch_size=B, cfg=cfg, **kw)


def test_checkpoints_are_the_standalone_trainers(tmp_path):
    """`save_model` -> a standalone CoOp(n_ctx = n_s) on `member_tokens` loads member s's file (bits, the token_prefix /
    token_suffix buffers of ITS prompts included) and resumes its optimiser state; a standalone file loads into the member;
    `resume_model` restores optimiser state and epoch and continues exactly where the first trainer does."""
    S = 3
    optims = [_oc("sgd"), _oc("adam", lr=1e-3), _oc("sgd", lr=0.004)]
    tr = _sweep("bf16", optims=optims, num_batches=2)
    for step in range(3):                                             # one epoch and a half
        tr.forward_backward(_bt(step))
    assert tr.epoch == 1 and tr.batch_idx == 1
    dirs = [str(tmp_path / f"member{s}") for s in range(S)]
    tr.save_model(dirs, is_best=True)
    d = tr.cfg.d_t
    for s in range(S):
        n = MIXED[s] * d
        solo = _solo(s, optims, num_batches=2)
        ck = solo.load_model(dirs[s])
        assert same(solo.engine.coop_params, tr.engine.cs_params[s, :n]) and solo.epoch == 0
        mine = solo.model.prompt_learner.state_dict()
        assert set(ck["state_dict"]) == set(mine) == {"ctx", "token_prefix", "token_suffix"}
        for k in ("token_prefix", "token_suffix"):
            assert same(torch.as_tensor(ck["state_dict"][k]), mine[k]), (s, k)
        assert solo.resume_model(dirs[s]) == 1 and solo._steps == 3
        for a, w in zip(tr._opt._state(), solo._opt._state()):
            if a is not None and w is not None:                       # (a plain-SGD run keeps its momentum row only)
                assert same(a[s, :n], w.view(-1)[:n]), f"member {s}: optimiser state"
        solo.save_model(str(tmp_path / f"solo{s}"), is_best=True)     # ... and back
        del solo
    again = _sweep("bf16", seeds=(7, 8, 9), optims=optims, num_batches=2)
    solos = [str(tmp_path / f"solo{s}") for s in range(S)]
    again.load_model(solos)
    assert same(again.engine.cs_params, tr.engine.cs_params) and again.epoch == 0 and again._steps == 0
    assert not bool(again.engine.cs_moms.any())
    assert again.resume_model(solos) == 1
    assert again.epoch == 1 and again.lr == tr.lr and again._steps == tr._steps
    for a, w in zip(again._opt._state(), tr._opt._state()):
        assert (a is None and w is None) or same(a, w)
    la, lb = again.forward_backward(_bt(5)), tr.forward_backward(_bt(5))
    assert la == lb and same(again.engine.cs_params, tr.engine.cs_params)
    with pytest.raises(ValueError, match=r"ctx has shape \(4, 512\), member 1 of this trainer \(1, 512\)"):
        again.load_model([solos[0], solos[0], solos[2]])
    with pytest.raises(IndexError, match="member 3 of 3"):
        tr.checkpoint_dict(3)


@pytest.mark.parametrize("mode", MODES)
def test_evaluation_agrees_with_the_standalone_trainers(mode):
    """`model_inference(image, s)` against the logits of a standalone CoOp(n_ctx = n_s) with member s's context, within the
    storage mode's logit bound of `_sibling_bounds` (the GEMM plans are those of the larger row counts, so not bits);
    `test_all` counts equal the argmax of `model_inference_all` on the same images, with and without `features=`."""
    from rpo_amd.features import ImageFeatures
    from rpo_amd.input_pipeline import DeviceImageSet
    cfg, sd, toks = _world()
    tr = _sweep(mode)
    probe = torch.from_numpy(synth.images(cfg, B, seed=555)).to(DEV)
    all_logits = tr.model_inference_all(probe)
    assert all_logits.shape == (3, B, cfg.n_cls) and not same(all_logits[0], all_logits[1])
    for s in range(3):
        solo = _solo(s, [None] * 3, mode, ctx=_ctx(s, MIXED[s]))
        want = solo.model_inference(probe).cpu().numpy()
        got = tr.model_inference(probe, s)
        assert same(got, all_logits[s])
        _, bound, _ = _sibling_bounds(DT[mode], want, tr.engine.Lmax)
        err = float(np.abs(got.cpu().numpy() - want).max())
        print(f"[coop sweep eval {mode}] member {s}: logits err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, f"member {s}"
        del solo
    n_test = 5                                                         # (more than B: model_inference_all walks chunks)
    labels = np.random.default_rng(91).integers(0, cfg.n_cls, n_test).tolist()
    test_set = DeviceImageSet(_decoded(n_test, seed=90), labels, DEV)
    buf = torch.zeros(n_test, 3, cfg.image_size, cfg.image_size, device=DEV)
    with torch.cuda.device(tr.device):
        image = tr._loop_transform(False, n_test).from_set(test_set, range(n_test), out=buf)
    pred = tr.model_inference_all(image).argmax(-1).cpu().numpy()
    assert pred.shape == (3, n_test)
    feats = ImageFeatures.build(tr, test_set)
    for res in (tr.test_all(test_set, verbose=False), tr.test_all(test_set, features=feats, verbose=False)):
        assert len(res) == 3
        for s in range(3):
            cm = np.zeros((cfg.n_cls, cfg.n_cls), np.int64)
            for t, p in zip(labels, pred[s]):
                cm[t, p] += 1
            assert np.array_equal(res[s]["confusion_matrix"], cm), f"member {s}"
            assert res[s]["total"] == n_test and res[s]["correct"] == int(np.trace(cm))
    assert tr.test(test_set, 2, verbose=False, features=feats)["correct"] == int((pred[2] == np.array(labels)).sum())
    with pytest.raises(IndexError, match="member 3 of 3"):
        tr.test(test_set, member=3)


@pytest.mark.parametrize("use_graph", [False, True])
def test_run_epoch_equals_forward_backward_on_the_same_batches(use_graph, tmp_path):
    """run_epoch over two batches of one resident set == two forward_backward calls on the batches `epoch_indices` gives
    that generator: per-step, per-member losses and final state, bit for bit.  `train` runs the remaining epochs, evaluates
    every member after each on cached features and keeps each member's best checkpoint."""
    from rpo_amd.features import ImageFeatures
    from rpo_amd.input_pipeline import DeviceImageSet, InputConfig, build_transform
    from rpo_amd.loop import epoch_indices
    cfg, sd, toks = _world()
    S, nb = 3, 2
    n = nb * B
    imgs, labs = _decoded(n, seed=60), np.random.default_rng(70).integers(0, cfg.n_cls, n).tolist()
    train_set = DeviceImageSet(imgs, labs, DEV)
    stage = build_transform(InputConfig(SIZE=(224, 224)), True, DEV, B)
    torch.manual_seed(5)
    order = epoch_indices(n, B, torch.Generator().manual_seed(40))
    plans = [[stage.plan(*imgs[i].shape[:2]) for i in batch] for batch in order]
    optims = [_oc(), _oc("adam", lr=1e-3), _oc(lr=0.004)]
    seq = _sweep("bf16", optims=optims, num_batches=nb, use_graph=use_graph)
    seq_loss = []
    for t in range(nb):
        bt = {"img": stage([imgs[i] for i in order[t]], plans[t]).clone(), "label": torch.tensor([labs[i] for i in order[t]])}
        seq_loss.append([np.float32(v) for v in seq.forward_backward(bt)["loss"]])
    tr = _sweep("bf16", optims=optims, num_batches=nb, use_graph=use_graph)
    out = tr.run_epoch(train_set, torch.Generator().manual_seed(40), plans)
    assert out["indices"] == order and out["loss"].is_cuda and out["loss"].shape == (nb, S) and "counts" not in out
    torch.cuda.synchronize()
    got = out["loss"].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), np.array(seq_loss, np.float32).view(np.uint32)), "per-step, per-member losses"
    assert same(tr.engine.cs_params, seq.engine.cs_params) and same(tr.engine.cs_moms, seq.engine.cs_moms)
    assert tr.epoch == 1 and tr.batch_idx == 0 and tr.lr == seq.lr and tr._steps == seq._steps == nb
    assert tr.captures == seq.captures == (1 if use_graph else 0)
    dirs = [str(tmp_path / f"m{s}") for s in range(S)]
    feats = ImageFeatures.build(tr, train_set)
    hist = tr.train(train_set, max_epoch=3, val_set=train_set, val_features=feats, directories=dirs, verbose=False)
    assert [h["epoch"] for h in hist] == [2, 3] and tr.epoch == 3 and tr.captures == (1 if use_graph else 0)
    assert all(len(h["loss"]) == S and len(h["val_acc"]) == S and np.isfinite(h["loss"]).all() for h in hist)
    assert all(os.path.exists(os.path.join(d, "prompt_learner", "model-best.pth.tar")) for d in dirs)
    assert tr.best_results == [max(h["val_acc"][s] for h in hist) for s in range(S)]


# ============================================================================================ 7. ResNet

@functools.lru_cache(maxsize=None)
def _rn_world():
    from rpo_amd.config import rn_clip
    cfg = rn_clip((1, 1, 1, 1), 64, 1024, layers_t=2)               # the "mini" config of tests/test_gpu_rn.py
    gold = dict(np.load(os.path.join(GOLDEN, "ref_rn_coop_mini_b3_ctx4.npz")))
    return cfg, synth.rn_clip_state_dict(cfg, seed=0, check=False), gold["tokenized_prompts"], gold["ctx"].astype(np.float32)


def _rn_bt(step):
    cfg = _rn_world()[0]
    return {"img": torch.from_numpy(synth.images(cfg, B, seed=70 + step)), "label": torch.from_numpy(synth.labels(cfg, B, seed=80 + step))}


def test_resnet_one_member_is_a_standalone_coop_bit_for_bit():
    from rpo_amd.coop import CoOp
    from rpo_amd.coop_sweep import CoOpSweep
    cfg, sd, toks, ctx = _rn_world()
    oc = _oc()
    solo = CoOp(sd, toks, N_MAX, oc, DEV, torch.bfloat16, batch_size=B, num_batches=10 ** 9, ctx=ctx)
    tr = CoOpSweep(sd, toks, [dict(ctx=ctx, optim=oc)], n_ctx=N_MAX, batch_size=B, num_batches=10 ** 9,
                   act_dtype=torch.bfloat16, device=DEV)
    assert tr.cfg.is_rn and tr.cfg == solo.cfg
    for step in range(2):
        want, got = solo.forward_backward(_rn_bt(step))["loss"], tr.forward_backward(_rn_bt(step))["loss"][0]
        assert np.isfinite(want) and np.float32(want).tobytes() == np.float32(got).tobytes(), (step, want, got)
        assert same(tr.engine.cs_grads[0], solo.engine.coop_grads), f"step {step}: gradients"
        assert same(tr.engine.cs_params[0], solo.engine.coop_params), f"step {step}: parameters"


def test_resnet_two_members_of_different_n_ctx_are_independent():
    from rpo_amd.coop_sweep import CoOpSweep
    cfg, sd, toks, ctx = _rn_world()
    rng = np.random.default_rng(3)
    other = [(0.02 * rng.standard_normal((n, cfg.d_t))).astype(np.float32) for n in (2, 3)]
    outs = []
    for c1 in other:
        tr = CoOpSweep(sd, toks, [dict(ctx=ctx, optim=_oc()), dict(ctx=c1, n_ctx=c1.shape[0], optim=_oc())], n_ctx=N_MAX,
                       batch_size=B, num_batches=10 ** 9, act_dtype=torch.bfloat16, device=DEV)
        loss = tr.forward_backward(_rn_bt(0))["loss"]
        assert np.isfinite(loss).all()
        outs.append((loss, tr.engine.cs_logits[:2 * B].view(2, B, -1).clone(), tr.engine.cs_grads.clone(), tr.engine.cs_params.clone()))
    (la, ga_l, ga, pa), (lb, gb_l, gb, pb) = outs
    assert np.float32(la[0]).tobytes() == np.float32(lb[0]).tobytes() and same(ga_l[0], gb_l[0])
    assert same(ga[0], gb[0]) and same(pa[0], pb[0])
    assert not same(ga_l[1], gb_l[1]) and not same(ga_l[0], ga_l[1])
