"""CoCoOpMulti on the GPU (rpo_amd/coop_multi.py, rpo_amd/engine_cocoop_multi.py, rpo_amd/csrc/cocoop_sets.hip; DESIGN.md
section 9r): the four member kernels against the ungrouped kernels (bits) and float64 (one rounding), then the step of S
members against the CPU oracle, a standalone CoCoOp (bits), the reference's fixture, itself with one member replaced, graph
replay, torch.optim and the standalone trainer's checkpoints and evaluation.  Every test here fails without the feature:
there are no `ops.*_sets` for CoCoOp, no `cocoop_multi_setup` and no `rpo_amd.coop_multi`."""
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
BOUNDS = {"f32": (TOL_F32, TOL_F32), "f16": (F16_LOGIT_ATOL, F16_GRAD_REL), "bf16": (BF16_LOGIT_ATOL, BF16_GRAD_REL)}
KEYS = ("ctx", "w1", "b1", "w2", "b2")
WIDTHS = {"ViT-B/16": (512, 32, 512), "ViT-L/14-text": (768, 48, 768)}          # e, h, d
N_CTX = 4
NAN = float("nan")


def bits(t):
    return torch.as_tensor(t).detach().contiguous().view(torch.int32).cpu()


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _relmax(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _layout(widths):
    from rpo_amd.engine_cocoop_multi import cocoop_row_layout
    e, h, d = WIDTHS[widths]
    return (e, h, d) + cocoop_row_layout(N_CTX, e, h, d)


def _rows(S, stride, length, seed, fill=True):
    """[S + 1, stride] on the device: S member rows of N(0, 0.05) (or NaN everywhere when not `fill`), NaN in the padding
    behind every row and in the whole guard row S."""
    g = torch.Generator().manual_seed(seed)
    t = torch.full((S + 1, stride), NAN)
    if fill:
        t[:S, :length] = 0.05 * torch.randn(S, length, generator=g)
    return t.to(DEV)


def _views(row, offs, e, h, d):
    o = offs
    return (row[o["w1"]:o["b1"]].view(h, e), row[o["b1"]:o["w2"]], row[o["w2"]:o["b2"]].view(d, h), row[o["b2"]:o["b2"] + d])


SB = [(1, 1), (3, 1), (2, 3), (5, 2)]


# ============================================================================================ 1. the kernels

@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("widths", list(WIDTHS))
@pytest.mark.parametrize("S,b", SB)
def test_metanet_sets_give_the_bits_of_the_ungrouped_kernels(S, b, widths, pad):
    """rpo_metanet_fwd_sets / rpo_metanet_bwd_sets against rpo_metanet_fwd / rpo_metanet_bwd(B = b) called with member s's
    four tensors on its slices: array_equal.  The padding behind every row and a guard row behind the last are NaN before
    and must be the same NaN bits after; the backward does not touch the ctx part of a gradient row; two calls give the
    same bits."""
    from rpo_amd import ops
    e, h, d, length, offs, stride = _layout(widths)
    stride += pad
    R = S * b
    g = torch.Generator().manual_seed(100 * S + b)
    params_all = _rows(S, stride, length, seed=7 * S + b)
    params = params_all[:S]
    img_f = (torch.randn(R, e, generator=g) * 0.7).to(DEV)
    d_bias = (torch.randn(R, d, generator=g) * 1e-2).to(DEV)
    f32 = lambda *s: torch.full(s, NAN, device=DEV)
    fn, hid, bias = f32(R, e), f32(R, h), f32(R, d)
    before = params_all.clone()
    ops.metanet_fwd_sets(img_f, params, N_CTX, fn, hid, bias, b)
    grads_all = _rows(S, stride, length, seed=0, fill=False)
    g_before = grads_all.clone()
    ops.metanet_bwd_sets(d_bias, fn, hid, params, grads_all[:S], N_CTX, b)
    torch.cuda.synchronize()
    assert same(params_all, before), "the forward / backward wrote into params"
    assert bool((hid == 0).any()) and bool((hid > 0).any()), "the case must have units on both sides of the ReLU"
    for s in range(S):
        sl = slice(s * b, (s + 1) * b)
        w1, b1, w2, b2 = _views(params[s], offs, e, h, d)
        rfn, rhid, rbias = f32(b, e), f32(b, h), f32(b, d)
        ops.metanet_fwd(img_f[sl], w1, b1, w2, b2, rfn, rhid, rbias)
        assert same(fn[sl], rfn) and same(hid[sl], rhid) and same(bias[sl], rbias), f"forward, member {s}"
        want = [torch.full_like(t, NAN).contiguous() for t in (w1, b1, w2, b2)]
        ops.metanet_bwd(d_bias[sl].contiguous(), rfn, rhid, w2.contiguous(), *want)
        got = _views(grads_all[s], offs, e, h, d)
        for name, a, w in zip(KEYS[1:], got, want):
            assert bool(torch.isfinite(w).all()) and same(a, w), f"backward, member {s}: g_{name}"
    # what no member owns: the ctx part of every gradient row, the padding, the guard row
    mask = torch.ones(S + 1, stride, dtype=torch.bool)
    mask[:S, offs["w1"]:length] = False
    assert torch.equal(bits(grads_all)[mask], bits(g_before)[mask]), "the backward wrote outside the four meta-net slices"
    first = (fn.clone(), hid.clone(), bias.clone(), grads_all.clone())
    ops.metanet_fwd_sets(img_f, params, N_CTX, fn, hid, bias, b)
    ops.metanet_bwd_sets(d_bias, fn, hid, params, grads_all[:S], N_CTX, b)
    assert all(same(a, w) for a, w in zip((fn, hid, bias, grads_all), first)), "two calls differ"


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("widths", list(WIDTHS))
@pytest.mark.parametrize("S,b", SB)
def test_shift_and_gradient_tail_against_float64(S, b, widths, pad):
    """rpo_cocoop_shift_sets and rpo_cocoop_grad_tail_sets against float64.  Every output is a sum of at most b * n_ctx
    fp32 terms added one after the other (and one multiplication by 1 / b): each of the at most b * n_ctx roundings moves it
    by at most 2^-24 of a partial sum, which sum |terms| bounds -- so |out - exact| <= (b * n_ctx) * 2^-24 * sum |terms|,
    derived, not measured.  b = 1: g_ctx == d_shift and loss == loss_img, bit for bit.  Padding, guard row and the meta-net
    part of the gradient rows keep their NaN bits."""
    from rpo_amd import ops
    e, h, d, length, offs, stride = _layout(widths)
    stride += pad
    R, nd = S * b, N_CTX * d
    g = torch.Generator().manual_seed(200 * S + b)
    params_all = _rows(S, stride, length, seed=11 * S + b)
    bias = torch.randn(R, d, generator=g).to(DEV)
    shift = torch.full((R, N_CTX, d), NAN, device=DEV)
    ops.cocoop_shift_sets(params_all[:S], bias, shift, b)
    ctx64 = params_all[:S, :nd].double().view(S, 1, N_CTX, d)
    want = ctx64 + bias.double().view(S, b, 1, d)
    lim = 2.0 ** -24 * (ctx64.abs() + bias.double().abs().view(S, b, 1, d)) * (b * N_CTX)
    err = (shift.double().view(S, b, N_CTX, d) - want).abs()
    assert bool((err <= lim).all()), f"shift: worst err / bound {float((err / lim).max()):.3f}"
    # ---- the tail
    d_shift = (torch.randn(R, N_CTX, d, generator=g) * 10.0 ** torch.randint(-6, 1, (R, 1, 1), generator=g).float()).to(DEV)
    loss_img = (torch.rand(R, generator=g) * 5).to(DEV)
    grads_all = _rows(S, stride, length, seed=0, fill=False)
    g_before = grads_all.clone()
    d_bias, loss = torch.full((R, d), NAN, device=DEV), torch.full((S,), NAN, device=DEV)
    ops.cocoop_grad_tail_sets(d_shift, loss_img, grads_all[:S], d_bias, loss, b)
    ds64 = d_shift.double().view(S, b, N_CTX, d)
    u = b * N_CTX * 2.0 ** -24
    for name, got, ref, mag in (("g_ctx", grads_all[:S, :nd].reshape(S, N_CTX, d), ds64.sum(1) / b, ds64.abs().sum(1) / b),
                                ("d_bias", d_bias.view(S, b, d), ds64.sum(2) / b, ds64.abs().sum(2) / b),
                                ("loss", loss, loss_img.double().view(S, b).sum(1) / b, loss_img.double().view(S, b).sum(1) / b)):
        err = (got.double() - ref).abs()
        worst = float((err / (u * mag).clamp_min(1e-300)).max())
        print(f"[tail S={S} b={b} {widths} pad={pad}] {name}: worst err / bound {worst:.3f}")
        assert bool(torch.isfinite(got).all()) and bool((err <= u * mag).all()), f"{name}: err / bound {worst:.3f}"
    if b == 1:
        assert same(grads_all[:S, :nd].reshape(R, N_CTX, d), d_shift) and same(loss, loss_img)
    mask = torch.ones(S + 1, stride, dtype=torch.bool)
    mask[:S, :nd] = False
    assert torch.equal(bits(grads_all)[mask], bits(g_before)[mask]), "the tail wrote outside the ctx part of the rows"
    first = (grads_all.clone(), d_bias.clone(), loss.clone())
    ops.cocoop_grad_tail_sets(d_shift, loss_img, grads_all[:S], d_bias, loss, b)
    assert all(same(a, w) for a, w in zip((grads_all, d_bias, loss), first)), "two calls differ"


# ============================================================================================ 2. the step against the oracle
# tests/test_gpu_model.py's `_sibling_case` per member: 7 classes of 8-29 tokens, n_ctx 4, depth-1 towers, every member with
# its own ctx / meta-net / images / labels.  The world (weights, tokens) is that of tests/test_gpu_cocoop_classset.py's
# SEED_7CLS (that file's note: the f16 logit bound is at the edge of what 16-bit storage gives on this class set).  The
# members are the first three seeds; seed 7 is the one a member is replaced by.  What the PARENT's code -- a standalone
# CoCoOpCustomCLIP on the member's two images, dense and shared-prefix -- gives on them against the same oracle (worst of
# seeds 0, 1, 2, 7; logits f16 / bf16, gradients f16 / bf16): 6.65e-3 / 5.75e-2 and 3.3e-3 / 2.1e-2 at bounds of 1.0e-2 (1.2e-2
# where max |logit| is 10.4) / 0.12 and 6e-3 / 5e-2.  The members of a step get those figures.  No bound is widened.
BASE7 = [4 + (7 * c) % 22 for c in range(7)]
WORLD_SEED = 40
MEMBER_SEEDS = (0, 1, 2)


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
    toks = synth.coop_tokens(synth.synthetic_tokens(cfg, BASE7, seed=17 + WORLD_SEED), N_CTX)
    sd = synth.clip_state_dict(cfg, seed=23 + WORLD_SEED, token_rows=np.unique(toks).tolist() + [49407])
    return cfg, sd, toks


@functools.lru_cache(maxsize=None)
def _member(seed):
    """(ctx, meta, images [2], labels [2]) of the member with this seed: `_sibling_case`'s construction, its meta-net's b1
    shifted by whole margins until both images clear the ReLU kink by 3 % of the pre-activations' spread.  A batch of b
    takes the first b images."""
    from oracle.rpo_oracle import plain_clip_forward
    cfg, sd, toks = _world()
    B = 2
    rng = np.random.default_rng(29 + WORLD_SEED + 1000 * seed)
    ctx = (0.02 * rng.standard_normal((N_CTX, cfg.d_t))).astype(np.float32)
    image, label = synth.images(cfg, B, seed=31 + WORLD_SEED + 1000 * seed), synth.labels(cfg, B, seed=37 + WORLD_SEED + 1000 * seed)
    label[0] = cfg.n_cls - 1
    e, h = cfg.embed, cfg.embed // 16
    u = lambda shape, fan: rng.uniform(-fan ** -0.5, fan ** -0.5, shape).astype(np.float32)
    meta = dict(w1=u((h, e), e), b1=u((h,), e), w2=u((cfg.d_t, h), h), b2=u((cfg.d_t,), h))
    _, imf, _ = plain_clip_forward(sd, image, toks, cfg.patch)
    a = (imf / imf.norm(dim=-1, keepdim=True)).double().numpy() @ meta["w1"].T.astype(np.float64)
    margin = 0.03 * float(np.abs(a).max())
    for j in range(h):
        shift = next(k * margin for k in sorted(range(-B - 1, B + 2), key=abs)
                     if np.abs(a[:, j] + meta["b1"][j] + k * margin).min() >= margin)
        meta["b1"][j] += np.float32(shift)
    # on the CPU, before any GPU run: the oracle itself clears the margin for this member, on both sides of the kink
    pre = a + meta["b1"].astype(np.float64)
    assert np.abs(pre).min() >= 0.99 * margin and (pre < 0).any() and (pre > 0).any(), f"member seed {seed}: ReLU margin"
    return ctx, meta, image, label


@functools.lru_cache(maxsize=None)
def _oracle(seed, b):
    """oracle.rpo_oracle.cocoop_loss_and_grads on this member ALONE with its first b images."""
    from oracle.rpo_oracle import cocoop_loss_and_grads
    cfg, sd, toks = _world()
    ctx, meta, image, label = _member(seed)
    logits, loss, g = cocoop_loss_and_grads(sd, image[:b], toks, ctx, meta, label[:b], cfg.patch)
    return logits.numpy(), float(loss), {k: v.numpy() for k, v in g.items()}


def _multi(mode, b, seeds=MEMBER_SEEDS, optims=None, replace=None, **kw):
    """A CoCoOpMulti of the members with these seeds on the 7-class world; `replace`: {member index: seed} swaps."""
    from rpo_amd.coop_multi import CoCoOpMulti
    cfg, sd, toks = _world()
    seeds = [(replace or {}).get(i, s) for i, s in enumerate(seeds)]
    members = []
    for i, s in enumerate(seeds):
        ctx, meta, _, _ = _member(s)
        members.append(dict(ctx=ctx, meta=meta, **({} if optims is None else dict(optim=optims[i]))))
    kw.setdefault("num_batches", 10 ** 9)
    tr = CoCoOpMulti(sd, toks, members, n_ctx=N_CTX, batch_size=b, act_dtype=DT[mode], cfg=cfg, device=DEV, **kw)
    return tr, seeds


def _batches(seeds, b):
    return [{"img": torch.from_numpy(_member(s)[2][:b]), "label": torch.from_numpy(_member(s)[3][:b])} for s in seeds]


def _grad_views(eng, s):
    return {k: v.cpu().numpy() for k, v in eng.cocoop_member_views(s, eng.cm_grads).items()}


def _check_against_oracle(mode, b, shared):
    act = DT[mode]
    for s in MEMBER_SEEDS:                                # the oracle (and its margin check) first, on the CPU
        _oracle(s, b)
    tr, seeds = _multi(mode, b, shared_prefix=shared)
    eng = tr.engine
    with torch.cuda.device(eng.dev):
        image, label = tr.parse_batch_train(_batches(seeds, b))
        logits = eng.cocoop_multi_forward_backward(image, label).cpu().numpy()
        loss = eng.cm_loss.cpu().numpy()
    assert eng.coop_shared == shared and logits.shape == (len(seeds) * b, len(BASE7)) and loss.shape == (len(seeds),)
    for i, s in enumerate(seeds):
        o_logits, o_loss, o_g = _oracle(s, b)
        lb_loss, lb_logits, gb = _sibling_bounds(act, o_logits, eng.Lmax)
        le, ll = float(np.abs(logits[i * b:(i + 1) * b] - o_logits).max()), abs(float(loss[i]) - o_loss)
        rel = {k: _relmax(v, o_g[k]) for k, v in _grad_views(eng, i).items()}
        print(f"\n[cocoop multi {mode} b={b} shared={shared} member {i}] logits err {le:.3e} (bound {lb_logits:.3e}, max |logit| "
              f"{np.abs(o_logits).max():.2f}) loss err {ll:.3e} (bound {lb_loss:.3e}) grads rel "
              + " ".join(f"{k} {v:.2e}" for k, v in rel.items()) + f" (bound {gb})")
        assert ll <= lb_loss and le <= lb_logits, f"member {i}"
        assert all(v <= gb for v in rel.values()), (i, rel)
    # the members differ (a set whose members agree would prove nothing)
    assert not np.array_equal(logits[:b], logits[b:2 * b])


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_every_member_against_the_oracle_on_that_member_alone(mode, b):
    """S = 3 members with different ctx / meta-net / images: every member's loss, logits and five gradients against
    oracle.rpo_oracle.cocoop_loss_and_grads run on that member alone, at `_sibling_bounds`."""
    _check_against_oracle(mode, b, shared=False)


@pytest.mark.parametrize("mode", MODES)
def test_shared_prefix_members_against_the_oracle(mode):
    """The b = 1 oracle case on the shared-prefix rows (`shared_prefix=True`), at the same bounds."""
    _check_against_oracle(mode, 1, shared=True)


# ============================================================================================ 3. S = 1

def _oc(name="sgd", **kw):
    from rpo_amd.trainer import OptimConfig
    kw.setdefault("lr", 0.002)
    return OptimConfig(name=name, momentum=0.9, weight_decay=5e-4, warmup_epoch=0, lr_scheduler="constant", max_epoch=10, **kw)


@pytest.mark.parametrize("mode,kind,amp", [("bf16", "sgd", False), ("f32", "adam", False), ("f16", "sgd", True)])
def test_one_member_of_one_image_is_a_standalone_cocoop_bit_for_bit(mode, kind, amp):
    """S = 1, b = 1: the same shapes through the same kernels -- three optimiser steps leave the parameters, the optimiser
    state and every step's loss bit-identical to a standalone CoCoOp given the same ctx / meta-net / OptimConfig."""
    from rpo_amd.coop import CoCoOp
    from rpo_amd.coop_multi import CoCoOpMulti
    cfg, sd, toks = _world()
    ctx, meta, _, _ = _member(MEMBER_SEEDS[0])
    oc = _oc(kind)
    solo = CoCoOp(sd, toks, N_CTX, oc, DEV, DT[mode], batch_size=1, num_batches=10 ** 9, ctx=ctx, meta=meta, cfg=cfg, amp=amp)
    tr = CoCoOpMulti(sd, toks, [dict(ctx=ctx, meta=meta, optim=oc)], n_ctx=N_CTX, batch_size=1, num_batches=10 ** 9,
                     act_dtype=DT[mode], cfg=cfg, device=DEV, amp=amp)
    n = solo.engine.coop_params.numel()
    assert tr.engine.cm_len == n and same(tr.engine.cm_params[0, :n], solo.engine.coop_params)
    for step in range(3):
        bt = {"img": torch.from_numpy(synth.images(cfg, 1, seed=70 + step)), "label": torch.from_numpy(synth.labels(cfg, 1, seed=80 + step))}
        want, got = solo.forward_backward(bt)["loss"], tr.forward_backward([bt])[0]["loss"]
        assert np.float32(want).tobytes() == np.float32(got).tobytes(), (step, want, got)
        assert same(tr.engine.cm_grads[0, :n], solo.engine.coop_grads), f"step {step}: gradients"
        assert same(tr.engine.cm_params[0, :n], solo.engine.coop_params), f"step {step}: parameters"
    for a, w in zip(tr._opt._state(), solo._opt._state()):
        assert (a is None) == (w is None) and (a is None or same(a[0, :n], w.view(-1)[:n])), "optimiser state"
    assert tr.skipped_steps == [0] and solo.skipped_steps == 0 and tr.checkpoint_dict(0)["steps"] == 3


def test_a_seeded_member_starts_where_the_seeded_standalone_trainer_starts():
    from rpo_amd.coop import CoCoOp
    from rpo_amd.coop_multi import CoCoOpMulti
    cfg, sd, toks = _world()
    tr = CoCoOpMulti(sd, toks, [dict(seed=3), dict(seed=11)], n_ctx=N_CTX, act_dtype=torch.bfloat16, cfg=cfg, device=DEV)
    for s, seed in enumerate((3, 11)):
        torch.manual_seed(seed)
        solo = CoCoOp(sd, toks, N_CTX, None, DEV, torch.bfloat16, cfg=cfg)
        assert same(tr.engine.cm_params[s, :tr.engine.cm_len], solo.engine.coop_params), f"seed {seed}"
        del solo


@pytest.mark.parametrize("mode", MODES)
def test_one_member_of_three_images_against_the_reference_fixture(mode):
    """S = 1, b = 3 on tests/golden/ref_cocoop_d2_b3_ctx4.npz (the reference's own cocoop.CustomCLIP + backward), at the
    bounds tests/test_gpu_model.py::test_cocoop_training_matches_reference_trainer applies to it."""
    from rpo_amd.config import vit_b16
    from rpo_amd.coop_multi import CoCoOpMulti
    gold = dict(np.load(os.path.join(GOLDEN, "ref_cocoop_d2_b3_ctx4.npz")))
    cfg = vit_b16(layers_v=2, layers_t=2, K=1)
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    tr = CoCoOpMulti(sd, gold["tokenized_prompts"], [dict(ctx=gold["ctx"], meta={k: gold[k] for k in KEYS[1:]})], n_ctx=4,
                     batch_size=3, act_dtype=DT[mode], device=DEV)
    eng = tr.engine
    image, label = torch.from_numpy(synth.images(cfg, 3)).cuda(), torch.from_numpy(gold["label"]).cuda()
    with torch.cuda.device(eng.dev):
        ev = eng.cocoop_multi_forward_backward(image, None).cpu().numpy()
        logits = eng.cocoop_multi_forward_backward(image, label).cpu().numpy()
        loss = float(eng.cm_loss[0])
    le, ll = float(np.abs(ev - gold["logits"]).max()), abs(loss - float(gold["loss"]))
    rel = {k: _relmax(v, gold["g_" + k]) for k, v in _grad_views(eng, 0).items()}
    lt, gt = BOUNDS[mode]
    print(f"\n[cocoop multi d2_b3 {mode}] logits err {le:.3e} loss err {ll:.3e} (bound {lt}) grads rel "
          + " ".join(f"{k} {v:.2e}" for k, v in rel.items()) + f" (bound {gt})")
    assert le <= lt and ll <= lt and np.array_equal(ev, logits)
    assert all(v <= gt for v in rel.values()), rel


# ============================================================================================ 4. isolation, amp, graphs

def _one_step(tr, seeds, b):
    out = tr.forward_backward(_batches(seeds, b))
    eng = tr.engine
    return ([o["loss"] for o in out], eng.logits[:len(seeds) * b].clone(), eng.cm_grads.clone(), eng.cm_params.clone())


@pytest.mark.parametrize("mode", MODES)
def test_replacing_a_member_leaves_the_others_bit_identical(mode):
    """S = 3: member 1's ctx, meta-net, image and label replaced by another member's -- every output, gradient and updated
    parameter of members 0 and 2 keeps its bits."""
    b = 1
    ta, sa = _multi(mode, b, optims=[_oc()] * 3)
    la, logits_a, ga, pa = _one_step(ta, sa, b)
    tb, sb_ = _multi(mode, b, optims=[_oc()] * 3, replace={1: 7})
    lb, logits_b, gb, pb = _one_step(tb, sb_, b)
    assert sa[1] != sb_[1] and not same(logits_a[1], logits_b[1]) and not same(pa[1], pb[1])
    for s in (0, 2):
        assert np.float32(la[s]).tobytes() == np.float32(lb[s]).tobytes(), f"member {s}: loss"
        assert same(logits_a[s * b:(s + 1) * b], logits_b[s * b:(s + 1) * b]), f"member {s}: logits"
        assert same(ga[s], gb[s]) and same(pa[s], pb[s]), f"member {s}: gradients / parameters"


def test_amp_skips_the_member_whose_gradients_are_not_finite():
    """amp=True, member 1's ctx set to NaN: members 0 and 2 step, bit-identical to the run without the NaN; member 1's row
    is untouched; skipped_steps == [0, 1, 0]."""
    b = 1
    clean, seeds = _multi("f16", b, optims=[_oc()] * 3, amp=True)
    _, _, _, p_clean = _one_step(clean, seeds, b)
    assert clean.skipped_steps == [0, 0, 0]
    tr, _ = _multi("f16", b, optims=[_oc()] * 3, amp=True)
    eng = tr.engine
    eng.cocoop_member_views(1)["ctx"].fill_(NAN)
    before = eng.cm_params.clone()
    losses, _, grads, after = _one_step(tr, seeds, b)
    assert tr.skipped_steps == [0, 1, 0]
    assert same(after[1], before[1]), "the skipped member's row changed"
    assert not np.isfinite(losses[1]) and np.isfinite(losses[0]) and np.isfinite(losses[2])
    assert not bool(torch.isfinite(grads[1, :eng.cm_len]).all())
    for s in (0, 2):
        assert same(after[s], p_clean[s]) and not same(after[s], before[s]), f"member {s}"
    assert not bool(tr._opt._state()[0][1].any()), "a skipped step wrote optimiser state"


@pytest.mark.parametrize("shared", [False, True])
def test_graph_replay_equals_eager_and_is_captured_once(shared):
    """Three steps, every one a new epoch with new rates (warm-up, then the cosine; adam beside sgd): graph replay leaves
    the parameters and optimiser state of eager launches, bit for bit, from ONE capture -- the rates are device data."""
    from rpo_amd.trainer import OptimConfig
    b = 2
    optims = [OptimConfig(lr=0.002, max_epoch=10, warmup_epoch=1, warmup_cons_lr=1e-5),
              OptimConfig(name="adam", lr=1e-3, max_epoch=10, warmup_epoch=1, warmup_cons_lr=1e-4),
              OptimConfig(lr=0.004, max_epoch=10, warmup_epoch=1, warmup_cons_lr=2e-5, momentum=0.8)]
    runs = []
    for use_graph in (False, True):
        tr, seeds = _multi("bf16", b, optims=optims, use_graph=use_graph, num_batches=1, shared_prefix=shared)
        lrs, losses = [], []
        for step in range(3):
            lrs.append(list(tr.lr))
            rot = seeds[step % 3:] + seeds[:step % 3]                  # (other images every step)
            losses.append([o["loss"] for o in tr.forward_backward(_batches(rot, b))])
        assert tr.epoch == 3 and tr.captures == (1 if use_graph else 0)
        assert lrs[0] != lrs[1] != lrs[2] and lrs[0] == [1e-5, 1e-4, 2e-5]
        runs.append((np.asarray(losses, np.float32), tr.engine.cm_params.clone(), [None if r is None else r.clone() for r in tr._opt._state()]))
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
    """sgd + adam + adamw members, two steps: each member's row equals torch.optim's rule applied to ITS gradients (read
    back after every step), under the tolerance rule of tests/test_gpu_optim.py, restated: torch runs on the CPU in float32
    and in float64 on the same fp32 gradients, E_ref = max |x32 - x64|, and the device row must lie within
    max(4 E_ref, 4 * 2^-24 * max |x64|) of the float64 run."""
    b = 1
    optims = [_oc("sgd"), _oc("adam", lr=1e-3), _oc("adamw", lr=1e-3)]
    tr, seeds = _multi("f32", b, optims=optims)
    eng = tr.engine
    n = eng.cm_len
    pairs = []
    for s, oc in enumerate(optims):
        p = [torch.nn.Parameter(eng.cm_params[s, :n].detach().cpu().to(dt).clone()) for dt in (torch.float32, torch.float64)]
        pairs.append((p, [_torch_opt(oc, [q], oc.lr) for q in p]))
    for step in range(2):
        tr.forward_backward(_batches(seeds, b))
        g = eng.cm_grads[:, :n].cpu()
        for s, (p, opts) in enumerate(pairs):
            for q, o in zip(p, opts):
                q.grad = g[s].to(q.dtype).clone()
                o.step()
    for s, (p, _) in enumerate(pairs):
        got, x32, x64 = eng.cm_params[s, :n].cpu().double(), p[0].detach().double(), p[1].detach()
        e_ref = float((x32 - x64).abs().max())
        bound = max(4.0 * e_ref, 4.0 * 2.0 ** -24 * float(x64.abs().max()))
        err = float((got - x64).abs().max())
        print(f"[cocoop multi optim] member {s} ({optims[s].name}): err {err:.3e} E_ref {e_ref:.3e} bound {bound:.3e}")
        assert bool(torch.isfinite(got).all()) and err <= bound, f"member {s} ({optims[s].name}): {err:.3e} > {bound:.3e}"
    assert tr._opt.table_driven and tr._opt.steps() == [2, 2, 2]


# ============================================================================================ 6. checkpoints, evaluation, epochs

def _decoded(n, seed):
    rng = np.random.default_rng(seed)
    sizes = [(375, 500), (500, 333), (224, 224), (97, 260), (301, 97), (60, 40), (230, 231), (256, 192)]
    return [rng.integers(0, 256, (*sizes[i % len(sizes)], 3), dtype=np.uint8) for i in range(n)]


def _same_result(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if k == "confusion_matrix":
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def test_checkpoints_and_evaluation_are_the_standalone_trainers(tmp_path):
    """`save_model` -> a standalone CoCoOp.load_model of member s's directory: `model(image)` logits bit-equal to
    `model_inference(image, member=s)`, and back (a standalone file into the members); `resume_model` restores optimiser
    state and epoch; `test(set, member=s)` with and without a conditional class set equals the standalone trainer's dict;
    `test_all` is the members' `test`."""
    from rpo_amd.coop import CoCoOp
    from rpo_amd.input_pipeline import DeviceImageSet
    cfg, sd, toks = _world()
    S, b = 3, 1
    optims = [_oc("sgd"), _oc("adam", lr=1e-3), _oc("sgd", lr=0.004)]
    tr, seeds = _multi("bf16", b, optims=optims, num_batches=2)
    for step in range(3):                                             # one epoch and a half
        tr.forward_backward(_batches(seeds[step % 3:] + seeds[:step % 3], b))
    assert tr.epoch == 1 and tr.batch_idx == 1
    dirs = [str(tmp_path / f"member{s}") for s in range(S)]
    tr.save_model(dirs, is_best=True)
    probe = torch.from_numpy(synth.images(cfg, S * b, seed=555)).to(DEV)
    n_test = 7
    test_set = DeviceImageSet(_decoded(n_test, seed=90), np.random.default_rng(91).integers(0, cfg.n_cls, n_test).tolist(), DEV)
    new_toks = toks[[5, 1, 4]]                                         # another class set (ids that have embedding rows)
    new_set = DeviceImageSet(_decoded(n_test, seed=92), np.random.default_rng(93).integers(0, len(new_toks), n_test).tolist(), DEV)
    ccs = tr.conditional_class_set(new_toks)
    n = tr.engine.cm_len
    all_res = tr.test_all(test_set, verbose=False)
    for s in range(S):
        # (the same engine batch capacity: evaluation then runs the same chunks on the same GEMM plans)
        solo = CoCoOp(sd, toks, N_CTX, optims[s], DEV, torch.bfloat16, batch_size=S * b, num_batches=2, cfg=cfg)
        solo.load_model(dirs[s])
        assert same(solo.engine.coop_params, tr.engine.cm_params[s, :n]) and solo.epoch == 0
        solo.model.prompt_learner.eval()
        assert same(solo.model(probe), tr.model_inference(probe, member=s)), f"member {s}: eval logits"
        res = tr.test(test_set, member=s, verbose=False)
        _same_result(res, solo.test(test_set, verbose=False), f"member {s}: test")
        _same_result(res, all_res[s], f"member {s}: test_all")
        _same_result(tr.test(new_set, member=s, verbose=False, classes=ccs),
                     solo.test(new_set, verbose=False, classes=solo.conditional_class_set(new_toks)), f"member {s}: classes")
        assert same(tr.model_inference(probe, member=s, classes=ccs),
                    solo.model_inference(probe, classes=solo.conditional_class_set(new_toks)))
        assert solo.resume_model(dirs[s]) == 1
        for a, w in zip(tr._opt._state(), solo._opt._state()):
            if a is not None and w is not None:                       # (a plain-SGD run keeps its momentum row only)
                assert same(a[s, :n], w.view(-1)[:n]), f"member {s}: optimiser state"
        # ... and back: the standalone trainer's own file into member s of a fresh trainer
        solo.save_model(str(tmp_path / f"solo{s}"), is_best=True)
    assert not same(tr.model_inference(probe, member=0), tr.model_inference(probe, member=1))
    again, _ = _multi("bf16", b, optims=optims, num_batches=2, replace={0: 7, 1: 7, 2: 7})
    again.load_model([str(tmp_path / f"solo{s}") for s in range(S)])
    assert same(again.engine.cm_params, tr.engine.cm_params) and again.epoch == 0 and again._steps == 0
    assert not bool(again.engine.cm_moms.any())
    assert again.resume_model([str(tmp_path / f"solo{s}") for s in range(S)]) == 1
    assert again.epoch == 1 and again.lr == tr.lr and again._steps == tr._steps
    for a, w in zip(again._opt._state(), tr._opt._state()):
        assert (a is None and w is None) or same(a, w)
    # resuming continues exactly where the first trainer does
    la, lb = again.forward_backward(_batches(seeds, b)), tr.forward_backward(_batches(seeds, b))
    assert la == lb and same(again.engine.cm_params, tr.engine.cm_params)
    with pytest.raises(IndexError, match="member 3 of 3"):
        tr.test(test_set, member=3)


@pytest.mark.parametrize("use_graph", [False, True])
def test_run_epoch_equals_forward_backward_on_the_same_batches(use_graph, tmp_path):
    """run_epoch over two batches per member, each member with its own resident set and generator == two forward_backward
    calls on the batches `epoch_indices` gives those generators: per-step losses and final state, bit for bit.  `train` runs
    the remaining epochs, evaluates every member after each and keeps each member's best checkpoint."""
    from rpo_amd.input_pipeline import DeviceImageSet, InputConfig, build_transform
    from rpo_amd.loop import epoch_indices
    cfg, sd, toks = _world()
    S, b, nb = 3, 1, 2
    sizes = [2, 2, 2]                                              # (b = 1: a set of nb images gives nb batches)
    imgs = [_decoded(n, seed=60 + s) for s, n in enumerate(sizes)]
    labs = [np.random.default_rng(70 + s).integers(0, cfg.n_cls, n).tolist() for s, n in enumerate(sizes)]
    sets = [DeviceImageSet(imgs[s], labs[s], DEV) for s in range(S)]
    stage = build_transform(InputConfig(SIZE=(224, 224)), True, DEV, b)
    torch.manual_seed(5)
    order = [epoch_indices(sizes[s], b, torch.Generator().manual_seed(40 + s)) for s in range(S)]
    plans = [[[stage.plan(*imgs[s][i].shape[:2]) for i in batch] for batch in order[s]] for s in range(S)]
    optims = [_oc(), _oc("adam", lr=1e-3), _oc(lr=0.004)]
    seq, _ = _multi("bf16", b, optims=optims, num_batches=nb, use_graph=use_graph)
    seq_loss = []
    for t in range(nb):
        batches = [{"img": stage([imgs[s][i] for i in order[s][t]], plans[s][t]).clone(),
                    "label": torch.tensor([labs[s][i] for i in order[s][t]])} for s in range(S)]
        seq_loss.append([np.float32(o["loss"]) for o in seq.forward_backward(batches)])
    tr, _ = _multi("bf16", b, optims=optims, num_batches=nb, use_graph=use_graph)
    with pytest.raises(ValueError, match="CoCoOpMulti.run_epoch.*same, non-zero number of batches"):
        tr.run_epoch([sets[0], sets[1], DeviceImageSet(imgs[0][:1], labs[0][:1], DEV)])
    out = tr.run_epoch(sets, [torch.Generator().manual_seed(40 + s) for s in range(S)], plans)
    assert out["indices"] == order and out["loss"].is_cuda and out["loss"].shape == (nb, S)
    torch.cuda.synchronize()
    got = out["loss"].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), np.array(seq_loss, np.float32).view(np.uint32)), "per-step, per-member losses"
    assert same(tr.engine.cm_params, seq.engine.cm_params) and same(tr.engine.cm_moms, seq.engine.cm_moms)
    assert tr.epoch == 1 and tr.batch_idx == 0 and tr.lr == seq.lr and tr._steps == seq._steps == nb
    assert tr.captures == seq.captures == (1 if use_graph else 0)
    dirs = [str(tmp_path / f"m{s}") for s in range(S)]
    hist = tr.train(sets, max_epoch=3, val_set=sets[1], directories=dirs, verbose=False)
    assert [h["epoch"] for h in hist] == [2, 3] and tr.epoch == 3 and tr.captures == (1 if use_graph else 0)
    assert all(len(h["loss"]) == S and len(h["val_acc"]) == S and np.isfinite(h["loss"]).all() for h in hist)
    assert all(os.path.exists(os.path.join(d, "prompt_learner", "model-best.pth.tar")) for d in dirs)
    assert tr.best_results == [max(h["val_acc"][s] for h in hist) for s in range(S)]
