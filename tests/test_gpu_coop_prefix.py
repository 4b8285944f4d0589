"""CoOp / CoCoOp training on the shared-prefix row layout, on the GPU (rpo_text_attn_bwd_prefix, rpo_amd/engine_coop_prefix.py;
DESIGN.md section 9q): the attention backward against float64 autograd and against rpo_text_attn_bwd_dense on the densely
gathered sequences, then `shared_prefix=True` models and trainers against the reference's fixtures, the CPU oracle, the
dense path, graph replay and checkpoints.  Every test here fails without the feature: there is no
`ops.text_attn_bwd_prefix` and no `shared_prefix` argument."""
import functools
import math
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
TOL = {"f32": 2e-5, "bf16": 1.5e-2, "f16": 2e-3}            # tests/test_gpu_ops.py's op-level budgets, restated
BOUNDS = {"f32": (TOL_F32, TOL_F32), "f16": (F16_LOGIT_ATOL, F16_GRAD_REL), "bf16": (BF16_LOGIT_ATOL, BF16_GRAD_REL)}


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


def q(t, mode):
    """value the kernel will actually see, as float64 on the CPU"""
    return t.to(DT[mode]).to(torch.float64)


def relerr(got, ref):
    got, ref = got.detach().to(torch.float64).cpu(), ref.to(torch.float64)
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def close(got, ref, mode, what, tol=None):
    got = got.detach().to(torch.float64).cpu()
    ref = ref.to(torch.float64)
    err = (got - ref).abs().max().item()
    den = max(ref.abs().max().item(), 1e-30)
    lim = (tol if tol is not None else TOL[mode])
    assert math.isfinite(err) and err <= lim * den, f"{what} [{mode}]: max err {err:.3e} vs max ref {den:.3e} (rel {err/den:.2e} > {lim})"


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def _relmax(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ============================================================================================ 1. the kernel

# (H, n_img, P, S, lens).  The class group of a workgroup is a function of n_cls * H (1 class up to 1024 (class, head) pairs,
# then ceil(n_cls H / 1024), at most 16): "groups" runs 9 groups of one class at CoOp's default n_ctx 16, "ragged" 67 groups
# of 3 whose last holds 2, "1000cls" 125 groups of 8 -- the ordered sum of the second launch over 10, 68 and 126 slots.
OP_CASES = {
    "smallest": (1, 1, 2, 3, [5]),                                                  # one class, the smallest legal shape
    "groups": (8, 1, 17, 24, [20, 23, 25, 28, 31, 33, 36, 38, 41]),
    "three_images": (8, 3, 5, 20, [8, 25, 13, 19, 22]),
    "L80": (12, 2, 17, 63, [80, 66, 65, 64, 20]),                                   # P + S = 80, keys on both sides of 64
    "max_suffix": (8, 1, 2, 78, [80, 5]),
    "max_prefix": (8, 1, 77, 3, [80, 78]),
    "ragged": (12, 2, 5, 6, [7 + (3 * c) % 5 for c in range(200)]),
    "1000cls": (8, 1, 5, 20, [8 + (7 * c) % 18 for c in range(1000)]),              # ImageNet's class count
}


def _rows(n_img, n_cls, P, S):
    pre = lambda b: slice(b * P, (b + 1) * P)
    suf = lambda b, c: slice(n_img * P + (b * n_cls + c) * S, n_img * P + (b * n_cls + c + 1) * S)
    return n_img * P + n_img * n_cls * S, pre, suf


@functools.lru_cache(maxsize=None)
def _op_inputs(name):
    H, n_img, P, S, lens = OP_CASES[name]
    rows, _, _ = _rows(n_img, len(lens), P, S)
    d = 64 * H
    qkv = rnd((rows, 3 * d), 211)
    qkv[:, :d] *= 1.5                                 # sharper softmax rows
    dout = torch.zeros(rows, d + 96)                  # d_out: [:, 32:32 + d] of a wider buffer
    dout[:, 32:32 + d] = rnd((rows, d), 212)
    return qkv, dout


@functools.lru_cache(maxsize=None)
def _op_reference(name, mode):
    """float64 autograd of the causal attention of every sequence (b, c) gathered densely -- the image's P prefix rows,
    then the first len[c] - P suffix rows of the class -- with the prefix-row gradients summed over the classes.  The shared
    prefix row's d_out is, in the model, the sum of its dense copies' d_out; here class 0's copy carries all of it and the
    other copies none (autograd is linear in d_out, so any split gives the same sum).  -> (ref [rows, 3d], valid [rows])"""
    from oracle import rows_oracle as R
    H, n_img, P, S, lens = OP_CASES[name]
    n_cls, d = len(lens), 64 * H
    rows, pre, suf = _rows(n_img, n_cls, P, S)
    qkv, dout = _op_inputs(name)
    q3, do3 = q(qkv, mode), q(dout[:, 32:32 + d], mode)
    ref = torch.zeros(rows, 3 * d, dtype=torch.float64)
    valid = torch.zeros(rows, dtype=torch.bool)
    valid[:n_img * P] = True
    for b in range(n_img):
        for c, L in enumerate(lens):
            ns = L - P
            sfx = slice(suf(b, c).start, suf(b, c).start + ns)
            seq = torch.cat([q3[pre(b)], q3[sfx]])
            dseq = torch.cat([do3[pre(b)] if c == 0 else torch.zeros(P, d, dtype=torch.float64), do3[sfx]])
            qa, ka, va = (seq[:, i * d:(i + 1) * d].clone().requires_grad_(True) for i in range(3))
            out = R.attn_causal_fwd(qa, ka, va, H, torch.arange(1, L + 1))
            g = torch.cat(torch.autograd.grad(out, (qa, ka, va), dseq), dim=1)
            ref[pre(b)] += g[:P]
            ref[sfx] = g[P:]
            valid[sfx] = True
    return ref, valid


def _launch(t, do_d, len_d, n_img, n_cls, P, S, H, mode):
    from rpo_amd import ops
    d = 64 * H
    g = torch.full((t.shape[0], 3 * d), float("nan"), dtype=DT[mode], device=DEV)
    ops.text_attn_bwd_prefix(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], do_d, g[:, :d], g[:, d:2 * d], g[:, 2 * d:], len_d,
                             n_img, n_cls, P, S, H, 0.125)
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("name", list(OP_CASES))
@pytest.mark.parametrize("mode", MODES)
def test_prefix_attention_backward_against_float64(mode, name):
    """dq, dk, dv of rpo_text_attn_bwd_prefix in the engine's layout (q / k / v column views of one packed [rows, 3d] buffer,
    q scaled by 1.5, d_out a column view of a wider buffer, NaN-filled outputs) against `_op_reference`, with the dense
    kernel's budget (f32 2e-5, 16-bit 8e-3 of max |ref|) on the prefix rows and on the suffix rows SEPARATELY, so a wrong
    class sum cannot hide under the suffix rows' scale.  Nothing stays NaN, rows at or past len[c] are exactly 0, a second
    launch gives the same bits, and image 1 of a launch over several images has the bits of a launch over it alone."""
    H, n_img, P, S, lens = OP_CASES[name]
    n_cls, d = len(lens), 64 * H
    assert min(lens) > P and max(lens) == P + S
    rows, pre, suf = _rows(n_img, n_cls, P, S)
    qkv, dout = _op_inputs(name)
    t = qkv.to(DEV, DT[mode])
    do_w = dout.to(DEV, DT[mode])
    do_d = do_w[:, 32:32 + d]
    len_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    g = _launch(t, do_d, len_d, n_img, n_cls, P, S, H, mode)
    got = g.cpu()
    assert not torch.isnan(got).any(), "an output element was never written"
    if name == "1000cls":
        assert bool(torch.isfinite(got.float()).all())
    ref, valid = _op_reference(name, mode)
    is_pre = torch.zeros(rows, dtype=torch.bool)
    is_pre[:n_img * P] = True
    tol = None if mode == "f32" else 8e-3
    errs = {}
    for i, nm in enumerate(("dq", "dk", "dv")):
        cs = slice(i * d, (i + 1) * d)
        pad = got[~valid, cs]
        assert pad.numel() == 0 or torch.count_nonzero(pad).item() == 0, f"{nm}: suffix rows at or past len[c] are not 0"
        for part, sel in (("prefix", is_pre), ("suffix", valid & ~is_pre)):
            errs[f"{nm}/{part}"] = relerr(got[sel, cs], ref[sel, cs])
    print(f"\n[prefix attn bwd {name} {mode}] rel err (bound {TOL['f32'] if tol is None else tol}) " +
          " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for i, nm in enumerate(("dq", "dk", "dv")):
        cs = slice(i * d, (i + 1) * d)
        for part, sel in (("prefix", is_pre), ("suffix", valid & ~is_pre)):
            close(got[sel, cs], ref[sel, cs], mode, f"prefix attn bwd {name} {nm} {part} rows", tol=tol)
    g2 = _launch(t, do_d, len_d, n_img, n_cls, P, S, H, mode)
    assert torch.equal(bits(g2), bits(g)), "a second launch changed bits"
    if n_img > 1:                                     # image 1 alone: its prefix rows, then its suffix rows
        sel = torch.cat([torch.arange(P, 2 * P), torch.arange(suf(1, 0).start, suf(1, n_cls - 1).stop)]).to(DEV)
        one = _launch(t.index_select(0, sel).contiguous(), do_w.index_select(0, sel).contiguous()[:, 32:32 + d], len_d, 1,
                      n_cls, P, S, H, mode)
        assert torch.equal(bits(one), bits(g.index_select(0, sel))), "image 1 of the launch != a launch over image 1 alone"
        assert not torch.equal(bits(g[:P]), bits(g[P:2 * P])), "images 0 and 1 have the same prefix gradients"


@pytest.mark.parametrize("name", list(OP_CASES))
def test_prefix_attention_backward_against_the_dense_kernel_f32(name):
    """f32: rpo_text_attn_bwd_dense on the densely gathered copies (the shared prefix d_out in class 0's copy, as
    `_op_reference`) agrees with the new kernel on every suffix row, and its prefix-row outputs summed over the classes in
    float64 agree on the prefix rows -- both within the f32 budget of `close`."""
    from rpo_amd import ops
    mode = "f32"
    H, n_img, P, S, lens = OP_CASES[name]
    n_cls, d, L = len(lens), 64 * H, P + S
    rows, pre, suf = _rows(n_img, n_cls, P, S)
    qkv, dout = _op_inputs(name)
    t, do_w = qkv.to(DEV), dout.to(DEV)
    len_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    g = _launch(t, do_w[:, 32:32 + d], len_d, n_img, n_cls, P, S, H, mode)
    idx = np.empty((n_img, n_cls, L), dtype=np.int64)
    for b in range(n_img):
        for c in range(n_cls):
            idx[b, c, :P] = np.arange(pre(b).start, pre(b).stop)
            idx[b, c, P:] = np.arange(suf(b, c).start, suf(b, c).stop)
    idx_d = torch.from_numpy(idx.reshape(-1)).to(DEV)
    td = t.index_select(0, idx_d).contiguous()
    dd = do_w.index_select(0, idx_d).contiguous().view(n_img, n_cls, L, d + 96)
    dd[:, 1:, :P] = 0
    dd = dd.view(-1, d + 96)
    gd = torch.full((n_img * n_cls * L, 3 * d), float("nan"), dtype=torch.float32, device=DEV)
    ops.text_attn_bwd_dense(td[:, :d], td[:, d:2 * d], td[:, 2 * d:], dd[:, 32:32 + d], gd[:, :d], gd[:, d:2 * d],
                            gd[:, 2 * d:], len_d.repeat(n_img).contiguous(), n_img * n_cls, L, H, 0.125)
    gd = gd.view(n_img, n_cls, L, 3 * d).double().cpu()
    got = g.cpu()
    want_suf = gd[:, :, P:].reshape(n_img * n_cls * S, 3 * d)
    want_pre = gd[:, :, :P].sum(1).reshape(n_img * P, 3 * d)
    for i, nm in enumerate(("dq", "dk", "dv")):
        cs = slice(i * d, (i + 1) * d)
        print(f"\n[prefix vs dense {name} {nm}] suffix rel {relerr(got[n_img * P:, cs], want_suf[:, cs]):.2e} prefix rel "
              f"{relerr(got[:n_img * P, cs], want_pre[:, cs]):.2e} (bound {TOL['f32']})")
        close(got[n_img * P:, cs], want_suf[:, cs], mode, f"{name} {nm} suffix rows vs the dense kernel")
        close(got[:n_img * P, cs], want_pre[:, cs], mode, f"{name} {nm} prefix rows vs the dense kernel's class sum")


@pytest.mark.parametrize("mode", MODES)
def test_prefix_attention_backward_refuses_81_positions(mode):
    from rpo_amd import ops
    from rpo_amd._lib import RPOLibraryError
    P, S, d = 17, 64, 64
    t = rnd((P + S, 3 * d), 5).to(DEV, DT[mode])
    do = rnd((P + S, d), 6).to(DEV, DT[mode])
    g = torch.full((P + S, 3 * d), float("nan"), dtype=DT[mode], device=DEV)
    len_d = torch.tensor([81], dtype=torch.int32, device=DEV)
    with pytest.raises(RPOLibraryError):
        ops.text_attn_bwd_prefix(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], do, g[:, :d], g[:, d:2 * d], g[:, 2 * d:], len_d, 1, 1,
                                 P, S, 1, 0.125)
    torch.cuda.synchronize()
    assert bool(torch.isnan(g.float()).all()), "a refused call wrote to its outputs"


# ============================================================================================ 2. the models (depth 2)

def _gold(name):
    return dict(np.load(os.path.join(GOLDEN, f"ref_{name}.npz")))


@functools.lru_cache(maxsize=None)
def _d2(model="vitb16"):
    from rpo_amd.config import vit_b16, vit_b32
    cfg = (vit_b16 if model == "vitb16" else vit_b32)(layers_v=2, layers_t=2, K=1)
    return cfg, synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))


@pytest.mark.parametrize("tag,model,B,n_ctx", [("coop_d2_b2_ctx16", "vitb16", 2, 16), ("coop_d2_b3_ctx4", "vitb16", 3, 4),
                                               ("coop_vitb32_d2_b3_ctx16", "vitb32", 3, 16)])
@pytest.mark.parametrize("mode", MODES)
def test_coop_shared_prefix_matches_the_reference_trainer(tag, model, B, n_ctx, mode):
    """CoOpCustomCLIP(shared_prefix=True): logits, cross-entropy and d loss / d ctx against the reference's own
    coop.CustomCLIP + backward, at the bounds test_coop_context_training_matches_reference_trainer holds the dense path to;
    the eval branch gives the training call's logits; the same batch again gives the same gradient bits."""
    from rpo_amd.coop import CoOpCustomCLIP
    from rpo_amd.engine_coop import shared_rows
    gold = _gold(tag)
    cfg, sd = _d2(model)
    m = CoOpCustomCLIP(sd, gold["tokenized_prompts"], n_ctx, DEV, DT[mode], max_batch=4, ctx=gold["ctx"], shared_prefix=True)
    image = torch.from_numpy(synth.images(cfg, B)).cuda()
    label = torch.from_numpy(gold["label"]).cuda()
    eng = m.engine
    n_cls = eng.cfg.n_cls
    assert eng.coop_shared and eng.cx[0].shape[0] == shared_rows(1, n_cls, eng.Lmax, n_ctx) < n_cls * eng.Lmax
    logits = eng.coop_forward_backward(image, label).cpu().numpy()
    loss, g = eng.loss.item(), eng.coop_grad.cpu().numpy()
    le, ll, gr = np.abs(logits - gold["logits"]).max(), abs(loss - float(gold["loss"])), _relmax(g, gold["ctx_grad"])
    lt, gt = BOUNDS[mode]
    print(f"\n[coop shared {tag} {mode}] rows {eng.cx[0].shape[0]} (dense {n_cls * eng.Lmax}) logits err {le:.3e} loss err "
          f"{ll:.3e} (bound {lt}) ctx_grad rel {gr:.3e} (bound {gt})")
    assert le <= lt and ll <= lt and gr <= gt
    assert np.array_equal(m(image).cpu().numpy(), logits)                       # eval branch: same logits, no backward
    eng.coop_forward_backward(image, label)
    assert np.array_equal(eng.coop_grad.cpu().numpy(), g)


@pytest.mark.parametrize("tag,B", [("cocoop_d2_b1_ctx4", 1), ("cocoop_d2_b3_ctx4", 3)])
@pytest.mark.parametrize("mode", MODES)
def test_cocoop_shared_prefix_matches_the_reference_trainer(tag, B, mode):
    """CoCoOpCustomCLIP(shared_prefix=True): logits, loss and the five gradients at the bounds of
    test_cocoop_training_matches_reference_trainer."""
    from rpo_amd.coop import CoCoOpCustomCLIP
    gold = _gold(tag)
    cfg, sd = _d2()
    meta = {k: gold[k] for k in ("w1", "b1", "w2", "b2")}
    m = CoCoOpCustomCLIP(sd, gold["tokenized_prompts"], 4, DEV, DT[mode], max_batch=B, ctx=gold["ctx"], meta=meta,
                         shared_prefix=True)
    image = torch.from_numpy(synth.images(cfg, B)).cuda()
    label = torch.from_numpy(gold["label"]).cuda()
    eng = m.engine
    m.prompt_learner.eval()
    logits = m(image).cpu().numpy()
    m.prompt_learner.train()
    loss = m(image, label).item()
    le, ll = np.abs(logits - gold["logits"]).max(), abs(loss - float(gold["loss"]))
    got = dict(ctx=eng.coop_grad, w1=eng.meta_grad[0], b1=eng.meta_grad[1], w2=eng.meta_grad[2], b2=eng.meta_grad[3])
    rel = {k: _relmax(v.cpu().numpy(), gold["g_" + k]) for k, v in got.items()}
    lt, gt = BOUNDS[mode]
    print(f"\n[cocoop shared {tag} {mode}] logits err {le:.3e} loss err {ll:.3e} (bound {lt}) grads rel " +
          " ".join(f"{k} {v:.2e}" for k, v in rel.items()) + f" (bound {gt})")
    assert eng.coop_shared and le <= lt and ll <= lt
    assert all(v <= gt for v in rel.values()), rel


# ---- against the CPU oracle at scale (depth 1): tests/test_gpu_model.py's `_sibling_case` (imported, so that a case's oracle
# runs once for both files) and its `_sibling_bounds`, restated
def _sibling_bounds(act, o_logits, Lmax):
    if act == torch.float32:
        return TOL_F32, TOL_F32, TOL_F32
    la, gr = (F16_LOGIT_ATOL, F16_GRAD_REL) if act == torch.float16 else (BF16_LOGIT_ATOL, BF16_GRAD_REL)
    return la, la * max(1.0, float(np.abs(o_logits).max()) / 8.7) * (2 if Lmax > 64 else 1), gr


@pytest.mark.parametrize("shape", ["coop_397cls", "coop_long_nctx16", "cocoop_100cls_b4"])
@pytest.mark.parametrize("mode", MODES)
def test_shared_prefix_training_against_the_oracle_at_scale(mode, shape):
    """CoOp at 397 classes (n_ctx 4, B 2: class groups of 4 in the attention backward's ordered sum), CoOp with n_ctx 16 on
    prompts of 76 / 65 / 36 / 25 / 71 tokens (P 17, S 59, keys past 64) and CoCoOp at 100 classes x 4 images, loss, logits
    and every gradient against oracle.rpo_oracle at the bounds of `_sibling_bounds`."""
    from rpo_amd.coop import CoCoOpCustomCLIP, CoOpCustomCLIP
    from test_gpu_model import SIB_LONG, SIB_MANY, _sibling_case
    act = DT[mode]
    case = {"coop_397cls": lambda: _sibling_case("coop", "ViT-B/16", SIB_MANY[397], 4, 2),
            "coop_long_nctx16": lambda: _sibling_case("coop", "ViT-B/16", SIB_LONG, 16, 2, "end", False),
            "cocoop_100cls_b4": lambda: _sibling_case("cocoop", "ViT-B/16", SIB_MANY[100], 4, 4)}[shape]()
    cfg, sd, toks, ctx, meta, image, label, o_logits, o_loss, o_g = case
    B = image.shape[0]
    im, lb = torch.from_numpy(image).cuda(), torch.from_numpy(label).cuda()
    if shape.startswith("coop"):
        m = CoOpCustomCLIP(sd, toks, ctx.shape[-2], DEV, act, max_batch=B, ctx=ctx, cfg=cfg, shared_prefix=True)
        eng = m.engine
        logits = eng.coop_forward_backward(im, lb).cpu().numpy()
        loss = eng.loss.item()
        got = dict(ctx=eng.coop_grad.cpu().numpy())
    else:
        m = CoCoOpCustomCLIP(sd, toks, ctx.shape[0], DEV, act, max_batch=B, ctx=ctx, meta=meta, cfg=cfg, shared_prefix=True)
        eng = m.engine
        m.prompt_learner.train()
        loss = m(im, lb).item()
        logits = eng.logits[:B].cpu().numpy()
        got = {k: v.cpu().numpy() for k, v in zip(("ctx", "w1", "b1", "w2", "b2"), [eng.coop_grad] + list(eng.meta_grad))}
    rel = {k: _relmax(v, o_g[k]) for k, v in got.items()}
    le, ll = float(np.abs(logits - o_logits).max()), abs(loss - o_loss)
    lb_loss, lb_logits, gb = _sibling_bounds(act, o_logits, eng.Lmax)
    print(f"\n[shared {shape} {mode}] rows {eng.cx[0].shape[0]} (dense {B * cfg.n_cls * eng.Lmax if 'cocoop' in shape else cfg.n_cls * eng.Lmax}) "
          f"logits err {le:.3e} (bound {lb_logits:.3e}, max |logit| {np.abs(o_logits).max():.2f}) loss err {ll:.3e} (bound "
          f"{lb_loss:.3e}) grads rel " + " ".join(f"{k} {v:.2e}" for k, v in rel.items()) + f" (bound {gb})")
    assert eng.coop_shared and ll <= lb_loss and le <= lb_logits
    assert all(v <= gb for v in rel.values()), rel


# ---- the trainers: shared against dense, graph replay, checkpoints
def _optim():
    from rpo_amd.trainer import OptimConfig
    return OptimConfig(lr=0.002, momentum=0.9, weight_decay=5e-4, warmup_epoch=0, lr_scheduler="constant")


def _trainer(kind, mode, shared, B, **kw):
    from rpo_amd.coop import CoCoOp, CoOp
    cfg, sd = _d2()
    if kind == "coop":
        gold = _gold("coop_d2_b3_ctx4")
        return CoOp(sd, gold["tokenized_prompts"], 4, _optim(), DEV, DT[mode], batch_size=B, num_batches=10 ** 9,
                    ctx=gold["ctx"], shared_prefix=shared, **kw)
    gold = _gold("cocoop_d2_b3_ctx4")
    return CoCoOp(sd, gold["tokenized_prompts"], 4, _optim(), DEV, DT[mode], batch_size=B, num_batches=10 ** 9,
                  ctx=gold["ctx"], meta={k: gold[k] for k in ("w1", "b1", "w2", "b2")}, shared_prefix=shared, **kw)


def _batch(B, step):
    cfg, _ = _d2()
    return {"img": torch.from_numpy(synth.images(cfg, B, seed=70 + step)),
            "label": torch.from_numpy(synth.labels(cfg, B, seed=80 + step))}


@pytest.mark.parametrize("kind,B,steps", [("coop", 3, 3), ("cocoop", 2, 2)])
def test_trainer_steps_shared_prefix_against_dense(kind, B, steps):
    """forward_backward steps of a shared-prefix trainer and a dense one from the same start, f32: the two paths differ
    only in fp32 summation order, so ctx agrees within 2e-7 absolute after each step (the bound
    test_coop_checkpoints_amp_and_cocoop_test_batches holds the dense path's update to against the reference's)."""
    a, b = _trainer(kind, "f32", True, B), _trainer(kind, "f32", False, B)
    assert a.engine.coop_shared and not b.engine.coop_shared
    start = a.engine.coop_ctx.clone()
    for step in range(steps):
        la, lb = a.forward_backward(_batch(B, step))["loss"], b.forward_backward(_batch(B, step))["loss"]
        err = float((a.engine.coop_ctx - b.engine.coop_ctx).abs().max())
        perr = float((a.engine.coop_params - b.engine.coop_params).abs().max())
        print(f"\n[{kind} shared vs dense] step {step + 1}: loss {la:.6f} / {lb:.6f} ctx diff {err:.2e} (bound 2e-7) all "
              f"parameters {perr:.2e}")
        assert abs(la - lb) <= TOL_F32 and err <= 2e-7
    assert float((a.engine.coop_ctx - start).abs().max()) > 0


@pytest.mark.parametrize("kind,B", [("coop", 3), ("cocoop", 2)])
def test_graph_replay_equals_eager_with_shared_prefix(kind, B):
    """use_graph=True (step 0 eager, step 1 captured and replayed, step 2 replayed) against eager launches, bf16: the same
    loss bits over 3 steps and the same parameters."""
    runs = []
    for use_graph in (False, True):
        tr = _trainer(kind, "bf16", True, B, use_graph=use_graph)
        ls = [tr.forward_backward(_batch(B, step))["loss"] for step in range(3)]
        if use_graph:
            assert tr._graph is not None, "the step was not replayed from a graph"
        torch.cuda.synchronize()
        runs.append((np.array(ls), tr.engine.coop_params.clone()))
    (la, pa), (lb, pb) = runs
    print(f"\n[{kind} shared graph] losses {la.tolist()}")
    assert np.isfinite(la).all() and la.tobytes() == lb.tobytes(), f"losses: eager {la.tolist()} vs graph {lb.tolist()}"
    assert torch.equal(pa, pb)


@pytest.mark.parametrize("mode", MODES)
def test_checkpoints_travel_between_the_layouts(mode, tmp_path):
    """A checkpoint of a shared-prefix trainer loads into a dense one and back: the same keys, the same parameters, and the
    same logits within the mode's logit bound (the layout is no part of the state)."""
    B = 3
    a, b = _trainer("coop", mode, True, B), _trainer("coop", mode, False, B)
    a.forward_backward(_batch(B, 0))
    fn = a.save_model(str(tmp_path / "shared"), epoch=1)
    assert set(torch.load(fn, weights_only=True)["state_dict"]) == {"ctx", "token_prefix", "token_suffix"}
    b.load_model(str(tmp_path / "shared"), epoch=1)
    assert torch.equal(b.engine.coop_ctx, a.engine.coop_ctx)
    image = _batch(B, 5)["img"].cuda()
    la, lb = a.model_inference(image), b.model_inference(image)
    lim = BOUNDS[mode][0]
    print(f"\n[checkpoint exchange {mode}] shared vs dense logits {float((la - lb).abs().max()):.3e} (bound {lim})")
    assert float((la - lb).abs().max()) <= lim
    b.forward_backward(_batch(B, 1))
    b.save_model(str(tmp_path / "dense"), epoch=2)
    a.load_model(str(tmp_path / "dense"), epoch=2)
    assert torch.equal(a.engine.coop_ctx, b.engine.coop_ctx)
    assert float((a.model_inference(image) - b.model_inference(image)).abs().max()) <= lim


def test_surface_above_the_engine_with_shared_prefix():
    """What sits above the engine does not know the layout: `amp=True` counts a skipped step and leaves the parameters
    alone, `classifier()` (what `test(features=)` classifies with) gives the dense trainer's text features, and class sets
    -- `class_set` for CoOp, `conditional_class_set` for CoCoOp -- give the dense trainer's logits at the same parameters."""
    B = 3
    new = dict(np.load(os.path.join(GOLDEN, "ref_classset_coop_end.npz")))["tokens"]
    image = _batch(B, 5)["img"].cuda()
    a, b = _trainer("coop", "f32", True, B, amp=True), _trainer("coop", "f32", False, B, amp=True)
    a.forward_backward(_batch(B, 0))
    assert a.skipped_steps == 0
    before = a.engine.coop_params.clone()
    bad = _batch(B, 1)
    bad["img"][0, 0, 0, 0] = float("inf")
    a.forward_backward(bad)
    assert a.skipped_steps == 1 and torch.equal(a.engine.coop_params, before)
    b.engine.coop_ctx.copy_(a.engine.coop_ctx)
    fa, fb = a.classifier()[0], b.classifier()[0]
    rel = relerr(fa, fb.double().cpu())
    la, lb = a.model_inference(image, classes=a.class_set(new)), b.model_inference(image, classes=b.class_set(new))
    print(f"\n[surface coop] classifier() shared vs dense rel {rel:.2e} (bound 2e-5); class-set logits diff "
          f"{float((la - lb).abs().max()):.3e} (bound {TOL_F32})")
    assert tuple(fa.shape) == tuple(fb.shape) and rel <= TOL["f32"]
    assert tuple(la.shape) == (B, new.shape[0]) and float((la - lb).abs().max()) <= TOL_F32
    ca, cb = _trainer("cocoop", "f32", True, 2), _trainer("cocoop", "f32", False, 2)
    ca.forward_backward(_batch(2, 0))
    cb.engine.coop_params.copy_(ca.engine.coop_params)
    for tr in (ca, cb):
        tr.model.prompt_learner.eval()
    la, lb = (tr.model_inference(image, classes=tr.conditional_class_set(new)) for tr in (ca, cb))
    base = float((ca.model_inference(image) - cb.model_inference(image)).abs().max())
    print(f"[surface cocoop] conditional class-set logits diff {float((la - lb).abs().max()):.3e}, built-in classes {base:.3e} "
          f"(bound {TOL_F32})")
    assert tuple(la.shape) == (B, new.shape[0]) and float((la - lb).abs().max()) <= TOL_F32 and base <= TOL_F32
