"""Cached image features on the GPU (rpo_amd/csrc/classify.hip, rpo_amd/features.py):
rpo_features_classify against float64 with a budget written out from its roundings, its predictions against the float64
argmax and against rpo_eval_accumulate's rule, its integer bookkeeping and its bit-level guarantees; `Engine.encode_image`;
`test(features=)`, `train(val_features=)` and `ZeroshotCLIP2.test_templates` against the paths that run the image tower.
Kernel tests: a few hundred tiny launches per case; model tests: depth 2, at most 12 images."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rpo_amd import ops, synth  # noqa: E402
from rpo_amd.config import rn_clip, vit_b16  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
U = 2.0 ** -24
GUARD = 64
NS, CS, ES, SS = (1, 31, 33, 65, 100), (1, 2, 31, 33, 129, 1000), (32, 512, 1024), (1, 3)
FLAGS = ((True, True), (True, False), (False, True), (False, False))


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


# ---- guarded device buffers: operands inside NaN, outputs inside sentinels ----------------------------------------------

def _guarded(host: torch.Tensor, fill):
    """(whole, view): `host` copied into the middle of a device allocation whose other elements are `fill`."""
    n = host.numel()
    whole = torch.full((n + 2 * GUARD,), fill, dtype=host.dtype, device=DEV)
    view = whole[GUARD:GUARD + n].view(host.shape)
    view.copy_(host)
    return whole, view


def _guards_intact(whole, n, fill):
    w = whole.cpu()
    edge = torch.cat([w[:GUARD], w[GUARD + n:]])
    return bool(torch.isnan(edge).all()) if fill != fill else bool((edge == fill).all())


class Call:
    """One rpo_features_classify call on guarded buffers; `run()` launches it and checks that nothing outside the outputs
    changed (the feature buffer's padding columns included)."""

    def __init__(self, f, t, bias, label, scale, nf, nc, ldf=None, want_logits=True):
        n, e = f.shape
        S, C, _ = t.shape
        ldf = e + 4 if ldf is None else ldf
        padded = torch.full((n, ldf), float("nan"), dtype=torch.float32)
        padded[:, :e] = f
        self.f_whole, fv = _guarded(padded, float("nan"))
        self.feat = fv[:, :e]
        self.t_whole, self.cls = _guarded(t.contiguous(), float("nan"))
        self.bias = None if bias is None else _guarded(bias.contiguous(), float("nan"))[1]
        self.label = label.to(DEV)
        self.scale, self.nf, self.nc = scale, nf, nc
        self.n, self.C, self.S, self.e = n, C, S, e
        self.counts_w, self.counts = _guarded(torch.zeros(S, 2, dtype=torch.int64), -7)
        self.cmat_w, self.cmat = _guarded(torch.zeros(S, C * C, dtype=torch.int32), -7)
        self.pred_w, self.pred = _guarded(torch.full((S, n), -3, dtype=torch.int32), -7)
        self.logits_w, self.logits = (None, None) if not want_logits else _guarded(torch.full((S, n, C), -5.0), -7.0)
        self.f_before, self.t_before = self.f_whole.clone(), self.t_whole.clone()

    def run(self):
        logits = self.logits
        ops.features_classify(self.feat, self.cls, self.bias, self.label, self.scale, self.nf, self.nc, self.counts,
                              self.cmat, self.pred, logits)
        torch.cuda.synchronize()
        same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))           # (NaN-safe, on the device)
        assert same(self.f_whole, self.f_before) and same(self.t_whole, self.t_before)
        assert _guards_intact(self.counts_w, self.counts.numel(), -7) and _guards_intact(self.cmat_w, self.cmat.numel(), -7)
        assert _guards_intact(self.pred_w, self.pred.numel(), -7)
        if logits is not None:
            assert _guards_intact(self.logits_w, logits.numel(), -7.0)
        return self

    def rule_pred(self):
        """rpo_eval_accumulate on this call's own logits_out: the evaluator's rule, per classifier."""
        out = torch.empty(self.S, self.n, dtype=torch.int32, device=DEV)
        for s in range(self.S):
            ops.eval_accumulate(self.logits[s], self.label, torch.zeros(2, dtype=torch.int64, device=DEV), None, out[s])
        return out.cpu()


def _counts_want(pred, label, C):
    """numpy integers: (correct, total) and the confusion matrix of one classifier."""
    pred, label = np.asarray(pred), np.asarray(label)
    ok = (label >= 0) & (label < C)
    cm = np.zeros((C, C), dtype=np.int64)
    np.add.at(cm, (label[ok], pred[ok]), 1)
    return [int((ok & (pred == label)).sum()), len(label)], cm


# ---- 1. values against float64 ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _big(e):
    """The largest case at width e -- 100 rows, 3 classifiers of 1000 classes -- and its float64 products, computed once;
    every smaller shape is a slice.  Rows and classes carry scales log-uniform over 1e-2 .. 1e2."""
    g = torch.Generator().manual_seed(9000 + e)
    f = torch.randn(100, e, generator=g) * 10.0 ** (4.0 * torch.rand(100, 1, generator=g) - 2.0)
    t = torch.randn(3, 1000, e, generator=g) * 10.0 ** (4.0 * torch.rand(3, 1000, 1, generator=g) - 2.0)
    bias = torch.randn(3, 1000, generator=g) * 3.0
    f64, t64 = f.double(), t.double()
    dot = torch.einsum("ie,sce->sic", f64, t64)
    mag = torch.einsum("ie,sce->sic", f64.abs(), t64.abs())
    return f, t, bias, dot, mag, f64.norm(dim=-1), t64.norm(dim=-1)


def _reference(e, n, C, S, with_bias, nf, nc, scale):
    """(float64 logits [S, n, C], budget): an fma chain of e terms, (e + 8) 2^-24 a_i r_sc sum_k |f_k| |t_k| (the + 8 covers
    the two norms, each a double sum rounded once, the products a_i r_sc and (a_i r_sc) dot, and the final rounding), plus
    one ulp of the bias."""
    f, t, bias, dot, mag, fn, tn = _big(e)
    a = (scale / fn[:n] if nf else torch.full((n,), float(scale), dtype=torch.float64))[None, :, None]
    r = (1.0 / tn[:S, :C] if nc else torch.ones(S, C, dtype=torch.float64))[:, None, :]
    ref = a * r * dot[:S, :n, :C]
    bud = (e + 8) * U * a * r * mag[:S, :n, :C]
    if with_bias:
        b32 = bias[:S, :C]
        ref = ref + b32.double()[:, None, :]
        bud = bud + torch.from_numpy(np.spacing(b32.abs().numpy())).double()[:, None, :]
    return ref, bud


@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("e", ES)
def test_logits_against_float64(e, S):
    """Every n x C of the issue's shapes, with and without bias, all four norm-flag combinations, ldf > e (a multiple of 4
    and not): each element of logits_out within the written-out budget; pred is the evaluator's rule on these logits."""
    f, t, bias, *_ = _big(e)
    worst = 0.0
    for n in NS:
        for C in CS:
            label = torch.from_numpy(np.random.default_rng(n * 1009 + C).integers(0, C, n))
            for with_bias in (False, True):
                for nf, nc in FLAGS:
                    ldf = e + (3 if (n + C) % 2 else 4)
                    c = Call(f[:n], t[:S, :C], bias[:S, :C] if with_bias else None, label, 100.0, nf, nc, ldf).run()
                    ref, bud = _reference(e, n, C, S, with_bias, nf, nc, 100.0)
                    got = c.logits.cpu().double()
                    assert torch.isfinite(got).all()
                    ratio = float(((got - ref).abs() / bud).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, f"n {n} C {C} e {e} S {S} bias {with_bias} norms {nf, nc}: err / budget {ratio:.3f}"
                    assert torch.equal(c.pred.cpu(), c.rule_pred()), (n, C, with_bias, nf, nc)
    print(f"\n[features_classify e {e} S {S}] worst err / budget {worst:.4f}")


# ---- 2. predictions ---------------------------------------------------------------------------------------------------------

def _cosine64(f, t, scale):
    f64, t64 = f.double(), t.double()
    fn, tn = f64.norm(dim=-1), t64.norm(dim=-1)
    a, r = (scale / fn)[None, :, None], (1.0 / tn)[:, None, :]
    e = f.shape[1]
    ref = a * r * torch.einsum("ie,sce->sic", f64, t64)
    bud = (e + 8) * U * a * r * torch.einsum("ie,sce->sic", f64.abs(), t64.abs())
    return ref, bud


@pytest.mark.parametrize("n,C,e", [(100, 1000, 512), (65, 129, 768), (33, 37, 1024)])
def test_planted_rows_predict_the_float64_argmax(n, C, e):
    """Row i = noise + 0.5 |noise| t_{y_i} (t normalised): the planted class leads by tens of logit units at scale 100, so
    every row must predict the float64 argmax -- no exclusions."""
    g = torch.Generator().manual_seed(n + C + e)
    S = 2
    t = torch.randn(S, C, e, generator=g)
    t = t / t.norm(dim=-1, keepdim=True)
    y = torch.randint(0, C, (n,), generator=g)
    noise = torch.randn(n, e, generator=g)
    f = noise + 0.5 * noise.norm(dim=-1, keepdim=True) * t[0, y]
    ref, _ = _cosine64(f, t[:1], 100.0)
    top2 = ref[0].topk(min(2, C), dim=1).values
    assert (ref[0].argmax(1) == y).all() and float((top2[:, 0] - top2[:, -1]).min()) > 10.0
    c = Call(f, t, None, y, 100.0, True, True).run()
    assert torch.equal(c.pred[0].cpu().long(), y)
    assert c.counts.cpu().tolist()[0] == [n, n]
    assert torch.equal(c.pred.cpu(), c.rule_pred())


@pytest.mark.parametrize("n,C,e,seed", [(100, 1000, 1024, 0), (100, 1000, 512, 1), (65, 129, 768, 2)])
def test_random_rows_predict_the_float64_argmax_outside_the_budget(n, C, e, seed):
    """Rows whose float64 top-2 gap is at most 2 (budget_1 + budget_2) are left out -- at most 5 % of them, asserted on the
    float64 side first; every other row must predict the float64 argmax."""
    g = torch.Generator().manual_seed(seed)
    S = 2
    f, t = torch.randn(n, e, generator=g), torch.randn(S, C, e, generator=g)
    ref, bud = _cosine64(f, t, 100.0)
    top = ref.topk(2, dim=2)
    gap = top.values[..., 0] - top.values[..., 1]
    room = 2.0 * bud.gather(2, top.indices).sum(-1)
    keep = gap > room
    assert float((~keep).double().mean()) <= 0.05, f"{int((~keep).sum())} of {keep.numel()} rows inside the budget"
    c = Call(f, t, None, torch.zeros(n, dtype=torch.int64), 100.0, True, True).run()
    pred = c.pred.cpu().long()
    assert torch.equal(pred[keep], top.indices[..., 0][keep])
    assert torch.equal(c.pred.cpu(), c.rule_pred())


# ---- 3. the rule itself on exact values ---------------------------------------------------------------------------------

def test_rule_on_exact_values_ties_zeros_infinities_and_nan():
    """Small-integer features and classifiers (norms off): every logit is exact in fp32, so logits_out must EQUAL the
    float64 values, and pred must equal torch.max(dim=1) on the CPU and rpo_eval_accumulate on the same logits -- on exact
    ties, +-0, +inf in two columns, an all -inf row, NaN in one and in several columns."""
    g = torch.Generator().manual_seed(5)
    n, C, e = 40, 37, 32
    f = torch.randint(-2, 3, (n, e), generator=g).float()
    t = torch.randint(-1, 2, (1, C, e), generator=g).float()
    t[0, 20] = t[0, 5]
    t[0, 33] = t[0, 5]                                              # exact ties between columns 5, 20, 33 in every row
    f[7] = 0.0                                                      # a row of zeros: every column +-0
    label = torch.randint(0, C, (n,), generator=g)
    inf, nan = float("inf"), float("nan")

    def check(f, t, bias, scale, what):
        c = Call(f, t, bias, label, scale, False, False, ldf=e + 3).run()
        got = c.logits.cpu()
        cpu = torch.max(got[0], dim=1).indices.int()
        assert torch.equal(c.pred[0].cpu(), cpu), what
        assert torch.equal(c.pred.cpu(), c.rule_pred()), what
        return got[0], c.pred[0].cpu()

    # ties and zeros, scale -1 with biases +0 / -0: a zero dot gives -0 under a -0 bias and +0 under a +0 bias
    bias = torch.zeros(1, C)
    bias[0, ::2] = -0.0
    got, pred = check(f, t, bias, -1.0, "ties / zeros")
    want = -(f.double() @ t[0].double().t())
    assert torch.equal(got.double(), want)                          # (-0 == +0 here; the signs are checked next)
    assert torch.equal(torch.signbit(got[7]), torch.signbit(bias[0])) and int(pred[7]) == 0
    tie = got[:, 5] >= got.max(dim=1).values
    assert tie.any() and (pred[tie] <= 5).all() and torch.equal(got[:, 5], got[:, 20])
    # +inf in two columns: the lower one, in every row
    b2 = torch.zeros(1, C)
    b2[0, 19] = b2[0, 7] = inf
    got, pred = check(f, t, b2, 1.0, "+inf")
    assert (pred == 7).all() and torch.isinf(got[:, 19]).all()
    # NaN in one column beats +inf; in several: the lowest
    b3 = b2.clone()
    b3[0, 11] = nan
    _, pred = check(f, t, b3, 1.0, "one NaN")
    assert (pred == 11).all()
    b3[0, 3] = b3[0, 30] = nan
    _, pred = check(f, t, b3, 1.0, "several NaN")
    assert (pred == 3).all()
    # an all -inf row: feature [inf, 0, ...] against classifiers whose first element is -1
    f4, t4 = f.clone(), t.clone()
    f4[9] = 0.0
    f4[9, 0] = inf
    t4[0, :, 0] = -1.0
    got, pred = check(f4, t4, None, 1.0, "-inf row")
    assert (got[9] == -inf).all() and int(pred[9]) == 0
    # a NaN classifier row: that column is NaN in every row
    t5 = t.clone()
    t5[0, 13, 4] = nan
    got, pred = check(f, t5, None, 1.0, "NaN classifier")
    assert torch.isnan(got[:, 13]).all() and (pred == 13).all()


# ---- 4. bookkeeping and the bit-level guarantees --------------------------------------------------------------------------

def test_bookkeeping_accumulates_and_rows_and_classifiers_are_independent():
    g = torch.Generator().manual_seed(44)
    n, n1, C, e, S = 100, 33, 37, 64, 3
    f, t, bias = torch.randn(n, e, generator=g), torch.randn(S, C, e, generator=g), torch.randn(S, C, generator=g)
    label = torch.randint(0, C, (n,), generator=g)
    label[2], label[40], label[99] = -1, C, -1                      # outside [0, C): counted, never correct, no cell
    whole = Call(f, t, bias, label, 50.0, True, True).run()
    pred, logits = whole.pred.cpu(), bits(whole.logits)
    for s in range(S):
        cnt, cm = _counts_want(pred[s].numpy(), label.numpy(), C)
        assert whole.counts[s].cpu().tolist() == cnt
        assert np.array_equal(whole.cmat[s].cpu().numpy().reshape(C, C), cm) and cm.sum() == n - 3
    # the same call again: counts and matrix double, pred and logits repeat bit for bit
    first_counts, first_cmat = whole.counts.cpu().clone(), whole.cmat.cpu().clone()
    whole.run()
    assert torch.equal(whole.counts.cpu(), 2 * first_counts) and torch.equal(whole.cmat.cpu(), 2 * first_cmat)
    assert torch.equal(whole.pred.cpu(), pred) and torch.equal(bits(whole.logits), logits)
    # rows [0, n1) then [n1, n) into the same counters: the bits of one call
    a = Call(f[:n1], t, bias, label[:n1], 50.0, True, True).run()
    b = Call(f[n1:], t, bias, label[n1:], 50.0, True, True)
    b.counts.copy_(a.counts)
    b.cmat.copy_(a.cmat)
    b.run()
    assert torch.equal(torch.cat([a.pred.cpu(), b.pred.cpu()], 1), pred)
    assert torch.equal(torch.cat([bits(a.logits), bits(b.logits)], 1), logits)
    assert torch.equal(b.counts.cpu(), first_counts) and torch.equal(b.cmat.cpu(), first_cmat)
    # classifier s alone: the bits it has among three
    for s in range(S):
        one = Call(f, t[s:s + 1], bias[s:s + 1], label, 50.0, True, True).run()
        assert torch.equal(one.pred.cpu()[0], pred[s]) and torch.equal(bits(one.logits)[0], logits[s])
        assert torch.equal(one.counts.cpu()[0], first_counts[s]) and torch.equal(one.cmat.cpu()[0], first_cmat[s])
    # without logits_out, cmat or pred: the same counts
    c = Call(f, t, bias, label, 50.0, True, True, want_logits=False)
    ops.features_classify(c.feat, c.cls, c.bias, c.label, 50.0, True, True, c.counts)
    torch.cuda.synchronize()
    assert torch.equal(c.counts.cpu(), first_counts) and int(c.cmat.abs().sum()) == 0 and (c.pred.cpu() == -3).all()


# ---- model-level fixtures -------------------------------------------------------------------------------------------------

def _decoded(n, seed):
    from test_gpu_loop import _decoded as d
    return d(n, seed)


def _image_set(n, seed, C):
    from rpo_amd.input_pipeline import DeviceImageSet
    labels = np.random.default_rng(seed + 1).integers(0, C, n).tolist()
    labels[0] = C - 1
    return DeviceImageSet(_decoded(n, seed), labels, DEV)


def _gold(name):
    return dict(np.load(os.path.join(GOLD, name)))


@functools.lru_cache(maxsize=None)
def _vit():
    cfg = vit_b16(layers_v=2, layers_t=2, K=1)
    return cfg, synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))


@functools.lru_cache(maxsize=None)
def _rn():
    cfg = rn_clip((1, 1, 1, 1), 64, 1024, layers_t=2)
    return cfg, synth.rn_clip_state_dict(cfg, seed=0, check=False)


def _same_result(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if k == "confusion_matrix":
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


# ---- 5. encode_image --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("tower", ["vit", "rn"])
def test_encode_image_is_the_plain_pass_and_matches_the_reference(tower, mode):
    """The bits of `img_cls_f` after `forward_plain` on the same batch; against the reference's `image_features` within the
    bounds the plain-CLIP tests use: ViT f32 1e-4 max(1, |max|) (tests/test_gpu_model.py; the 16-bit ViT modes are bounded
    there through the logits only), reduced RN the relative PLAIN_TOL["mini"] of tests/test_gpu_rn.py."""
    from rpo_amd.zeroshot import ZeroshotCLIP
    cfg, sd = _vit() if tower == "vit" else _rn()
    gold = _gold("ref_plainclip_d2_b3.npz" if tower == "vit" else "ref_rn_plainclip_mini_b3.npz")
    m = ZeroshotCLIP(sd, device=DEV, act_dtype=DT[mode], max_batch=4)
    image = torch.from_numpy(synth.images(cfg, 3)).to(DEV)
    m.engine.forward_plain(image)
    want = m.engine.img_cls_f[:3].clone()
    got = m.engine.encode_image(image)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, cfg.embed) and torch.equal(bits(got), bits(want))
    assert got.data_ptr() != m.engine.img_cls_f.data_ptr()
    assert torch.equal(bits(m.engine.encode_image(image.cpu())), bits(want))          # a host batch: moved, same bits
    ref = gold["image_features"]
    err = np.abs(got.cpu().numpy() - ref).max()
    if tower == "vit":
        if mode == "f32":
            assert err <= 1e-4 * max(1.0, np.abs(ref).max())
    else:
        assert err / np.abs(ref).max() <= {"f32": 1e-5, "f16": 1.5e-3, "bf16": 0.013}[mode]


# ---- 6. test(features=) == test() -------------------------------------------------------------------------------------------

def _precondition(tr, F, classes, extra_mag=None):
    """From float64 on the cached features: no row's top-2 gap is inside the budget of either path, summed over the two
    leaders.  The fused kernel's budget is test 1's.  The path through the head kernels gets twice that: the cosine head is
    the same expression with both norms as fp32 sums of e terms (e / 2 roundings each on the norm, so (2 e + 8) 2^-24 in
    all); LP's head is two fp32 chains, z = f W^T + b then z T^T, bounded the same way over `extra_mag`."""
    cls, bias, nf, nc, scale = tr.classifier(classes)
    f64, t64 = F.feat.cpu().double(), cls.cpu().double()
    e = f64.shape[1]
    a = (scale / f64.norm(dim=-1) if nf else torch.full((f64.shape[0],), float(scale), dtype=torch.float64))[:, None]
    r = (1.0 / t64.norm(dim=-1) if nc else torch.ones(t64.shape[0], dtype=torch.float64))[None, :]
    ref = a * r * (f64 @ t64.t())
    bud = (e + 8) * U * a * r * (f64.abs() @ t64.abs().t())
    if bias is not None:
        ref = ref + bias.cpu().double()[None]
        bud = bud + torch.from_numpy(np.spacing(bias.cpu().abs().numpy())).double()[None]
    bud = 2.0 * bud if extra_mag is None else torch.maximum(bud, 2.0 * (e + 8) * U * extra_mag)
    if ref.shape[1] < 2:
        return
    top = ref.topk(2, dim=1)
    gap = top.values[:, 0] - top.values[:, 1]
    room = bud.gather(1, top.indices).sum(-1)
    assert (gap > room).all(), f"a top-2 gap inside the budget: {float((gap - room).min()):.3e}"


def _lp_mag(tr, F, classes):
    """scale (|f| |W|^T + |b|) |T|^T: the magnitude the two fp32 chains of the LP head sum over."""
    eng = tr.engine
    if classes is None:
        T = eng.lp_text_f_n
    else:
        fcs = eng._cs_plain_current(classes)
        T = fcs / fcs.norm(dim=-1, keepdim=True)
    f64 = F.feat.cpu().double().abs()
    z = f64 @ eng.lp_w.cpu().double().abs().t() + eng.lp_b.cpu().double().abs()
    return eng.logit_scale_exp * z @ T.cpu().double().abs().t()


def _two_steps(tr, cfg, B):
    image = torch.from_numpy(synth.images(cfg, B)).to(DEV)
    label = torch.from_numpy(synth.labels(cfg, B)).to(DEV)
    with torch.cuda.device(tr.device):
        for _ in range(2):
            tr.step_async(image, label)
    torch.cuda.synchronize()


def _build(kind, mode):
    """(trainer, tokens of another class set for it)."""
    from lp_fixtures import c1_init
    from rpo_amd.coop import CoOp
    from rpo_amd.lp import LP
    from rpo_amd.zeroshot import ZeroshotCLIP, ZeroshotCLIP2
    cfg, sd = _rn() if kind == "zs_rn" else _vit()
    new = _gold("ref_classset_zeroshot.npz")["tokens"]
    if kind in ("zs", "zs_rn"):
        return ZeroshotCLIP(sd, device=DEV, act_dtype=DT[mode], max_batch=4), new
    if kind == "zs2":
        toks = _gold("ref_zsclip2_d2_b3.npz")["tokens"]
        return ZeroshotCLIP2(sd, toks, DEV, DT[mode], max_batch=4), toks[:3, :7]
    if kind == "coop":
        g = _gold("ref_classset_coop_end.npz")
        tr = CoOp(sd, synth.coop_tokens(synth.oxford_pets_base_tokens(), 4), n_ctx=4, device=DEV, act_dtype=DT[mode],
                  batch_size=4, ctx=g["ctx"])
        _two_steps(tr, tr.cfg, 4)
        return tr, g["tokens"]
    w, b = c1_init(cfg.embed)
    base = _gold("ref_lp_d2_b3.npz")["tokenized_prompts"]
    tr = LP(sd, base, device=DEV, act_dtype=DT[mode], batch_size=4, weight=w, bias=b, max_batch=4)
    _two_steps(tr, tr.cfg, 4)
    return tr, _gold("ref_classset_lp.npz")["tokens"]


@pytest.mark.parametrize("kind,mode", [("zs", "bf16"), ("zs_rn", "f16"), ("zs2", "f32"), ("coop", "f16"), ("lp", "f32")])
def test_test_on_cached_features_returns_the_dict_of_test(kind, mode):
    """12 images in chunks of 4: `test(set, features=F)` == `test(set)`, on the trained classes and on a `ClassSet`, after
    the precondition on the float64 gaps; F is refused by another engine and for another set."""
    from rpo_amd.features import ImageFeatures
    from rpo_amd.zeroshot import ZeroshotCLIP
    tr, new_tokens = _build(kind, mode)
    n = 12
    for classes in (None, tr.class_set(new_tokens)):
        C = tr.cfg.n_cls if classes is None else classes.n
        ds = _image_set(n, 300 + C, C)
        F = ImageFeatures.build(tr, ds, batch_size=4)
        assert tuple(F.feat.shape) == (n, tr.cfg.embed) and F.nbytes() == ImageFeatures.bytes_needed(tr.cfg, n)
        _precondition(tr, F, classes, _lp_mag(tr, F, classes) if kind == "lp" else None)
        want = tr.test(ds, batch_size=4, verbose=False, classes=classes)
        got = tr.test(ds, verbose=False, classes=classes, features=F)
        _same_result(got, want, (kind, mode, classes is not None))
        assert got["total"] == n and got["confusion_matrix"].shape == (C, C)
    # another engine (another storage mode), another set
    other = ZeroshotCLIP((_rn() if kind == "zs_rn" else _vit())[1], device=DEV,
                         act_dtype=DT["f32" if mode != "f32" else "f16"], max_batch=4)
    with pytest.raises(ValueError, match="act_dtype"):
        other.test(ds, verbose=False, features=F)
    with pytest.raises(ValueError, match="n_images"):
        tr.test(_image_set(5, 7, C), verbose=False, classes=classes, features=F)
    with pytest.raises(ValueError, match="budget"):
        ImageFeatures.build(tr, ds, budget_bytes=n * tr.cfg.embed * 4 - 1)


# ---- 7. train(val_features=) ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,mode", [("coop", "f16"), ("lp", "f32")])
def test_train_validates_on_cached_features_without_image_passes(kind, mode):
    from rpo_amd.features import ImageFeatures
    B, epochs = 4, 2
    train_set, val_set = _image_set(8, 500, 19), _image_set(8, 600, 19)
    hist, calls = [], []
    for cached in (True, False):
        tr, _ = _build(kind, mode)
        assert tr.cfg.n_cls == 19
        tr.num_batches = 2
        tr.epoch = tr.batch_idx = 0
        F = ImageFeatures.build(tr, val_set, batch_size=B) if cached else None
        count = [0]
        inner = tr.engine._plain_image_features

        def counted(image, inner=inner, count=count):
            count[0] += 1
            return inner(image)
        tr.engine._plain_image_features = counted
        torch.manual_seed(11)
        h = tr.train(train_set, max_epoch=epochs, val_set=val_set, generator=torch.Generator().manual_seed(3),
                     test_batch_size=B, verbose=False, val_features=F)
        hist.append([r["val_acc"] for r in h])
        calls.append(count[0])
        assert len(h) == epochs
    steps = epochs * 2
    assert calls[0] == steps, f"{calls[0] - steps} validation image passes with val_features"
    assert calls[1] == steps + epochs * (len(val_set) // B)
    assert hist[0] == hist[1]


# ---- 8. test_templates ------------------------------------------------------------------------------------------------------

def test_templates_each_equal_their_own_zeroshot_model():
    from rpo_amd.features import ImageFeatures
    from rpo_amd.zeroshot import ZeroshotCLIP
    m, _ = _build("zs2", "f32")
    toks = _gold("ref_zsclip2_d2_b3.npz")["tokens"]
    T = toks.shape[0]
    ds = _image_set(12, 700, m.cfg.n_cls)
    F = ImageFeatures.build(m, ds, batch_size=4)
    res = m.test_templates(ds, features=F)
    assert len(res) == T + 1
    _same_result(res[-1], m.test(ds, batch_size=4, verbose=False), "ensemble")
    single = ZeroshotCLIP(_vit()[1], toks[0], DEV, torch.float32, max_batch=4)
    for t in range(T):
        single.set_text_features(m.engine.encode_text(toks[t]))
        _same_result(res[t], single.test(ds, batch_size=4, verbose=False), f"template {t}")
    _same_result(m.test_templates(ds)[-1], res[-1], "features built on the fly")
