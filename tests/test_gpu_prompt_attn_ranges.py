"""The multi-set prompt attention (rpo_attn_prompt_fwd / rpo_attn_prompt_bwd, rpo_amd/csrc/attn_image.hip) and the two
paths it serves (the shared evaluation, the shared-batch sweep step) at the value ranges of a TRAINED CLIP.

tests/test_gpu_shared_eval.py and tests/test_gpu_shared_train_ops.py draw N(0, 1) inputs and bound max|err| by
TOL * max|ref|: every score stays within a few units, the running maximum settles in the first key tile, the rescale
factor never underflows and an element below the tensor's maximum is not looked at.  Both kernels have a softmax of
their own -- the forward an online loop with a peeled partial key tile (16-bit) or a masked loop (f32), the backward a
pass that carries the row maximum, the row sum AND delta = sum P o dP online and a second pass that rounds
P o (dP - delta) once -- so they get here what tests/test_gpu_ranges.py gives the single-set kernels: its score patterns
(sink, late peak, early peak, tied maxima, +80, -200, one per head), its float64 reference `attn64` and its per-element
budgets.  Nothing is re-derived: TOL, FLOOR, the budgets and the generator `_fill` are imported from that module.

Op level (seven shapes, each the smallest that reaches one code path; three storage modes; K / V in a packed in-proj
matrix and in a cache): per element against float64; nothing outside the launch's images is read; the invariances the
kernel comments promise (a second launch, a set alone, a permutation of the query rows, a NaN query row) hold bit for
bit at sharp scores.  tests/test_prompt_attn_ranges_host.py runs a float32 emulation of the two arrangements on the
same cases on the CPU: the budgets are attainable, so a failure here points at the kernel.

Model level: the shared-batch step and the shared evaluation on weights pushed into the trained regime
(test_gpu_ranges._trained_like), against OracleRPO at the project's model bounds, beside the standalone engine.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import test_gpu_multi as M
from helpers import TOL_F32, assert_within
from test_gpu_ranges import DT, FLOOR, HD, PATTERNS, TOL, _fill, _trained_like, attn64, block0_regime, q

pytestmark = pytest.mark.gpu

DEV = M.DEV
GUARD = 64
MODES = ("f32", "bf16", "f16")
# (sets, B, H, N, Kp); H = 6: every launch holds the six score patterns, d = 384
SHAPES = [(3, 2, 6, 197, 24),     # NT = 7, a 5-key partial tile, 72 queries: the 32-query tiles mix sets
          (2, 1, 6, 257, 33),     # NT = 9, the last tile holds ONE key, Kp no multiple of 32
          (2, 1, 6, 225, 16),     # the first NT = 9 shape: 8 tiles hold keys, the ninth is skipped
          (1, 2, 6, 288, 8),      # the limit: nine full tiles, no partial one
          (12, 1, 6, 33, 24),     # 9 query tiles for 8 waves (a wave takes a second tile); one full key tile + one key
          (1, 1, 6, 32, 1),       # exactly one full tile, one query
          (1, 1, 6, 5, 3)]        # fewer keys than a tile: the late peak sits in the partial tile
IDS = ["x".join(map(str, s)) for s in SHAPES]
CACHE_IMAGES, FIRST = 4, 1        # the cache layout: [4 N, 2 d], the launch reads images FIRST .. FIRST + B - 1


# ------------------------------------------------------------------------------------------------------------------
# inputs and the float64 reference, shared with the host emulation's test (built once per shape / mode, never changed)
# ------------------------------------------------------------------------------------------------------------------
def image_rows(sets, B, Kp, b):
    """rows of image b's queries in the set-major buffers (row (s B + b) Kp + j), ordered (s, j)"""
    return torch.cat([torch.arange((s * B + b) * Kp, (s * B + b + 1) * Kp) for s in range(sets)])


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """float32: queries [sets B Kp, d], K | V of the launch's B images [B, N, 2 d], da [sets B Kp, d].  Head h of every
    (set, image) follows PATTERNS[h % 6]: `_fill` gets an image's N keys and ALL its sets * Kp queries."""
    sets, B, H, N, Kp = shape
    d = HD * H
    g = torch.Generator().manual_seed(1000 * N + 10 * Kp + sets)
    qr = torch.empty(sets * B * Kp, d)
    kv = torch.randn(B, N, 2 * d, generator=g)                       # (V: N(0, 1))
    da = torch.randn(sets * B * Kp, d, generator=g)
    for b in range(B):
        rows = image_rows(sets, B, Kp, b)
        for h in range(H):
            qh, kh = torch.empty(sets * Kp, HD), torch.empty(N, HD)
            _fill(qh, kh, PATTERNS[h % len(PATTERNS)], g)
            qr[rows, h * HD:(h + 1) * HD] = qh
            kv[b, :, h * HD:(h + 1) * HD] = kh
    return qr, kv, da


@functools.lru_cache(maxsize=None)
def reference(shape, mode):
    """float64 out / dq of the values the kernels read in `mode`, with attn64's per-element budgets"""
    sets, B, H, N, Kp = shape
    d = HD * H
    qr, kv, da = (q(t, mode) for t in inputs(shape))
    r = {k_: torch.empty(sets * B * Kp, d, dtype=torch.float64) for k_ in ("out", "b_out", "dq", "b_dq")}
    pmax = 0.0
    for b in range(B):
        rows = image_rows(sets, B, Kp, b)
        a = attn64(qr[rows], kv[b, :, :d], kv[b, :, d:], H, TOL[mode], do=da[rows])
        for k_ in r:
            r[k_][rows] = a[k_]
        pmax = max(pmax, float(a["p"].amax(-1).max()))
    assert pmax > 0.999                                              # the rows are as sharp as intended
    return r


# ------------------------------------------------------------------------------------------------------------------
# launches
# ------------------------------------------------------------------------------------------------------------------
def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _wide(t, ld, dtype):
    """t [R, d] as the first d columns of a [R, ld] device matrix whose padding columns are NaN (nothing may read them)"""
    w = _nan((t.shape[0], ld), dtype)
    w[:, :t.shape[1]] = t.to(DEV, dtype)
    return w


def _guarded(rows, ld, dtype):
    whole = _nan((rows * ld + 2 * GUARD,), dtype)
    return whole, whole[GUARD:GUARD + rows * ld].view(rows, ld)


def _layouts(shape, mode, poison=False):
    """(name, matrix, column of K, first_image, image 0's row) of the two K / V layouts, holding the SAME K / V values.
    poison: NaN in everything the launch must not read -- the cache rows of the images outside FIRST .. FIRST + B - 1; in
    the packed matrix the K / V columns of the prompt rows B N .. and the q columns of every row."""
    sets, B, H, N, Kp = shape
    d, dt = HD * H, DT[mode]
    kv = inputs(shape)[1]
    g = torch.Generator().manual_seed(7)
    packed = torch.randn(B * (N + Kp), 3 * d, generator=g)
    packed[:B * N, d:] = kv.reshape(B * N, 2 * d)
    cache = torch.randn(CACHE_IMAGES * N, 2 * d, generator=g)
    cache[FIRST * N:(FIRST + B) * N] = kv.reshape(B * N, 2 * d)
    if poison:
        packed[B * N:, d:] = float("nan")
        packed[:, :d] = float("nan")
        cache[:FIRST * N] = float("nan")
        cache[(FIRST + B) * N:] = float("nan")
    first = torch.tensor([FIRST], dtype=torch.int32, device=DEV)
    return [("packed", packed.to(DEV, dt), d, None), ("cache", cache.to(DEV, dt), 0, first)]


def _launch(shape, mode, layout, q_dev, da_dev, sets=None):
    """one forward and one backward launch into NaN-filled, guarded outputs with ldo / lddq != d; returns (out, dq) [R, d]
    after checking that the guards and the padding columns are still NaN"""
    from rpo_amd import ops
    _, B, H, N, Kp = shape
    sets = shape[0] if sets is None else sets
    name, kv, c0, fi = layout
    d, dt, R = HD * H, DT[mode], sets * B * Kp
    k, v = kv[:, c0:c0 + d], kv[:, c0 + d:c0 + 2 * d]
    w_out, out = _guarded(R, d + 16, dt)
    w_dq, dq = _guarded(R, d + 40, dt)
    ops.attn_prompt_fwd(q_dev, k, v, out, B, H, N, Kp, sets, first_image=fi)
    ops.attn_prompt_bwd(q_dev, k, v, da_dev, dq, B, H, N, Kp, sets, first_image=fi)
    torch.cuda.synchronize()
    for what, whole, t in (("out", w_out, out), ("dq", w_dq, dq)):
        w = whole.float()
        assert bool(torch.isnan(w[:GUARD]).all()) and bool(torch.isnan(w[-GUARD:]).all()), f"{name}: guards of {what} written"
        assert bool(torch.isnan(t[:, d:].float()).all()), f"{name}: padding columns of {what} written"
    return out[:, :d], dq[:, :d]


def _operands(shape, mode):
    """queries and da on the device with ldq / ldda != d"""
    d = HD * shape[2]
    qr, _, da = inputs(shape)
    return _wide(qr, d + 8, DT[mode]), _wide(da, d + 24, DT[mode])


same = M.same


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_attn_prompt_sharp_scores_against_float64(shape, mode):
    """Forward and backward per element against float64 within attn64's b_out / b_dq (TOL and FLOOR of the mode), in both
    K / V layouts -- which hold the same values, so they must also give the same bits.  The dq budget was derived for
    kernels that round P and P o dP separately; this kernel rounds P o (dP - delta) once and sits inside it."""
    ref = reference(shape, mode)
    q_dev, da_dev = _operands(shape, mode)
    got = []
    for layout in _layouts(shape, mode):
        out, dq = _launch(shape, mode, layout, q_dev, da_dev)
        what = f"attn prompt {layout[0]} {mode} " + "x".join(map(str, shape))
        wf = assert_within(out, ref["out"], ref["b_out"], what + " fwd", floor=FLOOR[mode])
        wb = assert_within(dq, ref["dq"], ref["b_dq"], what + " bwd", floor=FLOOR[mode])
        print(f"[{what}] worst err / budget fwd {wf:.3f} bwd {wb:.3f}")
        got.append((out, dq))
    assert same(got[0][0], got[1][0]) and same(got[0][1], got[1][1]), "the packed and the cache layout differ"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_attn_prompt_reads_nothing_outside_the_launch(shape, mode):
    """NaN in every cache row outside images first .. first + B - 1, in the K / V columns of the packed matrix's prompt
    rows and in its q columns: both kernels' results stay finite and keep the unpoisoned launch's bits."""
    q_dev, da_dev = _operands(shape, mode)
    for clean, bad in zip(_layouts(shape, mode), _layouts(shape, mode, poison=True)):
        out, dq = _launch(shape, mode, clean, q_dev, da_dev)
        out_p, dq_p = _launch(shape, mode, bad, q_dev, da_dev)
        assert bool(torch.isfinite(out_p.float()).all()) and bool(torch.isfinite(dq_p.float()).all()), clean[0]
        assert same(out_p, out), f"{clean[0]}: fwd read rows outside the launch's images"
        assert same(dq_p, dq), f"{clean[0]}: bwd read rows outside the launch's images"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_attn_prompt_invariances_at_sharp_scores(shape, mode):
    """What the kernel comments promise, for both kernels and both layouts, on the sharp-score inputs: a second launch
    gives the same bits; set s of a multi-set launch has the bits of its own launch; permuting the Kp query rows of one
    image within one set permutes that image's output rows bit for bit; a NaN query row (and its da row) leaves every
    other row's bits alone and comes out non-finite itself."""
    sets, B, H, N, Kp = shape
    d, R = HD * H, sets * B * Kp
    q_dev, da_dev = _operands(shape, mode)
    for layout in _layouts(shape, mode):
        name = layout[0]
        out, dq = _launch(shape, mode, layout, q_dev, da_dev)
        assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dq.float()).all())
        out2, dq2 = _launch(shape, mode, layout, q_dev, da_dev)
        assert same(out2, out) and same(dq2, dq), f"{name}: a second launch gave other bits"
        if sets > 1:
            for s in range(sets):
                rows = slice(s * B * Kp, (s + 1) * B * Kp)
                o1, g1 = _launch(shape, mode, layout, q_dev[rows], da_dev[rows], sets=1)
                assert same(o1, out[rows]) and same(g1, dq[rows]), f"{name}: set {s} of {sets} != its own launch"
            assert not same(out[:B * Kp], out[B * Kp:2 * B * Kp])               # (the sets really differ)
        # the query rows of the last image in the last set, permuted
        r0 = ((sets - 1) * B + B - 1) * Kp
        if Kp > 1:
            perm = torch.randperm(Kp, generator=torch.Generator().manual_seed(Kp)).to(DEV)
            qp, dp = q_dev.clone(), da_dev.clone()
            qp[r0:r0 + Kp], dp[r0:r0 + Kp] = q_dev[r0 + perm], da_dev[r0 + perm]
            o1, g1 = _launch(shape, mode, layout, qp, dp)
            assert same(o1[r0:r0 + Kp], out[r0 + perm]) and same(g1[r0:r0 + Kp], dq[r0 + perm]), f"{name}: permuted rows"
            assert same(o1[:r0], out[:r0]) and same(g1[:r0], dq[:r0]), f"{name}: the permutation reached other rows"
        # one NaN query row in the middle of the launch (a 32-query tile it shares with rows of other sets where sets > 1)
        bad = R // 2
        qn, dn = q_dev.clone(), da_dev.clone()
        qn[bad, :d], dn[bad, :d] = float("nan"), float("nan")
        o1, g1 = _launch(shape, mode, layout, qn, dn)
        keep = torch.arange(R, device=DEV) != bad
        assert same(o1[keep], out[keep]) and same(g1[keep], dq[keep]), f"{name}: a NaN query row reached other rows"
        assert not bool(torch.isfinite(o1[bad].float()).any()) and not bool(torch.isfinite(g1[bad].float()).any()), \
            f"{name}: the NaN query row came out finite"


# ------------------------------------------------------------------------------------------------------------------
# model level: the shared-batch step and the shared evaluation in the trained regime
# ------------------------------------------------------------------------------------------------------------------
DEPTH, KMAX, B_MODEL = 2, 24, 4
MEMBER_K = (24, 8, 16)
# (mode, K_s) at which the STANDALONE Engine(K_s) -- the single-run path, no prompt kernel in it -- leaves the bf16
# gradient bound of 5e-2 against the oracle on these weights, measured g_text rel | g_img rel:
#   K = 8    standalone 5.05e-2 | 5.21e-2, shared path 5.05e-2 | 5.61e-2, the two paths 0 | 1.0e-2 apart
#   K = 16   standalone 2.27e-2 | 5.42e-2, shared path 2.25e-2 | 5.48e-2, the two paths 1.7e-3 | 1.0e-2 apart
# (K = 24: 2.76e-2 | 4.43e-2 and 2.74e-2 | 4.39e-2, inside).  It is the regime's limit at bf16 storage, not the shared
# path's: those members are held to the standalone engine at the same bounds, the others -- and every member in f32 and
# f16 -- to the oracle ("Prompt attention at trained ranges").
REGIME_LIMITED = {("bf16", 8), ("bf16", 16)}


def _cfg(K):
    return M._workload(DEPTH, K)[0]


@functools.lru_cache(maxsize=None)
def _trained():
    """test_gpu_multi's depth-2 weights pushed into the trained regime, on a PRIVATE copy of the state dict"""
    cfg, sd, toks = M._workload(DEPTH, KMAX)
    sd = copy.deepcopy(sd)
    _trained_like(sd, cfg)
    return sd, toks


def _batch():
    """the ONE batch: member 0's images and labels of tests/test_gpu_multi.py"""
    _, image, label = M._member(_cfg(KMAX), _trained()[0], 0, B_MODEL)
    return image, label


def _prompts(s, K):
    return M._member(_cfg(K), _trained()[0], s, B_MODEL)[0]


@functools.lru_cache(maxsize=None)
def _oracle(s, K):
    """OracleRPO(K) on the trained-like weights with member s's prompts and the shared batch: logits, loss, both prompt
    gradients, and the regime of its block 0"""
    from oracle.rpo_oracle import OracleRPO
    sd, toks = _trained()
    cfg = _cfg(K)
    image, label = _batch()
    ref = OracleRPO(sd, toks, K, cfg.patch)
    ref.set_prompts(*_prompts(s, K))
    regime = block0_regime(ref, cfg, image)
    out, gt, gi = ref.loss_and_grads(image, label)
    return out.logits.detach().numpy(), float(out.loss.detach()), gt.numpy(), gi.numpy(), regime


def _assert_regime(s, K):
    big, xmax, sharp = _oracle(s, K)[4]
    print(f"\n[prompt paths, trained regime] oracle member {s} K={K}, block 0: {big} residual channels above 100, max |x| "
          f"{xmax:.1f}; {100 * sharp:.1f} % of attention rows with a max weight above 0.9")
    assert big >= 1 and sharp > 0.0


def _errors(logits, loss, gt, gi, ref):
    return (float(np.abs(logits - ref[0]).max()), abs(loss - ref[1]), M._relmax(gt, ref[2]), M._relmax(gi, ref[3]))


def _inside(errs, mode):
    lt, gr = M.BOUNDS[mode]
    return errs[0] <= lt and errs[1] <= lt and errs[2] <= gr and errs[3] <= gr


@pytest.mark.parametrize("mode", MODES)
def test_shared_batch_step_in_trained_regime(mode):
    """Engine K = 24, members K = (24, 8, 16) with their own prompts on ONE batch of 4, depth 2, on trained-like weights
    (the oracle's block 0 shows the regime first).  Every member's logits, loss and prompt gradients (used rows) against
    OracleRPO(K_s) at test_gpu_multi.BOUNDS; gradient rows i >= K_s exact zeros.  Beside it a standalone Engine(K_s) --
    the single-run path, which does not use the prompt kernels -- on the same weights, prompts and batch: its errors
    against the oracle are printed next to the shared path's, and in f32 the two paths agree within TOL_F32 / 100.
    The (mode, K_s) of REGIME_LIMITED, where the STANDALONE engine leaves a bound, are held to the standalone engine."""
    from rpo_amd.engine import Engine
    from rpo_amd.sweep import member_row_to_flat
    from test_gpu_sweep import all_zero_bits
    sd, toks = _trained()
    cfg, B, S = _cfg(KMAX), B_MODEL, len(MEMBER_K)
    _assert_regime(0, KMAX)
    eng = Engine(cfg, sd, toks, torch.device(DEV), DT[mode], max_batch=B)
    eng.params.zero_()
    eng.prompt_train_setup(S, B, member_K=list(MEMBER_K))
    for s, k in enumerate(MEMBER_K):
        tp, ip = _prompts(s, k)
        eng.m_text_prompt[s, :k] = torch.from_numpy(tp).to(DEV)
        eng.m_img_prompt[s, :k] = torch.from_numpy(ip).to(DEV)
    im, lb = _batch()
    image, label = torch.from_numpy(im).to(DEV), torch.from_numpy(lb).to(DEV)
    eng.shared_forward_backward(image, label)
    torch.cuda.synchronize()
    lt, gr = M.BOUNDS[mode]
    for s, k in enumerate(MEMBER_K):
        ref = _oracle(s, k)
        logits, loss = eng.m_logits[s * B:(s + 1) * B].cpu().numpy(), float(eng.m_loss[s])
        gt, gi = eng.m_g_text[s, :k].cpu().numpy(), eng.m_g_img[s, :k].cpu().numpy()
        assert np.isfinite(logits).all() and np.isfinite(gt).all() and np.isfinite(gi).all() and np.isfinite(loss)
        assert all_zero_bits(eng.m_g_text[s, k:]) and all_zero_bits(eng.m_g_img[s, k:]), f"member {s}: inert gradient rows"
        solo = Engine(_cfg(k), sd, toks, torch.device(DEV), DT[mode], max_batch=B)
        solo.params.copy_(member_row_to_flat(eng.m_params[s], KMAX, k, cfg.d_t, cfg.d_v))
        solo.forward_backward(image, label)
        torch.cuda.synchronize()
        s_logits, s_loss = solo.logits[:B].cpu().numpy(), float(solo.loss)
        s_gt, s_gi = solo.g_text.cpu().numpy(), solo.g_img.cpu().numpy()
        e_sh, e_so = _errors(logits, loss, gt, gi, ref), _errors(s_logits, s_loss, s_gt, s_gi, ref)
        e_ps = _errors(logits, loss, gt, gi, (s_logits, s_loss, s_gt, s_gi))
        fmt = lambda e: f"logits {e[0]:.3e} loss {e[1]:.3e} g_text rel {e[2]:.3e} g_img rel {e[3]:.3e}"
        print(f"[shared step, trained regime {mode}] member {s} K={k} (max |logit| {np.abs(ref[0]).max():.1f}, bounds {lt} / {gr})\n"
              f"    shared vs oracle     {fmt(e_sh)}\n    standalone vs oracle {fmt(e_so)}\n    shared vs standalone {fmt(e_ps)}")
        if (mode, k) in REGIME_LIMITED:
            assert _inside(e_ps, mode), f"member {s}: shared vs standalone {fmt(e_ps)}"
        else:
            assert _inside(e_sh, mode), f"member {s}: shared vs oracle {fmt(e_sh)} (standalone: {fmt(e_so)})"
        if mode == "f32":
            dmax = max(float(np.abs(logits - s_logits).max()), abs(loss - s_loss), float(np.abs(gt - s_gt).max()),
                       float(np.abs(gi - s_gi).max()))
            print(f"    f32 shared vs standalone: worst |diff| {dmax:.3e} (bound {TOL_F32 / 100:.1e})")
            assert dmax <= TOL_F32 / 100
        del solo


@pytest.mark.parametrize("mode", MODES)
def test_shared_evaluation_in_trained_regime(mode):
    """RPOMulti.model_inference_all, S = 3 members (K = 24) on one batch of 4, on the trained-like weights: member s's
    slice within the logit bound of OracleRPO on that member; the per-member path beside it.  A FrozenImageKV of a set of
    mixed-size images (chunks 4, 1) gives `test_all` the bits of the live frozen pass."""
    from rpo_amd.frozen_kv import FrozenImageKV
    from rpo_amd.multi import RPOMulti
    from test_gpu_shared_eval import _collect, _image_set
    sd, toks = _trained()
    cfg, B, S = _cfg(KMAX), B_MODEL, 3
    _assert_regime(0, KMAX)
    tr = RPOMulti(cfg, sd, toks, n_runs=S, batch_size=B, prompts=[_prompts(s, KMAX) for s in range(S)], device=DEV,
                  act_dtype=DT[mode], num_batches=10 ** 9)
    image = torch.from_numpy(_batch()[0]).to(DEV)
    allm = tr.model_inference_all(image)
    assert tuple(allm.shape) == (S, B, cfg.n_cls) and bool(torch.isfinite(allm).all())
    assert M.same(allm, tr.model_inference_all(image)), "second call"
    lt = M.BOUNDS[mode][0]
    for s in range(S):
        ref = _oracle(s, KMAX)[0]
        err = float(np.abs(allm[s].cpu().numpy() - ref).max())
        one = float(np.abs(tr.model_inference(image, member=s).cpu().numpy() - ref).max())
        print(f"[shared eval, trained regime {mode}] member {s}: logits err vs oracle {err:.3e} (per-member path {one:.3e}, "
              f"bound {lt}, max |logit| {np.abs(ref).max():.1f})")
        assert err <= lt, f"member {s}: logits err {err:.3e} (per-member path {one:.3e})"
    assert not M.same(allm[0], allm[1])
    n = 5
    ds, _, _ = _image_set(n, 61)
    assert tr.engine.max_batch > B                                   # (so batch_size = B is what cuts the chunks)
    cache = FrozenImageKV.build(tr.engine, ds, batch_size=B)
    _, live = _collect(tr.test_all, n, image_set=ds, batch_size=B)
    _, cached = _collect(tr.test_all, n, image_set=ds, batch_size=B, frozen=cache)
    assert tuple(live.shape) == (S, n, cfg.n_cls) and bool(torch.isfinite(live).all())
    assert M.same(live, cached), "cache != live path"
