"""The multi-run RPO step on the device (rpo_amd/multi.py, rpo_amd/engine_multi.py, the "ABI 8 additions" of
include/rpo_amd.h).

Op level: every grouped entry point against the existing single-run entry point it generalises, BIT FOR BIT, with guard
regions around the outputs and each call run twice.  Model level: every member against `oracle.rpo_oracle.OracleRPO` run
on that member alone, at the project's model bounds (tests/helpers.py); in f32 also against a standalone `Engine`; three
SGD steps against standalone `RPO` trainers; isolation of the members from each other; graph replay against eager
launches across a learning-rate change; the single-run engine untouched; the epoch loop, evaluation and checkpoints.
"""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import BF16_GRAD_REL, BF16_LOGIT_ATOL, F16_GRAD_REL, F16_LOGIT_ATOL, TOL_F32
from rpo_amd import synth
from rpo_amd.config import vit_b16

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
GUARD = 64


def bits(t):
    t = t.detach().contiguous()
    if t.element_size() == 2:
        return t.view(torch.int16).cpu()
    return t.view(torch.int32).cpu()


def same(a, b):
    return torch.equal(bits(a), bits(b))


def guarded(shape, dtype, fill=float("nan")):
    """(whole, inner): a contiguous tensor of `shape` with GUARD sentinel elements on either side."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def guards_intact(whole):
    w = whole.detach().cpu()
    lo, hi = w[:GUARD], w[-GUARD:]
    ok = lambda g: bool(torch.isnan(g.float()).all()) if w.dtype.is_floating_point else bool((g == -7).all())
    return ok(lo) and ok(hi)


def rnd(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


# ===================================================================================================== op level

@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("S,ipg,N,Kp,d", [(3, 4, 197, 24, 768), (8, 1, 50, 7, 768), (1, 5, 17, 3, 512), (2, 3, 10, 24, 1024)])
def test_grouped_embedding_equals_single_calls(mode, S, ipg, N, Kp, d):
    """Image b takes its prompt rows from set b // ipg: row by row the bits of rpo_img_embed_norm_rows called with that
    set's prompt.  The sets are column blocks of a wider buffer (strided), as the trainer's parameter buffer is.
    Mutant: the set index computed from the prompt ROW ((row - B N) / ipg) instead of the image fails this test."""
    from rpo_amd import ops
    B = S * ipg
    R = B * (N + Kp)
    x_pre0 = rnd((R, d), 1)
    cls, pos = rnd((d,), 2), rnd((N, d), 3)
    wide = rnd((S, 40 + Kp * d), 4)                              # [S, other | prompt]: set stride 40 + Kp * d floats
    prompts = wide[:, 40:].unflatten(1, (Kp, d))
    g_pre, b_pre, g1, b1 = rnd((d,), 5), rnd((d,), 6, 0.1), rnd((d,), 7), rnd((d,), 8, 0.1)

    def run(fn, rows):
        x_pre = x_pre0.clone()
        w0, x0 = guarded((R, d), torch.float32)
        wh, h = guarded((R, d), DT[mode])
        fn(x_pre, x0, h, rows)
        torch.cuda.synchronize()
        assert guards_intact(w0) and guards_intact(wh)
        return x_pre, x0, h

    grouped = lambda x_pre, x0, h, rows: ops.img_embed_norm_grouped(x_pre, cls, pos, prompts, g_pre, b_pre, x0, g1, b1, h, B, N,
                                                                    Kp, ipg, rows=rows)
    for rows in (None, (B * N, R), (B * N + Kp, R - Kp) if B > 2 else (0, R)):
        got = run(grouped, rows)
        again = run(grouped, rows)
        assert all(same(a, b) or bool(torch.isnan(a.float()).any()) for a, b in zip(got, again))
        r0, r1 = rows or (0, R)
        for s in range(S):
            single = lambda x_pre, x0, h, rows_: ops.img_embed_norm(x_pre, cls, pos, prompts[s].contiguous(), g_pre, b_pre, x0,
                                                                    g1, b1, h, B, N, Kp, rows=rows_)
            ref = run(single, rows)
            p0, p1 = B * N + s * ipg * Kp, B * N + (s + 1) * ipg * Kp        # this set's prompt rows
            lo, hi = max(p0, r0), min(p1, r1)
            for a, b, what in zip(got, ref, ("x_pre", "x0", "h")):
                if hi > lo:
                    assert same(a[lo:hi], b[lo:hi]), f"set {s} prompt rows, {what}, rows={rows}"
                f0, f1 = r0, min(B * N, r1)
                if f1 > f0:
                    assert same(a[f0:f1], b[f0:f1]), f"frozen rows, {what}"
        # rows outside [r0, r1) are untouched
        if rows is not None:
            assert bool(torch.isnan(got[1][:r0].float()).all()) and bool(torch.isnan(got[1][r1:].float()).all())
    assert not same(prompts[0], prompts[-1]) or S == 1


@pytest.mark.parametrize("rows", [24, 70])
@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
def test_shared_cache_text_attention_equals_replicated_cache(mode, rows):
    """n_cls = S * n_kv virtual classes on ONE cache, forward and backward: the bits of the existing calls on a cache and
    `len` replicated S times.  16-bit with rows <= 64: the one-wave MFMA kernels; f32 or rows > 64: the VALU kernels.
    Mutant: `v % n_kv` dropped in the BACKWARD kernels only fails the dq half of this test."""
    from rpo_amd import ops
    H, dt = 8, DT[mode]
    d = H * 64
    for Lmax in (64, 77):
        for n_kv in (1, 19, 100):
            len_np = np.array([1 + (7 * c + 3) % Lmax for c in range(n_kv)], dtype=np.int32)
            len_np[0] = Lmax
            lens = torch.from_numpy(len_np).to(DEV)
            kv = rnd((n_kv * Lmax, 2 * d), 10 + n_kv, 0.5, dt)
            for S in (1, 3, 8):
                n = S * n_kv
                q = rnd((n * rows, d), 20 + S, 0.5, dt)
                da = rnd((n * rows, d), 30 + S, 0.5, dt)
                kv_rep, len_rep = kv.repeat(S, 1), lens.repeat(S)
                res = []
                for rep in range(2):
                    wo, out = guarded((n * rows, d), dt)
                    wq, dq = guarded((n * rows, d), dt)
                    ops.text_attn_fwd_shared(q, kv[:, :d], kv[:, d:], out, lens, n, n_kv, rows, Lmax, H)
                    ops.text_attn_bwd_shared(q, kv[:, :d], kv[:, d:], da, dq, lens, n, n_kv, rows, Lmax, H)
                    torch.cuda.synchronize()
                    assert guards_intact(wo) and guards_intact(wq)
                    res.append((out, dq))
                ref_out, ref_dq = torch.empty_like(q), torch.empty_like(q)
                ops.text_attn_fwd(q, kv_rep[:, :d], kv_rep[:, d:], ref_out, len_rep, n, rows, Lmax, H, causal=False)
                ops.text_attn_bwd(q, kv_rep[:, :d], kv_rep[:, d:], da, ref_dq, len_rep, n, rows, Lmax, H)
                torch.cuda.synchronize()
                what = f"{mode} rows {rows} Lmax {Lmax} n_kv {n_kv} S {S}"
                assert bool(torch.isfinite(ref_out.float()).all()) and bool(torch.isfinite(ref_dq.float()).all()), what
                assert same(res[0][0], ref_out), f"forward: {what}"
                assert same(res[0][1], ref_dq), f"backward: {what}"
                assert same(res[0][0], res[1][0]) and same(res[0][1], res[1][1]), f"second run: {what}"
                if S > 1 and n_kv > 1:                           # the sets really differ (a kernel reading set 0's q would show)
                    assert not same(res[0][0][:n_kv * rows], res[0][0][n_kv * rows:2 * n_kv * rows])


HEAD_CASES = [(C, B) for C in (1, 19, 128, 129, 1000) for B in (1, 4, 32)]


@pytest.mark.parametrize("C,B", HEAD_CASES)
def test_grouped_head_equals_single_calls(C, B):
    """Group s pairs images [sB, (s+1)B) with text features [sC, (s+1)C) only; per group the bits of rpo_head_fwd_bwd[_act]
    on the slices, in both class-count regimes (<= 128: two launches; above: the matrix-pipe path), training and eval
    form, with an out-of-range label in ONE group only.
    Mutants: pairing group s with text group 0, and the loss averaged over S * B, both fail this test."""
    from rpo_amd import ops
    K, e = (24, 512) if (C, B) in ((19, 4), (129, 4)) else (5, 512)
    for S, act in ((3, None), (8, torch.bfloat16)) if C <= 129 else ((3, torch.float16),):
        img = rnd((S * B, K, e), 100 + C + B)
        txt = rnd((S * C, K, e), 200 + C + B)
        label = torch.from_numpy(np.random.default_rng(C * 100 + B).integers(0, C, S * B)).to(DEV)
        bad = 1                                                   # this group's first label is out of range
        label[bad * B] = C + 3
        wsn = ops.head_workspace_floats(B, C, K, e)

        def grouped(lab):
            o = dict(logits=guarded((S * B, C), torch.float32), loss=guarded((S,), torch.float32),
                     d_img=guarded((S * B, K, e), torch.float32), d_txt=guarded((S * C, K, e), torch.float32),
                     ws=guarded((S * wsn,), torch.float32))
            if act is not None:
                o["a_img"], o["a_txt"] = guarded((S * B, K, e), act), guarded((S * C, K, e), act)
            ops.head_fwd_bwd_grouped(img, txt, lab, 100.0, o["logits"][1], o["loss"][1] if lab is not None else None,
                                     o["d_img"][1] if lab is not None else None, o["d_txt"][1] if lab is not None else None,
                                     o["ws"][1], S, **({} if act is None or lab is None else
                                                       dict(d_img_f_act=o["a_img"][1], d_text_f_act=o["a_txt"][1])))
            torch.cuda.synchronize()
            for k, (whole, _) in o.items():
                assert guards_intact(whole), f"guard of {k} (C {C} B {B} S {S})"
            return {k: v[1] for k, v in o.items()}

        got, again = grouped(label), grouped(label)
        ev = grouped(None)
        assert bool(torch.isnan(ev["loss"]).all()) and bool(torch.isnan(ev["d_img"]).all()) and bool(torch.isnan(ev["d_txt"]).all())
        for s in range(S):
            i0, i1, t0, t1 = s * B, (s + 1) * B, s * C, (s + 1) * C
            r = dict(logits=torch.empty(B, C, device=DEV), loss=torch.empty(1, device=DEV),
                     d_img=torch.empty(B, K, e, device=DEV), d_txt=torch.empty(C, K, e, device=DEV))
            kw = {}
            if act is not None:
                r["a_img"], r["a_txt"] = torch.empty(B, K, e, dtype=act, device=DEV), torch.empty(C, K, e, dtype=act, device=DEV)
                kw = dict(d_img_f_act=r["a_img"], d_text_f_act=r["a_txt"])
            ws = torch.empty(wsn, device=DEV)
            ops.head_fwd_bwd(img[i0:i1].contiguous(), txt[t0:t1].contiguous(), label[i0:i1].contiguous(), 100.0, r["logits"],
                             r["loss"], r["d_img"], r["d_txt"], ws, **kw)
            torch.cuda.synchronize()
            what = f"C {C} B {B} S {S} group {s}"
            assert same(got["logits"][i0:i1], r["logits"]) and same(ev["logits"][i0:i1], r["logits"]), f"logits: {what}"
            assert same(got["loss"][s:s + 1], r["loss"]), f"loss: {what}: {got['loss'][s].item()} vs {r['loss'].item()}"
            assert same(got["d_img"][i0:i1], r["d_img"]) and same(got["d_txt"][t0:t1], r["d_txt"]), f"gradients: {what}"
            if act is not None:
                assert same(got["a_img"][i0:i1], r["a_img"]) and same(got["a_txt"][t0:t1], r["a_txt"]), f"act copies: {what}"
            # the bad label poisons its own group and nothing else
            nan = bool(torch.isnan(got["loss"][s])), bool(torch.isnan(got["d_txt"][t0:t1]).any())
            assert nan == ((s == bad), (s == bad)), f"NaN containment: {what}: {nan}"
            assert bool(torch.isfinite(got["logits"][i0:i1]).all())
        for k in got:
            if k != "ws":
                assert same(got[k], again[k]), f"second run: {k} (C {C} B {B} S {S})"


@pytest.mark.parametrize("groups", [4, 19, 64, 100])
def test_grouped_sums_equal_single_calls(groups):
    """out[s, i, :] = sum_g src[(s groups + g) rows + i, :] in rpo_reduce_groups' order (both of its kernels: groups < 64 and
    >= 64), and the broadcast that is its forward; the sets are strided column blocks of a wider buffer."""
    from rpo_amd import ops
    rows = 24
    for S, d in ((1, 512), (3, 512), (8, 768)):
        src = rnd((S * groups * rows + 5, d + 8), 300 + groups)[:, :d]           # leading dimension d + 8
        res = []
        for rep in range(2):
            whole, wide = guarded((S, 16 + rows * d), torch.float32)
            out = wide[:, 16:].unflatten(1, (rows, d))
            ops.reduce_groups_sets(src, out, groups)
            torch.cuda.synchronize()
            assert guards_intact(whole) and bool(torch.isnan(wide[:, :16]).all())
            res.append(out.clone())
        assert same(res[0], res[1])
        for s in range(S):
            ref = torch.empty(rows, d, device=DEV)
            ops.reduce_groups(src[s * groups * rows:(s + 1) * groups * rows], ref, groups)
            assert same(res[0][s], ref), f"reduce: S {S} set {s} groups {groups}"
        # broadcast: dst[(s groups + g) rows + i] = set s, row i
        pw = rnd((S, 16 + rows * d), 400 + groups)
        sets = pw[:, 16:].unflatten(1, (rows, d))
        whole, dst = guarded((S * groups * rows, d), torch.float32)
        ops.broadcast_rows_sets(sets, dst, groups)
        torch.cuda.synchronize()
        assert guards_intact(whole)
        want = sets.unsqueeze(1).expand(S, groups, rows, d).reshape(S * groups * rows, d)
        assert same(dst, want), f"broadcast: S {S} groups {groups}"
        ref = torch.empty(groups * rows, d, device=DEV)
        ops.broadcast_rows(sets[S - 1].contiguous(), ref, groups)
        assert same(dst[(S - 1) * groups * rows:], ref)


# ===================================================================================================== model level

@functools.lru_cache(maxsize=4)
def _workload(depth, K):
    cfg = vit_b16(layers_v=depth, layers_t=depth, K=K)
    toks = synth.oxford_pets_base_tokens()
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407], logit_scale=float(np.log(100.0)))
    return cfg, sd, toks


def _member(cfg, sd, s, B, step=0):
    """Member s's own prompts, images and labels (all different between members and steps)."""
    tp, ip = synth.prompts(cfg, sd, seed=7 + 13 * s)
    return (tp, ip), synth.images(cfg, B, seed=1234 + 100 * s + 10 * step), synth.labels(cfg, B, seed=4321 + 100 * s + 10 * step)


@functools.lru_cache(maxsize=None)
def _oracle(depth, K, s, B):
    """OracleRPO on member s ALONE: logits, loss and both prompt gradients."""
    from oracle.rpo_oracle import OracleRPO
    cfg, sd, toks = _workload(depth, K)
    (tp, ip), image, label = _member(cfg, sd, s, B)
    m = OracleRPO(sd, toks, cfg.K, cfg.patch)
    m.set_prompts(tp, ip)
    out, gt, gi = m.loss_and_grads(image, label)
    return out.logits.detach().numpy(), float(out.loss.detach()), gt.numpy(), gi.numpy()


def _relmax(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


BOUNDS = {"f32": (TOL_F32, TOL_F32), "bf16": (BF16_LOGIT_ATOL, BF16_GRAD_REL), "f16": (F16_LOGIT_ATOL, F16_GRAD_REL)}


def _multi_engine(cfg, sd, toks, mode, S, B):
    from rpo_amd.engine import Engine
    eng = Engine(cfg, sd, toks, torch.device(DEV), DT[mode], max_batch=S * B)
    eng.multi_setup(S, B)
    return eng


def _load_members(eng, cfg, sd, S, B):
    nt = cfg.K * cfg.d_t
    images, labels = [], []
    for s in range(S):
        (tp, ip), im, lb = _member(cfg, sd, s, B)
        eng.m_params[s, :nt] = torch.from_numpy(tp).reshape(-1).to(DEV)
        eng.m_params[s, nt:] = torch.from_numpy(ip).reshape(-1).to(DEV)
        images.append(im)
        labels.append(lb)
    return torch.from_numpy(np.concatenate(images)).to(DEV), torch.from_numpy(np.concatenate(labels)).to(DEV)


def _check_members(depth, K, mode, S, B):
    from rpo_amd.engine import Engine
    cfg, sd, toks = _workload(depth, K)
    eng = _multi_engine(cfg, sd, toks, mode, S, B)
    image, label = _load_members(eng, cfg, sd, S, B)
    eng.multi_forward_backward(image, label)
    torch.cuda.synchronize()
    lt, gr = BOUNDS[mode]
    n = cfg.n_cls
    worst = [0.0, 0.0, 0.0, 0.0]
    for s in range(S):
        o_logits, o_loss, o_gt, o_gi = _oracle(depth, K, s, B)
        logits = eng.m_logits[s * B:(s + 1) * B].cpu().numpy()
        loss = float(eng.m_loss[s])
        gt, gi = eng.m_g_text[s].cpu().numpy(), eng.m_g_img[s].cpu().numpy()
        assert np.isfinite(logits).all() and np.isfinite(gt).all() and np.isfinite(gi).all()
        errs = (np.abs(logits - o_logits).max(), abs(loss - o_loss), _relmax(gt, o_gt), _relmax(gi, o_gi))
        worst = [max(a, b) for a, b in zip(worst, errs)]
        assert errs[0] <= lt and errs[1] <= lt, f"member {s}: logits err {errs[0]:.3e} loss err {errs[1]:.3e} (bound {lt})"
        assert errs[2] <= gr and errs[3] <= gr, f"member {s}: g_text rel {errs[2]:.3e} g_img rel {errs[3]:.3e} (bound {gr})"
    print(f"\n[multi d{depth} K{K} {mode} S={S} B={B}] worst over members vs oracle: logits {worst[0]:.3e} loss {worst[1]:.3e} "
          f"g_text rel {worst[2]:.3e} g_img rel {worst[3]:.3e}")
    if mode == "f32":
        # ... and against a standalone Engine on the same member (its own plans: batch B, n_cls * K text rows)
        solo = Engine(cfg, sd, toks, torch.device(DEV), torch.float32, max_batch=B)
        dmax, equal = 0.0, True
        for s in range(S):
            solo.params.copy_(eng.m_params[s])
            solo.forward_backward(image[s * B:(s + 1) * B].contiguous(), label[s * B:(s + 1) * B].contiguous())
            torch.cuda.synchronize()
            pairs = ((eng.m_logits[s * B:(s + 1) * B], solo.logits[:B]), (eng.m_loss[s:s + 1], solo.loss),
                     (eng.m_grads[s], solo.grads))
            for a, b in pairs:
                dmax = max(dmax, float((a - b).abs().max()))
                equal = equal and same(a, b)
        print(f"[multi d{depth} K{K} f32 S={S} B={B}] vs standalone Engine: worst |diff| {dmax:.3e}, bit-equal: {equal}")
        assert dmax <= TOL_F32 / 100
    return eng


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_members_match_the_oracle_run_on_each_member_alone(mode, S, B):
    """Depth 2, 19 classes, K = 24: per-member logits, loss, g_text and g_img within the project's model bounds of OracleRPO
    on that member alone; every member has its own prompts, images and labels.  f32: also within TOL_F32 / 100 of a
    standalone Engine on the member (the worst difference is printed)."""
    _check_members(2, 24, mode, S, B)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_members_match_the_oracle_at_depth_12(mode):
    """The reference's own configuration: 12 + 12 layers, K = 24, three members of batch 4."""
    _check_members(12, 24, mode, 3, 4)


def _optim(**kw):
    from rpo_amd.trainer import OptimConfig
    return OptimConfig(**kw)


def _trainer(mode, S, B, use_graph=True, num_batches=10 ** 9, optim=None, depth=2, K=24, prompts=None):
    from rpo_amd.multi import RPOMulti
    cfg, sd, toks = _workload(depth, K)
    prompts = prompts or [_member(cfg, sd, s, B)[0] for s in range(S)]
    return RPOMulti(cfg, sd, toks, n_runs=S, batch_size=B, prompts=prompts, optim=optim, device=DEV, act_dtype=DT[mode],
                    num_batches=num_batches, use_graph=use_graph)


def _step_batch(cfg, sd, S, B, step):
    ims, lbs = zip(*[_member(cfg, sd, s, B, step)[1:] for s in range(S)])
    return torch.from_numpy(np.concatenate(ims)).to(DEV), torch.from_numpy(np.concatenate(lbs)).to(DEV)


# three optimiser steps: f32 within 1e-6 (the bound of test_two_ranks_equal_one_rank_global_batch); the 16-bit modes within
# the trajectory bounds of tests/test_gpu_model.py (TRAJ_TOL: f16 1e-3, bf16 5e-3)
SGD_TOL = {"f32": 1e-6, "f16": 1e-3, "bf16": 5e-3}


@pytest.mark.parametrize("mode", ["f32", "f16", "bf16"])
def test_three_sgd_steps_equal_standalone_trainers(mode):
    from test_gpu_model import TRAJ_TOL
    from rpo_amd.trainer import RPO
    assert SGD_TOL["f16"] == TRAJ_TOL[torch.float16] and SGD_TOL["bf16"] == TRAJ_TOL[torch.bfloat16]
    S, B = 3, 4
    cfg, sd, toks = _workload(2, 24)
    oc = _optim(lr=0.01, warmup_epoch=0, lr_scheduler="constant")
    tr = _trainer(mode, S, B, optim=oc)
    solos = [RPO(cfg, sd, toks, oc, DEV, DT[mode], batch_size=B, num_batches=10 ** 9, prompts=_member(cfg, sd, s, B)[0])
             for s in range(S)]
    nt = cfg.K * cfg.d_t
    for step in range(3):
        image, label = _step_batch(cfg, sd, S, B, step)
        loss = tr.step_async(image, label).clone()
        torch.cuda.synchronize()
        for s, solo in enumerate(solos):
            l1 = solo.step_async(image[s * B:(s + 1) * B].contiguous(), label[s * B:(s + 1) * B].contiguous()).clone()
            solo._join_side()
            torch.cuda.synchronize()
            ep = float((tr.engine.m_params[s] - solo.engine.params).abs().max())
            em = float((tr.engine.m_mom[s] - solo.engine.mom).abs().max())
            el = abs(float(loss[s]) - float(l1))
            print(f"[multi sgd {mode}] step {step + 1} member {s}: prompts err {ep:.2e} momentum err {em:.2e} loss err {el:.2e}")
            assert ep <= SGD_TOL[mode], f"step {step + 1} member {s}: prompts differ by {ep:.3e}"
            # momentum: f32 at the prompts' bound.  16-bit: SGD_TOL bounds the PROMPTS, which move by lr x momentum; the
            # momentum itself is a sum of at most three gradients with weights <= 1 (1 + 0.9 + 0.81), and each run's gradient
            # is within GRAD_REL x max|gradient| of the exact one (tests/helpers.py), so the two runs are within
            # 2.71 x 2 x GRAD_REL of the momentum's largest entry.  The loss: 1e-6 in f32, the logits' bound otherwise.
            em_tol = 1e-6 if mode == "f32" else 2.71 * 2 * BOUNDS[mode][1] * float(solo.engine.mom.abs().max())
            assert em <= em_tol, f"step {step + 1} member {s}: momentum differs by {em:.3e} (bound {em_tol:.3e})"
            assert el <= (1e-6 if mode == "f32" else BOUNDS[mode][0])
    assert float((tr.engine.m_params[0, :nt] - torch.from_numpy(_member(cfg, sd, 0, B)[0][0]).reshape(-1).to(DEV)).abs().max()) > 0


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_members_are_isolated_from_each_other(mode):
    """One step; then the same step with ONLY member j's images, labels and prompts changed -- an all-NaN prompt and an
    out-of-range label among them.  Every other member's logits, loss, gradients and updated prompts are bit-identical;
    member j's outputs are NaN where a standalone run's are."""
    from rpo_amd.trainer import RPO
    S, B, j = 3, 4, 1
    cfg, sd, toks = _workload(2, 24)
    oc = _optim(lr=0.01, warmup_epoch=0, lr_scheduler="constant")
    image, label = _step_batch(cfg, sd, S, B, 0)

    def run(prompts, image, label):
        tr = _trainer(mode, S, B, use_graph=False, optim=oc, prompts=prompts)
        tr.step_async(image, label)
        torch.cuda.synchronize()
        e = tr.engine
        return dict(logits=e.m_logits.clone(), loss=e.m_loss.clone(), grads=e.m_grads.clone(), params=e.m_params.clone(),
                    mom=e.m_mom.clone())

    prompts = [_member(cfg, sd, s, B)[0] for s in range(S)]
    base = run(prompts, image, label)
    assert all(bool(torch.isfinite(v).all()) for v in base.values())
    tp_j, ip_j = synth.prompts(cfg, sd, seed=991)
    tp_j = np.full_like(tp_j, np.nan)                              # the whole text prompt of member j
    image2, label2 = image.clone(), label.clone()
    image2[j * B:(j + 1) * B] = torch.from_numpy(synth.images(cfg, B, seed=77)).to(DEV)
    label2[j * B:(j + 1) * B] = torch.from_numpy(synth.labels(cfg, B, seed=78)).to(DEV)
    label2[j * B + 2] = cfg.n_cls + 5
    prompts2 = list(prompts)
    prompts2[j] = (tp_j, ip_j)
    other = run(prompts2, image2, label2)
    for s in range(S):
        if s == j:
            continue
        for k in base:
            a = base[k][s * B:(s + 1) * B] if k == "logits" else base[k][s]
            b = other[k][s * B:(s + 1) * B] if k == "logits" else other[k][s]
            assert same(a, b), f"member {s}: {k} changed when only member {j} did"
    solo = RPO(cfg, sd, toks, oc, DEV, DT[mode], batch_size=B, num_batches=10 ** 9, use_graph=False, prompts=(tp_j, ip_j))
    solo.step_async(image2[j * B:(j + 1) * B].contiguous(), label2[j * B:(j + 1) * B].contiguous())
    torch.cuda.synchronize()
    se = solo.engine
    for got, want, what in ((other["logits"][j * B:(j + 1) * B], se.logits[:B], "logits"), (other["loss"][j:j + 1], se.loss, "loss"),
                            (other["grads"][j], se.grads, "gradients"), (other["params"][j], se.params, "updated prompts")):
        assert torch.equal(torch.isnan(got).cpu(), torch.isnan(want).cpu()), f"member {j}: NaN pattern of {what}"
    assert bool(torch.isnan(other["loss"][j])) and bool(torch.isnan(other["grads"][j]).all())


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_graph_replay_equals_eager_across_an_lr_recapture(mode, S):
    """One captured graph per learning rate against the same launches issued eagerly, bit for bit, over the warm-up ->
    cosine change of the default schedule.  S = 1 is the single-member trainer: the same holds."""
    B, nb = 4, 2
    cfg, sd, toks = _workload(2, 24)
    g, e = _trainer(mode, S, B, use_graph=True, num_batches=nb), _trainer(mode, S, B, use_graph=False, num_batches=nb)
    lrs = []
    for step in range(5):
        image, label = _step_batch(cfg, sd, S, B, step)
        batches = [{"img": image[s * B:(s + 1) * B], "label": label[s * B:(s + 1) * B]} for s in range(S)]
        lrs.append(g.lr)
        assert g.lr == e.lr
        og, oe = g.forward_backward(batches), e.forward_backward(batches)
        torch.cuda.synchronize()
        assert [np.float32(o["loss"]).tobytes() for o in og] == [np.float32(o["loss"]).tobytes() for o in oe], f"step {step}"
        assert [o["acc"] for o in og] == [o["acc"] for o in oe]
        for k in ("m_logits", "m_grads", "m_params", "m_mom"):
            assert same(getattr(g.engine, k), getattr(e.engine, k)), f"step {step}: {k}"
    assert len(set(lrs)) >= 2 and g.epoch == 2 and g._graph is not None and g._graph[1] == g.lr


def test_single_run_step_is_untouched_by_a_multi_trainer():
    """A freshly built plain RPO step gives the same bits before and after a multi trainer was created, stepped and
    destroyed in the process; an engine without multi_setup has none of its buffers."""
    from rpo_amd.trainer import RPO
    cfg, sd, toks = _workload(2, 24)
    B = 4
    (tp, ip), im, lb = _member(cfg, sd, 0, B)
    image, label = torch.from_numpy(im).to(DEV), torch.from_numpy(lb).to(DEV)

    def plain():
        tr = RPO(cfg, sd, toks, None, DEV, torch.bfloat16, batch_size=B, num_batches=10 ** 9, prompts=(tp, ip))
        assert tr.engine.multi_S == 0 and tr.engine._multi is None and not hasattr(tr.engine, "m_params")
        out = []
        for _ in range(2):
            loss = tr.step_async(image, label).clone()
            tr._join_side()
            torch.cuda.synchronize()
            out += [loss, tr.engine.logits[:B].clone(), tr.engine.grads.clone(), tr.engine.params.clone()]
        return out, tr.engine.hbm_bytes()

    before, bytes_before = plain()
    mt = _trainer("bf16", 3, B)
    for step in range(2):
        mt.step_async(*_step_batch(cfg, sd, 3, B, step))
    mt.model_inference(image, member=2)
    torch.cuda.synchronize()
    del mt
    after, bytes_after = plain()
    assert bytes_before == bytes_after
    assert all(same(a, b) for a, b in zip(before, after))


def _decoded(n, seed):
    rng = np.random.default_rng(seed)
    sizes = [(375, 500), (500, 333), (224, 224), (97, 260), (301, 97), (60, 40), (230, 231), (256, 192)]
    return [rng.integers(0, 256, (*sizes[i % len(sizes)], 3), dtype=np.uint8) for i in range(n)]


@pytest.mark.parametrize("mode,use_graph", [("f32", True), ("bf16", True), ("bf16", False)])
def test_run_epoch_evaluation_and_checkpoints(mode, use_graph, tmp_path):
    """run_epoch over per-member resident sets == per-step forward_backward on the same batches (losses and state, bit for
    bit), each member in the batch order `epoch_indices` gives its generator; `test(member=s)` and `model_inference` equal
    a standalone RPO loaded from member s's checkpoint; a second multi trainer resumes from the files."""
    from rpo_amd.input_pipeline import DeviceImageSet, InputConfig, build_transform
    from rpo_amd.loop import epoch_indices
    from rpo_amd.multi import RPOMulti
    from rpo_amd.trainer import RPO
    S, B, nb, epochs = 3, 4, 2, 2
    cfg, sd, toks = _workload(2, 24)
    sizes = [B * nb, B * nb + 1, B * nb + 3]                      # different sets, the same number of batches
    imgs = [_decoded(n, seed=60 + s) for s, n in enumerate(sizes)]
    labs = [np.random.default_rng(70 + s).integers(0, cfg.n_cls, n).tolist() for s, n in enumerate(sizes)]
    sets = [DeviceImageSet(imgs[s], labs[s], DEV) for s in range(S)]
    stage = build_transform(InputConfig(SIZE=(224, 224)), True, DEV, B)
    torch.manual_seed(5)
    order = [[epoch_indices(sizes[s], B, g) for g in [torch.Generator().manual_seed(40 + s)] * epochs] for s in range(S)]
    plans = [[[[stage.plan(*imgs[s][i].shape[:2]) for i in batch] for batch in ep] for ep in order[s]] for s in range(S)]

    seq = _trainer(mode, S, B, use_graph=use_graph, num_batches=nb)
    seq_loss = []
    for ep in range(epochs):
        for t in range(nb):
            batches = [{"img": stage([imgs[s][i] for i in order[s][ep][t]], plans[s][ep][t]).clone(),
                        "label": torch.tensor([labs[s][i] for i in order[s][ep][t]])} for s in range(S)]
            seq_loss.append([np.float32(o["loss"]) for o in seq.forward_backward(batches)])
    tr = _trainer(mode, S, B, use_graph=use_graph, num_batches=nb)
    gens = [torch.Generator().manual_seed(40 + s) for s in range(S)]
    losses = []
    for ep in range(epochs):
        out = tr.run_epoch(sets, gens, [plans[s][ep] for s in range(S)])
        assert out["indices"] == [order[s][ep] for s in range(S)]
        assert out["loss"].is_cuda and out["loss"].shape == (nb, S)
        losses.append(out["loss"])
    torch.cuda.synchronize()
    got = torch.cat(losses).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), np.array(seq_loss, np.float32).view(np.uint32)), "per-step, per-member losses"
    assert same(tr.engine.m_params, seq.engine.m_params) and same(tr.engine.m_mom, seq.engine.m_mom)
    assert tr.epoch == epochs and tr.batch_idx == 0 and tr.lr == seq.lr and tr._steps == seq._steps == nb * epochs
    with pytest.raises(ValueError, match="same, non-zero number of batches"):
        tr.run_epoch([sets[0], sets[1], DeviceImageSet(imgs[0][:B], labs[0][:B], DEV)], gens)
    # ---- evaluation and checkpoints, per member
    dirs = [str(tmp_path / f"member{s}") for s in range(S)]
    tr.save_model(dirs, is_best=True)
    n_test = 9
    test_imgs = _decoded(n_test, seed=90)
    test_set = DeviceImageSet(test_imgs, np.random.default_rng(91).integers(0, cfg.n_cls, n_test).tolist(), DEV)
    probe = torch.from_numpy(synth.images(cfg, B, seed=555)).to(DEV)
    for s in range(S):
        # (the same engine batch capacity: evaluation then runs the same chunks on the same GEMM plans)
        solo = RPO(cfg, sd, toks, None, DEV, DT[mode], batch_size=S * B, num_batches=nb, prompts=_member(cfg, sd, 0, B)[0])
        solo.load_model(dirs[s])
        assert same(solo.engine.params, tr.engine.m_params[s]) and same(solo.engine.mom, tr.engine.m_mom[s])
        assert solo.epoch == tr.epoch and solo.lr == tr.lr and solo._steps == tr._steps
        assert same(tr.model_inference(probe, member=s), solo.model_inference(probe)), f"member {s}: eval logits"
        a, b = tr.test(test_set, member=s, verbose=False), solo.test(test_set, verbose=False)
        assert a["correct"] == b["correct"] and a["total"] == b["total"] == n_test and a["accuracy"] == b["accuracy"]
        assert np.array_equal(a["confusion_matrix"], b["confusion_matrix"])
    # members differ, and evaluating one does not disturb training state
    assert not same(tr.model_inference(probe, member=0), tr.model_inference(probe, member=1))
    assert same(tr.engine.m_params, seq.engine.m_params)
    again = _trainer(mode, S, B, use_graph=use_graph, num_batches=nb)
    again.load_model(dirs)
    assert same(again.engine.m_params, tr.engine.m_params) and same(again.engine.m_mom, tr.engine.m_mom)
    assert again.epoch == tr.epoch and again.lr == tr.lr and again._steps == tr._steps
    # ... and continues exactly where the first one does
    image, label = _step_batch(cfg, sd, S, B, 9)
    la, lb = again.step_async(image, label).clone(), tr.step_async(image, label).clone()
    torch.cuda.synchronize()
    assert same(la, lb) and same(again.engine.m_params, tr.engine.m_params)


def test_run_epoch_on_one_shared_set_equals_per_member_copies():
    """Members that share ONE resident set (part of it spilled to the host) see what they see with a copy of the set each:
    every member has its own transform, so the shared path is the per-member path."""
    from rpo_amd.input_pipeline import DeviceImageSet, InputConfig, build_transform
    S, B, nb = 3, 4, 3
    cfg, sd, toks = _workload(2, 24)
    n = B * nb + 2
    imgs = _decoded(n, seed=61)
    labs = np.random.default_rng(71).integers(0, cfg.n_cls, n).tolist()
    shared = DeviceImageSet(imgs, labs, DEV, budget_bytes=sum(im.size for im in imgs) * 2 // 3)
    assert shared.plan.spilled and len(shared.plan.spilled) < n
    res = []
    for sets in (shared, [DeviceImageSet(imgs, labs, DEV) for _ in range(S)]):
        tr = _trainer("bf16", S, B, num_batches=nb)
        torch.manual_seed(11)                                     # the transforms draw their crops from the global generator
        out = tr.run_epoch(sets, [torch.Generator().manual_seed(80 + s) for s in range(S)])
        torch.cuda.synchronize()
        assert len({id(t) for t in tr._member_tfs}) == S
        res.append((out["indices"], out["loss"].clone(), tr.engine.m_params.clone(), tr.engine.m_mom.clone()))
    assert res[0][0] == res[1][0] and res[0][0][0] != res[0][0][1]
    assert bool(torch.isfinite(res[0][1]).all())
    assert all(same(a, b) for a, b in zip(res[0][1:], res[1][1:]))


def test_seeds_initialise_members_as_standalone_runs():
    from rpo_amd.trainer import RPO
    from rpo_amd.multi import RPOMulti
    cfg, sd, toks = _workload(2, 24)
    tr = RPOMulti(cfg, sd, toks, n_runs=3, batch_size=1, seeds=[1, 2, 3], device=DEV)
    for s, seed in enumerate((1, 2, 3)):
        torch.manual_seed(seed)
        solo = RPO(cfg, sd, toks, None, DEV, batch_size=1)
        assert same(tr.engine.m_params[s], solo.engine.params), f"seed {seed}"
