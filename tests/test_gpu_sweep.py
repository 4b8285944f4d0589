"""The sweep trainer on the device (rpo_amd/sweep.py) and its two entry points.

Op level, BIT FOR BIT with guard regions and each call run twice: rpo_head_fwd_bwd_grouped_k against rpo_head_fwd_bwd[_act]
called with K = k on compacted copies of each group's first k rows (inert rows NaN); rpo_sgd_step_sets against
rpo_sgd_step / rpo_sgd_step_guarded per set on the used ranges.  Model level: members with K = (24, 8, 16) in an engine of
K = 24, each against `OracleRPO` built with K = K_s on that member alone at the project's model bounds, in f32 also against
a standalone Engine with cfg.K = K_s; three SGD steps with per-member optimiser settings against standalone RPO(K_s)
trainers; isolation (NaN in inert rows changes nothing; amp skips only the member whose used rows are bad); one graph
capture across learning-rate changes; the default paths untouched; the epoch loop, evaluation and checkpoints.

The bit helpers, guard regions, workload and bounds are those of tests/test_gpu_multi.py.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import test_gpu_multi as M
from helpers import TOL_F32
from rpo_amd import synth

pytestmark = pytest.mark.gpu

DEV, DT, BOUNDS, SGD_TOL = M.DEV, M.DT, M.BOUNDS, M.SGD_TOL
same, bits, guarded, guards_intact, rnd = M.same, M.bits, M.guarded, M.guards_intact, M.rnd
NAN = float("nan")


def all_zero_bits(t):
    return not bool(bits(t).any())


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ===================================================================================================== op level: the head

def _head_k(img, txt, lab, ks, S, B, C, K, e, act):
    """One guarded call of the _k form; returns the inner tensors."""
    from rpo_amd import ops
    wsn = ops.head_workspace_floats(B, C, K, e)
    o = dict(logits=guarded((S * B, C), torch.float32), loss=guarded((S,), torch.float32),
             d_img=guarded((S * B, K, e), torch.float32), d_txt=guarded((S * C, K, e), torch.float32),
             ws=guarded((S * wsn,), torch.float32))
    if act is not None:
        o["a_img"], o["a_txt"] = guarded((S * B, K, e), act), guarded((S * C, K, e), act)
    train = lab is not None
    ops.head_fwd_bwd_grouped(img, txt, lab, 100.0, o["logits"][1], o["loss"][1] if train else None,
                             o["d_img"][1] if train else None, o["d_txt"][1] if train else None, o["ws"][1], S,
                             k_used=ks, **({} if act is None or not train else
                                           dict(d_img_f_act=o["a_img"][1], d_text_f_act=o["a_txt"][1])))
    torch.cuda.synchronize()
    for name, (whole, _) in o.items():
        assert guards_intact(whole), f"guard of {name} (C {C} B {B} K {K} e {e})"
    return {name: v[1] for name, v in o.items()}


def _head_ref(img, txt, lab, s, k, B, C, e, act):
    """rpo_head_fwd_bwd[_act] with K = k on the compacted copies of group s's first k rows."""
    from rpo_amd import ops
    r = dict(logits=torch.empty(B, C, device=DEV), loss=torch.empty(1, device=DEV), d_img=torch.empty(B, k, e, device=DEV),
             d_txt=torch.empty(C, k, e, device=DEV))
    kw = {}
    if act is not None and lab is not None:
        r["a_img"], r["a_txt"] = torch.empty(B, k, e, dtype=act, device=DEV), torch.empty(C, k, e, dtype=act, device=DEV)
        kw = dict(d_img_f_act=r["a_img"], d_text_f_act=r["a_txt"])
    ws = torch.empty(ops.head_workspace_floats(B, C, k, e), device=DEV)
    train = lab is not None
    ops.head_fwd_bwd(img[s * B:(s + 1) * B, :k].contiguous(), txt[s * C:(s + 1) * C, :k].contiguous(),
                     lab[s * B:(s + 1) * B].contiguous() if train else None, 100.0, r["logits"], r["loss"] if train else None,
                     r["d_img"] if train else None, r["d_txt"] if train else None, ws, **kw)
    torch.cuda.synchronize()
    return r


def _head_inputs(S, B, C, K, e, ks, seed):
    img, txt = rnd((S * B, K, e), 100 + seed), rnd((S * C, K, e), 200 + seed)
    for s, k in enumerate(ks):                                    # inert rows may hold anything: NaN
        if 0 <= k < K:
            img[s * B:(s + 1) * B, k:] = NAN
            txt[s * C:(s + 1) * C, k:] = NAN
    lab = torch.from_numpy(np.random.default_rng(seed).integers(0, C, S * B)).to(DEV)
    return img, txt, lab


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("C", [1, 19, 128, 129])
@pytest.mark.parametrize("K,ks", [(4, [1, 3, 4]), (24, [24, 16, 8])])
def test_head_with_per_group_k_equals_the_head_on_compacted_rows(K, ks, C, B):
    """Per group the bits of rpo_head_fwd_bwd[_act] with K = k on the compacted [B, k, e] / [C, k, e] copies, in both class-
    count regimes (128 | 129 is the boundary), e = 512 (vector loads) and 96 (not), training with bf16 act copies, training
    without, and eval.  The inert feature rows hold NaN; their gradient rows and act copies are exact zeros.
    Mutants: the average over K instead of k_used fails the logits here; the loss weight with K instead of
    k_used fails the gradients (and only them)."""
    S = len(ks)
    for e in (512, 96):
        img, txt, lab = _head_inputs(S, B, C, K, e, ks, seed=7 * C + B + e)
        kd = i32(ks)
        for form, act in (("train+act", torch.bfloat16), ("train", None), ("eval", None)):
            label = None if form == "eval" else lab
            got, again = _head_k(img, txt, label, kd, S, B, C, K, e, act), _head_k(img, txt, label, kd, S, B, C, K, e, act)
            for name in got:
                if name != "ws":
                    assert torch.equal(bits(got[name]), bits(again[name])), f"second run: {name} ({form} C {C} B {B} K {K} e {e})"
            if form == "eval":
                assert bool(torch.isnan(got["loss"]).all()) and bool(torch.isnan(got["d_img"]).all())
                assert bool(torch.isnan(got["d_txt"]).all())                              # eval writes logits only
            for s, k in enumerate(ks):
                what = f"{form} C {C} B {B} K {K} e {e} group {s} k {k}"
                r = _head_ref(img, txt, label, s, k, B, C, e, act)
                i0, i1, t0, t1 = s * B, (s + 1) * B, s * C, (s + 1) * C
                assert bool(torch.isfinite(r["logits"]).all()), what
                assert same(got["logits"][i0:i1], r["logits"]), f"logits: {what}"
                if form == "eval":
                    continue
                assert same(got["loss"][s:s + 1], r["loss"]), f"loss: {what}: {got['loss'][s].item()} vs {r['loss'].item()}"
                assert same(got["d_img"][i0:i1, :k], r["d_img"]) and same(got["d_txt"][t0:t1, :k], r["d_txt"]), f"gradients: {what}"
                assert all_zero_bits(got["d_img"][i0:i1, k:]) and all_zero_bits(got["d_txt"][t0:t1, k:]), f"inert rows: {what}"
                if act is not None:
                    assert same(got["a_img"][i0:i1, :k], r["a_img"]) and same(got["a_txt"][t0:t1, :k], r["a_txt"]), f"act: {what}"
                    assert all_zero_bits(got["a_img"][i0:i1, k:]) and all_zero_bits(got["a_txt"][t0:t1, k:]), f"inert act: {what}"


@pytest.mark.parametrize("C", [19, 129])
def test_head_k_out_of_range_poisons_its_own_group_only(C):
    """k_used = 0 in one group and K + 1 in another: those groups' logits and loss are NaN, the group between them has the
    bits of the plain head, and nothing is written outside the outputs."""
    K, B, e, ks = 4, 4, 512, [0, 3, 5]
    img, txt, lab = _head_inputs(3, B, C, K, e, [K, 3, K], seed=C)
    for label in (lab, None):
        got = _head_k(img, txt, label, i32(ks), 3, B, C, K, e, torch.bfloat16)
        for s in (0, 2):
            assert bool(torch.isnan(got["logits"][s * B:(s + 1) * B]).all()), f"group {s}: logits"
            if label is not None:
                assert bool(torch.isnan(got["loss"][s])), f"group {s}: loss"
                assert bool(torch.isnan(got["d_img"][s * B:(s + 1) * B]).all()) and bool(torch.isnan(got["d_txt"][s * C:(s + 1) * C]).all())
        r = _head_ref(img, txt, label, 1, 3, B, C, e, torch.bfloat16)
        assert same(got["logits"][B:2 * B], r["logits"])
        if label is not None:
            assert same(got["loss"][1:2], r["loss"]) and same(got["d_img"][B:2 * B, :3], r["d_img"])
            assert same(got["d_txt"][C:2 * C, :3], r["d_txt"]) and all_zero_bits(got["d_txt"][C:2 * C, 3:])


# ===================================================================================================== op level: the optimiser

SEG0, SEG1, PAD = 4 * 64, 4 * 96, 16
USED = [[4 * 64, 4 * 96], [1 * 64, 1 * 96], [3 * 64, 2 * 96]]          # full, partial, partial (a different share per segment)
HYPER = [[0.01, 0.9, 5e-4, 1.0], [0.02, 0.8, 0.0, 0.5], [0.005, 0.0, 1e-3, 0.25]]
P_FILL, BUF_FILL = 7.5, -3.25


def _sgd_state(seed):
    """p / g / buf [3, seg0 + seg1 + PAD]: random in the used ranges, sentinels in p and buf everywhere else."""
    n = SEG0 + SEG1 + PAD
    p, g, buf = rnd((3, n), seed), rnd((3, n), seed + 1), rnd((3, n), seed + 2)
    mask = torch.zeros(3, n, dtype=torch.bool, device=DEV)
    for s, (u0, u1) in enumerate(USED):
        mask[s, :u0] = True
        mask[s, SEG0:SEG0 + u1] = True
    p[~mask], buf[~mask] = P_FILL, BUF_FILL
    return p, g, buf, mask


def _used_flat(t, s):
    u0, u1 = USED[s]
    return torch.cat([t[s, :u0], t[s, SEG0:SEG0 + u1]]).contiguous()


def _sets_call(p, g, buf, first, found=None):
    """rpo_sgd_step_sets on guarded copies of (p, buf); returns the stepped copies."""
    from rpo_amd import ops
    (wp, p2), (wb, b2) = guarded(tuple(p.shape), torch.float32), guarded(tuple(p.shape), torch.float32)
    p2.copy_(p)
    b2.copy_(buf)
    ops.sgd_step_sets(p2, g, b2, torch.tensor(HYPER, dtype=torch.float32, device=DEV), SEG0, SEG1, first, used=i32(USED),
                      found_inf=found)
    torch.cuda.synchronize()
    assert guards_intact(wp) and guards_intact(wb)
    return p2, b2


def test_sgd_step_sets_equals_sgd_step_per_set():
    """Elementwise form: per set the bits of rpo_sgd_step with that set's (lr, momentum, weight decay, grad_scale) on its used
    ranges, first_step 1 then 0; everything outside the used ranges is bit-unchanged.
    Mutant: set 0's `hyper` row taken for every set fails sets 1 and 2 here."""
    from rpo_amd import ops
    p, g, buf, mask = _sgd_state(500)
    ref_p, ref_b = [_used_flat(p, s) for s in range(3)], [_used_flat(buf, s) for s in range(3)]
    for first in (True, False):
        p2, b2 = _sets_call(p, g, buf, first)
        pa, ba = _sets_call(p, g, buf, first)
        assert same(p2, pa) and same(b2, ba), "second run"
        assert same(p2[~mask], p[~mask]) and same(b2[~mask], buf[~mask]), "unused elements were written"
        assert bool((p2[~mask] == P_FILL).all()) and bool((b2[~mask] == BUF_FILL).all())
        for s in range(3):
            lr, mom, wd, gs = (float(np.float32(v)) for v in HYPER[s])
            ops.sgd_step(ref_p[s], _used_flat(g, s), ref_b[s], lr, mom, wd, gs, first_step=first)
            torch.cuda.synchronize()
            assert same(_used_flat(p2, s), ref_p[s]) and same(_used_flat(b2, s), ref_b[s]), f"set {s}, first_step {first}"
        p, buf = p2.clone(), b2.clone()
        g = rnd(tuple(g.shape), 600)
    assert not same(_used_flat(p, 1)[:64], _used_flat(p, 0)[:64])


def test_sgd_step_sets_guarded_scans_and_skips_per_set():
    """Guarded form: per set the bits and [flag, count] semantics of rpo_sgd_step_guarded on the set's used ranges.  Inf in set
    1's USED gradients: set 1 is untouched and counted, the others are stepped.  NaN only in set 2's UNUSED range: stepped.
    Mutant: a scan that includes the unused elements skips set 2 here."""
    from rpo_amd import ops
    p, g, buf, mask = _sgd_state(700)
    g[1, SEG0 + 5] = float("inf")                                  # used by set 1 (u1 = 96)
    g[2, 3 * 64:SEG0] = NAN                                       # not used by set 2
    g[2, SEG0 + 2 * 96:] = NAN
    counts = [2, 5, 7]
    for first in (True, False):
        found = i32([[9, n] for n in counts])
        p2, b2 = _sets_call(p, g, buf, first, found)
        found2 = i32([[9, n] for n in counts])
        pa, ba = _sets_call(p, g, buf, first, found2)
        assert same(p2, pa) and same(b2, ba) and torch.equal(found.cpu(), found2.cpu())
        assert found.cpu().tolist() == [[0, 2], [1, 5 + 1], [0, 7]]
        assert same(p2[1], p[1]) and same(b2[1], buf[1]), "the skipped set was written"
        assert same(p2[~mask], p[~mask]) and same(b2[~mask], buf[~mask]), "unused elements were written"
        for s in (0, 2):
            lr, mom, wd, gs = (float(np.float32(v)) for v in HYPER[s])
            rp, rb, rf = _used_flat(p, s), _used_flat(buf, s), i32([9, counts[s]])
            ops.sgd_step_guarded(rp, _used_flat(g, s), rb, lr, mom, wd, gs, first, rf)
            torch.cuda.synchronize()
            assert rf.cpu().tolist() == [0, counts[s]]
            assert same(_used_flat(p2, s), rp) and same(_used_flat(b2, s), rb), f"set {s}, first_step {first}"
            assert bool(torch.isfinite(_used_flat(p2, s)).all())
        p, buf = p2.clone(), b2.clone()


# ===================================================================================================== model level

MEMBER_K = (24, 8, 16)
KMAX = 24


@functools.lru_cache(maxsize=None)
def _wl(K):
    """The workload of tests/test_gpu_multi.py at K prompts: the CLIP weights and tokens do not depend on K."""
    cfg, sd, toks = M._workload(2, K)
    ref = M._workload(2, KMAX)[1]
    assert set(sd) == set(ref) and all(np.array_equal(sd[k], ref[k]) for k in sd)
    return cfg, sd, toks


def _member(s, B, step=0):
    """Member s at its own K: (text_prompt [K_s, d_t], img_prompt [K_s, d_v]), images, labels -- what `_oracle` runs."""
    cfg, sd, _ = _wl(MEMBER_K[s])
    return M._member(cfg, sd, s, B, step)


def _step_batch(S, B, step):
    ims, lbs = zip(*[_member(s, B, step)[1:] for s in range(S)])
    return torch.from_numpy(np.concatenate(ims)).to(DEV), torch.from_numpy(np.concatenate(lbs)).to(DEV)


def _flat(prompts):
    return torch.cat([torch.from_numpy(prompts[0]).reshape(-1), torch.from_numpy(prompts[1]).reshape(-1)])


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_members_with_their_own_K_match_the_oracle_built_with_that_K(mode, B):
    """Depth 2, 19 classes, engine K = 24, members K = (24, 8, 16) with their own prompts, images and labels: logits, loss and
    both gradients (used rows) within the project's model bounds of OracleRPO(K = K_s) on that member alone; the gradient
    rows i >= K_s are exact zeros.  f32: also within TOL_F32 / 100 of a standalone Engine with cfg.K = K_s (not bit
    equality: the GEMM plans are those of the larger row counts)."""
    from rpo_amd.engine import Engine
    S = len(MEMBER_K)
    cfg, sd, toks = _wl(KMAX)
    eng = Engine(cfg, sd, toks, torch.device(DEV), DT[mode], max_batch=S * B)
    eng.multi_setup(S, B, member_K=list(MEMBER_K))
    assert not bool(eng.m_params.any())                            # inert rows start at zero
    images, labels = [], []
    for s, k in enumerate(MEMBER_K):
        (tp, ip), im, lb = _member(s, B)
        eng.m_text_prompt[s, :k] = torch.from_numpy(tp).to(DEV)
        eng.m_img_prompt[s, :k] = torch.from_numpy(ip).to(DEV)
        images.append(im)
        labels.append(lb)
    image, label = torch.from_numpy(np.concatenate(images)).to(DEV), torch.from_numpy(np.concatenate(labels)).to(DEV)
    eng.multi_forward_backward(image, label)
    torch.cuda.synchronize()
    lt, gr = BOUNDS[mode]
    for s, k in enumerate(MEMBER_K):
        o_logits, o_loss, o_gt, o_gi = M._oracle(2, k, s, B)
        logits, loss = eng.m_logits[s * B:(s + 1) * B].cpu().numpy(), float(eng.m_loss[s])
        gt, gi = eng.m_g_text[s, :k].cpu().numpy(), eng.m_g_img[s, :k].cpu().numpy()
        assert o_gt.shape == gt.shape and o_gi.shape == gi.shape
        errs = (np.abs(logits - o_logits).max(), abs(loss - o_loss), M._relmax(gt, o_gt), M._relmax(gi, o_gi))
        print(f"\n[sweep {mode} B={B}] member {s} K={k} vs oracle: logits {errs[0]:.3e} loss {errs[1]:.3e} g_text rel "
              f"{errs[2]:.3e} g_img rel {errs[3]:.3e}")
        assert np.isfinite(logits).all() and np.isfinite(gt).all() and np.isfinite(gi).all()
        assert errs[0] <= lt and errs[1] <= lt, f"member {s}: logits err {errs[0]:.3e} loss err {errs[1]:.3e} (bound {lt})"
        assert errs[2] <= gr and errs[3] <= gr, f"member {s}: g_text rel {errs[2]:.3e} g_img rel {errs[3]:.3e} (bound {gr})"
        assert all_zero_bits(eng.m_g_text[s, k:]) and all_zero_bits(eng.m_g_img[s, k:]), f"member {s}: inert gradient rows"
    if mode == "f32":
        from rpo_amd.sweep import member_row_to_flat
        dmax = 0.0
        for s, k in enumerate(MEMBER_K):
            kcfg = _wl(k)[0]
            solo = Engine(kcfg, sd, toks, torch.device(DEV), torch.float32, max_batch=B)
            solo.params.copy_(member_row_to_flat(eng.m_params[s], KMAX, k, cfg.d_t, cfg.d_v))
            solo.forward_backward(image[s * B:(s + 1) * B].contiguous(), label[s * B:(s + 1) * B].contiguous())
            torch.cuda.synchronize()
            for a, b in ((eng.m_logits[s * B:(s + 1) * B], solo.logits[:B]), (eng.m_loss[s:s + 1], solo.loss),
                         (member_row_to_flat(eng.m_grads[s], KMAX, k, cfg.d_t, cfg.d_v), solo.grads)):
                dmax = max(dmax, float((a - b).abs().max()))
        print(f"[sweep f32 B={B}] vs standalone Engine(K_s): worst |diff| {dmax:.3e}")
        assert dmax <= TOL_F32 / 100


def _optims():
    from rpo_amd.trainer import OptimConfig
    return [OptimConfig(lr=0.01, weight_decay=5e-4), OptimConfig(lr=0.02, momentum=0.8), OptimConfig(lr=0.005, warmup_epoch=1)]


def _sweep(mode, B, S=3, use_graph=True, num_batches=1, optims=None, amp=False, Ks=MEMBER_K):
    from rpo_amd.sweep import RPOSweep
    cfg, sd, toks = _wl(KMAX)
    optims = optims or _optims()
    members = [dict(prompts=M._member(_wl(Ks[s])[0], sd, s, B)[0], K=Ks[s], optim=optims[s]) for s in range(S)]
    return RPOSweep(cfg, sd, toks, members=members, batch_size=B, device=DEV, act_dtype=DT[mode], num_batches=num_batches,
                    use_graph=use_graph, amp=amp)


def _used(tr, t, s):
    from rpo_amd.sweep import member_row_to_flat
    return member_row_to_flat(t[s], tr.cfg.K, tr.member_K[s], tr.cfg.d_t, tr.cfg.d_v)


@pytest.mark.parametrize("mode", ["f32", "f16", "bf16"])
def test_three_sgd_steps_equal_standalone_trainers_with_their_own_K_and_optimiser(mode):
    """Members (K 24, lr 0.01, wd 5e-4), (K 8, lr 0.02, momentum 0.8), (K 16, lr 0.005, one warm-up epoch) with num_batches =
    1 -- the rate changes after every step -- against standalone RPO(K_s, optim_s) trainers at SGD_TOL; ONE graph capture."""
    from rpo_amd.trainer import RPO
    S, B = 3, 4
    sd, toks = _wl(KMAX)[1:]
    ocs = _optims()
    tr = _sweep(mode, B, optims=ocs)
    solos = [RPO(_wl(k)[0], sd, toks, ocs[s], DEV, DT[mode], batch_size=B, num_batches=1, prompts=_member(s, B)[0])
             for s, k in enumerate(MEMBER_K)]
    for step in range(3):
        image, label = _step_batch(S, B, step)
        assert tr.lr == [solo.lr for solo in solos]
        loss = tr.step_async(image, label).clone()
        tr._loop_advance()
        torch.cuda.synchronize()
        for s, solo in enumerate(solos):
            l1 = solo.step_async(image[s * B:(s + 1) * B].contiguous(), label[s * B:(s + 1) * B].contiguous()).clone()
            solo._join_side()
            solo._loop_advance()
            torch.cuda.synchronize()
            ep = float((_used(tr, tr.engine.m_params, s) - solo.engine.params).abs().max())
            em = float((_used(tr, tr.engine.m_mom, s) - solo.engine.mom).abs().max())
            el = abs(float(loss[s]) - float(l1))
            print(f"[sweep sgd {mode}] step {step + 1} member {s}: prompts err {ep:.2e} momentum err {em:.2e} loss err {el:.2e}")
            assert ep <= SGD_TOL[mode], f"step {step + 1} member {s}: prompts differ by {ep:.3e}"
            # momentum and loss: the bounds of tests/test_gpu_multi.py (the weights 1 + m + m^2 <= 2.71 for m <= 0.9)
            em_tol = 1e-6 if mode == "f32" else 2.71 * 2 * BOUNDS[mode][1] * float(solo.engine.mom.abs().max())
            assert em <= em_tol, f"step {step + 1} member {s}: momentum differs by {em:.3e} (bound {em_tol:.3e})"
            assert el <= (1e-6 if mode == "f32" else BOUNDS[mode][0])
    assert tr.epoch == 3 and tr.captures == 1
    nt = KMAX * tr.cfg.d_t
    for s, k in enumerate(MEMBER_K):                               # inert rows: still zero, parameters and momentum
        for t in (tr.engine.m_params, tr.engine.m_mom):
            assert all_zero_bits(t[s, k * tr.cfg.d_t:nt]) and all_zero_bits(t[s, nt + k * tr.cfg.d_v:])


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_inert_rows_and_other_members_cannot_reach_a_member(mode):
    """Two eager steps.  NaN in member 1's INERT prompt rows (text and image): every member's logits, loss, used gradients,
    updated used parameters and momentum -- member 1's included -- are the clean run's bits, with and without amp, and amp
    skips nothing.  NaN in member 1's USED rows under amp: member 1 alone skips (both steps), the others are the clean bits."""
    S, B, j = 3, 4, 1
    kj = MEMBER_K[j]

    def run(amp, poison):
        tr = _sweep(mode, B, use_graph=False, num_batches=10 ** 9, amp=amp)
        e = tr.engine
        if poison == "inert":
            e.m_text_prompt[j, kj:] = NAN
            e.m_img_prompt[j, kj:] = NAN
        elif poison == "used":
            e.m_text_prompt[j, 0, 3] = NAN
        before = e.m_params.clone()
        for step in range(2):
            tr.step_async(*_step_batch(S, B, step))
        torch.cuda.synchronize()
        out = [dict(logits=e.m_logits[s * B:(s + 1) * B].clone(), loss=e.m_loss[s].clone(), grads=_used(tr, e.m_grads, s),
                    params=_used(tr, e.m_params, s), mom=_used(tr, e.m_mom, s)) for s in range(S)]
        return out, tr.skipped_steps(), before, e.m_params.clone(), e.m_mom.clone()

    clean = run(False, None)[0]
    assert all(bool(torch.isfinite(v).all()) for m in clean for v in m.values())
    for amp in (False, True):
        got, skipped, _, _, _ = run(amp, "inert")
        assert skipped == [0, 0, 0]
        for s in range(S):
            for name in clean[s]:
                assert same(got[s][name], clean[s][name]), f"amp {amp}: member {s}: {name} changed with NaN in member {j}'s inert rows"
    got, skipped, before, after, mom = run(True, "used")
    assert skipped == [0, 2, 0]
    for s in (0, 2):
        for name in clean[s]:
            assert same(got[s][name], clean[s][name]), f"member {s}: {name} changed when member {j} went bad"
    assert bool(torch.isnan(got[j]["loss"])) and bool(torch.isnan(got[j]["grads"]).any())
    assert same(after[j], before[j]) and all_zero_bits(mom[j]), "the skipped member was written"


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_graph_replay_equals_eager_with_one_capture_across_lr_changes(mode, S):
    """ONE captured graph against the same launches issued eagerly, bit for bit, over the warm-up -> cosine change of every
    member's own schedule: the rates are device data, refreshed by a copy in front of the step."""
    B, nb = 4, 2
    Ks = MEMBER_K if S == 3 else (16,)
    g, e = (_sweep(mode, B, S=S, use_graph=ug, num_batches=nb, Ks=Ks) for ug in (True, False))
    lrs = []
    for step in range(6):
        image, label = _step_batch(S, B, step)
        batches = [{"img": image[s * B:(s + 1) * B], "label": label[s * B:(s + 1) * B]} for s in range(S)]
        lrs.append(tuple(g.lr))
        assert g.lr == e.lr
        og, oe = g.forward_backward(batches), e.forward_backward(batches)
        torch.cuda.synchronize()
        assert [np.float32(o["loss"]).tobytes() for o in og] == [np.float32(o["loss"]).tobytes() for o in oe], f"step {step}"
        assert [o["acc"] for o in og] == [o["acc"] for o in oe]
        for k in ("m_logits", "m_grads", "m_params", "m_mom"):
            assert same(getattr(g.engine, k), getattr(e.engine, k)), f"step {step}: {k}"
    assert len(set(lrs)) == 3 and g.epoch == 3
    assert g.captures == 1 and e.captures == 0


def test_default_paths_are_untouched_by_a_sweep_trainer():
    """A plain RPO step and an RPOMulti step give the same bits before and after an RPOSweep was created, stepped, evaluated
    and destroyed in the process."""
    from rpo_amd.trainer import RPO
    cfg, sd, toks = _wl(KMAX)
    B = 4
    (tp, ip), im, lb = M._member(cfg, sd, 0, B)
    image, label = torch.from_numpy(im).to(DEV), torch.from_numpy(lb).to(DEV)

    def plain():
        tr = RPO(cfg, sd, toks, None, DEV, torch.bfloat16, batch_size=B, num_batches=10 ** 9, prompts=(tp, ip))
        out = []
        for _ in range(2):
            loss = tr.step_async(image, label).clone()
            tr._join_side()
            torch.cuda.synchronize()
            out += [loss, tr.engine.logits[:B].clone(), tr.engine.grads.clone(), tr.engine.params.clone()]
        return out

    def multi():
        mt = M._trainer("bf16", 3, B)
        assert mt.engine.m_k_used is None
        out = []
        for step in range(2):
            loss = mt.step_async(*M._step_batch(cfg, sd, 3, B, step)).clone()
            torch.cuda.synchronize()
            out += [loss, mt.engine.m_logits.clone(), mt.engine.m_grads.clone(), mt.engine.m_params.clone(), mt.engine.m_mom.clone()]
        out.append(mt.model_inference_all(image))
        return out

    before = plain() + multi()
    sw = _sweep("bf16", B)
    for step in range(2):
        sw.step_async(*_step_batch(3, B, step))
    sw.model_inference(image, member=1)
    sw.model_inference_all(image)
    torch.cuda.synchronize()
    del sw
    after = plain() + multi()
    assert all(same(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_run_epoch_evaluation_and_checkpoints_per_member(mode, tmp_path):
    """run_epoch over per-member resident sets == per-step forward_backward (losses [num_batches, S], parameters, momentum,
    bit for bit).  `test(member=s)`, `model_inference(member=s)` and member s's slice of `model_inference_all` agree with a
    standalone RPO(K = K_s) loaded from member s's saved file, and with each other, at the mode's logit bound.  f32: a fresh
    RPOSweep loaded from the files continues bit-identically."""
    from rpo_amd.input_pipeline import DeviceImageSet, InputConfig, build_transform
    from rpo_amd.loop import epoch_indices
    from rpo_amd.trainer import RPO
    S, B, nb, epochs = 3, 4, 2, 2
    cfg, sd, toks = _wl(KMAX)
    ocs = _optims()
    sizes = [B * nb, B * nb + 1, B * nb + 3]
    imgs = [M._decoded(n, seed=60 + s) for s, n in enumerate(sizes)]
    labs = [np.random.default_rng(70 + s).integers(0, cfg.n_cls, n).tolist() for s, n in enumerate(sizes)]
    sets = [DeviceImageSet(imgs[s], labs[s], DEV) for s in range(S)]
    stage = build_transform(InputConfig(SIZE=(224, 224)), True, DEV, B)
    torch.manual_seed(5)
    order = [[epoch_indices(sizes[s], B, g) for g in [torch.Generator().manual_seed(40 + s)] * epochs] for s in range(S)]
    plans = [[[[stage.plan(*imgs[s][i].shape[:2]) for i in batch] for batch in ep] for ep in order[s]] for s in range(S)]
    seq = _sweep(mode, B, num_batches=nb, optims=ocs)
    seq_loss = []
    for ep in range(epochs):
        for t in range(nb):
            batches = [{"img": stage([imgs[s][i] for i in order[s][ep][t]], plans[s][ep][t]).clone(),
                        "label": torch.tensor([labs[s][i] for i in order[s][ep][t]])} for s in range(S)]
            seq_loss.append([np.float32(o["loss"]) for o in seq.forward_backward(batches)])
    tr = _sweep(mode, B, num_batches=nb, optims=ocs)
    gens = [torch.Generator().manual_seed(40 + s) for s in range(S)]
    losses = []
    for ep in range(epochs):
        out = tr.run_epoch(sets, gens, [plans[s][ep] for s in range(S)])
        assert out["indices"] == [order[s][ep] for s in range(S)] and out["loss"].shape == (nb, S)
        losses.append(out["loss"])
    torch.cuda.synchronize()
    got = torch.cat(losses).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), np.array(seq_loss, np.float32).view(np.uint32)), "per-step, per-member losses"
    assert same(tr.engine.m_params, seq.engine.m_params) and same(tr.engine.m_mom, seq.engine.m_mom)
    assert tr.epoch == epochs and tr.batch_idx == 0 and tr.lr == seq.lr and tr._steps == nb * epochs and tr.captures == 1
    # ---- evaluation and checkpoints, per member
    dirs = [str(tmp_path / f"member{s}") for s in range(S)]
    tr.save_model(dirs, is_best=True)
    n_test, lt = 9, BOUNDS[mode][0]
    test_set = DeviceImageSet(M._decoded(n_test, seed=90), np.random.default_rng(91).integers(0, cfg.n_cls, n_test).tolist(), DEV)
    probe = torch.from_numpy(synth.images(cfg, B, seed=555)).to(DEV)
    all_logits = tr.model_inference_all(probe)
    all_tests = tr.test_all(test_set, verbose=False)
    for s, k in enumerate(MEMBER_K):
        solo = RPO(_wl(k)[0], sd, toks, ocs[s], DEV, DT[mode], batch_size=S * B, num_batches=nb, prompts=_member(s, B)[0])
        solo.load_model(dirs[s])
        assert same(solo.engine.params, _used(tr, tr.engine.m_params, s)) and same(solo.engine.mom, _used(tr, tr.engine.m_mom, s))
        assert solo.epoch == tr.epoch and solo.lr == tr.lr[s] and solo._steps == tr._steps
        want = solo.model_inference(probe).clone()
        one = tr.model_inference(probe, member=s)
        errs = [float((a - b).abs().max()) for a, b in ((one, want), (all_logits[s], want), (one, all_logits[s]))]
        print(f"[sweep eval {mode}] member {s} K={k}: member vs solo {errs[0]:.2e}, all vs solo {errs[1]:.2e}, member vs all {errs[2]:.2e}")
        assert bool(torch.isfinite(one).all()) and max(errs) <= lt, f"member {s}: eval logits differ by {errs} (bound {lt})"
        # test(): the same counts wherever the standalone run's decision is not within the logit bound of a tie
        eval_images = solo._loop_transform(False, n_test).from_set(
            test_set, range(n_test), out=torch.zeros(n_test, 3, cfg.image_size, cfg.image_size, device=DEV))
        top2 = solo.model_inference(eval_images).topk(min(2, cfg.n_cls), dim=1).values
        ties = int((top2[:, 0] - top2[:, 1] <= 2 * lt).sum())
        a, b = tr.test(test_set, member=s, verbose=False), solo.test(test_set, verbose=False)
        for res in (a, all_tests[s]):
            assert res["total"] == b["total"] == n_test and abs(res["correct"] - b["correct"]) <= ties
    assert not same(tr.model_inference(probe, member=0), tr.model_inference(probe, member=1))
    assert same(tr.engine.m_params, seq.engine.m_params)           # evaluating disturbs no training state
    if mode == "f32":
        again = _sweep(mode, B, num_batches=nb, optims=ocs)
        again.load_model(dirs)
        assert same(again.engine.m_params, tr.engine.m_params) and same(again.engine.m_mom, tr.engine.m_mom)
        assert again.epoch == tr.epoch and again.lr == tr.lr and again._steps == tr._steps
        image, label = _step_batch(S, B, 9)
        la, lb = again.step_async(image, label).clone(), tr.step_async(image, label).clone()
        torch.cuda.synchronize()
        assert same(la, lb) and same(again.engine.m_params, tr.engine.m_params) and same(again.engine.m_mom, tr.engine.m_mom)


def test_seeds_initialise_members_as_standalone_runs_of_their_own_K():
    from rpo_amd.sweep import RPOSweep
    from rpo_amd.trainer import RPO
    cfg, sd, toks = _wl(KMAX)
    tr = RPOSweep(cfg, sd, toks, members=[dict(seed=1, K=24), dict(seed=2, K=8), dict(seed=3, K=16)], batch_size=1, device=DEV)
    for s, (seed, k) in enumerate(zip((1, 2, 3), MEMBER_K)):
        torch.manual_seed(seed)
        solo = RPO(_wl(k)[0], sd, toks, None, DEV, batch_size=1)
        assert same(_used(tr, tr.engine.m_params, s), solo.engine.params), f"seed {seed} K {k}"
