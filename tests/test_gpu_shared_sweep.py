"""The shared-batch sweep step on the device (rpo_amd/engine_prompt_train.py, rpo_amd/shared_sweep.py):
the members of an RPO sweep trained on ONE batch, the frozen image rows run once.

Engine K = 24, members K = (24, 8, 16) with their own prompts on ONE batch: every member against `OracleRPO(K = K_s)` run on
that member's prompts with the shared images at the project's model bounds, in f32 also against a standalone
Engine(cfg.K = K_s); member 0 against the real reference's golden; three steps with per-member optimiser settings against
standalone RPO(K_s, optim_s) trainers; the result independent of the prompts that ride in the frozen pass; isolation of the
members; graph replay against eager launches; the existing paths untouched; the epoch loop, evaluation and checkpoints;
one case at depth 12.

The bit helpers, workload and bounds are those of tests/test_gpu_multi.py and tests/test_gpu_sweep.py.
"""
import functools

import numpy as np
import pytest
import torch

import test_gpu_multi as M
import test_gpu_sweep as W
from helpers import CASES, TOL_F32, load_golden, workload
from rpo_amd import synth

pytestmark = pytest.mark.gpu

DEV, DT, BOUNDS, SGD_TOL = M.DEV, M.DT, M.BOUNDS, M.SGD_TOL
same, all_zero_bits = M.same, W.all_zero_bits
MEMBER_K, KMAX, _wl, _member = W.MEMBER_K, W.KMAX, W._wl, W._member
NAN = float("nan")


def _batch(B, step=0, depth=2):
    """The ONE batch of a step: member 0's images and labels of tests/test_gpu_multi.py."""
    cfg, sd, _ = M._workload(depth, KMAX)
    _, im, lb = M._member(cfg, sd, 0, B, step)
    return torch.from_numpy(im).to(DEV), torch.from_numpy(lb).to(DEV)


@functools.lru_cache(maxsize=None)
def _oracle_shared(depth, K, s, B):
    """OracleRPO(K) on member s's prompts with the SHARED batch; where member s's own batch is the shared one (s = 0), the
    cached oracle of tests/test_gpu_multi.py."""
    if s == 0:
        return M._oracle(depth, K, 0, B)
    from oracle.rpo_oracle import OracleRPO
    cfg, sd, toks = M._workload(depth, K)
    (tp, ip), _, _ = M._member(cfg, sd, s, B)
    _, image, label = M._member(cfg, sd, 0, B)
    m = OracleRPO(sd, toks, cfg.K, cfg.patch)
    m.set_prompts(tp, ip)
    out, gt, gi = m.loss_and_grads(image, label)
    return out.logits.detach().numpy(), float(out.loss.detach()), gt.numpy(), gi.numpy()


def _shared_engine(mode, B, Ks=MEMBER_K, depth=2, kmax=KMAX):
    """Engine(K = kmax) built for B images with the shared-batch step's buffers; member s carries its own prompts."""
    from rpo_amd.engine import Engine
    cfg, sd, toks = M._workload(depth, kmax)
    eng = Engine(cfg, sd, toks, torch.device(DEV), DT[mode], max_batch=B)
    eng.params.zero_()
    eng.prompt_train_setup(len(Ks), B, member_K=list(Ks))
    assert not bool(eng.m_params.any())
    for s, k in enumerate(Ks):
        tp, ip = M._member(M._workload(depth, k)[0], sd, s, B)[0]
        eng.m_text_prompt[s, :k] = torch.from_numpy(tp).to(DEV)
        eng.m_img_prompt[s, :k] = torch.from_numpy(ip).to(DEV)
    return eng, cfg, sd, toks


def _check_against_oracle(eng, depth, Ks, B, mode, tag):
    lt, gr = BOUNDS[mode]
    for s, k in enumerate(Ks):
        o_logits, o_loss, o_gt, o_gi = _oracle_shared(depth, k, s, B)
        logits, loss = eng.m_logits[s * B:(s + 1) * B].cpu().numpy(), float(eng.m_loss[s])
        gt, gi = eng.m_g_text[s, :k].cpu().numpy(), eng.m_g_img[s, :k].cpu().numpy()
        assert o_gt.shape == gt.shape and o_gi.shape == gi.shape
        errs = (np.abs(logits - o_logits).max(), abs(loss - o_loss), M._relmax(gt, o_gt), M._relmax(gi, o_gi))
        print(f"\n[{tag} {mode} B={B}] member {s} K={k} vs oracle: logits {errs[0]:.3e} loss {errs[1]:.3e} g_text rel "
              f"{errs[2]:.3e} g_img rel {errs[3]:.3e}")
        assert np.isfinite(logits).all() and np.isfinite(gt).all() and np.isfinite(gi).all()
        assert errs[0] <= lt and errs[1] <= lt, f"member {s}: logits err {errs[0]:.3e} loss err {errs[1]:.3e} (bound {lt})"
        assert errs[2] <= gr and errs[3] <= gr, f"member {s}: g_text rel {errs[2]:.3e} g_img rel {errs[3]:.3e} (bound {gr})"
        assert all_zero_bits(eng.m_g_text[s, k:]) and all_zero_bits(eng.m_g_img[s, k:]), f"member {s}: inert gradient rows"


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_members_on_one_batch_match_the_oracle_built_with_their_K(mode, B):
    """Depth 2, 19 classes: logits, loss and both gradients (used rows) of every member within BOUNDS[mode] of
    OracleRPO(K = K_s) on that member's prompts with the shared images; gradient rows i >= K_s exact zeros; the byte count
    of `prompt_train_bytes` is the allocation.  f32: also within TOL_F32 / 100 of a standalone Engine(cfg.K = K_s) on the
    same batch -- the bound the own-batch sweep and the shared evaluation hold to (the worst difference is printed)."""
    from rpo_amd.engine import Engine
    from rpo_amd.engine_prompt_train import prompt_train_bytes
    from rpo_amd.sweep import member_row_to_flat
    S = len(MEMBER_K)
    eng, cfg, sd, toks = _shared_engine(mode, B)
    assert eng.prompt_train_hbm_bytes() == prompt_train_bytes(cfg, S, B, DT[mode])
    image, label = _batch(B)
    eng.shared_forward_backward(image, label)
    torch.cuda.synchronize()
    _check_against_oracle(eng, 2, MEMBER_K, B, mode, "shared")
    if mode == "f32":
        dmax = 0.0
        for s, k in enumerate(MEMBER_K):
            solo = Engine(_wl(k)[0], sd, toks, torch.device(DEV), torch.float32, max_batch=B)
            solo.params.copy_(member_row_to_flat(eng.m_params[s], KMAX, k, cfg.d_t, cfg.d_v))
            solo.forward_backward(image, label)
            torch.cuda.synchronize()
            for a, b in ((eng.m_logits[s * B:(s + 1) * B], solo.logits[:B]), (eng.m_loss[s:s + 1], solo.loss),
                         (member_row_to_flat(eng.m_grads[s], KMAX, k, cfg.d_t, cfg.d_v), solo.grads)):
                dmax = max(dmax, float((a - b).abs().max()))
        print(f"[shared f32 B={B}] vs standalone Engine(K_s): worst |diff| {dmax:.3e} (bound {TOL_F32 / 100:.1e})")
        assert dmax <= TOL_F32 / 100


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_member_zero_matches_the_reference_golden(mode):
    """The real reference's golden d2_k8_b3: a two-member shared sweep on the golden's images, member 0 with the golden's
    prompts and K = 8, member 1 with K = 16 and other prompts.  Member 0's logits, loss and gradients within the bounds the
    golden's own tests use for the mode (tests/test_gpu_model.py: TOL_F32; BF16_* / F16_* of tests/helpers.py = BOUNDS)."""
    import dataclasses
    from rpo_amd.engine import Engine
    tag = "d2_k8_b3"
    g = load_golden(tag)
    cfg8, sd, toks, tp, ip, image, label = workload(tag)
    B, Ks = CASES[tag][2], (8, 16)
    cfg = dataclasses.replace(cfg8, K=16)
    eng = Engine(cfg, sd, toks, torch.device(DEV), DT[mode], max_batch=B)
    eng.params.zero_()
    eng.prompt_train_setup(2, B, member_K=list(Ks))
    tp1, ip1 = synth.prompts(cfg, sd, seed=33)
    for s, (t, i) in enumerate(((tp, ip), (tp1, ip1))):
        eng.m_text_prompt[s, :Ks[s]] = torch.from_numpy(t).to(DEV)
        eng.m_img_prompt[s, :Ks[s]] = torch.from_numpy(i).to(DEV)
    eng.shared_forward_backward(torch.from_numpy(image).to(DEV), torch.from_numpy(label).to(DEV))
    torch.cuda.synchronize()
    lt, gr = BOUNDS[mode]
    logits, loss = eng.m_logits[:B].cpu().numpy(), float(eng.m_loss[0])
    gt, gi = eng.m_g_text[0, :8].cpu().numpy(), eng.m_g_img[0, :8].cpu().numpy()
    errs = (np.abs(logits - g["logits"]).max(), abs(loss - float(g["loss"])), M._relmax(gt, g["g_text"]), M._relmax(gi, g["g_img"]))
    print(f"\n[shared golden {tag} {mode}] member 0: logits {errs[0]:.3e} loss {errs[1]:.3e} g_text rel {errs[2]:.3e} g_img rel "
          f"{errs[3]:.3e}")
    assert np.isfinite(logits).all() and errs[0] <= lt and errs[1] <= lt
    assert errs[2] <= gr and errs[3] <= gr
    assert bool(torch.isfinite(eng.m_logits).all()) and not same(eng.m_logits[:B], eng.m_logits[B:])


def _shared(mode, B, S=3, use_graph=True, num_batches=1, optims=None, amp=False, Ks=MEMBER_K):
    from rpo_amd.shared_sweep import RPOSharedSweep
    cfg, sd, toks = _wl(KMAX)
    optims = optims or W._optims()
    members = [dict(prompts=M._member(_wl(Ks[s])[0], sd, s, B)[0], K=Ks[s], optim=optims[s]) for s in range(S)]
    return RPOSharedSweep(cfg, sd, toks, members=members, batch_size=B, device=DEV, act_dtype=DT[mode],
                          num_batches=num_batches, use_graph=use_graph, amp=amp)


_used = W._used


@pytest.mark.parametrize("mode", ["f32", "f16", "bf16"])
def test_three_steps_equal_standalone_trainers_fed_the_same_batches(mode):
    """Members (K 24, lr 0.01, wd 5e-4), (K 8, lr 0.02, momentum 0.8), (K 16, lr 0.005, one warm-up epoch) with num_batches =
    1 -- the rate changes after every step -- against standalone RPO(K_s, optim_s) trainers fed the SAME batches, at SGD_TOL
    on the prompts (momentum and loss: bounds derived beside the assertion); ONE graph capture."""
    from rpo_amd.trainer import RPO
    S, B = 3, 4
    sd, toks = _wl(KMAX)[1:]
    ocs = W._optims()
    tr = _shared(mode, B, optims=ocs)
    assert tr.engine.max_batch == B and tuple(tr._image.shape[:1]) == (B,)
    solos = [RPO(_wl(k)[0], sd, toks, ocs[s], DEV, DT[mode], batch_size=B, num_batches=1, prompts=_member(s, B)[0])
             for s, k in enumerate(MEMBER_K)]
    for step in range(3):
        image, label = _batch(B, step)
        assert tr.lr == [solo.lr for solo in solos]
        loss = tr.step_async(image, label).clone()
        tr._loop_advance()
        torch.cuda.synchronize()
        for s, solo in enumerate(solos):
            l1 = solo.step_async(image, label).clone()
            solo._join_side()
            solo._loop_advance()
            torch.cuda.synchronize()
            ep = float((_used(tr, tr.engine.m_params, s) - solo.engine.params).abs().max())
            em = float((_used(tr, tr.engine.m_mom, s) - solo.engine.mom).abs().max())
            el = abs(float(loss[s]) - float(l1))
            print(f"[shared sgd {mode}] step {step + 1} member {s}: prompts err {ep:.2e} momentum err {em:.2e} loss err {el:.2e}")
            assert ep <= SGD_TOL[mode], f"step {step + 1} member {s}: prompts differ by {ep:.3e}"
            # momentum: a sum of at most three gradients with weights 1 + m + m^2 <= 2.71 (tests/test_gpu_multi.py).  16-bit:
            # each run's gradient within GRAD_REL x max|gradient| of the exact one.  f32: the two runs' gradients within
            # TOL_F32 / 100 of each other, the bound of the f32 comparison with a standalone Engine above (absolute: the
            # momentum's entries are not O(1), so one ulp of a large entry exceeds the 1e-6 that bounds the prompts).
            em_tol = 2.71 * TOL_F32 / 100 if mode == "f32" else 2.71 * 2 * BOUNDS[mode][1] * float(solo.engine.mom.abs().max())
            assert em <= em_tol, f"step {step + 1} member {s}: momentum differs by {em:.3e} (bound {em_tol:.3e})"
            # the loss: f32 within TOL_F32 / 100, the same engine-against-engine bound (a loss of a few units has an ulp of
            # 2.4e-7, and the logits behind it are O(10) at scale 100); 16-bit: the logits' bound
            assert el <= (TOL_F32 / 100 if mode == "f32" else BOUNDS[mode][0])
    assert tr.epoch == 3 and tr.captures == 1
    nt = KMAX * tr.cfg.d_t
    for s, k in enumerate(MEMBER_K):                               # inert rows: still zero, parameters and momentum
        for t in (tr.engine.m_params, tr.engine.m_mom):
            assert all_zero_bits(t[s, k * tr.cfg.d_t:nt]) and all_zero_bits(t[s, nt + k * tr.cfg.d_v:])


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_the_prompts_that_ride_in_the_frozen_pass_change_no_bit(mode):
    """The frozen pass carries the single-run parameters in its rows N .. N + K; no frozen row reads them.  Two different
    parameter sets there (zeros; random values): m_loss, m_logits and m_grads bit-identical."""
    B = 4
    eng, cfg, sd, toks = _shared_engine(mode, B)
    image, label = _batch(B)
    outs = []
    for ride in (None, 5):
        if ride is None:
            eng.params.zero_()
        else:
            eng.params.copy_(M.rnd((eng.params.numel(),), ride, 0.5))
        eng.shared_forward_backward(image, label)
        torch.cuda.synchronize()
        outs.append((eng.m_loss.clone(), eng.m_logits.clone(), eng.m_grads.clone()))
    assert all(bool(torch.isfinite(t).all()) for t in outs[0])
    assert all(same(a, b) for a, b in zip(*outs)), "the riding prompts reached a member's result"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_a_bad_member_cannot_reach_the_others(mode):
    """Two eager steps with NaN in member 1's USED prompt rows, text and image (its image queries share 32-query tiles with
    members 0 and 2 in every attention launch): member 0's and member 2's logits, loss, used gradients, parameters and
    momentum keep the clean run's bits, with and without amp; under amp member 1 alone skips, both steps."""
    S, B, j = 3, 4, 1

    def run(amp, poison):
        tr = _shared(mode, B, use_graph=False, num_batches=10 ** 9, amp=amp)
        e = tr.engine
        if poison:
            e.m_text_prompt[j, 0, 3] = NAN
            e.m_img_prompt[j, 2, 5] = NAN
        before = e.m_params.clone()
        for step in range(2):
            tr.step_async(*_batch(B, step))
        torch.cuda.synchronize()
        out = [dict(logits=e.m_logits[s * B:(s + 1) * B].clone(), loss=e.m_loss[s].clone(), grads=_used(tr, e.m_grads, s),
                    params=_used(tr, e.m_params, s), mom=_used(tr, e.m_mom, s)) for s in range(S)]
        return out, tr.skipped_steps(), before, e.m_params.clone(), e.m_mom.clone()

    clean = run(False, False)[0]
    assert all(bool(torch.isfinite(v).all()) for m in clean for v in m.values())
    for amp in (False, True):
        got, skipped, before, after, mom = run(amp, True)
        assert skipped == ([0, 2, 0] if amp else [0, 0, 0])
        for s in (0, 2):
            for name in clean[s]:
                assert same(got[s][name], clean[s][name]), f"amp {amp}: member {s}: {name} changed when member {j} went bad"
        assert bool(torch.isnan(got[j]["loss"])) and bool(torch.isnan(got[j]["grads"]).any())
        if amp:
            assert same(after[j], before[j]) and all_zero_bits(mom[j]), "the skipped member was written"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_graph_replay_equals_eager_and_a_twin_trainer(mode):
    """ONE captured graph against the same launches issued eagerly, bit for bit, over the rate changes of every member's own
    schedule; a second graph trainer built alike ends the run with equal bits."""
    S, B, nb = 3, 4, 2
    g, g2, e = (_shared(mode, B, use_graph=ug, num_batches=nb) for ug in (True, True, False))
    for step in range(4):
        image, label = _batch(B, step)
        batch = {"img": image, "label": label}
        assert g.lr == e.lr
        og, og2, oe = g.forward_backward(batch), g2.forward_backward(batch), e.forward_backward(batch)
        torch.cuda.synchronize()
        assert len(og) == S and set(og[0]) == {"loss", "acc"}
        assert [np.float32(o["loss"]).tobytes() for o in og] == [np.float32(o["loss"]).tobytes() for o in oe], f"step {step}"
        assert [o["acc"] for o in og] == [o["acc"] for o in oe]
        for k in ("m_logits", "m_grads", "m_params", "m_mom"):
            assert same(getattr(g.engine, k), getattr(e.engine, k)), f"step {step}: {k}"
    for k in ("m_logits", "m_grads", "m_params", "m_mom", "m_loss"):
        assert same(getattr(g.engine, k), getattr(g2.engine, k)), f"twin trainer: {k}"
    assert g.epoch == 2 and g.captures == 1 and g2.captures == 1 and e.captures == 0


def test_existing_paths_are_untouched_by_a_shared_sweep_trainer():
    """A plain RPO step and an RPOSweep step give the same bits before and after an RPOSharedSweep was created, stepped,
    evaluated and destroyed in the process."""
    from rpo_amd.trainer import RPO
    cfg, sd, toks = _wl(KMAX)
    B = 4
    (tp, ip), im, lb = M._member(cfg, sd, 0, B)
    image, label = torch.from_numpy(im).to(DEV), torch.from_numpy(lb).to(DEV)

    def plain():
        tr = RPO(cfg, sd, toks, None, DEV, torch.bfloat16, batch_size=B, num_batches=10 ** 9, prompts=(tp, ip))
        assert tr.engine.pt_rows == 0 and not hasattr(tr.engine, "_pt")
        out = []
        for _ in range(2):
            loss = tr.step_async(image, label).clone()
            tr._join_side()
            torch.cuda.synchronize()
            out += [loss, tr.engine.logits[:B].clone(), tr.engine.grads.clone(), tr.engine.params.clone()]
        return out

    def sweep():
        sw = W._sweep("bf16", B)
        out = []
        for step in range(2):
            loss = sw.step_async(*W._step_batch(3, B, step)).clone()
            torch.cuda.synchronize()
            out += [loss, sw.engine.m_logits.clone(), sw.engine.m_grads.clone(), sw.engine.m_params.clone(), sw.engine.m_mom.clone()]
        out.append(sw.model_inference_all(image))
        return out

    before = plain() + sweep()
    sh = _shared("bf16", B)
    for step in range(2):
        sh.step_async(*_batch(B, step))
    sh.model_inference(image, member=1)
    sh.model_inference_all(image)
    torch.cuda.synchronize()
    del sh
    after = plain() + sweep()
    assert all(same(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_run_epoch_evaluation_and_checkpoints_on_one_set(mode, tmp_path):
    """run_epoch over ONE resident set with ONE generator == per-step forward_backward on the same batches (losses
    [num_batches, S], parameters, momentum, bit for bit).  `test_all` afterwards agrees with `test(member=s)`; member s's file
    loads into a standalone RPO(K = K_s) (same bits, eval logits at the mode's bound), and that trainer's own file loads
    back into a fresh RPOSharedSweep."""
    from rpo_amd.input_pipeline import DeviceImageSet, InputConfig, build_transform
    from rpo_amd.loop import epoch_indices
    from rpo_amd.trainer import RPO
    S, B, nb, epochs = 3, 4, 2, 2
    cfg, sd, toks = _wl(KMAX)
    ocs = W._optims()
    n = B * nb + 3
    imgs = M._decoded(n, seed=60)
    labs = np.random.default_rng(70).integers(0, cfg.n_cls, n).tolist()
    one_set = DeviceImageSet(imgs, labs, DEV)
    stage = build_transform(InputConfig(SIZE=(224, 224)), True, DEV, B)
    torch.manual_seed(5)
    order = [epoch_indices(n, B, g) for g in [torch.Generator().manual_seed(40)] * epochs]
    plans = [[[stage.plan(*imgs[i].shape[:2]) for i in batch] for batch in ep] for ep in order]
    seq = _shared(mode, B, num_batches=nb, optims=ocs)
    seq_loss = []
    for ep in range(epochs):
        for t in range(nb):
            batch = {"img": stage([imgs[i] for i in order[ep][t]], plans[ep][t]).clone(),
                     "label": torch.tensor([labs[i] for i in order[ep][t]])}
            seq_loss.append([np.float32(o["loss"]) for o in seq.forward_backward(batch)])
    tr = _shared(mode, B, num_batches=nb, optims=ocs)
    gen = torch.Generator().manual_seed(40)
    losses = []
    for ep in range(epochs):
        out = tr.run_epoch(one_set, gen, plans[ep])
        assert out["indices"] == order[ep] and out["loss"].shape == (nb, S)
        losses.append(out["loss"])
    torch.cuda.synchronize()
    got = torch.cat(losses).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), np.array(seq_loss, np.float32).view(np.uint32)), "per-step, per-member losses"
    assert same(tr.engine.m_params, seq.engine.m_params) and same(tr.engine.m_mom, seq.engine.m_mom)
    assert tr.epoch == epochs and tr.batch_idx == 0 and tr.lr == seq.lr and tr._steps == nb * epochs and tr.captures == 1
    with pytest.raises(ValueError, match="ONE image set"):
        tr.run_epoch([one_set] * S, gen)
    # ---- evaluation and checkpoints, per member
    dirs = [str(tmp_path / f"member{s}") for s in range(S)]
    tr.save_model(dirs, is_best=True)
    n_test, lt = 9, BOUNDS[mode][0]
    test_set = DeviceImageSet(M._decoded(n_test, seed=90), np.random.default_rng(91).integers(0, cfg.n_cls, n_test).tolist(), DEV)
    probe = torch.from_numpy(synth.images(cfg, B, seed=555)).to(DEV)
    all_logits = tr.model_inference_all(probe)
    all_tests = tr.test_all(test_set, verbose=False)
    back = [str(tmp_path / f"solo{s}") for s in range(S)]
    for s, k in enumerate(MEMBER_K):
        solo = RPO(_wl(k)[0], sd, toks, ocs[s], DEV, DT[mode], batch_size=B, num_batches=nb, prompts=_member(s, B)[0])
        solo.load_model(dirs[s])
        assert same(solo.engine.params, _used(tr, tr.engine.m_params, s)) and same(solo.engine.mom, _used(tr, tr.engine.m_mom, s))
        assert solo.epoch == tr.epoch and solo.lr == tr.lr[s] and solo._steps == tr._steps
        want = solo.model_inference(probe).clone()
        one = tr.model_inference(probe, member=s)
        errs = [float((a - b).abs().max()) for a, b in ((one, want), (all_logits[s], want), (one, all_logits[s]))]
        print(f"[shared eval {mode}] member {s} K={k}: member vs solo {errs[0]:.2e}, all vs solo {errs[1]:.2e}, member vs all {errs[2]:.2e}")
        assert bool(torch.isfinite(one).all()) and max(errs) <= lt, f"member {s}: eval logits differ by {errs} (bound {lt})"
        a = tr.test(test_set, member=s, verbose=False)
        assert a["total"] == all_tests[s]["total"] == n_test and a["correct"] == all_tests[s]["correct"]
        solo.save_model(back[s], is_best=True)
    assert same(tr.engine.m_params, seq.engine.m_params)           # evaluating disturbs no training state
    again = _shared(mode, B, num_batches=nb, optims=ocs)
    again.load_model(back)
    assert same(again.engine.m_params, tr.engine.m_params) and same(again.engine.m_mom, tr.engine.m_mom)
    assert again.epoch == tr.epoch and again.lr == tr.lr and again._steps == tr._steps
    image, label = _batch(B, 9)
    la, lb = again.step_async(image, label).clone(), tr.step_async(image, label).clone()
    torch.cuda.synchronize()
    assert same(la, lb) and same(again.engine.m_params, tr.engine.m_params) and same(again.engine.m_mom, tr.engine.m_mom)


def test_members_match_the_oracle_at_depth_12():
    """The reference's own depth: 12 + 12 layers, K = 24, bf16, three members on ONE batch of 4 against the oracle at BOUNDS
    (member 0's oracle is the cached one of tests/test_gpu_multi.py: its own batch is the shared one)."""
    B, Ks = 4, (24, 24, 24)
    eng, cfg, sd, toks = _shared_engine("bf16", B, Ks=Ks, depth=12)
    eng.shared_forward_backward(*_batch(B, depth=12))
    torch.cuda.synchronize()
    _check_against_oracle(eng, 12, Ks, B, "bf16", "shared d12")
