"""Many prompt sets per frozen image pass (rpo_attn_prompt_fwd, rpo_amd/engine_prompt_rows.py, rpo_amd/frozen_kv.py,
`RPOMulti.model_inference_all` / `test_all`, `RPO.test(frozen=...)`, `train(val_frozen=...)`).

Op level: the new attention entry point against float64 (oracle.rows_oracle.attn_rows_fwd) at the bounds of
tests/test_gpu_ops.py::test_attn_readonly_fwd, with K / V inside a packed in-proj matrix and inside a cache, guard elements
around the output and untouched padding columns; a set of a multi-set launch bit for bit its own launch.
Model level: every member's logits against `OracleRPO` on that member alone at the project's model bounds; in f32 also
against the existing per-member path; a `FrozenImageKV` against the live path bit for bit, before and after a training
step; the training state untouched by evaluation; the single-run trainer's `test(frozen=...)` and `train(val_frozen=...)`.
"""
import math

import numpy as np
import pytest
import torch

from helpers import TOL_F32
from test_gpu_loop import _decoded, _staging
from test_gpu_multi import BOUNDS, DEV, DT, _member, _oracle, _step_batch, _trainer, _workload, same

pytestmark = pytest.mark.gpu

from oracle import rows_oracle as R  # noqa: E402  (checker only)

OP_TOL = {"f32": 2e-5, "bf16": 1.5e-2, "f16": 2e-3}          # tests/test_gpu_ops.py: TOL, what test_attn_readonly_fwd uses
GUARD = 64


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


def _close(got, ref, mode, what):
    got = got.detach().to(torch.float64).cpu()
    err = (got - ref).abs().max().item()
    den = max(ref.abs().max().item(), 1e-30)
    print(f"{what} [{mode}]: max err {err:.3e} vs max ref {den:.3e} (rel {err / den:.2e}, bound {OP_TOL[mode]})")
    assert math.isfinite(err) and err <= OP_TOL[mode] * den, f"{what} [{mode}]: rel {err / den:.2e} > {OP_TOL[mode]}"


def _guarded_out(rows, ldo, dtype):
    whole = torch.full((rows * ldo + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + rows * ldo].view(rows, ldo)


# ===================================================================================================== op level

@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("sets,B,H,N,Kp", [(3, 2, 2, 197, 24), (8, 1, 2, 50, 7), (2, 3, 1, 257, 48), (1, 1, 1, 5, 1),
                                           (3, 1, 2, 224, 40)])
def test_attn_prompt_fwd_against_float64(mode, sets, B, H, N, Kp):
    """Row (s B + b) Kp + j reads the N frozen keys of image first + b and nothing else.  Twice per shape: K / V inside a
    packed [B (N + Kp), 3 d] matrix with first_image = NULL (ldkv = 3 d), and inside a [4 N, 2 d] cache with first_image = 1
    (ldkv = 2 d).  ldq and ldo are not d; the padding columns of `out` and the guard elements around it stay NaN; a
    multi-set launch gives every set the bits of a launch on that set alone."""
    from rpo_amd import ops
    dt, d = DT[mode], 64 * H
    Rq = sets * B * Kp
    ldq, ldo = d + 8, d + 16
    qf = _rnd((Rq, ldq), 31) * 1.5                                  # sharper softmax, as test_attn_readonly_fwd
    q_dev = qf.to(DEV, dt)
    q64 = q_dev.cpu().to(torch.float64)[:, :d]
    packed = _rnd((B * (N + Kp), 3 * d), 32)
    cache = _rnd((4 * N, 2 * d), 33)
    first = torch.tensor([1], dtype=torch.int32, device=DEV)
    layouts = [("packed", packed.to(DEV, dt), d, None, 0), ("cache", cache.to(DEV, dt), 0, first, 1)]
    for name, kv, c0, fi, f0 in layouts:
        k, v = kv[:, c0:c0 + d], kv[:, c0 + d:c0 + 2 * d]
        kv64 = kv.cpu().to(torch.float64)
        whole, out = _guarded_out(Rq, ldo, dt)
        ops.attn_prompt_fwd(q_dev, k, v, out, B, H, N, Kp, sets, first_image=fi)
        torch.cuda.synchronize()
        ref = torch.empty(Rq, d, dtype=torch.float64)
        for s in range(sets):
            for b in range(B):
                rows = slice((s * B + b) * Kp, (s * B + b + 1) * Kp)
                fr = slice((f0 + b) * N, (f0 + b + 1) * N)
                ref[rows] = R.attn_rows_fwd(q64[rows], kv64[fr, c0:c0 + d], kv64[fr, c0 + d:c0 + 2 * d], H)
        _close(out[:, :d], ref, mode, f"attn prompt fwd {name} sets{sets} B{B} H{H} N{N} K{Kp}")
        w = whole.float().cpu()
        assert bool(torch.isnan(w[:GUARD]).all()) and bool(torch.isnan(w[-GUARD:]).all()), f"{name}: guard elements written"
        assert bool(torch.isnan(out[:, d:].float()).all()), f"{name}: padding columns of out written"
        # each set alone: the same bits
        if sets > 1:
            for s in range(sets):
                _, one = _guarded_out(B * Kp, ldo, dt)
                ops.attn_prompt_fwd(q_dev[s * B * Kp:(s + 1) * B * Kp], k, v, one, B, H, N, Kp, 1, first_image=fi)
                assert same(one[:, :d], out[s * B * Kp:(s + 1) * B * Kp, :d]), f"{name}: set {s} of {sets} != its own launch"
            assert not same(out[:B * Kp, :d], out[B * Kp:2 * B * Kp, :d])          # (the sets really differ)


# ===================================================================================================== model level

def _member_images(cfg, sd, s, B):
    return torch.from_numpy(_member(cfg, sd, s, B)[1]).to(DEV)


def _check_all_members(depth, mode, S, B):
    cfg, sd, toks = _workload(depth, 24)
    tr = _trainer(mode, S, B, depth=depth)
    lt = BOUNDS[mode][0]
    worst, worst_path = 0.0, 0.0
    for s in range(S):
        image = _member_images(cfg, sd, s, B)                       # (the oracle recipe gives every member its own images)
        allm = tr.model_inference_all(image)
        assert tuple(allm.shape) == (S, B, cfg.n_cls) and bool(torch.isfinite(allm).all())
        err = float(np.abs(allm[s].cpu().numpy() - _oracle(depth, 24, s, B)[0]).max())
        worst = max(worst, err)
        if mode == "f32":
            for m in range(S):
                worst_path = max(worst_path, float((allm[m] - tr.model_inference(image, member=m)).abs().max()))
        assert same(allm, tr.model_inference_all(image)), "second call"
    print(f"\n[shared eval d{depth} {mode} S={S} B={B}] worst logits err vs oracle {worst:.3e} (bound {lt})"
          + (f", vs model_inference(member=s) {worst_path:.3e} (bound {TOL_F32 / 100:.1e})" if mode == "f32" else ""))
    assert worst <= lt
    if mode == "f32":
        assert worst_path <= TOL_F32 / 100
    if S > 1:
        assert not same(allm[0], allm[1])


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_model_inference_all_matches_the_oracle_on_each_member(mode, S, B):
    """Depth 2, 19 classes, K = 24: member s's slice of `model_inference_all` within the project's logit bound of OracleRPO
    run on that member alone; f32: every slice also within TOL_F32 / 100 of the existing path `model_inference(member=s)`."""
    _check_all_members(2, mode, S, B)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_model_inference_all_matches_the_oracle_at_depth_12(mode):
    _check_all_members(12, mode, 3, 4)


def _image_set(n, seed, C=19):
    from rpo_amd.input_pipeline import DeviceImageSet
    imgs = _decoded(n, seed)
    labels = np.random.default_rng(seed + 1).integers(0, C, n).tolist()
    return DeviceImageSet(imgs, labels, DEV), imgs, labels


def _collect(fn, n, **kw):
    """(result, logits [S, n, C]) of a `test_all` / `test(frozen=...)` call, the logits copied chunk by chunk by the hook."""
    got = {}

    def hook(b0, logits):
        got[b0] = logits.detach().clone()
    res = fn(hook=hook, verbose=False, **kw)
    torch.cuda.synchronize()
    logits = torch.cat([got[b0] for b0 in sorted(got)], dim=1)
    assert logits.shape[1] == n
    return res, logits


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_frozen_cache_equals_live_path_and_the_host_evaluator(mode):
    """9 images of mixed sizes through an engine of max_batch 4 (chunks 4, 4, 1): `test_all` on a `FrozenImageKV` gives
    the bits of `test_all` on the live frozen pass, equal result dicts and confusion matrices, each what
    `evaluator.Classification` computes on the host from those logits; the cache survives a training step (both paths move,
    together); the training state is not touched; the next graph-replayed step equals that of a twin that never evaluated."""
    from rpo_amd.evaluator import Classification
    from rpo_amd.frozen_kv import FrozenImageKV
    S, B, n = 2, 2, 9
    cfg, sd, toks = _workload(2, 24)
    tr, twin = _trainer(mode, S, B), _trainer(mode, S, B)
    assert tr.engine.max_batch == 4
    ds, imgs, labels = _image_set(n, 61)
    for step in range(2):                                            # (step 0 eager, step 1 captures the graph)
        image, label = _step_batch(cfg, sd, S, B, step)
        la, lb = tr.step_async(image, label).clone(), twin.step_async(image, label).clone()
        assert same(la, lb)
    eng = tr.engine
    torch.cuda.synchronize()
    state = [t.detach().clone() for t in (eng.m_params, eng.m_mom, eng.params)]
    cache = FrozenImageKV.build(eng, ds, batch_size=100)
    assert cache.nbytes() == FrozenImageKV.bytes_needed(cfg, n, DT[mode])
    live, live_logits = _collect(tr.test_all, n, image_set=ds)
    cached, cached_logits = _collect(tr.test_all, n, image_set=ds, frozen=cache)
    assert tuple(live_logits.shape) == (S, n, cfg.n_cls) and bool(torch.isfinite(live_logits).all())
    assert same(live_logits, cached_logits), "cache != live path"
    _same_results(live, cached)
    for s in range(S):
        ev = Classification(cfg.n_cls)
        ev.process(live_logits[s].cpu().argmax(1).tolist(), labels)
        want = ev.evaluate(verbose=False)
        for k in want:
            assert live[s][k] == want[k], (s, k)
        assert np.array_equal(live[s]["confusion_matrix"], ev.cmat) and live[s]["total"] == n
    # same chunks through model_inference_all
    stage = _staging(False, 4)
    for b0 in (0, 4, 8):
        assert same(tr.model_inference_all(stage(imgs[b0:b0 + 4])), live_logits[:, b0:b0 + 4])
    torch.cuda.synchronize()
    for before, t in zip(state, (eng.m_params, eng.m_mom, eng.params)):
        assert same(before, t), "evaluation changed the training state"
    # the next step: a twin that never evaluated
    image, label = _step_batch(cfg, sd, S, B, 2)
    la, lb = tr.step_async(image, label).clone(), twin.step_async(image, label).clone()
    assert same(la, lb) and same(tr.engine.m_params, twin.engine.m_params)
    # ... and the cache is still the live path, while both moved with the prompts
    live2, live2_logits = _collect(tr.test_all, n, image_set=ds)
    cached2, cached2_logits = _collect(tr.test_all, n, image_set=ds, frozen=cache)
    assert same(live2_logits, cached2_logits)
    _same_results(live2, cached2)
    assert not same(live2_logits, live_logits)
    assert set(live2[0]) == set(tr.test(ds, member=0, verbose=False))          # (the keys of the per-member path's dict)


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_single_run_trainer_takes_a_frozen_cache(mode):
    from rpo_amd.frozen_kv import FrozenImageKV
    from rpo_amd.input_pipeline import DeviceImageSet
    from rpo_amd.trainer import RPO
    cfg, sd, toks = _workload(2, 24)
    B, n = 4, 9
    tr = RPO(cfg, sd, toks, None, DEV, DT[mode], batch_size=B, num_batches=2, prompts=_member(cfg, sd, 0, B)[0])
    ds, imgs, labels = _image_set(n, 71)
    cache = FrozenImageKV.build(tr.engine, ds)
    res, logits = _collect(tr.test, n, image_set=ds, frozen=cache)
    stage = _staging(False, B)
    ref = torch.cat([tr.model_inference(stage(imgs[b0:b0 + B])) for b0 in range(0, n, B)])
    err = float((logits[0] - ref).abs().max())
    print(f"\n[RPO.test(frozen) {mode}] worst logits diff vs the existing eval path {err:.3e} (bound {BOUNDS[mode][0]})")
    assert err <= BOUNDS[mode][0]
    plain = tr.test(ds, verbose=False)
    assert set(res) == set(plain) and res["total"] == plain["total"] == n
    # the validation pass of train() on the cache
    train_set = DeviceImageSet(imgs[:8], labels[:8], DEV)
    hist = tr.train(train_set, max_epoch=2, val_set=ds, val_frozen=cache, verbose=False)
    assert len(hist) == 2 and all("val_acc" in r and 0.0 <= r["val_acc"] <= 100.0 for r in hist)
    # a cache of another set length / another storage mode is refused
    with pytest.raises(ValueError, match="n_images"):
        tr.test(train_set, verbose=False, frozen=cache)
    other = torch.float32 if mode != "f32" else torch.bfloat16
    tr2 = RPO(cfg, sd, toks, None, DEV, other, batch_size=B, num_batches=2, prompts=_member(cfg, sd, 0, B)[0])
    with pytest.raises(ValueError, match="act_dtype"):
        tr2.test(ds, verbose=False, frozen=cache)
    with pytest.raises(ValueError, match="bytes"):
        FrozenImageKV.build(tr.engine, ds, budget_bytes=1000)
