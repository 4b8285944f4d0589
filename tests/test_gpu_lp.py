"""The linear probe on the MI355X: rpo_lp_head_fwd_bwd against a float64 restatement, the LP trainer against the reference's
own numbers (tools/make_golden_lp.py), its trajectory, graph replay, checkpoints, amp and data parallel.

Measured errors are printed by the tests (`-s`) and quoted in the docstrings."""
import functools
import os
import socket
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from lp_fixtures import c1_init, sgd_replay, write_reference_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the 16-bit bounds of tests/test_gpu_model.py (measured there for the towers these modes share), scaled by max(1, |logit|)
BF16_LOGIT_ATOL, BF16_GRAD_REL = 0.12, 0.05
F16_LOGIT_ATOL, F16_GRAD_REL = 1e-2, 6e-3
F32_LOGIT, F32_LOSS, F32_GRAD = 1e-4, 1e-4, 1e-3

DP_SEEDS = [(700, 800), (701, 801)]


def DP_OPTIM():
    from rpo_amd.trainer import OptimConfig
    return OptimConfig(lr=5e-4, max_epoch=30, lr_scheduler="constant", warmup_epoch=0)


@functools.lru_cache(maxsize=2)
def lp_workload(depth: int):
    """(cfg, state dict, token ids) of the fixtures: synthetic CLIP weights (seed 0, logit scale log 100), the reference's
    token ids of "A photo of a {cls_name}" for the 19 Oxford-Pets base classes."""
    from rpo_amd import synth
    from rpo_amd.config import vit_b16
    g = np.load(os.path.join(GOLD, "ref_lp_d2_b3.npz" if depth == 2 else "ref_lp_full_b32.npz"))
    toks = g["tokenized_prompts"]
    cfg = vit_b16(layers_v=depth, layers_t=depth, K=1)
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist(), logit_scale=float(np.log(100.0)))
    return cfg, sd, toks


def _case_init(g, case: int, e: int):
    if case == 0:
        return np.eye(e, dtype=np.float32), np.zeros(e, np.float32)
    w, b = c1_init(e)
    assert zlib.crc32(w.tobytes()) == int(g["c1_w0_crc32"]), "W0 of case c1 is not what the fixture was generated from"
    assert np.array_equal(b, g["c1_b0"])
    return w, b


def _relmax(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- 1. the op ---------------------------------------------------------------------------------------------------------
def _lp_ref64(x, w, bias, t, label, scale):
    z = x @ w.t() + bias
    logits = scale * (z @ t.t())
    p = torch.softmax(logits, dim=1)
    B = x.shape[0]
    oh = torch.nn.functional.one_hot(label, t.shape[0]).double()
    loss = torch.nn.functional.cross_entropy(logits, label)
    dz = scale * ((p - oh) / B) @ t
    return z, logits, loss, dz.t() @ x, dz.sum(0)


@pytest.mark.gpu
@pytest.mark.parametrize("e", [512, 768])
def test_lp_head_op_against_float64(e):
    """z, logits, loss, g_w, g_bias of rpo_lp_head_fwd_bwd against torch in float64, relative max error <= 1e-5, for
    B in {1, 3, 32, 100} x C in {1, 19, 37, 100, 397, 1000}; eval leaves loss / g_* alone; a bad label gives a NaN loss;
    two calls give the same bits; g_bias = g_w + e*e works.  Measured worst relmax (MI355X): e = 512 z 2.6e-7, logits 4.2e-7,
    loss 2.2e-7, g_w 5.9e-7, g_bias 5.9e-7; e = 768 3.4e-7, 4.5e-7, 1.7e-7, 4.9e-7, 4.0e-7."""
    from rpo_amd import ops
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    worst = {}
    for B in (1, 3, 32, 100):
        for C in (1, 19, 37, 100, 397, 1000):
            gen = torch.Generator().manual_seed(B * 10007 + C * 31 + e)
            x = torch.randn(B, e, generator=gen, dtype=torch.float64)
            w = torch.randn(e, e, generator=gen, dtype=torch.float64) * (0.02 / e ** 0.5) + 0.01 * torch.eye(e, dtype=torch.float64)
            bias = torch.randn(e, generator=gen, dtype=torch.float64) * 0.01
            t = torch.randn(C, e, generator=gen, dtype=torch.float64)
            t = t / t.norm(dim=1, keepdim=True)
            label = torch.randint(0, C, (B,), generator=gen)
            f = lambda a: a.float().to(dev).contiguous()
            xd, wd, bd, td, ld = f(x), f(w), f(bias), f(t), label.to(dev)
            x, w, bias, t = (a.float().double() for a in (x, w, bias, t))        # the fp32 inputs the kernel sees
            scale = 100.0
            z = torch.empty(B, e, device=dev)
            logits = torch.empty(B, C, device=dev)
            loss = torch.full((1,), -7.0, device=dev)
            g = torch.full((e * e + e,), -3.0, device=dev)
            ws = torch.empty(ops.lp_head_workspace_floats(B, C, e), device=dev)
            # eval: sentinels untouched
            ops.lp_head_fwd_bwd(xd, wd, bd, td, None, scale, z, logits, None, None, None, ws)
            torch.cuda.synchronize()
            assert float(loss.item()) == -7.0 and bool((g == -3.0).all())
            rz, rl, rloss, rgw, rgb = _lp_ref64(x, w, bias, t, label, scale)
            ez, el = _relmax(z.cpu(), rz), _relmax(logits.cpu(), rl)
            # training, flat [g_w | g_bias]
            ops.lp_head_fwd_bwd(xd, wd, bd, td, ld, scale, z, logits, loss, g[:e * e].view(e, e), g[e * e:], ws)
            torch.cuda.synchronize()
            first = (z.clone(), logits.clone(), loss.clone(), g.clone())
            errs = dict(z=ez, logits=el, loss=abs(loss.item() - rloss.item()) / max(abs(rloss.item()), 1e-30),
                        g_w=_relmax(g[:e * e].view(e, e).cpu(), rgw), g_bias=_relmax(g[e * e:].cpu(), rgb))
            for k, v in errs.items():
                worst[k] = max(worst.get(k, 0.0), v)
                assert v <= 1e-5, (B, C, e, k, v)
            ops.lp_head_fwd_bwd(xd, wd, bd, td, ld, scale, z, logits, loss, g[:e * e].view(e, e), g[e * e:], ws)
            torch.cuda.synchronize()
            for a, b in zip(first, (z, logits, loss, g)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (B, C, e, "not bit-identical")
            # an out-of-range target: NaN loss
            bad = ld.clone()
            bad[0] = C
            ops.lp_head_fwd_bwd(xd, wd, bd, td, bad, scale, z, logits, loss, g[:e * e].view(e, e), g[e * e:], ws)
            torch.cuda.synchronize()
            assert torch.isnan(loss).all(), (B, C, e)
    print(f"\nlp head e={e}: worst relmax", {k: f"{v:.2e}" for k, v in worst.items()})


# ---- 2. reference parity ------------------------------------------------------------------------------------------------
def _parity(act, cfg, sd, toks, w0, b0, image, label, ref, tag):
    from rpo_amd.lp import LPCustomCLIP
    B = image.shape[0]
    m = LPCustomCLIP(sd, toks, "cuda:0", act, max_batch=B, weight=w0, bias=b0, cfg=cfg)
    eng = m.engine
    with torch.cuda.device(eng.dev):
        logits = m(torch.from_numpy(image).cuda()).cpu().numpy()
        eng.lp_forward_backward(torch.from_numpy(image).cuda(), torch.from_numpy(label).cuda())
        torch.cuda.synchronize()
        loss = float(eng.loss.item())
        gw, gb = eng.lp_gw.cpu().numpy(), eng.lp_gb.cpu().numpy()
    rl = ref["logits"]
    rgw = ref["dz"].astype(np.float64).T @ ref["image_features"].astype(np.float64)
    scale = max(1.0, float(np.abs(rl).max()))
    la, ls, gr = {torch.float32: (F32_LOGIT, F32_LOSS, F32_GRAD), torch.float16: (F16_LOGIT_ATOL, F16_LOGIT_ATOL, F16_GRAD_REL),
                  torch.bfloat16: (BF16_LOGIT_ATOL, BF16_LOGIT_ATOL, BF16_GRAD_REL)}[act]
    el = float(np.abs(logits - rl).max())
    elo = abs(loss - float(ref["loss"])) / abs(float(ref["loss"]))
    egw, egb = _relmax(gw, rgw), _relmax(gb, ref["g_bias"])
    print(f"\n{tag} {act}: logits max abs {el:.3e} (bound {la * scale:.3e}), loss rel {elo:.2e}, g_w rel {egw:.2e}, "
          f"g_bias rel {egb:.2e}")
    assert el <= la * scale and elo <= ls and egw <= gr and egb <= gr
    top2 = np.sort(rl, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * la * scale           # (16-bit: only where the reference's margin is clear)
    if act == torch.float32:
        assert np.array_equal(logits.argmax(1), rl.argmax(1))
    else:
        assert np.array_equal(logits.argmax(1)[clear], rl.argmax(1)[clear])


@pytest.mark.gpu
@pytest.mark.parametrize("act", [torch.float32, torch.float16, torch.bfloat16])
def test_lp_matches_reference_d2(act):
    """Both (W, b) cases of ref_lp_d2_b3 (identity: saturated softmax; seeded W: logits O(1-10)): eval logits, loss,
    lp_layer's weight / bias gradients.  Measured (identity c0 / seeded c1): f32 logits max abs 4.3e-4 / 1.1e-5 (bounds
    1.5e-2 / 3.8e-4), loss rel 3.8e-7 / 1.4e-6, gradients rel 1.8e-6 / 3.5e-6; f16 logits 0.12 / 3.1e-3, loss 2.5e-5 /
    1.2e-4, gradients 8.7e-4 / 9.1e-4; bf16 logits 1.4 / 2.3e-2, loss 1.6e-3 / 7.4e-5, gradients 7.1e-3 / 1.1e-2."""
    from rpo_amd import synth
    g = np.load(os.path.join(GOLD, "ref_lp_d2_b3.npz"))
    cfg, sd, toks = lp_workload(2)
    assert np.array_equal(toks, g["tokenized_prompts"])
    image, label = synth.images(cfg, 3), g["label"]
    for case in (0, 1):
        w0, b0 = _case_init(g, case, cfg.embed)
        ref = {k: g[f"c{case}_{k}"] for k in ("logits", "loss", "dz", "g_bias")}
        ref["image_features"] = g["image_features"]
        _parity(act, cfg, sd, toks, w0, b0, image, label, ref, f"d2_b3 c{case}")


@pytest.mark.gpu
@pytest.mark.parametrize("act", [torch.float32, torch.bfloat16])
def test_lp_matches_reference_full_b32(act):
    """Full ViT-B/16, B = 32, identity init (ref_lp_full_b32).  Measured: f32 logits max abs 5.6e-4 (bound 2.2e-2), loss rel
    4.2e-6, gradients rel 4.0e-6; bf16 logits 1.2 (bound 26), loss 5.9e-3, gradients 1.4e-2."""
    from rpo_amd import synth
    g = dict(np.load(os.path.join(GOLD, "ref_lp_full_b32.npz")))
    cfg, sd, toks = lp_workload(12)
    e = cfg.embed
    _parity(act, cfg, sd, toks, np.eye(e, dtype=np.float32), np.zeros(e, np.float32), synth.images(cfg, 32), g["label"], g,
            "full_b32")


# ---- 3. trajectory, graph replay, epoch boundary --------------------------------------------------------------------------
def _run_traj(cfg, sd, toks, w0, b0, seeds, use_graph, act=torch.float32, B=3):
    from rpo_amd import synth
    from rpo_amd.lp import LP
    from rpo_amd.trainer import OptimConfig
    oc = OptimConfig(lr=5e-4, max_epoch=30, lr_scheduler="constant", warmup_epoch=0)     # torch.optim.SGD(lr=5e-4)
    tr = LP(sd, toks, oc, "cuda:0", act, batch_size=B, num_batches=10 ** 9, use_graph=use_graph, weight=w0, bias=b0,
            cfg=cfg, max_batch=B)
    losses = [tr.forward_backward({"img": torch.from_numpy(synth.images(cfg, B, seed=int(si))),
                                   "label": torch.from_numpy(synth.labels(cfg, B, seed=int(li)))})["loss"]
              for si, li in seeds]
    return tr, np.asarray(losses), tr.engine.lp_params.cpu().numpy()


@pytest.mark.gpu
def test_lp_trajectory_matches_reference_and_graph_is_bit_identical():
    """Four LP steps (f32) reproduce the reference's per-step losses (relative 1e-5: they reach ~1.4e3, where 1e-5 abs
    is below one fp32 ulp) and its final W and b within 1e-5 abs -- all of W as rebuilt from the reference's per-step
    gradient factors (tests/lp_fixtures.sgd_replay, checked against the reference's dense W by the generator), and its
    stored dense rows 0-7 and diagonal directly; with use_graph=True the bits equal eager.  Measured: losses rel 1.7e-6 /
    3.0e-6, W abs 1.8e-7 / 1.1e-7, b abs 4.2e-8 / 3.2e-8 (c0 / c1)."""
    g = np.load(os.path.join(GOLD, "ref_lp_d2_b3.npz"))
    cfg, sd, toks = lp_workload(2)
    e = cfg.embed
    lr, mom, wd = (float(v) for v in g["sgd_hparams"])
    for case in (0, 1):
        w0, b0 = _case_init(g, case, e)
        tr, losses, p = _run_traj(cfg, sd, toks, w0, b0, g["traj_seeds"], False)
        rl = g[f"c{case}_traj_losses"]
        rw, _, _, _ = sgd_replay(w0, b0, g[f"c{case}_traj_dz"], g[f"c{case}_traj_x"], lr, mom, wd)
        w = p[:e * e].reshape(e, e)
        nr = g[f"c{case}_w_final_rows"].shape[0]
        ew = max(float(np.abs(w - rw).max()), float(np.abs(w[:nr] - g[f"c{case}_w_final_rows"]).max()),
                 float(np.abs(np.diag(w) - g[f"c{case}_w_final_diag"]).max()))
        eb = float(np.abs(p[e * e:] - g[f"c{case}_b_final"]).max())
        el = float((np.abs(losses - rl) / np.abs(rl)).max())
        print(f"\ntraj c{case}: losses {losses.round(4).tolist()} (ref {rl.round(4).tolist()}) rel {el:.2e}, "
              f"W abs {ew:.2e}, b abs {eb:.2e}")
        assert el <= 1e-5 and ew <= 1e-5 and eb <= 1e-5
        _, lg, pg = _run_traj(cfg, sd, toks, w0, b0, g["traj_seeds"], True)
        assert np.array_equal(pg.view(np.uint32), p.view(np.uint32)) and np.array_equal(lg, losses), "graph != eager"
        del tr


@pytest.mark.gpu
def test_lp_epoch_boundary_updates_the_learning_rate():
    """update_lr() after the last batch of an epoch: the ctxv1 schedule goes from the 1e-5 warm-up to 5e-4."""
    from rpo_amd import synth
    from rpo_amd.lp import LP
    cfg, sd, toks = lp_workload(2)
    tr = LP(sd, toks, None, "cuda:0", torch.float32, batch_size=3, num_batches=2, use_graph=True, cfg=cfg, max_batch=3)
    lrs = [tr.lr]
    for s in range(3):
        tr.forward_backward({"img": torch.from_numpy(synth.images(cfg, 3, seed=900 + s)),
                             "label": torch.from_numpy(synth.labels(cfg, 3, seed=950 + s))})
        lrs.append(tr.lr)
    assert lrs == [1e-5, 1e-5, 5e-4, 5e-4] and tr.epoch == 1, lrs
    assert np.isfinite(tr.engine.lp_params.cpu().numpy()).all()


# ---- 4. checkpoints -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lp_load_reference_checkpoint_and_resume_bit_exact(tmp_path):
    """load_model on the reference's lp_layer checkpoint (rebuilt from ref_lp_ckpt.npz by
    tests/lp_fixtures.write_reference_checkpoint) reproduces the eval logits it gave there; save_model ->
    resume_model -> one more step equals an uninterrupted run bit for bit.  Measured: logits max abs 4.9e-4 at |logits| up
    to 724."""
    from rpo_amd import synth
    from rpo_amd.lp import LP
    from rpo_amd.trainer import OptimConfig
    cfg, sd, toks = lp_workload(2)
    ck = np.load(os.path.join(GOLD, "ref_lp_ckpt.npz"))
    tr = LP(sd, toks, None, "cuda:0", torch.float32, batch_size=3, cfg=cfg, max_batch=3)
    ref_dir = str(tmp_path / "ref")
    write_reference_checkpoint(os.path.join(GOLD, "ref_lp_ckpt.npz"), ref_dir)
    tr.load_model(ref_dir, epoch=1)
    logits = tr.model_inference(torch.from_numpy(synth.images(cfg, 3, seed=int(ck["image_seed"])))).cpu().numpy()
    err = float(np.abs(logits - ck["logits"]).max())
    print(f"\nreference checkpoint: eval logits max abs {err:.3e} (|logits| max {np.abs(ck['logits']).max():.1f})")
    assert err <= F32_LOGIT * max(1.0, float(np.abs(ck["logits"]).max()))
    assert np.array_equal(logits.argmax(1), ck["logits"].argmax(1))

    oc = OptimConfig(lr=5e-4, max_epoch=30, lr_scheduler="constant", warmup_epoch=0)
    batch = lambda s: {"img": torch.from_numpy(synth.images(cfg, 3, seed=1000 + s)),
                       "label": torch.from_numpy(synth.labels(cfg, 3, seed=1100 + s))}
    a = LP(sd, toks, oc, "cuda:0", torch.float32, batch_size=3, num_batches=10 ** 9, cfg=cfg, max_batch=3)
    a.forward_backward(batch(0))
    a.forward_backward(batch(1))
    a.save_model(str(tmp_path), epoch=0)
    a.forward_backward(batch(2))
    want = a.engine.lp_params.cpu().numpy()
    b = LP(sd, toks, oc, "cuda:0", torch.float32, batch_size=3, num_batches=10 ** 9, cfg=cfg, max_batch=3)
    assert b.resume_model(str(tmp_path), epoch=0) == 0
    b.forward_backward(batch(2))
    assert np.array_equal(b.engine.lp_params.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- 5. amp ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lp_amp_trains_finite_and_skips_a_nonfinite_step():
    """prec="amp" (f16 storage, guarded SGD): finite training; a batch whose image holds +Inf makes every gradient
    non-finite and that step is skipped (layer unchanged) and counted."""
    from rpo_amd import synth
    from rpo_amd.lp import LP
    cfg, sd, toks = lp_workload(2)
    tr = LP(sd, toks, None, "cuda:0", prec="amp", batch_size=3, cfg=cfg, max_batch=3)
    assert tr.amp and tr.engine.act == torch.float16
    for s in range(2):
        out = tr.forward_backward({"img": torch.from_numpy(synth.images(cfg, 3, seed=300 + s)),
                                   "label": torch.from_numpy(synth.labels(cfg, 3, seed=400 + s))})
        assert np.isfinite(out["loss"])
    before = tr.engine.lp_params.cpu().numpy()
    assert np.isfinite(before).all() and tr.skipped_steps == 0
    img = synth.images(cfg, 3, seed=302)
    img[0, 0, 0, 0] = np.inf
    tr.forward_backward({"img": torch.from_numpy(img), "label": torch.from_numpy(synth.labels(cfg, 3, seed=402))})
    assert tr.skipped_steps == 1
    assert np.array_equal(tr.engine.lp_params.cpu().numpy().view(np.uint32), before.view(np.uint32))


# ---- 6. data parallel -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lp_two_ranks_equal_one_rank_global_batch(tmp_path):
    """Two ranks on cuda:0 over gloo (RPO_ALL_RANKS_ON_GPU0=1), B = 2 each, 2 steps: the final W and b equal one process at
    B = 4 within 1e-6 relative (sum all-reduce of the flat [W | b] gradient, grad_scale 1/2).  Measured: 1.2e-7."""
    from rpo_amd import synth
    from rpo_amd.lp import LP
    cfg, sd, toks = lp_workload(2)
    tr = LP(sd, toks, DP_OPTIM(), "cuda:0", torch.float32, batch_size=4, num_batches=10 ** 9, cfg=cfg, max_batch=4)
    for si, li in DP_SEEDS:
        tr.forward_backward({"img": torch.from_numpy(synth.images(cfg, 4, seed=si)),
                             "label": torch.from_numpy(synth.labels(cfg, 4, seed=li))})
    want = tr.engine.lp_params.cpu().numpy()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "dp.npz")
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    base.update(RPO_DIST_BACKEND="gloo", RPO_ALL_RANKS_ON_GPU0="1", HSA_ENABLE_IPC_MODE_LEGACY="0", WORLD_SIZE="2",
                MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2")
    worker = os.path.join(ROOT, "tests", "lp_dp_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, out, "4", "2"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True, env=dict(base, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=600)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-2000:] for l in logs)
    got = np.load(out)
    assert int(got["world"]) == 2
    err = _relmax(got["params"], want)
    print(f"\ndp2 vs one process: relmax {err:.2e}")
    assert err <= 1e-6
