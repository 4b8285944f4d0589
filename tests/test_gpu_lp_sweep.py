"""`LPSweep` (rpo_amd/lp_sweep.py) against standalone `LP` runs, bit for bit: every member of a sweep
ends every step where `LP(optim=that member's)` on the same batches ends it, its checkpoints are that run's files in both
directions, and its evaluation returns that run's integers.  Standalone `LP` is pinned to the reference in
tests/test_gpu_lp.py, so nothing here has a tolerance.  Depth-2 workload of that file, B = 3."""
import functools

import numpy as np
import pytest
import torch

from lp_fixtures import c1_init
from test_gpu_loop import _decoded, _staging
from test_gpu_lp import lp_workload

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, NB, EPOCHS = 3, 3, 2
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _bits(t):
    return torch.as_tensor(t).detach().cpu().contiguous().view(torch.int32)


def _members(e, max_epoch=4):
    """Plain SGD; SGD with weight decay and Nesterov; Adam started from the seeded layer of the LP fixtures."""
    from rpo_amd.trainer import OptimConfig
    w1, b1 = c1_init(e)
    return [dict(optim=OptimConfig(lr=5e-4, max_epoch=max_epoch, warmup_epoch=1, warmup_cons_lr=1e-5)),
            dict(optim=OptimConfig(lr=2e-3, momentum=0.8, weight_decay=5e-4, sgd_nesterov=True, max_epoch=max_epoch,
                                   warmup_epoch=1, warmup_cons_lr=2e-5)),
            dict(optim=OptimConfig(name="adam", lr=1e-3, max_epoch=max_epoch, warmup_epoch=1, warmup_cons_lr=1e-4),
                 weight=w1, bias=b1)]


def _batch(cfg, i):
    from rpo_amd import synth
    return {"img": torch.from_numpy(synth.images(cfg, B, seed=2000 + i)), "label": torch.from_numpy(synth.labels(cfg, B, seed=2100 + i))}


def _same_checkpoint(got, want, what):
    """Two `checkpoint_dict`s: the same keys, and the layer, the optimiser state and the bookkeeping equal (tensors as bits)."""
    assert list(got) == list(want), what
    for k in ("epoch", "steps", "scheduler", "val_result"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("weight", "bias"):
        assert torch.equal(_bits(got["state_dict"][k]), _bits(want["state_dict"][k])), (what, k)
    go, wo = got["optimizer"], want["optimizer"]
    assert go["param_groups"] == wo["param_groups"], (what, go["param_groups"], wo["param_groups"])
    assert list(go["state"]) == list(wo["state"]), what
    for i in go["state"]:
        assert list(go["state"][i]) == list(wo["state"][i]), (what, i)
        for k, v in go["state"][i].items():
            assert torch.equal(_bits(v), _bits(wo["state"][i][k])), (what, "optimizer state", i, k)


@functools.lru_cache(maxsize=None)
def _standalone(mode: str, amp: bool = False):
    """Three standalone `LP` runs (eager) of EPOCHS x NB steps on the seeded batches: per member (per-step losses as float32
    bits, checkpoint_dict, eval logits of batch 0, skipped steps).  Computed once per storage mode, shared, left unchanged."""
    from rpo_amd.lp import LP
    cfg, sd, toks = lp_workload(2)
    members = _members(cfg.embed)
    if amp:                 # plain SGD | Adam from 1e38 I (every step of it overflows) | SGD with weight decay and Nesterov
        members = [members[0], dict(optim=members[2]["optim"], weight=1e38 * np.eye(cfg.embed, dtype=np.float32)), members[1]]
    out = []
    for m in members:
        tr = LP(sd, toks, m["optim"], DEV, DT[mode], batch_size=B, num_batches=NB, amp=amp, weight=m.get("weight"),
                bias=m.get("bias"), cfg=cfg, max_batch=5)
        losses = [np.float32(tr.forward_backward(_batch(cfg, i))["loss"]) for i in range(EPOCHS * NB)]
        logits = tr.model_inference(_batch(cfg, 0)["img"]).cpu()
        out.append((np.asarray(losses, np.float32), tr.checkpoint_dict(), logits, tr.skipped_steps, tr.lr))
        del tr
    return members, out


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_every_member_steps_as_its_standalone_lp(mode, use_graph):
    """2 epochs of 3 batches through forward_backward: per member the per-step losses and every tensor of checkpoint_dict
    (layer and optimiser state) have the standalone run's bits; the learning rates behind the epoch boundary are each
    member's own lr_at_epoch; with use_graph the step is captured once although every rate changed."""
    from rpo_amd.lp_sweep import LPSweep
    from rpo_amd.trainer import lr_at_epoch
    cfg, sd, toks = lp_workload(2)
    members, solo = _standalone(mode)
    sw = LPSweep(sd, toks, members, DEV, DT[mode], batch_size=B, num_batches=NB, use_graph=use_graph, cfg=cfg, max_batch=5)
    assert sw.lr == [1e-5, 2e-5, 1e-4]
    losses = np.asarray([sw.forward_backward(_batch(cfg, i))["loss"] for i in range(EPOCHS * NB)], np.float32)     # [steps, S]
    assert sw.epoch == EPOCHS and sw.batch_idx == 0 and sw._steps == EPOCHS * NB
    assert sw.lr == [lr_at_epoch(m["optim"], EPOCHS) for m in members] and len(set(sw.lr)) == 3
    assert sw.captures == (1 if use_graph else 0), "the rates are device data: one capture serves every epoch"
    assert sw.skipped_steps() == [0, 0, 0]
    for s, (want_losses, want_ck, want_logits, _, want_lr) in enumerate(solo):
        what = f"{mode} graph={use_graph} member {s}"
        assert np.array_equal(losses[:, s].view(np.uint32), want_losses.view(np.uint32)), \
            (what, "per-step losses", losses[:, s].tolist(), want_losses.tolist())
        _same_checkpoint(sw.checkpoint_dict(s), want_ck, what)
        assert sw.lr[s] == want_lr
        got = sw.model_inference(_batch(cfg, 0)["img"], member=s).cpu()
        assert torch.equal(_bits(got), _bits(want_logits)), (what, "model_inference")
    # the members differ (a sweep whose members agree would prove nothing)
    p = sw.engine.lps_params.cpu()
    assert not torch.equal(p[0], p[1]) and not torch.equal(p[0], p[2])


def test_amp_skips_per_member():
    """fp16 + amp, three members; the Adam member starts from 1e38 I: its z overflows, its gradients are not finite, every
    one of its steps is skipped and counted -- its row keeps its bits, its optimiser state stays zero and its device step
    counter is not advanced -- while the other two members equal their standalone LP(amp) runs."""
    from rpo_amd.lp_sweep import LPSweep
    cfg, sd, toks = lp_workload(2)
    members, solo = _standalone("f16", True)
    assert members[1]["optim"].name == "adam"
    sw = LPSweep(sd, toks, members, DEV, prec="amp", batch_size=B, num_batches=NB, cfg=cfg, max_batch=5)
    assert sw.amp and sw.engine.act == torch.float16
    before = sw.engine.lps_params[1].clone()
    n = EPOCHS * NB
    losses = np.asarray([sw.forward_backward(_batch(cfg, i))["loss"] for i in range(n)], np.float32)
    assert sw.skipped_steps() == [0, n, 0]
    assert torch.equal(_bits(sw.engine.lps_params[1]), _bits(before)), "a skipped member's row changed"
    assert sw._opt.steps() == [n, 0, n], "a skipped step advanced the member's step counter"
    for row in sw._opt._state():
        assert row is None or not bool(row[1].any()), "a skipped step wrote optimiser state"
    assert not np.isfinite(losses[:, 1]).any()
    for s in (0, 2):
        want_losses, want_ck, _, skipped, _ = solo[s]
        assert skipped == 0 and np.array_equal(losses[:, s].view(np.uint32), want_losses.view(np.uint32)), s
        _same_checkpoint(sw.checkpoint_dict(s), want_ck, f"amp member {s}")
    assert solo[1][3] == n                                               # (the standalone run skips them too)


def _image_set(n, seed, n_cls):
    from rpo_amd.input_pipeline import DeviceImageSet
    imgs = _decoded(n, seed)
    labels = np.random.default_rng(seed + 1).integers(0, n_cls, n).tolist()
    return imgs, DeviceImageSet(imgs, labels, DEV)


def _same_result(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if k == "confusion_matrix":
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def test_epoch_loop_checkpoints_and_shared_evaluation(tmp_path):
    """train() for 2 epochs on a 12-image set with a validation set on cached features; per member the files load into a
    standalone LP, which evaluates to the same integers and whose resumed third epoch equals the sweep's bit for bit;
    model-best is each member's own best epoch."""
    from rpo_amd.features import ImageFeatures
    from rpo_amd.loop import epoch_indices
    from rpo_amd.lp import LP
    from rpo_amd.lp_sweep import LPSweep
    from rpo_amd.trainer import load_checkpoint_file
    cfg, sd, toks = lp_workload(2)
    n, nb = 12, 4
    imgs, train_set = _image_set(n, 61, cfg.n_cls)
    _, V = _image_set(n, 71, cfg.n_cls)
    members = _members(cfg.embed, max_epoch=3)
    stage = _staging(True, B)
    torch.manual_seed(7)
    g_plan = torch.Generator().manual_seed(40)
    order = [epoch_indices(n, B, g_plan) for _ in range(3)]
    plans = [[[stage.plan(*imgs[i].shape[:2]) for i in batch] for batch in ep] for ep in order]

    sw = LPSweep(sd, toks, members, DEV, torch.float32, batch_size=B, num_batches=nb, use_graph=True, cfg=cfg, max_batch=5)
    F = ImageFeatures.build(sw, V)
    dirs = [str(tmp_path / f"best{s}") for s in range(3)]
    gen = torch.Generator().manual_seed(40)
    hist = sw.train(train_set, max_epoch=2, val_set=V, val_features=F, directories=dirs, generator=gen, verbose=False,
                    plans=plans[:2])
    assert [h["epoch"] for h in hist] == [1, 2] and sw.epoch == 2 and sw.captures == 1
    assert all(len(h["loss"]) == 3 and len(h["val_acc"]) == 3 for h in hist)
    for s in range(3):                                                   # model-best: the member's own best epoch
        accs = [h["val_acc"][s] for h in hist]
        best = 1 + int(np.argmax(accs))                                  # (the first of equals: `>` keeps the earlier)
        ck = load_checkpoint_file(str(tmp_path / f"best{s}" / "lp_layer" / "model-best.pth.tar"))
        assert ck["epoch"] == best and ck["val_result"] == accs[best - 1] == sw.best_results[s], (s, accs, ck["epoch"])
    # ---- the state behind epoch 2, member by member, in a standalone LP
    last = [str(tmp_path / f"last{s}") for s in range(3)]
    sw.save_model(last)
    all_live, all_cached = sw.test_all(V, verbose=False), sw.test_all(V, features=F, verbose=False)
    solos = []
    for s, m in enumerate(members):
        lp = LP(sd, toks, m["optim"], DEV, torch.float32, batch_size=B, num_batches=nb, cfg=cfg, max_batch=5)
        assert lp.resume_model(last[s], epoch=2) == 2
        _same_checkpoint(lp.checkpoint_dict(), sw.checkpoint_dict(s), f"member {s} resumed")
        want = lp.test(V, features=F, verbose=False)
        _same_result(all_live[s], want, f"test_all(V)[{s}]")
        _same_result(all_cached[s], want, f"test_all(V, features=F)[{s}]")
        assert want["total"] == n and want["confusion_matrix"].sum() == n
        solos.append(lp)
    _same_result(sw.test(V, member=1, features=F, verbose=False), all_cached[1], "test(member=1)")
    # ---- a third epoch: the sweep's, and each resumed standalone run's on the same order and plans
    state = gen.get_state()
    res = sw.run_epoch(train_set, gen, plans[2])
    assert res["indices"] == order[2] and tuple(res["loss"].shape) == (nb, 3)
    for s, lp in enumerate(solos):
        g = torch.Generator()
        g.set_state(state)
        out = lp.run_epoch(train_set, g, plans[2])
        assert out["indices"] == order[2]
        assert torch.equal(_bits(out["loss"]), _bits(res["loss"][:, s])), (s, "third-epoch losses")
        _same_checkpoint(lp.checkpoint_dict(), sw.checkpoint_dict(s), f"member {s} after the third epoch")
    # ---- and back: the standalone files load into a sweep
    back = [str(tmp_path / f"back{s}") for s in range(3)]
    for lp, d in zip(solos, back):
        lp.save_model(d)
    sw2 = LPSweep(sd, toks, members, DEV, torch.float32, batch_size=B, num_batches=nb, cfg=cfg, max_batch=5)
    sw2.load_model(back, epoch=3)
    for s in range(3):
        _same_checkpoint(sw2.checkpoint_dict(s), sw.checkpoint_dict(s), f"member {s} loaded from a standalone file")
