"""The shared members' bookkeeping (rpo_amd/members.py) on the device: `RPOSweep` now uploads a new epoch's rates at the end of
the epoch (`MemberScheduleMixin.update_lr`) and no longer in front of the next step; both are on the step's stream ahead of
that step's launches, so the device must see the same table before the same launch."""
import numpy as np
import pytest
import torch

import test_gpu_multi as M

pytestmark = pytest.mark.gpu

DEV, same = M.DEV, M.same


def test_sweep_epoch_rates_reach_the_device_before_the_next_step_on_both_paths():
    """Depth 1, members K = (1, 2) -- one plain SGD, one Adam, so the optimiser is table-driven -- batch 2, two batches per
    epoch, two epochs: per-step `forward_backward` and `run_epoch` on the same batches end with equal bits in `m_params`,
    `m_mom`, Adam's second row and every returned loss, and after each epoch the optimiser's `hyper` table is
    `hyper_table(optim_cfgs, epoch)` of the epoch that starts."""
    from rpo_amd import optim
    from rpo_amd.input_pipeline import DeviceImageSet, InputConfig, build_transform
    from rpo_amd.loop import epoch_indices
    from rpo_amd.sweep import RPOSweep
    from rpo_amd.trainer import OptimConfig, lr_at_epoch
    S, B, nb, epochs, Ks = 2, 2, 2, 2, (1, 2)
    cfg, sd, toks = M._workload(1, max(Ks))
    ocs = [OptimConfig(lr=0.01, weight_decay=5e-4, max_epoch=4, warmup_epoch=1), OptimConfig(name="adam", lr=1e-3, max_epoch=4)]

    def sweep():
        members = [dict(prompts=M._member(M._workload(1, Ks[s])[0], sd, s, B)[0], K=Ks[s], optim=ocs[s]) for s in range(S)]
        return RPOSweep(cfg, sd, toks, members=members, batch_size=B, device=DEV, act_dtype=torch.float32, num_batches=nb)

    def table_is_of(tr, epoch):
        assert tr._opt.table_driven and tr._opt.epoch == tr.epoch == epoch
        return torch.equal(M.bits(tr._opt.hyper), M.bits(optim.hyper_table(ocs, epoch)))

    sizes = [B * nb, B * nb + 1]
    imgs = [M._decoded(n, seed=160 + s) for s, n in enumerate(sizes)]
    labs = [np.random.default_rng(170 + s).integers(0, cfg.n_cls, n).tolist() for s, n in enumerate(sizes)]
    sets = [DeviceImageSet(imgs[s], labs[s], DEV) for s in range(S)]
    stage = build_transform(InputConfig(SIZE=(224, 224)), True, DEV, B)
    torch.manual_seed(5)
    order = [[epoch_indices(sizes[s], B, g) for g in [torch.Generator().manual_seed(140 + s)] * epochs] for s in range(S)]
    plans = [[[[stage.plan(*imgs[s][i].shape[:2]) for i in batch] for batch in ep] for ep in order[s]] for s in range(S)]
    seq, seq_loss = sweep(), []
    assert table_is_of(seq, 0)
    for ep in range(epochs):
        for t in range(nb):
            batches = [{"img": stage([imgs[s][i] for i in order[s][ep][t]], plans[s][ep][t]).clone(),
                        "label": torch.tensor([labs[s][i] for i in order[s][ep][t]])} for s in range(S)]
            seq_loss.append([np.float32(o["loss"]) for o in seq.forward_backward(batches)])
        assert table_is_of(seq, ep + 1), f"forward_backward: the table after epoch {ep}"
    tr, losses = sweep(), []
    gens = [torch.Generator().manual_seed(140 + s) for s in range(S)]
    for ep in range(epochs):
        out = tr.run_epoch(sets, gens, [plans[s][ep] for s in range(S)])
        assert out["indices"] == [order[s][ep] for s in range(S)] and out["loss"].shape == (nb, S)
        losses.append(out["loss"])
        assert table_is_of(tr, ep + 1), f"run_epoch: the table after epoch {ep}"
    torch.cuda.synchronize()
    got = torch.cat(losses).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), np.array(seq_loss, np.float32).view(np.uint32)), "per-step, per-member losses"
    assert same(tr.engine.m_params, seq.engine.m_params) and same(tr.engine.m_mom, seq.engine.m_mom)
    assert same(tr._opt.s1, seq._opt.s1) and tr._opt.steps() == seq._opt.steps()
    assert tr.lr == seq.lr == [lr_at_epoch(oc, epochs) for oc in ocs] and tr._steps == seq._steps == nb * epochs
    assert tr.captures == seq.captures == 1                        # rates are device data: one graph serves every epoch
