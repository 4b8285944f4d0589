"""Host-side checks of the epoch loops: the train loader's order against torch.utils.data itself, the evaluator's
metrics against a float64 restatement, the packing plan of a device-resident set, and the control flow of `run_epoch`
against a recording fake trainer.  No GPU."""
import re

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from rpo_amd.evaluator import Classification
from rpo_amd.input_pipeline import plan_packing
from rpo_amd.loop import LoopMixin, epoch_indices
from rpo_amd.optim import make_optimizer
from rpo_amd.trainer import OptimConfig, lr_at_epoch


# ---- 1. epoch_indices == DataLoader(range(n), batch_size, shuffle=True, drop_last=True) ---------------------------------

LOADER_CASES = [(12, 4, 0), (13, 4, 1), (3, 4, 2), (304, 32, 3), (100, 7, 5), (1, 1, 11), (64, 64, 7)]


@pytest.mark.parametrize("n,bs,seed", LOADER_CASES)
def test_epoch_indices_with_generator(n, bs, seed):
    g = torch.Generator()
    g.manual_seed(seed)
    ref = [b.tolist() for b in DataLoader(range(n), bs, shuffle=True, drop_last=True, generator=g)]
    ref_next = torch.empty((), dtype=torch.int64).random_(generator=g).item()
    g2 = torch.Generator()
    g2.manual_seed(seed)
    got = epoch_indices(n, bs, g2)
    assert got == ref
    assert len(got) == n // bs and all(len(b) == bs for b in got)
    assert torch.empty((), dtype=torch.int64).random_(generator=g2).item() == ref_next


@pytest.mark.parametrize("n,bs,seed", LOADER_CASES)
def test_epoch_indices_global_rng(n, bs, seed):
    torch.manual_seed(seed)
    ref = [b.tolist() for b in DataLoader(range(n), bs, shuffle=True, drop_last=True)]
    ref_next = torch.rand(4).tolist()
    torch.manual_seed(seed)
    got = epoch_indices(n, bs)
    assert got == ref
    assert torch.rand(4).tolist() == ref_next


def test_epoch_indices_two_epochs_continue_the_stream():
    g, g2 = torch.Generator(), torch.Generator()
    g.manual_seed(9)
    g2.manual_seed(9)
    dl = DataLoader(range(23), 5, shuffle=True, drop_last=True, generator=g)
    for _ in range(3):
        assert epoch_indices(23, 5, g2) == [b.tolist() for b in dl]


# ---- 2. evaluator --------------------------------------------------------------------------------------------------------

def _restate(y_true, y_pred, n_cls):
    """float64 restatement from the lists: Dassl's accuracy, sklearn's macro F1 over np.unique(y_true), per-class recall.
    A sample whose label is outside [0, n_cls) counts in the total only."""
    total = len(y_true)
    correct = sum(1 for t, p in zip(y_true, y_pred) if t == p and 0 <= t < n_cls)
    pairs = [(t, p) for t, p in zip(y_true, y_pred) if 0 <= t < n_cls]
    f1s, recs = [], []
    for c in sorted({t for t, _ in pairs}):
        tp = float(sum(1 for t, p in pairs if t == c and p == c))
        n_pred = float(sum(1 for _, p in pairs if p == c))
        n_true = float(sum(1 for t, _ in pairs if t == c))
        P = tp / n_pred if n_pred else 0.0
        R = tp / n_true
        f1s.append(2 * P * R / (P + R) if P + R > 0 else 0.0)
        recs.append(R)
    acc = 100.0 * correct / total
    return dict(total=total, correct=correct, accuracy=acc, error_rate=100.0 - acc,
                macro_f1=100.0 * float(np.mean(f1s)) if f1s else 0.0,
                mean_perclass_accuracy=100.0 * float(np.mean(recs)) if recs else 0.0)


EVAL_CASES = {
    "predicted_but_absent": ([0, 0, 1, 1, 1], [0, 2, 1, 1, 2], 3),          # class 2 never true: not in the macro mean
    "never_predicted": ([0, 1, 2, 2, 1, 0], [0, 0, 0, 0, 1, 0], 3),         # class 2 never predicted: F1 0
    "all_wrong": ([0, 1, 2, 3], [1, 2, 3, 0], 4),
    "one_class": ([0, 0, 0], [0, 0, 0], 1),
    "out_of_range": ([0, 5, -1, 1, 1, 2], [0, 1, 1, 1, 0, 2], 3),
    "mixed": ([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5], [3, 1, 4, 2, 5, 9, 2, 5, 5, 3, 6], 10),
}


@pytest.mark.parametrize("case", sorted(EVAL_CASES))
def test_evaluator_metrics(case, capsys):
    y_true, y_pred, n_cls = EVAL_CASES[case]
    ev = Classification(n_cls)
    ev.process(y_pred[:2], y_true[:2])                      # two calls: the evaluator accumulates
    ev.process(y_pred[2:], y_true[2:])
    res = ev.evaluate()
    ref = _restate(y_true, y_pred, n_cls)
    assert res["total"] == ref["total"] and res["correct"] == ref["correct"]
    for k in ("accuracy", "error_rate", "macro_f1", "mean_perclass_accuracy"):
        assert abs(res[k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), (k, res[k], ref[k])
    # the same from device-style counts + a flat confusion matrix
    ev2 = Classification(n_cls)
    cm = np.zeros((n_cls, n_cls), dtype=np.int32)
    for t, p in zip(y_true, y_pred):
        if 0 <= t < n_cls:
            cm[t, p] += 1
    ev2.process_counts(np.array([ref["correct"], ref["total"]], dtype=np.int64), cm.reshape(-1))
    res2 = ev2.evaluate(verbose=False)
    assert all(res2[k] == res[k] for k in ("total", "correct", "accuracy", "error_rate", "macro_f1"))
    # the lines the reference's parse_test_res.py reads: "* <keyword>: <number>%"
    out = capsys.readouterr().out
    for keyword, key in (("accuracy", "accuracy"), ("error", "error_rate"), ("macro_f1", "macro_f1")):
        m = re.compile(fr"\* {keyword}: ([\.\deE+-]+)%").search(out)
        assert m is not None, (keyword, out)
        assert abs(float(m.group(1)) - ref[key]) <= 0.05 + 1e-9
    ev.reset()
    assert ev.total == 0 and ev.correct == 0 and not ev.cmat.any()


# ---- 3. packing plan -------------------------------------------------------------------------------------------------------

def _check_plan(sizes, plan):
    spans = sorted((o, o + h * w * 3) for (h, w), o in zip(sizes, plan.offsets) if o >= 0)
    assert all(o % 16 == 0 for o, _ in spans)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert not spans or spans[-1][1] <= plan.resident_bytes


def test_packing_plan_alignment_and_budget():
    sizes = [(375, 500), (333, 500), (1, 1), (7, 5), (500, 375), (224, 224), (3, 3)]
    plan = plan_packing(sizes)
    _check_plan(sizes, plan)
    assert plan.spilled == [] and plan.tail_bytes == 0
    assert plan.offsets[0] == 0 and plan.offsets[2] == plan.offsets[1] + (333 * 500 * 3 + 15) // 16 * 16

    budget = 375 * 500 * 3 + 600                            # the first image, then only the small ones fit
    plan = plan_packing(sizes, budget)
    _check_plan(sizes, plan)
    assert plan.spilled == [1, 4, 5] and plan.resident_bytes <= budget
    al = lambda h, w: (h * w * 3 + 15) // 16 * 16
    assert plan.tail_bytes == al(333, 500) + al(500, 375) + al(224, 224)
    assert plan_packing(sizes, budget, max_batch=2).tail_bytes == al(333, 500) + al(500, 375)
    assert plan_packing(sizes, 0).spilled == list(range(len(sizes)))


def test_packing_plan_offsets_past_4gib():
    sizes = [(4000, 6000)] * 70                             # 72 MB each: 5 GB in all (plan only, nothing is allocated)
    plan = plan_packing(sizes)
    _check_plan(sizes, plan)
    assert plan.offsets[-1] > 2 ** 32 and plan.resident_bytes == 70 * 72_000_000
    assert plan.offsets[-1] == 69 * 72_000_000


# ---- 4. run_epoch's control flow against a recording fake -------------------------------------------------------------------

class _NoRead(torch.Tensor):
    """A loss scalar that records every attempt to read it on the host."""
    reads = []

    def item(self):
        _NoRead.reads.append("item")
        return super().item()

    def __float__(self):
        _NoRead.reads.append("float")
        return super().__float__()

    def tolist(self):
        _NoRead.reads.append("tolist")
        return super().tolist()


class _Cfg:
    n_cls, image_size = 5, 8


class _FakeSet:
    def __init__(self, n):
        self.labels = [i % 5 for i in range(n)]
        self.labels_dev = torch.tensor(self.labels)

    def __len__(self):
        return len(self.labels)

    def check_labels(self, n_cls):
        self.checked = n_cls


class _FakeTrainer(LoopMixin):
    def __init__(self, batch_size, num_batches, takes_next, reports_acc):
        self.cfg, self.device = _Cfg(), torch.device("cpu")
        self.batch_size, self.num_batches = batch_size, num_batches
        self._takes_next_image, self._reports_acc = takes_next, reports_acc
        self.optim_cfg = OptimConfig()
        self.epoch = self.batch_idx = 0
        self.lr = lr_at_epoch(self.optim_cfg, 0)
        self._opt = make_optimizer([self.optim_cfg], 1, 1, 0, "cpu")
        self.log, self.lr_updates = [], 0
        self._bufs = [torch.zeros(batch_size, 3, 8, 8) for _ in range(2)]

    # the device pieces of LoopMixin, on the CPU
    def _loop_buffers(self):
        return self._bufs

    def _loop_fill(self, image_set, indices, plans, out):
        out.fill_(float(indices[0]))                        # the buffer now "holds" this batch
        self.log.append(("fill", id(out), tuple(indices), plans))

    def _loop_labels(self, image_set, batches):
        return image_set.labels_dev[torch.tensor(batches)]

    def _loop_new_losses(self, nb):
        return torch.zeros(nb)

    def _loop_new_counts(self):
        return torch.zeros(2, dtype=torch.int64)

    def _loop_accumulate(self, label, counts):
        self.log.append(("acc", tuple(label.tolist())))
        counts += torch.tensor([1, label.numel()])

    def _loop_device(self):
        import contextlib
        return contextlib.nullcontext()

    def step_async(self, image, label, **kw):
        assert self._takes_next_image or not kw
        nxt = kw.get("next_image")
        self.log.append(("step", id(image), float(image[0, 0, 0, 0]), None if nxt is None else id(nxt),
                         tuple(label.tolist()), self.lr, "next_image" in kw))
        return torch.tensor([float(len(self.log))]).as_subclass(_NoRead)


class _FakeRPO(_FakeTrainer):
    def update_lr(self):
        self.lr_updates += 1
        self.epoch += 1
        self.lr = lr_at_epoch(self.optim_cfg, self.epoch)


@pytest.mark.parametrize("kind", ["rpo", "coop"])
def test_run_epoch_control_flow(kind):
    bs, nb = 4, 3
    ds = _FakeSet(bs * nb + 2)                              # 14 images: the last partial batch is dropped
    tr = _FakeRPO(bs, nb, True, False) if kind == "rpo" else _FakeTrainer(bs, nb, False, True)
    _NoRead.reads.clear()
    g, g_ref = torch.Generator(), torch.Generator()
    g.manual_seed(4)
    g_ref.manual_seed(4)
    expect = epoch_indices(len(ds), bs, g_ref)
    for epoch in range(2):
        tr.log.clear()
        plans = [[("plan", epoch, t, i) for i in range(bs)] for t in range(nb)]
        out = tr.run_epoch(ds, g, plans)
        if epoch == 1:
            expect = epoch_indices(len(ds), bs, g_ref)
        assert out["indices"] == expect and ds.checked == 5
        steps = [e for e in tr.log if e[0] == "step"]
        fills = [e for e in tr.log if e[0] == "fill"]
        assert len(steps) == nb and len(fills) == nb
        assert [f[2] for f in fills] == [tuple(b) for b in expect] and [f[3] for f in fills] == plans
        for t, s in enumerate(steps):
            assert s[1] == id(tr._bufs[t & 1])                                  # buffers alternate
            assert s[2] == float(expect[t][0])                                  # ... and hold batch t when step t runs
            assert s[4] == tuple(ds.labels[i] for i in expect[t])
            assert s[5] == lr_at_epoch(tr.optim_cfg, epoch)                     # the epoch's rate for every step of it
            if kind == "rpo":
                assert s[6]                                                     # next_image is always named ...
                if t + 1 < nb:
                    assert s[3] == steps[t + 1][1] == id(tr._bufs[(t + 1) & 1])  # ... and is the next call's image
                else:
                    assert s[3] is None                                         # but not behind the epoch's last batch
            else:
                assert not s[6]
        # batch t + 1 is filled BEFORE step t is enqueued
        order = [e[0] for e in tr.log if e[0] in ("fill", "step")]
        assert order == ["fill", "fill", "step", "fill", "step", "step"]
        assert tr.epoch == epoch + 1 and tr.batch_idx == 0 and tr.lr == lr_at_epoch(tr.optim_cfg, epoch + 1)
        if kind == "rpo":
            assert tr.lr_updates == epoch + 1 and "counts" not in out
        else:
            assert out["counts"].tolist() == [nb, nb * bs]
            assert [e[1] for e in tr.log if e[0] == "acc"] == [s[4] for s in steps]
        assert out["loss"].shape == (nb,) and torch.all(out["loss"] > 0)
    assert _NoRead.reads == [], f"the loop read a device scalar: {_NoRead.reads}"


def test_run_epoch_refuses_a_set_of_another_length():
    tr = _FakeTrainer(4, 3, False, False)
    with pytest.raises(ValueError, match="num_batches"):
        tr.run_epoch(_FakeSet(17))                          # 4 batches of 4
    with pytest.raises(ValueError, match="num_batches"):
        tr.run_epoch(_FakeSet(11))                          # 2 batches of 4
    tr.batch_idx = 1
    with pytest.raises(RuntimeError, match="epoch boundary"):
        tr.run_epoch(_FakeSet(12))
