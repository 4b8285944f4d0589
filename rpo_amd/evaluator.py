"""Dassl's `Classification` evaluator on a confusion matrix.

The reference's test loop (`TrainerBase.test`, un-vendored Dassl) feeds every batch's logits to
`Classification.process(output, label)` -- `pred = output.max(1)[1]`, correct / total, the lists behind
`sklearn.metrics.f1_score(average="macro", labels=np.unique(y_true))` -- and `evaluate()` prints the `* accuracy: X%`
lines that `parse_test_res.py:126-130` reads back.  Here the per-batch half is `rpo_eval_accumulate` (integer sums in
device buffers); this module is the host half: numpy on the counts and the confusion matrix, read back once.

Dassl and sklearn are not dependencies of this package: the metrics are restated from their published behaviour.

A sample whose label lies outside [0, n_cls) counts in `total`, is never correct and has no cell in the matrix, so it
takes no part in the per-class figures.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional, Sequence

import numpy as np


def confusion_matrix(y_true: Sequence[int], y_pred: Sequence[int], n_cls: int) -> np.ndarray:
    """int64 [n_cls, n_cls], row = true class; pairs with a label outside [0, n_cls) are left out."""
    cm = np.zeros((n_cls, n_cls), dtype=np.int64)
    for t, p in zip(y_true, y_pred):
        if 0 <= int(t) < n_cls and 0 <= int(p) < n_cls:
            cm[int(t), int(p)] += 1
    return cm


def metrics(correct: int, total: int, cmat: Optional[np.ndarray]) -> "OrderedDict[str, float]":
    """accuracy = 100 correct / total, error_rate = 100 - accuracy; from the matrix: macro_f1 = 100 x the mean over
    the classes PRESENT IN THE TRUE LABELS of 2PR / (P + R) (0 where P + R = 0, sklearn's zero-division default),
    per-class accuracy (recall) of those classes and its mean."""
    out: "OrderedDict[str, float]" = OrderedDict()
    out["total"], out["correct"] = int(total), int(correct)
    acc = 100.0 * float(correct) / float(total) if total > 0 else 0.0
    out["accuracy"], out["error_rate"] = acc, 100.0 - acc
    if cmat is None:
        return out
    cm = np.asarray(cmat, dtype=np.float64)
    tp = np.diag(cm)
    n_true, n_pred = cm.sum(1), cm.sum(0)
    present = n_true > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(n_pred > 0, tp / n_pred, 0.0)
        rec = np.where(n_true > 0, tp / n_true, 0.0)
        f1 = np.where(prec + rec > 0, 2.0 * prec * rec / (prec + rec), 0.0)
    out["macro_f1"] = 100.0 * float(f1[present].mean()) if present.any() else 0.0
    out["perclass_accuracy"] = {int(c): 100.0 * float(rec[c]) for c in np.nonzero(present)[0]}
    out["mean_perclass_accuracy"] = 100.0 * float(rec[present].mean()) if present.any() else 0.0
    return out


class Classification:
    """`reset()` / `process(...)` / `evaluate()` as Dassl's evaluator; `process_counts` takes what
    `rpo_eval_accumulate` summed on the device."""

    def __init__(self, n_cls: int, per_class_result: bool = False, classnames: Optional[Sequence[str]] = None):
        self.n_cls, self.per_class_result, self.classnames = int(n_cls), per_class_result, classnames
        self.reset()

    def reset(self) -> None:
        self.correct = self.total = 0
        self.cmat = np.zeros((self.n_cls, self.n_cls), dtype=np.int64)

    def process(self, y_pred: Sequence[int], y_true: Sequence[int]) -> None:
        """Host lists of predictions and labels (Dassl's argument order: output first)."""
        y_pred, y_true = [int(p) for p in y_pred], [int(t) for t in y_true]
        assert len(y_pred) == len(y_true)
        self.total += len(y_true)
        self.correct += sum(1 for p, t in zip(y_pred, y_true) if p == t and 0 <= t < self.n_cls)
        self.cmat += confusion_matrix(y_true, y_pred, self.n_cls)

    def process_counts(self, counts, cmat) -> None:
        """counts = (correct, total), cmat [n_cls * n_cls] (row = true) as read back from the device."""
        counts = np.asarray(counts).reshape(-1)
        self.correct += int(counts[0])
        self.total += int(counts[1])
        self.cmat += np.asarray(cmat, dtype=np.int64).reshape(self.n_cls, self.n_cls)

    def evaluate(self, verbose: bool = True) -> "OrderedDict[str, float]":
        res = metrics(self.correct, self.total, self.cmat)
        if verbose:
            print("=> result\n"
                  f"* total: {res['total']:,}\n"
                  f"* correct: {res['correct']:,}\n"
                  f"* accuracy: {res['accuracy']:.1f}%\n"
                  f"* error: {res['error_rate']:.1f}%\n"
                  f"* macro_f1: {res['macro_f1']:.1f}%")
            if self.per_class_result:
                print("=> per-class result")
                for c, a in res["perclass_accuracy"].items():
                    name = self.classnames[c] if self.classnames is not None else ""
                    n = int(self.cmat[c].sum())
                    print(f"* class: {c} ({name})\ttotal: {n:,}\tcorrect: {int(self.cmat[c, c]):,}\tacc: {a:.1f}%")
                print(f"* average: {res['mean_perclass_accuracy']:.1f}%")
        return res


def harmonic_mean(base: float, new: float) -> float:
    """The H of the base-to-new tables: 2 b n / (b + n) of the base and new accuracies; 0 where either is 0 (the limit,
    and what a model that fails one half deserves -- the bare formula divides by zero when both are)."""
    base, new = float(base), float(new)
    if base < 0 or new < 0:
        raise ValueError(f"harmonic_mean: accuracies must be >= 0, got {base}, {new}")
    if base == 0.0 or new == 0.0:
        return 0.0
    return 2.0 * base * new / (base + new)


def base_to_new(trainer, base_set, new_set, new_classes, **test_kw) -> dict:
    """The base-to-new protocol on ONE trained model (scripts/rpo/base2new_test.sh with SUB=base, then SUB=new, in the
    reference two processes that rebuild CLIP): `trainer.test(base_set)` on the classes it was built with,
    `trainer.test(new_set, classes=...)` on the new half, and their harmonic mean.  `new_classes`: a `ClassSet` of the
    trainer's engine, or the new classes' token ids [n', 77] (the set is then built here).  `test_kw` goes to both calls.
    -> {"base": accuracy, "new": accuracy, "H": harmonic_mean, "base_result": .., "new_result": ..}."""
    from .class_set import ClassSet
    if not isinstance(new_classes, ClassSet):
        new_classes = trainer.class_set(new_classes)
    base = trainer.test(base_set, **test_kw)
    new = trainer.test(new_set, classes=new_classes, **test_kw)
    return {"base": base["accuracy"], "new": new["accuracy"], "H": harmonic_mean(base["accuracy"], new["accuracy"]),
            "base_result": base, "new_result": new}
