"""Epoch loops: Dassl's `train()` / `run_epoch()` / `test()` (un-vendored; every script under the reference's
`scripts/*/` reaches them) for the trainers of this package, on a device-resident few-shot set.

    train_set = DeviceImageSet(images, labels, device)            # decoded uint8 images, uploaded once
    trainer   = RPO(cfg, sd, batch_size=32, num_batches=len(train_set) // 32)
    trainer.train(train_set, max_epoch=15, val_set=val_set, directory="output/run")

`run_epoch` never reads a device scalar: per batch it builds the transform's descriptors on the host, runs the
resident transform into one of two image buffers the loop owns, and enqueues `step_async` -- for RPO with
`next_image` = the other buffer, already holding batch t + 1, so that batch's patch embedding runs under this step's
backward (the path `bench.py` times).  Losses come back stacked in one device tensor; the training accuracy that the
reference's CoOp / LP steps report is summed on the device by `rpo_eval_accumulate`.  `test` does the same for the
evaluator: eval transform, the trainer's eval forward, `rpo_eval_accumulate` on the un-cloned logits, one read-back.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from . import ops
from .config import refuse_long_grid
from .evaluator import Classification


def epoch_indices(n: int, batch_size: int, generator: Optional[torch.Generator] = None) -> List[List[int]]:
    """The index batches of `DataLoader(range(n), batch_size, shuffle=True, drop_last=True[, generator=g])`, with the
    RNG it draws from left where a full pass of that loader leaves it (pinned against torch.utils.data in
    tests/test_loop_host.py).  Draw for draw: the loader's base seed (one int64 `random_()` from `generator`, or from
    the global RNG); without a generator a second global draw that seeds a fresh `torch.Generator` for the sampler;
    `randperm(n)`; and the sampler's closing `randperm(n)[:0]`, which it draws when it is exhausted."""
    if n <= 0 or batch_size <= 0:
        raise ValueError("n and batch_size must be positive")
    torch.empty((), dtype=torch.int64).random_(generator=generator)            # _BaseDataLoaderIter._base_seed
    g = generator
    if g is None:                                                              # RandomSampler.__iter__
        g = torch.Generator()
        g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
    perm = torch.randperm(n, generator=g).tolist()
    torch.randperm(n, generator=g)
    return [perm[i:i + batch_size] for i in range(0, n - batch_size + 1, batch_size)]


class EvalMixin:
    """`test` for anything with an eval forward: `cfg`, `device`, `engine` and `_eval_logits` (ZeroshotCLIP and, through
    LoopMixin, the four trainers)."""

    def _loop_transform(self, is_train: bool, max_batch: int):
        from .input_pipeline import DeviceTransform, InputConfig
        tfs = self.__dict__.setdefault("_loop_tfs", {})
        key = (is_train, max_batch)
        if key not in tfs:
            icfg = InputConfig(SIZE=(self.cfg.image_size, self.cfg.image_size))
            # (resident sets: the staging slots of __call__ are not used, so they are not sized for images)
            tfs[key] = DeviceTransform(icfg, is_train, self.device, max_batch, max_image_bytes=16)
        return tfs[key]

    def _eval_logits(self, image: torch.Tensor, classes=None) -> torch.Tensor:
        """What `model_inference` computes, as the engine's own logits buffer (no clone): valid until the next forward.
        `classes`: against that `ClassSet` (its own buffer), through the trainer's `_class_logits`."""
        return self.model(image) if classes is None else self._class_logits(image, classes)

    def _class_logits(self, image: torch.Tensor, classes) -> torch.Tensor:
        raise NotImplementedError(f"{type(self).__name__}: evaluation on another class set (classes=...) is not built")

    def class_set(self, tokens, chunk=None):
        """A `ClassSet` (rpo_amd/class_set.py) of int ids [n', 77] for `model_inference` / `test(..., classes=)`: classes
        the model was not built with -- the new half of a base-to-new split, another dataset's names."""
        with torch.cuda.device(self.device):
            return self.engine.class_set(tokens, chunk)

    def _n_classes(self, image_set, classes) -> int:
        """The class count an evaluation is sized by; with a class set, the set's labels are checked against it (the
        evaluator kernel indexes the confusion matrix by the label)."""
        if classes is None:
            return self.cfg.n_cls
        self.engine._cs_check(classes)
        image_set.check_labels(classes.n)
        return classes.n

    def _test_chunk(self, batch_size: int, classes) -> int:
        """Images `test` hands to the eval forward at a time: what the engine's image pass takes."""
        return max(1, min(batch_size, self.engine.max_batch))

    # ---- cached image features (rpo_amd/features.py): for the trainers whose image feature depends on nothing they train
    _features_why_not: Optional[str] = None        # why `features=` / `val_features=` cannot serve this trainer, or None

    def _refuse_features(self, features, what: str) -> None:
        if features is not None and self._features_why_not is not None:
            raise NotImplementedError(f"{type(self).__name__}.{what}: {self._features_why_not}")

    def classifier(self, classes=None):
        """(cls [C, e], bias [C] or None, norm_feat, norm_cls, scale) of `rpo_features_classify` for the model as it
        stands -- or for a `ClassSet`: logits = scale (/ |f|) (/ |cls|) <f, cls> + bias on the image feature f."""
        raise NotImplementedError(f"{type(self).__name__}: no classifier on cached image features")

    def _test_features(self, image_set, features, verbose: bool, per_class_result: bool, classes) -> dict:
        """`test` on an `ImageFeatures` of this engine and set: one rpo_features_classify launch, one read-back."""
        from .features import classify_many
        self._n_classes(image_set, classes)
        features.check(self.engine, image_set)
        with torch.cuda.device(self.device):
            cls, bias, norm_feat, norm_cls, scale = self.classifier(classes)
            return classify_many(features, cls.unsqueeze(0), None if bias is None else bias.unsqueeze(0), norm_feat,
                                 norm_cls, scale, verbose=verbose, per_class_result=per_class_result)[0]

    @torch.no_grad()
    def test(self, image_set, batch_size: int = 100, verbose: bool = True, per_class_result: bool = False, classes=None,
             features=None):
        """Dassl's `test()`: eval transform (resize + center crop) from the resident set, the eval forward,
        `rpo_eval_accumulate` on the same stream, one read-back, `Classification.evaluate()` -> its dict
        (+ "confusion_matrix").  Runs chunks of min(batch_size, engine.max_batch), the last one ragged.
        `classes`: a `ClassSet` -- the evaluator and the confusion matrix are sized by ITS class count.
        `features`: an `ImageFeatures` of this engine and set (ZeroshotCLIP(2), CoOp, LP) -- no image pass at all: the
        current classifier over the cached features in one fused launch."""
        self._refuse_features(features, "test(features=...)")
        if features is not None:
            return self._test_features(image_set, features, verbose, per_class_result, classes)
        n, C = len(image_set), self._n_classes(image_set, classes)
        chunk = self._test_chunk(batch_size, classes)
        ev = Classification(C, per_class_result)
        with torch.cuda.device(self.device):
            tf = self._loop_transform(False, chunk)
            S = self.cfg.image_size
            bufs = self.__dict__.setdefault("_test_bufs", {})
            if chunk not in bufs:
                bufs[chunk] = torch.zeros(chunk, 3, S, S, dtype=torch.float32, device=self.device)
            counts = torch.zeros(2, dtype=torch.int64, device=self.device)
            cmat = torch.zeros(C * C, dtype=torch.int32, device=self.device)
            for b0 in range(0, n, chunk):
                B = min(chunk, n - b0)
                image = tf.from_set(image_set, range(b0, b0 + B), out=bufs[chunk][:B])
                logits = self._eval_logits(image) if classes is None else self._eval_logits(image, classes=classes)
                ops.eval_accumulate(logits, image_set.labels_dev[b0:b0 + B], counts, cmat)
            ev.process_counts(counts.cpu().numpy(), cmat.cpu().numpy())         # the one read-back
        res = ev.evaluate(verbose=verbose)
        res["confusion_matrix"] = ev.cmat.copy()
        return res


    @torch.no_grad()
    def _test_shared(self, image_set, S: int, sides, batch_size: int = 100, frozen=None, verbose: bool = True,
                     per_class_result: bool = False, hook=None, classes=None) -> List[dict]:
        """`test` for S prompt sets at once on the shared frozen image rows (rpo_amd/engine_prompt_rows.py): per chunk
        (those of `test`) one frozen pass -- none with `frozen`, a `FrozenImageKV` of this set -- and ONE prompt-row pass +
        grouped head for all sets; every set has its own counts / confusion matrix, filled by `rpo_eval_accumulate` on
        its slice of the logits; one read-back.  `sides()` -> (img_prompts [S, K, d_v], text_f [S * n_cls * K, e], k_used), called once
        with the device current; k_used is None, or int32 [S] on the device for sets that average over their own number
        of pairs (`RPOSweep`).  `hook(b0, logits [S, B, n_cls])` sees each chunk's logits (the engine's buffer).
        `classes`: a `ClassSet` -- `sides()` then returns ITS text features [S * n' * K, e]; everything is sized by n'."""
        refuse_long_grid(self.cfg, f"{type(self).__name__}: evaluation on shared frozen image rows (test_all, test(frozen=...))")
        eng, n, C = self.engine, len(image_set), self._n_classes(image_set, classes)
        if frozen is not None:
            frozen.check(eng, image_set)
        chunk = max(1, min(batch_size, eng.max_batch))
        evs = [Classification(C, per_class_result) for _ in range(S)]
        with torch.cuda.device(self.device):
            eng.prompt_rows_setup(S, chunk)
            img_prompts, text_f, k_used = sides()
            counts = torch.zeros(S, 2, dtype=torch.int64, device=self.device)
            cmat = torch.zeros(S, C * C, dtype=torch.int32, device=self.device)
            if frozen is None:
                tf = self._loop_transform(False, chunk)
                size = self.cfg.image_size
                bufs = self.__dict__.setdefault("_test_bufs", {})
                if chunk not in bufs:
                    bufs[chunk] = torch.zeros(chunk, 3, size, size, dtype=torch.float32, device=self.device)
            for b0 in range(0, n, chunk):
                B = min(chunk, n - b0)
                if frozen is None:
                    eng.frozen_pass(tf.from_set(image_set, range(b0, b0 + B), out=bufs[chunk][:B]))
                    kv = eng.live_kv()
                    kv.set_first(0, B)
                else:
                    kv = frozen.kv
                    kv.set_first(b0, B)
                logits = eng.shared_eval_logits(B, kv, img_prompts, text_f, k_used=k_used, classes=classes)
                if hook is not None:
                    hook(b0, logits)
                for s in range(S):
                    ops.eval_accumulate(logits[s], image_set.labels_dev[b0:b0 + B], counts[s], cmat[s])
            counts_h, cmat_h = counts.cpu().numpy(), cmat.cpu().numpy()         # the one read-back
        out = []
        for s, ev in enumerate(evs):
            ev.process_counts(counts_h[s], cmat_h[s])
            res = ev.evaluate(verbose=verbose)
            res["confusion_matrix"] = ev.cmat.copy()
            out.append(res)
        return out


class LoopMixin(EvalMixin):
    """`run_epoch` / `test` / `train` for a trainer that has `step_async`, `batch_size`, `num_batches`, `batch_idx`,
    `epoch`, `lr`, `optim_cfg`, `_opt` (rpo_amd/optim.py), `cfg`, `device`, `engine` (RPO, CoOp, CoCoOp, LP).  The small
    `_loop_*` methods are everything the control flow touches on the device."""

    _takes_next_image = False          # step_async(image, label, next_image=...) (RPO)
    _reports_acc = False               # forward_backward reports "acc" (CoOp, LP)
    _takes_frozen = False              # test(..., frozen=FrozenImageKV) (RPO)

    def _loop_buffers(self):
        if getattr(self, "_loop_bufs", None) is None:
            S = self.cfg.image_size
            self._loop_bufs = [torch.zeros(self.batch_size, 3, S, S, dtype=torch.float32, device=self.device)
                               for _ in range(2)]
        return self._loop_bufs

    def _loop_fill(self, image_set, indices: Sequence[int], plans, out: torch.Tensor) -> None:
        self._loop_transform(True, self.batch_size).from_set(image_set, indices, plans, out=out)

    def _loop_labels(self, image_set, batches: List[List[int]]) -> torch.Tensor:
        """int64 [num_batches, batch_size] on the device: one small upload per epoch."""
        idx = torch.tensor(batches, dtype=torch.int64).to(self.device)
        return image_set.labels_dev[idx]

    def _loop_new_losses(self, nb: int) -> torch.Tensor:
        return torch.zeros(nb, dtype=torch.float32, device=self.device)

    def _loop_loss(self) -> torch.Tensor:
        """The device loss of the step just enqueued: a scalar, or [S] for a trainer that steps S members (LPSweep)."""
        return self.engine.loss

    def _loop_new_counts(self) -> torch.Tensor:
        return torch.zeros(2, dtype=torch.int64, device=self.device)

    def _loop_accumulate(self, label: torch.Tensor, counts: torch.Tensor) -> None:
        ops.eval_accumulate(self.engine.logits[:self.batch_size], label, counts)

    def _loop_device(self):
        return torch.cuda.device(self.device)

    # ---- the batch of a `forward_backward` ------------------------------------------------------------------
    def parse_batch_train(self, batch):
        """One Dassl-style batch {"img": float [B, 3, H, W], "label": [B]} on the device (CoOp, CoCoOp, LP and the sweeps
        on shared batches; `RPO` has its own, which also takes decoded images)."""
        img = batch["img"].to(self.device, dtype=torch.float32, non_blocking=True).contiguous()
        label = torch.as_tensor(batch["label"])
        if not label.is_cuda:
            lo, hi = int(label.min()), int(label.max())
            if lo < 0 or hi >= self.cfg.n_cls:
                raise IndexError(f"Target {hi if hi >= self.cfg.n_cls else lo} is out of bounds (n_cls = {self.cfg.n_cls})")
        return img, label.to(self.device, dtype=torch.int64, non_blocking=True)

    # ---- bookkeeping ---------------------------------------------------------------------------------------
    def _loop_advance(self) -> None:
        """What every `forward_backward` does after its step: the LR / epoch update behind the epoch's last batch."""
        if (self.batch_idx + 1) == self.num_batches:
            self.update_lr()
            self.batch_idx = 0
        else:
            self.batch_idx += 1

    def update_lr(self) -> None:
        from .trainer import lr_at_epoch
        self.epoch += 1
        self.lr = lr_at_epoch(self.optim_cfg, self.epoch)
        self._opt.set_epoch(self.epoch)

    # ---- the step of the trainers whose whole step is one graph (CoOp, CoCoOp, LP) -------------------------
    def step_async(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        """One optimisation step (`_enqueue`: forward, backward, the optimiser's step), nothing synchronised; returns the
        device loss scalar.  With use_graph the launches of a step are replayed from ONE HIP graph, captured after the first
        (eager) step and again whenever the optimiser's `graph_key` changes (plain SGD: the learning rate, a kernel
        argument; device data otherwise: one capture serves every epoch)."""
        self._opt.set_epoch(self.epoch)
        key = self._opt.graph_key()
        if not self.use_graph or self._steps == 0 or image.shape[0] != self.batch_size:
            self._enqueue(image, label)
        else:
            if self._graph is None or self._graph[1] != key:
                self._img = torch.empty_like(image)
                self._lab = torch.empty_like(label)
                self._img.copy_(image); self._lab.copy_(label)
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._enqueue(self._img, self._lab)
                self._graph = (g, key)
                self.captures = getattr(self, "captures", 0) + 1
                # (capture does not execute: the replay below is this step)
            if image.data_ptr() != self._img.data_ptr():
                self._img.copy_(image, non_blocking=True)
            self._lab.copy_(label, non_blocking=True)
            self._graph[0].replay()
        self._steps += 1
        return self._loop_loss()

    # ---- the loops -----------------------------------------------------------------------------------------
    def run_epoch(self, image_set, generator: Optional[torch.Generator] = None, plans=None) -> Dict[str, torch.Tensor]:
        """One epoch over `image_set` (a `DeviceImageSet`) in the order of Dassl's train loader (`epoch_indices`).
        `plans`: per batch, the `SamplePlan`s of its images (default: drawn by the transform, batch by batch).
        Returns {"loss": float32 [num_batches] on the device, "indices": the batches, and for CoOp / LP "counts":
        int64 [2] on the device (correct, total) of the epoch's training predictions}.  Nothing is synchronised."""
        bs, nb = self.batch_size, len(image_set) // self.batch_size
        if nb != self.num_batches:
            raise ValueError(f"the set has {len(image_set)} images = {nb} batches of {bs}; the trainer was built with "
                             f"num_batches = {self.num_batches} (its LR schedule counts on it)")
        if self.batch_idx != 0:
            raise RuntimeError("run_epoch starts at an epoch boundary (batch_idx != 0: forward_backward is mid-epoch)")
        image_set.check_labels(self.cfg.n_cls)
        batches = epoch_indices(len(image_set), bs, generator)
        if plans is not None and len(plans) != nb:
            raise ValueError(f"{len(plans)} plan lists for {nb} batches")
        with self._loop_device():
            bufs = self._loop_buffers()
            labels = self._loop_labels(image_set, batches)
            losses = self._loop_new_losses(nb)
            counts = self._loop_new_counts() if self._reports_acc else None
            self._loop_fill(image_set, batches[0], None if plans is None else plans[0], bufs[0])
            for t in range(nb):
                cur, nxt = bufs[t & 1], None
                if t + 1 < nb:                     # batch t + 1 is in its buffer before step t is enqueued
                    nxt = bufs[(t + 1) & 1]
                    self._loop_fill(image_set, batches[t + 1], None if plans is None else plans[t + 1], nxt)
                if self._takes_next_image:
                    loss = self.step_async(cur, labels[t], next_image=nxt)
                else:
                    loss = self.step_async(cur, labels[t])
                losses[t].copy_(loss.reshape(losses.shape[1:]), non_blocking=True)
                if counts is not None:
                    self._loop_accumulate(labels[t], counts)
                if getattr(self, "detect_anomaly", False):
                    self.check_finite()            # (a debug mode: one sync per step, as forward_backward)
                self._loop_advance()
        out = {"loss": losses, "indices": batches}
        if counts is not None:
            out["counts"] = counts
        return out

    def train(self, train_set, max_epoch: Optional[int] = None, val_set=None, directory: Optional[str] = None,
              generator: Optional[torch.Generator] = None, test_batch_size: int = 100, verbose: bool = True,
              val_frozen=None, val_features=None) -> List[dict]:
        """Dassl's `train()`: `run_epoch` until `max_epoch` (default: the optimiser config's), and after each epoch its
        `after_epoch`: with a validation set `test(val_set)` -> `after_epoch_eval` (keeps `model-best`); without one
        the last epoch's model is saved.  Returns one record per epoch (mean loss, training accuracy where the
        trainer reports it, validation accuracy).  `val_frozen`: a `FrozenImageKV` of `val_set` -- the validation images'
        frozen pass is then never repeated (RPO only: its frozen image rows never read a prompt).  `val_features`: an
        `ImageFeatures` of `val_set` (CoOp, LP: what they train sits behind the image feature) -- no validation image
        pass in any epoch.  CoCoOp has neither: its text features depend on the image."""
        max_epoch = self.optim_cfg.max_epoch if max_epoch is None else max_epoch
        self._refuse_features(val_features, "train(val_features=...)")
        if val_features is not None:
            if val_set is None:
                raise ValueError(f"{type(self).__name__}.train: val_features are the features of val_set; pass both")
            val_features.check(self.engine, val_set)
        if val_frozen is not None and not self._takes_frozen:
            raise NotImplementedError(f"{type(self).__name__}.train: val_frozen is RPO's (its frozen image rows never read a "
                                      "prompt); this trainer evaluates through its own image pass")
        if val_frozen is not None:
            refuse_long_grid(self.cfg, f"{type(self).__name__}.train(val_frozen=...)")
        val_kw = {} if val_frozen is None else {"frozen": val_frozen}
        if val_features is not None:
            val_kw["features"] = val_features
        history = []
        while self.epoch < max_epoch:
            res = self.run_epoch(train_set, generator)
            rec = {"epoch": self.epoch, "loss": float(res["loss"].mean().item())}        # one read per epoch
            if "counts" in res:
                c = res["counts"].tolist()
                rec["acc"] = 100.0 * c[0] / max(1, c[1])
            if val_set is not None:
                rec["val_acc"] = self.test(val_set, test_batch_size, verbose=verbose, **val_kw)["accuracy"]
                if directory:
                    self.after_epoch_eval(directory, rec["val_acc"])
            elif directory and self.epoch == max_epoch:
                self.save_model(directory)
            if verbose:
                print("epoch [{}/{}] ".format(self.epoch, max_epoch)
                      + " ".join(f"{k} {v:.4f}" for k, v in rec.items() if k != "epoch") + f" lr {self.lr:.4e}")
            history.append(rec)
        return history

    def after_epoch_eval(self, directory: str, val_result: float) -> bool:
        """Dassl's `after_epoch` bookkeeping for `model-best`: keep the checkpoint with the best validation result."""
        is_best = val_result > self.best_result
        if is_best:
            self.best_result = val_result
            self.save_model(directory, is_best=True, val_result=val_result)
        return is_best
