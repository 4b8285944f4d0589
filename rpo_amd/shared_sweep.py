"""``RPOSharedSweep``: the points of an RPO hyper-parameter sweep trained on ONE shared batch -- the frozen image rows run once
per step for all members (rpo_amd/engine_prompt_train.py).

``RPOSweep`` (rpo_amd/sweep.py) gives every member its own batch and pushes S x B images through the whole image tower.  The
members of a sweep are usually meant to see the same data; when they do, the frozen rows and their per-block K / V are the
same for all of them, and only the S x B x K prompt rows differ.  This trainer is ``RPOSweep`` with that data contract, as
``CoOpSweep`` and ``LPSweep`` are "the members of ONE step on ONE shared batch":

    batch_size        the ONE shared batch of B images; the engine is built for B images (its evaluation chunk is then
                      min(test batch, B), as a standalone ``RPO``'s), not for S x B
    step_async        image [B, ...], label [B]
    forward_backward  ONE Dassl-style batch in, a list of S {"loss", "acc"} out
    run_epoch         ONE resident set and ONE generator: the order a standalone run sees

Inherited unchanged: the per-member optimiser table and schedule, the amp skip (`skipped_steps`), `test` / `test_all` /
`model_inference` through the shared prompt-row evaluation, `save_model` / `load_model` -- a member's checkpoint is the file of
a standalone ``RPO(K = K_s)``, in both directions.  Member s ends a step where a standalone ``RPO(K_s, optim_s)`` fed the same
batch ends it, up to the summation order of the GEMM plans.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import members as _members
from .config import refuse_long_grid
from .custom_clip import refuse_rn
from .loop import epoch_indices
from .multi import _WHY_NO_DP
from .sweep import RPOSweep


class RPOSharedSweep(RPOSweep):
    _loop_name = "RPOSharedSweep"

    def __init__(self, cfg, state_dict: Dict[str, np.ndarray], tokens: Optional[np.ndarray] = None,
                 members: Sequence[dict] = (), batch_size: int = 4, device: str | torch.device = "cuda:0",
                 act_dtype: torch.dtype = torch.bfloat16, num_batches: int = 1, use_graph: bool = True, amp: bool = False,
                 world_size: int = 1):
        """members: as ``RPOSweep``'s -- dict(seed= | prompts=(text_prompt [K_s, d_t], img_prompt [K_s, d_v]), K=K_s,
        optim=OptimConfig).  batch_size: the shared batch."""
        # ---- refusals of this trainer, by its name and before any device is touched; `RPOSweep` refuses members that
        # differ in what a sweep shares, also before it touches one
        refuse_rn(cfg, "RPOSharedSweep")
        _members.refuse_world_size("RPOSharedSweep", world_size, _WHY_NO_DP)
        refuse_long_grid(cfg, "RPOSharedSweep")
        super().__init__(cfg, state_dict, tokens, members, batch_size, device, act_dtype, num_batches, use_graph, amp, world_size)

    def _build(self, cfg, state_dict, tokens, S: int, B: int, prompts, device, act_dtype, num_batches: int, use_graph: bool,
               member_K: Optional[Sequence[int]] = None) -> None:
        """`RPOMulti._build` with the engine built for the B shared images and the shared-batch step's buffers."""
        self.cfg, self.n_runs, self.batch_size, self.num_batches = cfg, S, B, num_batches
        self.use_graph = use_graph
        self.epoch = self.batch_idx = self._steps = 0
        self._graph = None
        self._warm = False
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        from .engine import make_engine
        from . import synth
        if tokens is None:
            if cfg.n_cls != 19:
                raise ValueError("tokens [n_cls, context] are required for any class set other than the bundled "
                                 "Oxford-Pets base split")
            tokens = synth.oxford_pets_base_tokens()
        with torch.cuda.device(self.device):
            # the image tower's workspace and GEMM plans are those of B images: a standalone RPO's at this batch size
            self.engine = make_engine(cfg, state_dict, tokens, self.device, act_dtype, B)
            self.engine.params.zero_()               # (the prompts that ride in the frozen pass: finite, read by no result)
            self.engine.prompt_train_setup(S, B, member_K=member_K)
            self.set_prompts(prompts)
            self._image = torch.zeros(B, 3, cfg.image_size, cfg.image_size, device=self.device)
            self._label = torch.zeros(B, dtype=torch.int64, device=self.device)

    # ------------------------------------------------------------------ the step
    def _forward_backward(self, image: torch.Tensor, label: torch.Tensor) -> None:
        self.engine.shared_forward_backward(image, label)

    def step_async(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        """One optimisation step of every member on the ONE batch image [B, 3, H, W], label [B]; nothing synchronised.
        Returns loss [S] on the device.  Graph capture as `MemberLoopMixin.step_async`: the whole step -- text tower, frozen
        pass, the members' prompt rows, the grouped head, both backward chains, the optimiser's launch -- is ONE HIP graph,
        captured after the first (eager) step."""
        assert torch.cuda.current_device() == self.device.index, "set the trainer's device current (torch.cuda.set_device)"
        B = self.batch_size
        assert image.shape[0] == B and label.shape == (B,), f"step_async takes the ONE shared batch of B = {B} images"
        if image.data_ptr() != self._image.data_ptr():
            self._image.copy_(image, non_blocking=True)
        self._label.copy_(label, non_blocking=True)
        self._opt.set_epoch(self.epoch)
        key = self._opt.graph_key()
        if not self.use_graph or self._steps == 0:
            self._enqueue(self._image, self._label)
            self._warm = True
        else:
            if self._graph is None or self._graph[1] != key:
                if not self._warm:                      # (a resumed run: kernel attributes are set by an eager launch)
                    self._forward_backward(self._image, self._label)
                    self._warm = True
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._enqueue(self._image, self._label)
                self._graph = (g, key)
                self.captures += 1
            self._graph[0].replay()
        self._steps += 1
        self._eval_member = None
        self._after_step()
        return self._loop_loss()

    def parse_batch_train(self, batch: dict):
        """ONE Dassl-style batch {"img": float [B, 3, H, W], "label": [B]} -> the device batch every member sees."""
        if not isinstance(batch, dict):
            raise ValueError("RPOSharedSweep takes ONE batch {'img', 'label'} for all members, not one per member")
        lab = torch.as_tensor(batch["label"])
        if not lab.is_cuda and lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= self.cfg.n_cls):
            raise IndexError(f"target out of bounds (n_cls = {self.cfg.n_cls}; labels must be renumbered after the base/new "
                             "split)")
        img = torch.as_tensor(batch["img"]).to(self.device, dtype=torch.float32).contiguous()
        return img, lab.to(self.device, dtype=torch.int64).contiguous()

    def forward_backward(self, batch: dict) -> List[Dict[str, float]]:
        """trainers/rpo.py:290-316 for every member on ONE batch: a list of S {"loss", "acc"}."""
        S = self.n_runs
        with torch.cuda.device(self.device):
            image, label = self.parse_batch_train(batch)
            loss = self.step_async(image, label)
            pred = self.engine.m_logits.view(S, self.batch_size, -1).argmax(2)
            acc = (pred == label[None]).float().mean(1) * 100.0
            loss, acc = loss.tolist(), acc.tolist()                                    # D2H sync, as the reference (:311)
        self._loop_advance()
        return [{"loss": float(loss[s]), "acc": float(acc[s])} for s in range(S)]

    # ------------------------------------------------------------------ the epoch loop
    def run_epoch(self, image_set, generator: Optional[torch.Generator] = None, plans=None) -> Dict[str, object]:
        """One epoch of every member over ONE resident set in the order `epoch_indices` gives a standalone run with this
        generator.  `plans`: per batch, the `SamplePlan`s of its images (default: drawn by the transform).  No device scalar
        is read, and batch t + 1 is in its buffer before step t is enqueued.  Returns {"loss": float32 [num_batches, S] on
        the device, "indices": the batches}."""
        if isinstance(image_set, (list, tuple)) or isinstance(generator, (list, tuple)):
            raise ValueError("RPOSharedSweep.run_epoch takes ONE image set and ONE generator: the members share every batch")
        S, B = self.n_runs, self.batch_size
        batches = epoch_indices(len(image_set), B, generator)
        nb = len(batches)
        if nb == 0 or nb != self.num_batches:
            raise ValueError(f"the set gives {nb} batches of {B}; the trainer was built with num_batches = {self.num_batches} "
                             "(its LR schedule counts on it)")
        if self.batch_idx != 0:
            raise RuntimeError("run_epoch starts at an epoch boundary (batch_idx != 0: forward_backward is mid-epoch)")
        image_set.check_labels(self.cfg.n_cls)
        with torch.cuda.device(self.device):
            if getattr(self, "_loop_bufs", None) is None:
                self._loop_bufs = [torch.zeros_like(self._image) for _ in range(2)]
            if getattr(self, "_shared_tf", None) is None:
                from .input_pipeline import DeviceTransform, InputConfig
                icfg = InputConfig(SIZE=(self.cfg.image_size, self.cfg.image_size))
                self._shared_tf = DeviceTransform(icfg, True, self.device, B, max_image_bytes=16)
            tf = self._shared_tf
            labels = torch.stack([image_set.labels_dev[torch.tensor(bt, dtype=torch.int64).to(self.device)] for bt in batches])
            losses = torch.zeros(nb, S, dtype=torch.float32, device=self.device)
            fill = lambda t, out: tf.from_set(image_set, batches[t], None if plans is None else plans[t], out=out)
            fill(0, self._loop_bufs[0])
            for t in range(nb):
                cur = self._loop_bufs[t & 1]
                if t + 1 < nb:
                    fill(t + 1, self._loop_bufs[(t + 1) & 1])
                loss = self.step_async(cur, labels[t])
                losses[t].copy_(loss, non_blocking=True)
                self._loop_advance()
        return {"loss": losses, "indices": batches}

    def train(self, image_set, max_epoch: Optional[int] = None, generator: Optional[torch.Generator] = None,
              directories: Optional[Sequence[str]] = None, verbose: bool = True, plans=None) -> List[dict]:
        """`run_epoch` on the ONE set until `max_epoch` (default: the members' shared one); the last epoch's models are saved
        to `directories`.  One record per epoch: the members' mean losses (one read per epoch)."""
        history = self._train_members(
            max_epoch, lambda i: self.run_epoch(image_set, generator, None if plans is None else plans[i]), verbose=verbose)
        if directories:
            self.save_model(directories)
        return history
