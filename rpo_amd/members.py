"""What the member trainers -- ``RPOMulti``, ``RPOSweep``, ``LPSweep``, ``CoCoOpMulti``, ``CoOpSweep`` -- share, stated once
(DESIGN.md section 9t).  All of it is host-side bookkeeping; no kernel is reached from here except through the trainer's own
engine calls.

    plain functions        refuse_world_size, member_optim_configs, check_member_dict, seeded_prompts, member_batches,
                           member_checkpoint / read_member_checkpoint (``RPO``'s own file format, per member)
    MemberMixin            all five: `_check_member`, the directory count, the equal-epochs and all-or-none-state checks
    MemberScheduleMixin    the four with `optim_cfgs`: `update_lr`, `skipped_steps`, the member-form `train` loop
    MemberLoopMixin        the member-major trainers (RPOMulti, RPOSweep, CoCoOpMulti): `parse_batch_train`, `run_epoch` and
                           the graph-captured `step_async`
    MemberCheckpointMixin  the three whose files are torch's layout (LPSweep, CoCoOpMulti, CoOpSweep): one codec

A trainer keeps its refusals, its members' starting rows, its engine calls, its evaluation and the shape of its checkpoint.
"""
from __future__ import annotations

import contextlib
import os
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import optim as _optim
from .config import RPOConfig
from .custom_clip import init_prompts
from .loop import epoch_indices
from .trainer import OptimConfig, checkpoint_dict, load_checkpoint_file, lr_at_epoch, write_checkpoint


# ---------------------------------------------------------------------- refusals and validation of a constructor
def refuse_world_size(who: str, world_size: int, why: str) -> None:
    """Data parallelism is not built for a member trainer; `why` is the trainer's own reason clause."""
    if world_size != 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError(f"{who}: world_size > 1 is not supported ({why}); run one {who} per GPU with different "
                                  "members")


def member_optim_configs(who: str, members: Sequence[dict], default: Callable[[], OptimConfig],
                         counts: str = "the schedules count") -> List[OptimConfig]:
    """Fills in each member dict's `optim` (`default()` where it has none), validates it (radam and the other refusals
    of rpo_amd/optim.py) and returns the configs.  One loop runs all members, so a different `max_epoch` is refused;
    `counts` is the trainer's own clause of that sentence."""
    for m in members:
        m["optim"] = m.get("optim") or default()
        _optim.validate(m["optim"])
    cfgs = [m["optim"] for m in members]
    epochs = [oc.max_epoch for oc in cfgs]
    if any(ep != epochs[0] for ep in epochs):
        raise ValueError(f"{who}: the members differ in max_epoch ({epochs}): one loop runs all members, and {counts} on its "
                         "length -- run schedules of different lengths as separate trainers")
    return cfgs


def check_member_dict(who: str, s: int, m: dict, keys, tensors: Sequence[str], tensors_text: str) -> bool:
    """Member s's dict `m` of a CoOp-family trainer: no key outside `keys`, exactly one of `seed` or its `tensors` (the keys
    that bring them; `tensors_text` names them in the refusal), no `ctx_init` next to a given `ctx`.  True when the member
    brings its tensors."""
    unknown = set(m) - set(keys)
    if unknown:
        raise ValueError(f"{who}: member {s} has unknown keys {sorted(unknown)}")
    seeded = m.get("seed") is not None
    given = any(m.get(k) is not None for k in tensors)
    if seeded == given:
        raise ValueError(f"{who}: member {s} must have exactly one of seed=... or {tensors_text}; it has "
                         + ("both" if seeded else "neither"))
    if given and m.get("ctx_init") is not None:
        raise ValueError(f"{who}: member {s}: ctx_init initialises a seeded member; this one brings its ctx")
    return given


# ---------------------------------------------------------------------- the RPO family's members: prompts, batches, files
def seeded_prompts(state_dict: Dict[str, np.ndarray], cfg: RPOConfig, seeds: Sequence[int]) -> List[tuple]:
    """Member s's initial (text_prompt, img_prompt) as ``RPO`` draws them under ``torch.manual_seed(seeds[s])``: the same
    draws from the global CPU generator in the same order (custom_clip.init_prompts).  Leaves the global generator where
    the last member's construction would."""
    out = []
    for seed in seeds:
        torch.manual_seed(int(seed))
        out.append(init_prompts(state_dict, cfg.K, cfg.d_t, cfg.d_v))
    return out


def member_batches(set_sizes: Sequence[int], batch_size: int, generators: Sequence[Optional[torch.Generator]],
                   who: str = "RPOMulti") -> List[list]:
    """Per member, the index batches of one epoch: `epoch_indices` with that member's set size and generator, i.e. exactly
    the order a standalone run sees.  Every member must get the same number of batches (a step advances all of them)."""
    if len(set_sizes) != len(generators):
        raise ValueError(f"{len(set_sizes)} image sets for {len(generators)} generators")
    nbs = [n // batch_size for n in set_sizes]
    if any(nb != nbs[0] for nb in nbs) or nbs[0] == 0:
        raise ValueError(f"{who}.run_epoch: the members' sets have {list(set_sizes)} images = {nbs} batches of {batch_size}; "
                         "every member must have the same, non-zero number of batches per epoch (a step advances all members)")
    return [epoch_indices(n, batch_size, g) for n, g in zip(set_sizes, generators)]


def member_checkpoint(flat_params: torch.Tensor, flat_mom: Optional[torch.Tensor], cfg: RPOConfig, epoch: int,
                      oc: OptimConfig, lr: float, steps: int, val_result: Optional[float] = None,
                      optimizer: Optional[dict] = None) -> dict:
    """The dict a standalone ``RPO.save_model`` pickles for a run whose flat [text | img] parameters / momentum (or
    `optimizer` entry) are these."""
    nt = cfg.K * cfg.d_t
    p = flat_params.detach().cpu()
    state = {"text_prompt": p[:nt].reshape(cfg.K, cfg.d_t), "img_prompt": p[nt:].reshape(cfg.K, cfg.d_v)}
    return checkpoint_dict(state, epoch, flat_mom, oc, lr, steps, nt, val_result, optimizer)


def _model_path(directory: str, name: str, epoch: Optional[int]) -> str:
    """`<directory>/<name>/model-best.pth.tar`, or the file of `epoch`; a missing file is refused by its path."""
    path = os.path.join(directory, name, "model-best.pth.tar" if epoch is None else f"model.pth.tar-{epoch}")
    if not os.path.exists(path):
        raise FileNotFoundError(f'Model not found at "{path}"')
    return path


def read_member_checkpoint(directory: str, epoch: Optional[int], cfg: RPOConfig):
    """(flat params, checkpoint dict) of a file ``RPO.save_model`` / ``RPOMulti.save_model`` wrote."""
    model_path = _model_path(directory, "prompt_learner", epoch)
    ck = load_checkpoint_file(model_path)
    sd = ck["state_dict"]
    tp, ip = sd["text_prompt"].float(), sd["img_prompt"].float()
    if tuple(tp.shape) != (cfg.K, cfg.d_t) or tuple(ip.shape) != (cfg.K, cfg.d_v):
        raise ValueError(f"{model_path}: prompts {tuple(tp.shape)} / {tuple(ip.shape)}, this trainer has K = {cfg.K}, "
                         f"widths {cfg.d_t} / {cfg.d_v}")
    flat = torch.cat([tp.reshape(-1), ip.reshape(-1)])
    return flat, ck


# ---------------------------------------------------------------------- all five trainers
class MemberMixin:
    """The checks every member trainer makes on a member index, on per-member directories and on the members' files: needs
    `n_runs` and, for the state check, `_opt`."""

    _one_counter = " (one step counter covers every member)"     # why a mix of files with and without state is refused

    def _check_member(self, member: int) -> None:
        if not 0 <= member < self.n_runs:
            raise IndexError(f"member {member} of {self.n_runs}")

    def _check_directories(self, directories: Sequence[str]) -> None:
        if len(directories) != self.n_runs:
            raise ValueError(f"{len(directories)} directories for {self.n_runs} members")

    def _files_epoch(self, cks: Sequence[dict], what: str, why: str = "one loop runs all members") -> int:
        """The epoch the members' files agree on; files of different epochs are refused."""
        epochs = [int(ck.get("epoch", 0)) for ck in cks]
        if any(ep != epochs[0] for ep in epochs):
            raise ValueError(f"{type(self).__name__}.{what}: the checkpoints are of epochs {epochs}; {why}")
        return epochs[0]

    def _files_steps(self, cks: Sequence[dict], have: Sequence[bool], what: str) -> Optional[int]:
        """Every file carries optimiser state (`have`) -- then the `_steps` to go on with is the files', returned here -- or
        none does (None); a mix is refused."""
        if any(have) != all(have):
            raise ValueError(f"{type(self).__name__}.{what}: some checkpoints carry "
                             + ("optimiser state and some do not" + self._one_counter if self._opt.table_driven else
                                "momentum and some do not (one first-step flag covers every member)"))
        return max(1, max(int(ck.get("steps", 1)) for ck in cks)) if all(have) else None


# ---------------------------------------------------------------------- the four with one optimiser config per member
class MemberScheduleMixin(MemberMixin):
    """Members with their own `optim_cfgs` (RPOSweep, LPSweep, CoCoOpMulti, CoOpSweep): needs `lr` [S], `epoch`, `_opt`,
    `_found_inf` (int32 [S, 2] with amp, else None) and `run_epoch`."""

    def update_lr(self) -> None:
        """The next epoch's rates: the `set_epoch` here and the one in front of the next step are on one stream, and the
        second returns at once for an epoch the table already holds, so the device sees the same table before the same launch."""
        self.epoch += 1
        self.lr = [lr_at_epoch(oc, self.epoch) for oc in self.optim_cfgs]
        self._opt.set_epoch(self.epoch)

    def skipped_steps(self) -> List[int]:
        """amp: per member, the steps skipped so far because its own gradients held Inf / NaN (one D2H read)."""
        if self._found_inf is None:
            return [0] * self.n_runs
        return [int(v) for v in self._found_inf[:, 1].tolist()]

    def _check_val_features(self, val_set, val_features) -> None:
        """`train(val_features=...)`: cached image features of the validation set, of this engine."""
        if val_features is not None:
            if val_set is None:
                raise ValueError(f"{type(self).__name__}.train: val_features are the features of val_set; pass both")
            val_features.check(self.engine, val_set)

    def _train_members(self, max_epoch: Optional[int], run_epoch: Callable[[int], dict],
                       evaluate: Optional[Callable[[], List[dict]]] = None, directories: Optional[Sequence[str]] = None,
                       verbose: bool = True) -> List[dict]:
        """The member form of `loop.LoopMixin.train`: `run_epoch(i)` (i: the epoch of this call) until `max_epoch` (default:
        the members' shared one).  After each epoch, with `evaluate` (-> per member, the validation set's evaluator dict),
        `after_epoch_eval` keeps each member's best in its directory; without it the last epoch's models are saved.  One
        record per epoch: {"epoch", "loss": the members' mean losses [S] (one read per epoch) [, "val_acc": [S]]}."""
        max_epoch = self.optim_cfgs[0].max_epoch if max_epoch is None else max_epoch
        if directories is not None:
            self._check_directories(directories)
        history = []
        while self.epoch < max_epoch:
            res = run_epoch(len(history))
            rec = {"epoch": self.epoch, "loss": res["loss"].mean(0).tolist()}
            if evaluate is not None:
                rec["val_acc"] = [r["accuracy"] for r in evaluate()]
                if directories:
                    self.after_epoch_eval(directories, rec["val_acc"])
            elif directories and self.epoch == max_epoch:
                self.save_model(directories)
            if verbose:
                print("epoch [{}/{}] loss ".format(self.epoch, max_epoch) + " ".join(f"{v:.4f}" for v in rec["loss"])
                      + ("" if "val_acc" not in rec else " val_acc " + " ".join(f"{v:.2f}" for v in rec["val_acc"])))
            history.append(rec)
        return history


# ---------------------------------------------------------------------- the member-major trainers
class MemberLoopMixin:
    """The member-major step, batch and epoch loop of a trainer that advances S members of `batch_size` images at once
    (`RPOMulti`, `RPOSweep`, `CoCoOpMulti`): needs `n_runs`, `batch_size`, `num_batches`, `batch_idx`, `epoch`, `cfg`,
    `device`, `use_graph`, `_opt`, `_steps`, `_graph`, `_warm`, `_image` / `_label` (the step's own [S*B] buffers),
    `update_lr`, and the trainer's engine calls: `_forward_backward(image, label)`, `_enqueue(image, label)` (that plus the
    optimiser's step) and `_loop_loss()` (the [S] loss buffer)."""

    _loop_name = "RPOMulti"                             # who the refusals of the loop name

    def parse_batch_train(self, batches: Sequence[dict]):
        """S Dassl-style batches {"img": float [B, 3, H, W], "label": [B]} -> one member-major device batch."""
        if len(batches) != self.n_runs:
            raise ValueError(f"{len(batches)} batches for {self.n_runs} members")
        n = self.cfg.n_cls
        for s, b in enumerate(batches):
            lab = torch.as_tensor(b["label"])
            if not lab.is_cuda and lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= n):
                raise IndexError(f"member {s}: target out of bounds (n_cls = {n}; labels must be renumbered after the "
                                 "base/new split)")
        img = torch.cat([torch.as_tensor(b["img"]).to(self.device, dtype=torch.float32) for b in batches]).contiguous()
        label = torch.cat([torch.as_tensor(b["label"]).to(self.device, dtype=torch.int64) for b in batches]).contiguous()
        return img, label

    def _loop_advance(self) -> None:
        if (self.batch_idx + 1) == self.num_batches:
            self.update_lr()
            self.batch_idx = 0
        else:
            self.batch_idx += 1

    # ------------------------------------------------------------------ the step
    def _after_step(self) -> None:
        """What a step invalidates besides `_eval_member` (RPOMulti: the cached text features)."""

    def step_async(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        """One optimisation step of every member, nothing synchronised: image [S*B, 3, H, W] and label [S*B], member-major
        (member s owns rows [s B, (s+1) B)).  Returns loss [S] on the device.  With use_graph the whole step -- the towers,
        the grouped head, the backward chains, the optimiser's launch -- is ONE HIP graph, captured after the first (eager)
        step and again whenever the optimiser's `graph_key` changes (plain SGD without a table: the learning rate, a kernel
        argument; rates and step counters that are device data need no recapture).  Unlike `loop.LoopMixin.step_async` it
        owns its static buffers from construction, takes no ragged batch and warms a resumed run before it captures."""
        assert torch.cuda.current_device() == self.device.index, "set the trainer's device current (torch.cuda.set_device)"
        SB = self.n_runs * self.batch_size
        assert image.shape[0] == SB and label.shape == (SB,), f"step_async takes S * B = {SB} images, member-major"
        if image.data_ptr() != self._image.data_ptr():
            self._image.copy_(image, non_blocking=True)
        self._label.copy_(label, non_blocking=True)
        self._opt.set_epoch(self.epoch)                 # (in front of the step, on its stream; nothing within an epoch)
        key = self._opt.graph_key()                     # what a captured step has baked in besides addresses
        if not self.use_graph or self._steps == 0:
            self._enqueue(self._image, self._label)
            self._warm = True
        else:
            if self._graph is None or self._graph[1] != key:
                if not self._warm:                      # (a resumed run: kernel attributes are set by an eager launch, not in
                    self._forward_backward(self._image, self._label)    # a capture; it writes only what the step overwrites)
                    self._warm = True
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._enqueue(self._image, self._label)
                self._graph = (g, key)                 # (capture does not execute: the replay below is this step)
                self.captures += 1
            self._graph[0].replay()
        self._steps += 1
        self._eval_member = None
        self._after_step()
        return self._loop_loss()

    # ------------------------------------------------------------------ the epoch loop
    def run_epoch(self, image_sets, generators: Optional[Sequence[Optional[torch.Generator]]] = None,
                  plans=None) -> Dict[str, object]:
        """One epoch of every member over its own resident set (`image_sets`: one `DeviceImageSet` per member, or one
        shared set) in the order `epoch_indices` gives a standalone run with that member's generator.  `plans`: per member,
        per batch, the `SamplePlan`s of its images (default: drawn by the transform, member by member within a step).
        As `loop.LoopMixin.run_epoch`: no device scalar is read, and batch t + 1 is in its buffer before step t is
        enqueued.  Returns {"loss": float32 [num_batches, S] on the device, "indices": per member, the batches}."""
        S, B = self.n_runs, self.batch_size
        sets = list(image_sets) if isinstance(image_sets, (list, tuple)) else [image_sets] * S
        if len(sets) != S:
            raise ValueError(f"{len(sets)} image sets for {S} members")
        gens = list(generators) if generators is not None else [None] * S
        batches = member_batches([len(ds) for ds in sets], B, gens, self._loop_name)
        nb = len(batches[0])
        if nb != self.num_batches:
            raise ValueError(f"the sets give {nb} batches of {B} per member; the trainer was built with num_batches = "
                             f"{self.num_batches} (its LR schedule counts on it)")
        if self.batch_idx != 0:
            raise RuntimeError("run_epoch starts at an epoch boundary (batch_idx != 0: forward_backward is mid-epoch)")
        for ds in set(sets):
            ds.check_labels(self.cfg.n_cls)
        with torch.cuda.device(self.device):
            if getattr(self, "_loop_bufs", None) is None:
                self._loop_bufs = [torch.zeros_like(self._image) for _ in range(2)]
            # one transform (= one pair of descriptor slots) per MEMBER, also when members share a set: a slot is reused
            # only after its call of two turns ago has been read, so with one transform for several members the host would
            # wait for the step before inside every fill and the one-batch lookahead would be gone.  (A shared set's spill
            # tail is guarded by the set's own events and every call is on one stream.)  The transforms hold no set.
            if getattr(self, "_member_tfs", None) is None:
                from .input_pipeline import DeviceTransform, InputConfig
                icfg = InputConfig(SIZE=(self.cfg.image_size, self.cfg.image_size))
                self._member_tfs = [DeviceTransform(icfg, True, self.device, B, max_image_bytes=16) for _ in range(S)]
            tfs = self._member_tfs
            labels = torch.stack([ds.labels_dev[torch.tensor(bt, dtype=torch.int64).to(self.device)]
                                  for ds, bt in zip(sets, batches)], 1).reshape(nb, S * B)      # [nb, S*B] member-major
            losses = torch.zeros(nb, S, dtype=torch.float32, device=self.device)

            def fill(t, out):
                for s in range(S):
                    tfs[s].from_set(sets[s], batches[s][t], None if plans is None else plans[s][t], out=out[s * B:(s + 1) * B])

            fill(0, self._loop_bufs[0])
            for t in range(nb):
                cur = self._loop_bufs[t & 1]
                if t + 1 < nb:
                    fill(t + 1, self._loop_bufs[(t + 1) & 1])
                loss = self.step_async(cur, labels[t])
                losses[t].copy_(loss, non_blocking=True)
                self._loop_advance()
        return {"loss": losses, "indices": batches}


# ---------------------------------------------------------------------- one file per member in torch's layout
class MemberCheckpointMixin:
    """Per member, the file the standalone trainer writes and reads (LPSweep, CoCoOpMulti, CoOpSweep), on top of
    `MemberScheduleMixin`.  The trainer supplies `named_parameters(member)` (in torch.optim's parameter order),
    `_param_shapes(member)`, `_checkpoint_name` (the registered model's name = the sub-directory) and, where the standalone
    file holds buffers besides the parameters, `_checkpoint_extra(member)`."""

    _checkpoint_name = "prompt_learner"

    def _checkpoint_extra(self, member: int) -> Dict[str, torch.Tensor]:
        return {}

    def checkpoint_dict(self, member: int, epoch: Optional[int] = None, val_result: Optional[float] = None) -> dict:
        """The dict the standalone trainer with `optim_cfgs[member]` in this state pickles."""
        self._check_member(member)
        epoch = self.epoch if epoch is None else epoch
        optimizer = self._opt.state_dict(self._param_shapes(member), s=member, lr=self.lr[member], steps=self._steps)
        state = {n: t.detach().cpu().clone() for n, t in self.named_parameters(member)}
        state.update(self._checkpoint_extra(member))
        return {"state_dict": state, "epoch": int(epoch), "optimizer": optimizer, "scheduler": {"last_epoch": int(epoch)},
                "val_result": val_result, "steps": int(self._steps)}

    def _save_member(self, member: int, directory: str, epoch, is_best: bool, val_result) -> str:
        ck = self.checkpoint_dict(member, epoch, val_result)
        return write_checkpoint(directory, ck, ck["epoch"], is_best, name=self._checkpoint_name)

    def save_model(self, directories: Sequence[str], epoch: Optional[int] = None, is_best: bool = False,
                   val_results: Optional[Sequence[Optional[float]]] = None) -> List[str]:
        """Per member `<directories[s]>/<_checkpoint_name>/model.pth.tar-<epoch>` (+ `model-best.pth.tar`): the standalone
        trainer's file."""
        self._check_directories(directories)
        return [self._save_member(s, d, epoch, is_best, None if val_results is None else val_results[s])
                for s, d in enumerate(directories)]

    def after_epoch_eval(self, directories: Sequence[str], val_results: Sequence[float]) -> List[bool]:
        """`LoopMixin.after_epoch_eval` per member: keep the checkpoint with the member's best validation result."""
        best = []
        for s, v in enumerate(val_results):
            is_best = v > self.best_results[s]
            if is_best:
                self.best_results[s] = v
                self._save_member(s, directories[s], None, True, v)
            best.append(is_best)
        return best

    def _read(self, directories: Sequence[str], epoch: Optional[int]) -> List[dict]:
        """The members' checkpoint dicts, every tensor checked for its name and shape; nothing on the device is touched."""
        self._check_directories(directories)
        got = []
        for s, d in enumerate(directories):
            path = _model_path(d, self._checkpoint_name, epoch)
            sd = load_checkpoint_file(path)
            names = [n for n, _ in self.named_parameters(s)]
            for name, want in zip(names, self._param_shapes(s)):
                if name not in sd["state_dict"]:
                    raise ValueError(f"{path}: the checkpoint lacks {name}: it was not written by the standalone trainer of a "
                                     f"{type(self).__name__} member ({self._checkpoint_name}: {', '.join(names)})")
                sh = tuple(torch.as_tensor(sd["state_dict"][name]).shape)
                if sh != tuple(want):
                    raise ValueError(f"{path}: {name} has shape {sh}, member {s} of this trainer {tuple(want)}")
            got.append(sd)
        return got

    def _on_device(self):
        """The trainer's device made current (a trainer on host buffers has none to set)."""
        return torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()

    def _load_weights(self, got: Sequence[dict]) -> None:
        with torch.no_grad(), self._on_device():
            for s, ck in enumerate(got):                                 # (buffers beside the parameters are dropped, as
                for name, p in self.named_parameters(s):                 #  the reference's load_model drops them)
                    p.copy_(torch.as_tensor(ck["state_dict"][name]).to(p.dtype).reshape(p.shape))

    def _resume(self, directories: Sequence[str], epoch: Optional[int], what: str) -> int:
        """The standalone trainer's `resume_model` for every member: the weights plus the optimiser state, the epoch and the
        learning rates of the files.  Every file is read and checked, the epochs and the all-or-none optimiser state too,
        before anything on the device is touched.  Returns the epoch to continue from."""
        got = self._read(directories, epoch)
        ep = self._files_epoch(got, what)
        has = [bool((ck.get("optimizer") or {}).get("state")) for ck in got]
        steps = self._files_steps(got, has, what)
        with torch.no_grad(), self._on_device():
            for s, ck in enumerate(got):
                if has[s] and not self._opt.load_state_dict(ck["optimizer"], self._param_shapes(s), s=s,
                                                            steps=ck.get("steps", 1)):
                    raise ValueError(f"{type(self).__name__}.{what}: member {s}'s checkpoint holds optimiser state that is "
                                     f"not {self.optim_cfgs[s].name}'s for its tensors' shapes")
        self._load_weights(got)
        if steps is not None:
            self._steps = steps
        self.epoch = ep
        self.lr = [lr_at_epoch(oc, self.epoch) for oc in self.optim_cfgs]
        with self._on_device():
            self._opt.set_epoch(self.epoch)
            if self._found_inf is not None:                              # the skip counts are the resumed run's own
                self._found_inf.zero_()
        self._graph = None
        return self.epoch
