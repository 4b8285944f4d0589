"""``RPOMulti``: S independent RPO runs ("members": the seeds of one recipe) advanced by ONE step on the shared frozen
towers (rpo_amd/engine_multi.py).

The reference's recipe is three seeds per dataset at batch 4 (configs/trainers/RPO/main_K24.yaml `BATCH_SIZE: 4`,
scripts/rpo/base2new_generalization_main.sh `for seed in 1 2 3`), run one after the other.  Here the members share
one CLIP, one class set, K, the storage mode and the optimiser schedule; each has its own text / image prompts,
momentum, batch of B images with labels, and loss.  Member s ends a step where a standalone ``RPO`` with the same
prompts, batch and learning rate ends it: the summation orders are the standalone run's, only the GEMM plans are those
of the larger row counts (S * B images, S * n_cls * K text rows).

The surface is ``RPO``'s with a member axis: ``forward_backward`` takes S Dassl-style batches, ``step_async`` one
member-major [S*B] batch, ``run_epoch`` one resident set and one generator per member; evaluation and checkpoints are
per member and interchangeable with a standalone ``RPO``'s.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import optim as _optim
from .config import RPOConfig, refuse_long_grid
from .custom_clip import init_prompts, refuse_rn
from .loop import EvalMixin, epoch_indices
from .trainer import OptimConfig, checkpoint_dict, load_checkpoint_file, lr_at_epoch, write_checkpoint


def _one_of(values, what: str):
    """Members share `what`: a sequence of per-member values is accepted only when they are all equal."""
    if isinstance(values, (list, tuple)):
        if any(v != values[0] for v in values[1:]):
            raise ValueError(f"RPOMulti: per-member {what} is not supported -- the members share one {what} (they run as one "
                             f"batch through the same kernels and one optimiser launch); run members that differ in {what} "
                             "as separate trainers")
        return values[0]
    return values


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


def read_member_checkpoint(directory: str, epoch: Optional[int], cfg: RPOConfig):
    """(flat params, checkpoint dict) of a file ``RPO.save_model`` / ``RPOMulti.save_model`` wrote."""
    model_file = "model-best.pth.tar" if epoch is None else f"model.pth.tar-{epoch}"
    model_path = os.path.join(directory, "prompt_learner", model_file)
    if not os.path.exists(model_path):
        raise FileNotFoundError(f'Model not found at "{model_path}"')
    ck = load_checkpoint_file(model_path)
    sd = ck["state_dict"]
    tp, ip = sd["text_prompt"].float(), sd["img_prompt"].float()
    if tuple(tp.shape) != (cfg.K, cfg.d_t) or tuple(ip.shape) != (cfg.K, cfg.d_v):
        raise ValueError(f"{model_path}: prompts {tuple(tp.shape)} / {tuple(ip.shape)}, this trainer has K = {cfg.K}, "
                         f"widths {cfg.d_t} / {cfg.d_v}")
    flat = torch.cat([tp.reshape(-1), ip.reshape(-1)])
    return flat, ck


class MemberLoopMixin:
    """The member-major batch and epoch loop of a trainer that advances S members of `batch_size` images by one
    `step_async(image [S*B], label [S*B])` (`RPOMulti`, `RPOSweep`, `CoCoOpMulti`): needs `n_runs`, `batch_size`, `num_batches`,
    `batch_idx`, `cfg`, `device`, `_image` (the step's own [S*B] image buffer), `update_lr`."""

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


class RPOMulti(MemberLoopMixin, EvalMixin):
    _found_inf = None                                   # amp is refused here; `RPOSweep` has one verdict per member
    _features_why_not = ("RPO's image rows read its members' prompts, so no image feature outlives a step; what an image set "
                         "can cache for RPO is the frozen rows' K / V: FrozenImageKV.build(engine, image_set) and "
                         "test_all(..., frozen=...)")
    _one_counter = " (one step counter covers every member)"     # why a mix of files with and without state is refused
    captures = 0                                        # HIP graphs of the step captured so far (one per distinct learning rate)

    def __init__(self, cfg, state_dict: Dict[str, np.ndarray], tokens: Optional[np.ndarray] = None, n_runs: int = 1,
                 batch_size: int = 4, prompts: Optional[Sequence[tuple]] = None, seeds: Optional[Sequence[int]] = None,
                 optim=None, device: str | torch.device = "cuda:0", act_dtype: torch.dtype = torch.bfloat16,
                 num_batches: int = 1, use_graph: bool = True, amp: bool = False, world_size: int = 1):
        # ---- refusals, before any device is touched
        cfg = _one_of(cfg, "K / class set / backbone (config)")
        optim = _one_of(optim, "learning rate / optimiser schedule")
        refuse_rn(cfg, "RPOMulti")
        if amp:
            raise NotImplementedError("RPOMulti: amp=True is not supported (GradScaler's skip is one verdict per optimiser "
                                      "step; the members would need one each): run amp members as separate RPO trainers")
        if world_size != 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise NotImplementedError("RPOMulti: world_size > 1 is not supported (the members fill the card that data "
                                      "parallelism would split); run one RPOMulti per GPU with different members")
        S, B = int(n_runs), int(batch_size)
        if S < 1 or B < 1:
            raise ValueError(f"RPOMulti: n_runs = {n_runs}, batch_size = {batch_size}: both must be >= 1")
        if (prompts is None) == (seeds is None):
            raise ValueError("RPOMulti: pass exactly one of prompts=[(text_prompt, img_prompt)] * n_runs or seeds=[...]")
        if len(prompts if prompts is not None else seeds) != S:
            raise ValueError(f"RPOMulti: {len(prompts if prompts is not None else seeds)} prompts / seeds for n_runs = {S}")
        self.optim_cfg = optim or OptimConfig()
        _optim.validate(self.optim_cfg)
        self.lr = lr_at_epoch(self.optim_cfg, 0)
        if prompts is None:
            prompts = seeded_prompts(state_dict, cfg, seeds)
        self._build(cfg, state_dict, tokens, S, B, prompts, device, act_dtype, num_batches, use_graph)
        n = self.engine.m_params.numel()                # the members share the config: the flat [S, text | img] buffer is ONE
        with torch.cuda.device(self.device):            # set, one launch (the update is elementwise)
            self._opt = _optim.make_optimizer([self.optim_cfg], n, n, 0, self.device, s0=self.engine.m_mom)

    def _build(self, cfg, state_dict, tokens, S: int, B: int, prompts, device, act_dtype, num_batches: int, use_graph: bool,
               member_K: Optional[Sequence[int]] = None) -> None:
        """Everything behind the refusals: the loop state, the engine for S * B images and the members' buffers (shared with
        `RPOSweep`, whose members bring their own K: `member_K`)."""
        self.cfg, self.n_runs, self.batch_size, self.num_batches = cfg, S, B, num_batches
        self.use_graph = use_graph
        self.epoch = self.batch_idx = self._steps = 0
        self._graph = None                              # (HIP graph of one step, the optimiser's `graph_key` it was captured with)
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
            # the image tower's workspace, GEMM plans and row-unit hints are those of S * B images
            self.engine = make_engine(cfg, state_dict, tokens, self.device, act_dtype, S * B)
            self.engine.multi_setup(S, B, **({} if member_K is None else dict(member_K=member_K)))
            self.set_prompts(prompts)
            self._image = torch.zeros(S * B, 3, cfg.image_size, cfg.image_size, device=self.device)
            self._label = torch.zeros(S * B, dtype=torch.int64, device=self.device)

    # ------------------------------------------------------------------ members' state
    def set_prompts(self, prompts: Sequence[tuple]) -> None:
        eng, nt = self.engine, self.cfg.K * self.cfg.d_t
        host = torch.empty(self.n_runs, eng.m_params.shape[1])
        for s, (tp, ip) in enumerate(prompts):
            host[s, :nt] = torch.from_numpy(np.asarray(tp, dtype=np.float32)).reshape(-1)
            host[s, nt:] = torch.from_numpy(np.asarray(ip, dtype=np.float32)).reshape(-1)
        eng.m_params.copy_(host)
        self._eval_member = None

    # ------------------------------------------------------------------ the step
    def _enqueue(self, image: torch.Tensor, label: torch.Tensor) -> None:
        eng = self.engine
        eng.multi_forward_backward(image, label)
        self._opt.step(eng.m_params, eng.m_grads, self._found_inf, first_step=(self._steps == 0))

    def step_async(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        """One optimisation step of every member, nothing synchronised: image [S*B, 3, H, W] and label [S*B], member-major
        (member s owns rows [s B, (s+1) B)).  Returns loss [S] on the device.  With use_graph the whole step -- both
        towers, the grouped head, both backward chains, the SGD launch -- is ONE HIP graph, captured after the first
        (eager) step and again whenever the optimiser's `graph_key` changes (plain SGD: the learning rate, a kernel argument)."""
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
                    self.engine.multi_forward_backward(self._image, self._label)    # a capture; it writes only what the step
                    self._warm = True                                                 # overwrites)
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._enqueue(self._image, self._label)
                self._graph = (g, key)                 # (capture does not execute: the replay below is this step)
                self.captures += 1
            self._graph[0].replay()
        self._steps += 1
        self._eval_member = None
        self.engine.text_f_version = -1
        return self.engine.m_loss

    def forward_backward(self, batches: Sequence[dict]) -> List[Dict[str, float]]:
        """trainers/rpo.py:290-316 for every member: a list of S batches in, a list of S {"loss", "acc"} out."""
        S, B = self.n_runs, self.batch_size
        with torch.cuda.device(self.device):
            image, label = self.parse_batch_train(batches)
            loss = self.step_async(image, label)
            pred = self.engine.m_logits.argmax(1)
            acc = (pred == label).view(S, B).float().mean(1) * 100.0                 # compute_accuracy()[0], per member
            loss, acc = loss.tolist(), acc.tolist()                                    # D2H sync, as the reference (:311)
        self._loop_advance()
        return [{"loss": float(loss[s]), "acc": float(acc[s])} for s in range(S)]

    def update_lr(self) -> None:
        self.epoch += 1
        self.lr = lr_at_epoch(self.optim_cfg, self.epoch)
        self._opt.set_epoch(self.epoch)

    # ------------------------------------------------------------------ evaluation: the single-run path, one member
    def _select(self, member: int) -> None:
        if not 0 <= member < self.n_runs:
            raise IndexError(f"member {member} of {self.n_runs}")
        if self._eval_member != member:
            self.engine.multi_load_member(member)
            self._eval_member = member

    @torch.no_grad()
    def model_inference(self, image: torch.Tensor, member: int = 0, classes=None) -> torch.Tensor:
        """logits [B, n_cls] of member `member` (trainers/rpo.py:229-232 eval branch, through `Engine.forward_eval`);
        `classes`: a `ClassSet` (`class_set(tokens)`) -- logits [B, n'] against it."""
        with torch.cuda.device(self.device):
            self._select(member)
            image = image.to(device=self.device, dtype=torch.float32).contiguous()
            return self.engine.forward_eval(image, classes=classes).clone()

    def _eval_logits(self, image: torch.Tensor, classes=None) -> torch.Tensor:
        return self.engine.forward_eval(image, classes=classes)

    def test(self, image_set, member: int = 0, batch_size: int = 100, verbose: bool = True, per_class_result: bool = False,
             classes=None, features=None):
        """Dassl's `test()` for member `member` (loop.EvalMixin.test); `classes`: against that `ClassSet`."""
        self._refuse_features(features, "test(features=...)")
        with torch.cuda.device(self.device):
            self._select(member)
        return super().test(image_set, batch_size, verbose, per_class_result, classes=classes)

    # ------------------------------------------------------------------ evaluation: all members per frozen image pass
    def _shared_sides(self, classes=None):
        """(img_prompts [S, K, d_v], text_f [S * n_cls * K, e], k_used): k_used is None here -- every member averages over
        all K pairs; `RPOSweep` returns its members' own K as int32 [S] on the device.  `classes`: the members' text
        features of that `ClassSet`, computed one member after the other through the single-run parameters."""
        eng = self.engine
        if classes is None:
            return eng.m_img_prompt, eng.multi_text_features(), None
        S, rows = self.n_runs, classes.n * self.cfg.K
        text_f = classes.shared_buffers(S, 1)["text_f"][:S * rows]
        for s in range(S):
            eng.multi_load_member(s)
            eng.class_text_features(classes, out=text_f[s * rows:(s + 1) * rows])
        self._eval_member = S - 1                    # (whose prompts the single-run parameters now hold)
        return eng.m_img_prompt, text_f, None

    @torch.no_grad()
    def _sides_logits(self, image: torch.Tensor, sides) -> torch.Tensor:
        """One frozen image pass for the batch, then the prompt rows of the sets `sides()` names: logits [S', B, n_cls]."""
        eng = self.engine
        with torch.cuda.device(self.device):
            image = image.to(device=self.device, dtype=torch.float32).contiguous()
            B = image.shape[0]
            eng.prompt_rows_setup(self.n_runs, B)
            img_prompts, text_f, k_used = sides()
            eng.frozen_pass(image)
            kv = eng.live_kv()
            kv.set_first(0, B)
            return eng.shared_eval_logits(B, kv, img_prompts, text_f, k_used=k_used).clone()

    @torch.no_grad()
    def model_inference_all(self, image: torch.Tensor) -> torch.Tensor:
        """logits [S, B, n_cls] of every member for one batch: ONE frozen image pass, then the S * B * K prompt rows of all
        members on its K / V (rpo_amd/engine_prompt_rows.py).  Member s's slice is what `model_inference(image, member=s)`
        computes, up to the summation order of the GEMM plans."""
        return self._sides_logits(image, self._shared_sides)

    def test_all(self, image_set, batch_size: int = 100, frozen=None, verbose: bool = True, per_class_result: bool = False,
                 hook=None, classes=None, features=None) -> List[dict]:
        """Dassl's `test()` for EVERY member in one pass over the set: per chunk one frozen image pass (none with `frozen`,
        a `FrozenImageKV` of this set) and one prompt-row pass for all S members.  Returns, per member, the dict
        `test(image_set, member=s)` returns.  `classes`: against that `ClassSet`."""
        self._refuse_features(features, "test_all(features=...)")
        refuse_long_grid(self.cfg, f"{type(self).__name__}.test_all")
        return self._test_shared(image_set, self.n_runs, lambda: self._shared_sides(classes), batch_size, frozen, verbose,
                                 per_class_result, hook, classes=classes)

    # ------------------------------------------------------------------ checkpoints: per member, a standalone RPO's files
    def save_model(self, directories: Sequence[str], epoch: Optional[int] = None, is_best: bool = False,
                   val_results: Optional[Sequence[Optional[float]]] = None) -> List[str]:
        """Per member, the file a standalone `RPO.save_model(directories[s])` writes (same keys, Dassl layout, momentum)."""
        if len(directories) != self.n_runs:
            raise ValueError(f"{len(directories)} directories for {self.n_runs} members")
        epoch = self.epoch if epoch is None else epoch
        p = self.engine.m_params.detach().cpu()
        n, shapes, out = p.shape[1], [(self.cfg.K, self.cfg.d_t), (self.cfg.K, self.cfg.d_v)], []
        for s, d in enumerate(directories):
            entry = self._opt.state_dict(shapes, lr=self.lr, steps=self._steps, gather=lambda row: row[s * n:(s + 1) * n])
            ck = member_checkpoint(p[s], None, self.cfg, epoch, self.optim_cfg, self.lr, self._steps,
                                   None if val_results is None else val_results[s], entry)
            out.append(write_checkpoint(d, ck, epoch, is_best))
        return out

    def load_model(self, directories: Sequence[str], epoch: Optional[int] = None) -> None:
        """Reads S files written by standalone runs (or by `save_model`): prompts, momentum, epoch (trainers/rpo.py:325-357).
        The members share the schedule: files of different epochs are refused."""
        if len(directories) != self.n_runs:
            raise ValueError(f"{len(directories)} directories for {self.n_runs} members")
        got = [read_member_checkpoint(d, epoch, self.cfg) for d in directories]
        epochs = [int(ck.get("epoch", 0)) for _, ck in got]
        if any(e != epochs[0] for e in epochs):
            raise ValueError(f"RPOMulti.load_model: the checkpoints are of epochs {epochs}; the members share one schedule")
        eng, n = self.engine, self.engine.m_params.shape[1]
        shapes = [(self.cfg.K, self.cfg.d_t), (self.cfg.K, self.cfg.d_v)]
        self._load_states(got, lambda s: dict(param_shapes=shapes, scatter=lambda d, r: d[s * n:(s + 1) * n].copy_(r)))
        eng.m_params.copy_(torch.stack([p for p, _ in got]))
        self.epoch = epochs[0]
        self.lr = lr_at_epoch(self.optim_cfg, self.epoch)
        self._opt.set_epoch(self.epoch)
        self._eval_member = None
        eng.text_f_version = -1

    def _load_states(self, got, member_kw) -> None:
        """The members' optimiser states from their files (`member_kw(s)`: where member s's state goes): every file has
        one -- then `_steps` is the files' -- or none has; a mix is refused."""
        have = [self._opt.load_state_dict(ck.get("optimizer"), steps=ck.get("steps", 1), **member_kw(s))
                for s, (_, ck) in enumerate(got)]
        if any(have) != all(have):
            raise ValueError(f"{type(self).__name__}.load_model: some checkpoints carry "
                             + ("optimiser state and some do not" + self._one_counter if self._opt.table_driven else
                                "momentum and some do not (one first-step flag covers every member)"))
        if all(have):
            self._steps = max(1, max(int(ck.get("steps", 1)) for _, ck in got))
