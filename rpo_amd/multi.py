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

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import members as _members
from . import optim as _optim
from .config import refuse_long_grid
from .custom_clip import refuse_rn
from .loop import EvalMixin
from .members import (MemberLoopMixin, member_batches, member_checkpoint,  # noqa: F401  (importable from here, where they
                      read_member_checkpoint, seeded_prompts)               # were written, under their names)
from .trainer import OptimConfig, lr_at_epoch, write_checkpoint


def _one_of(values, what: str):
    """Members share `what`: a sequence of per-member values is accepted only when they are all equal."""
    if isinstance(values, (list, tuple)):
        if any(v != values[0] for v in values[1:]):
            raise ValueError(f"RPOMulti: per-member {what} is not supported -- the members share one {what} (they run as one "
                             f"batch through the same kernels and one optimiser launch); run members that differ in {what} "
                             "as separate trainers")
        return values[0]
    return values


_WHY_NO_DP = "the members fill the card that data parallelism would split"


class RPOMulti(_members.MemberMixin, MemberLoopMixin, EvalMixin):
    _found_inf = None                                   # amp is refused here; `RPOSweep` has one verdict per member
    _features_why_not = ("RPO's image rows read its members' prompts, so no image feature outlives a step; what an image set "
                         "can cache for RPO is the frozen rows' K / V: FrozenImageKV.build(engine, image_set) and "
                         "test_all(..., frozen=...)")
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
        _members.refuse_world_size("RPOMulti", world_size, _WHY_NO_DP)
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

    # ------------------------------------------------------------------ the step: `MemberLoopMixin.step_async` enqueues these
    def _forward_backward(self, image: torch.Tensor, label: torch.Tensor) -> None:
        self.engine.multi_forward_backward(image, label)

    def _enqueue(self, image: torch.Tensor, label: torch.Tensor) -> None:
        eng = self.engine
        self._forward_backward(image, label)
        self._opt.step(eng.m_params, eng.m_grads, self._found_inf, first_step=(self._steps == 0))

    def _loop_loss(self) -> torch.Tensor:
        return self.engine.m_loss

    def _after_step(self) -> None:
        self.engine.text_f_version = -1

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
        self._check_member(member)
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
        self._check_directories(directories)
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
        self._check_directories(directories)
        got = [read_member_checkpoint(d, epoch, self.cfg) for d in directories]
        ep = self._files_epoch([ck for _, ck in got], "load_model", "the members share one schedule")
        eng, n = self.engine, self.engine.m_params.shape[1]
        shapes = [(self.cfg.K, self.cfg.d_t), (self.cfg.K, self.cfg.d_v)]
        self._load_states(got, lambda s: dict(param_shapes=shapes, scatter=lambda d, r: d[s * n:(s + 1) * n].copy_(r)))
        eng.m_params.copy_(torch.stack([p for p, _ in got]))
        self.epoch = ep
        self.lr = lr_at_epoch(self.optim_cfg, self.epoch)
        self._opt.set_epoch(self.epoch)
        self._eval_member = None
        eng.text_f_version = -1

    def _load_states(self, got, member_kw) -> None:
        """The members' optimiser states from their files (`member_kw(s)`: where member s's state goes): every file has
        one -- then `_steps` is the files' -- or none has; a mix is refused."""
        have = [self._opt.load_state_dict(ck.get("optimizer"), steps=ck.get("steps", 1), **member_kw(s))
                for s, (_, ck) in enumerate(got)]
        steps = self._files_steps([ck for _, ck in got], have, "load_model")
        if steps is not None:
            self._steps = steps
