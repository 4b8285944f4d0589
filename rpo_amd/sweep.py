"""``RPOSweep``: the points of a hyper-parameter sweep as the members of ONE step on the shared frozen towers -- each
member with its own K, its own optimiser settings and schedule, and (amp) its own Inf / NaN verdict.

``RPOMulti`` (rpo_amd/multi.py) advances S runs of one recipe.  The sweeps of the method vary what it holds fixed: K is the
paper's ablated hyper-parameter (the reference ships configs/trainers/RPO/main_K4.yaml, main.yaml, main_K24.yaml), the
OPTIM block is tuned per dataset, PREC amp is one of the trainer's three precisions (trainers/rpo.py:298-304).  Nothing
reads a prompt, so prompt row i of a member depends on no other prompt row: a member that uses the
first K_s of the engine's K = max K_s rows IS a standalone K_s run as soon as the head averages over K_s pairs
(rpo_head_fwd_bwd_grouped_k) and the optimiser and the checkpoint see those rows only (rpo_sgd_step_sets, the gather /
scatter below).  The other rows ("inert") are zero, get zero gradients and ride along: a member costs what a K member costs.

The optimiser settings live in a device table [S, 4] = (lr, momentum, weight decay, grad_scale): a new epoch's learning
rates are one small copy on the step's stream, and the step's HIP graph is captured ONCE (`captures`).

The surface is ``RPOMulti``'s, whose step, epoch loop and shared evaluation this class inherits; evaluation of one member
goes through the shared prompt-row pass with that member's K, and a member's checkpoint is the file a standalone
``RPO`` with ``cfg.K = K_s`` writes and reads.
"""
from __future__ import annotations

import dataclasses
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops, optim as _optim
from .custom_clip import init_prompts, refuse_rn
from .multi import RPOMulti, member_checkpoint, read_member_checkpoint
from .trainer import OptimConfig, _prompt_shapes, lr_at_epoch, write_checkpoint


def member_row_to_flat(row: torch.Tensor, K: int, K_s: int, d_t: int, d_v: int) -> torch.Tensor:
    """A member's row [K d_t | K d_v] of the engine's buffers -> the flat vector [K_s d_t | K_s d_v] of a standalone run with
    K_s prompts (its `params` / `mom`): the leading K_s rows of both blocks."""
    nt = K * d_t
    return torch.cat([row[:K_s * d_t], row[nt:nt + K_s * d_v]])


def flat_to_member_row(flat: torch.Tensor, K: int, K_s: int, d_t: int, d_v: int) -> torch.Tensor:
    """The inverse: a standalone run's flat [K_s d_t | K_s d_v] into a row [K d_t | K d_v] whose inert columns are zero."""
    if flat.numel() != K_s * (d_t + d_v):
        raise ValueError(f"{flat.numel()} floats for K_s = {K_s} prompts of widths {d_t} / {d_v}")
    nt = K * d_t
    row = torch.zeros(K * (d_t + d_v), dtype=flat.dtype, device=flat.device)
    row[:K_s * d_t] = flat[:K_s * d_t]
    row[nt:nt + K_s * d_v] = flat[K_s * d_t:]
    return row


def used_table(member_K: Sequence[int], d_t: int, d_v: int) -> torch.Tensor:
    """int32 [S, 2]: the leading floats of the text / img segment of each member's row that are its own (rpo_sgd_step_sets)."""
    return torch.tensor([[k * d_t, k * d_v] for k in member_K], dtype=torch.int32)


def hyper_table(optims: Sequence[OptimConfig], epoch: int, grad_scale: float = 1.0) -> torch.Tensor:
    """float32 [S, 4]: (lr_at_epoch(optim_s, epoch), momentum, weight decay, grad_scale) per member, rounded to float32 as the
    scalar arguments of rpo_sgd_step are."""
    return torch.tensor([[lr_at_epoch(oc, epoch), oc.momentum, oc.weight_decay, grad_scale] for oc in optims],
                        dtype=torch.float64).to(torch.float32)


def sweep_prompts(state_dict: Dict[str, np.ndarray], members: Sequence[dict], d_t: int, d_v: int) -> List[tuple]:
    """Member s's initial (text_prompt [K_s, d_t], img_prompt [K_s, d_v]): its `prompts`, or what a standalone ``RPO`` with
    cfg.K = K_s draws under ``torch.manual_seed(seed)`` (custom_clip.init_prompts), member by member."""
    out = []
    for m in members:
        if m.get("prompts") is not None:
            tp, ip = m["prompts"]
            out.append((np.asarray(tp, dtype=np.float32), np.asarray(ip, dtype=np.float32)))
        else:
            torch.manual_seed(int(m["seed"]))
            out.append(init_prompts(state_dict, int(m["K"]), d_t, d_v))
    return out


def _shared(members: Sequence[dict], key: str, default, what: str):
    """A setting all members share: a member may repeat it, a different value is refused by name."""
    vals = [m.get(key, default) for m in members]
    vals = [default if v is None else v for v in vals]
    ref = default if default is not None else vals[0]
    if any(v != ref for v in vals):
        raise ValueError(f"RPOSweep: the members differ in {what} ({key} = {vals}); the members of a sweep share one {what} "
                         "-- run those that differ as separate trainers")
    return ref


class RPOSweep(RPOMulti):
    def __init__(self, cfg, state_dict: Dict[str, np.ndarray], tokens: Optional[np.ndarray] = None,
                 members: Sequence[dict] = (), batch_size: int = 4, device: str | torch.device = "cuda:0",
                 act_dtype: torch.dtype = torch.bfloat16, num_batches: int = 1, use_graph: bool = True, amp: bool = False,
                 world_size: int = 1):
        """members: per member dict(seed= | prompts=(text_prompt [K_s, d_t], img_prompt [K_s, d_v]), K=K_s, optim=OptimConfig).
        `cfg` gives the CLIP, the class set and the widths; its K is replaced by max K_s."""
        # ---- refusals, before any device is touched
        members = [dict(m) for m in members]
        S, B = len(members), int(batch_size)
        if S < 1 or B < 1:
            raise ValueError(f"RPOSweep: {S} members, batch_size = {batch_size}: both must be >= 1")
        cfg = _shared(members, "cfg", cfg, "CLIP / class set / backbone (config)")
        refuse_rn(cfg, "RPOSweep")
        if world_size != 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise NotImplementedError("RPOSweep: world_size > 1 is not supported (the members fill the card that data "
                                      "parallelism would split); run one RPOSweep per GPU with different members")
        _shared(members, "batch_size", B, "batch size")
        act_dtype = _shared(members, "act_dtype", act_dtype, "storage mode (act_dtype)")
        for s, m in enumerate(members):
            if (m.get("seed") is None) == (m.get("prompts") is None):
                raise ValueError(f"RPOSweep: member {s} needs exactly one of seed= or prompts=(text_prompt, img_prompt)")
            if "K" not in m or int(m["K"]) < 1:
                raise ValueError(f"RPOSweep: member {s} has K = {m.get('K')}: every member names its own K >= 1")
            m["K"] = int(m["K"])
            m["optim"] = m.get("optim") or OptimConfig()
            _optim.validate(m["optim"])
        self.optim_cfgs = [m["optim"] for m in members]
        epochs = [oc.max_epoch for oc in self.optim_cfgs]
        if any(e != epochs[0] for e in epochs):
            raise ValueError(f"RPOSweep: the members differ in max_epoch ({epochs}): one loop runs all members, and the cosine "
                             "schedule counts on its length -- run schedules of different lengths as separate trainers")
        self.member_K = [m["K"] for m in members]
        for s, m in enumerate(members):
            if m.get("prompts") is not None:
                tp, ip = m["prompts"]
                if tuple(np.shape(tp)) != (m["K"], cfg.d_t) or tuple(np.shape(ip)) != (m["K"], cfg.d_v):
                    raise ValueError(f"RPOSweep: member {s}'s prompts are {np.shape(tp)} / {np.shape(ip)} for K = {m['K']}, "
                                     f"widths {cfg.d_t} / {cfg.d_v}")
        self.amp = bool(amp)
        self.member_cfgs = [dataclasses.replace(cfg, K=k) for k in self.member_K]
        cfg = dataclasses.replace(cfg, K=max(self.member_K))           # the engine's K: it checks its own limits
        self.lr = [lr_at_epoch(oc, 0) for oc in self.optim_cfgs]
        self._hyper_epoch = None                                       # the epoch whose rates the device table holds
        self._build(cfg, state_dict, tokens, S, B, sweep_prompts(state_dict, members, cfg.d_t, cfg.d_v), device, act_dtype,
                    num_batches, use_graph, member_K=self.member_K)
        with torch.cuda.device(self.device):
            self._hyper = torch.zeros(S, 4, dtype=torch.float32, device=self.device)
            # every epoch's table, uploaded once: a new epoch's rates are then one device-side [S, 4] copy on the step's stream
            self._hyper_epochs = torch.stack([hyper_table(self.optim_cfgs, e)
                                              for e in range(self.optim_cfgs[0].max_epoch + 1)]).to(self.device)
            self._used = used_table(self.member_K, cfg.d_t, cfg.d_v).to(self.device)
            self._found_inf = torch.zeros(S, 2, dtype=torch.int32, device=self.device) if self.amp else None
            # a member that is not plain SGD: every member goes through rpo_optim_step_sets, `kind` and `hyper` per member
            # (plain-SGD members keep their momentum in m_mom and get the bits of rpo_sgd_step_sets)
            if not all(_optim.is_plain_sgd(oc) for oc in self.optim_cfgs):
                self._opt = _optim.OptimState(self.optim_cfgs, self.engine.m_params.stride(0), cfg.K * cfg.d_t,
                                              cfg.K * cfg.d_v, self.device, s0=self.engine.m_mom, used=self._used)

    # ------------------------------------------------------------------ members' state
    def _dims(self, s: int):
        return self.cfg.K, self.member_K[s], self.cfg.d_t, self.cfg.d_v

    def set_prompts(self, prompts: Sequence[tuple]) -> None:
        """Member s's (text_prompt [K_s, d_t], img_prompt [K_s, d_v]) into the leading rows of its row; the inert rows zero."""
        host = torch.stack([flat_to_member_row(torch.cat([torch.from_numpy(np.asarray(tp, dtype=np.float32)).reshape(-1),
                                                          torch.from_numpy(np.asarray(ip, dtype=np.float32)).reshape(-1)]),
                                               *self._dims(s)) for s, (tp, ip) in enumerate(prompts)])
        self.engine.m_params.copy_(host)
        self.engine.text_f_version = -1
        self._eval_member = None

    def skipped_steps(self) -> List[int]:
        """amp: per member, the steps skipped so far because its own used gradients held Inf / NaN (one D2H read)."""
        if self._found_inf is None:
            return [0] * self.n_runs
        return [int(v) for v in self._found_inf[:, 1].tolist()]

    # ------------------------------------------------------------------ the step
    def _graph_key(self):
        return 0                                        # the rates are device data: one capture serves every epoch

    def _refresh_hyper(self) -> None:
        if self._opt is not None:
            self._opt.set_epoch(self.epoch)
        elif self._hyper_epoch != self.epoch:
            if 0 <= self.epoch < self._hyper_epochs.shape[0]:
                self._hyper.copy_(self._hyper_epochs[self.epoch])
            else:                                       # (past the schedule's end: the formula still gives a rate)
                self._hyper.copy_(hyper_table(self.optim_cfgs, self.epoch))
            self._hyper_epoch = self.epoch

    def _enqueue(self, image: torch.Tensor, label: torch.Tensor) -> None:
        eng, cfg = self.engine, self.cfg
        eng.multi_forward_backward(image, label)
        if self._opt is not None:
            self._opt.step(eng.m_params, eng.m_grads, self._found_inf)
            return
        ops.sgd_step_sets(eng.m_params, eng.m_grads, eng.m_mom, self._hyper, cfg.K * cfg.d_t, cfg.K * cfg.d_v,
                          first_step=(self._steps == 0), used=self._used, found_inf=self._found_inf)

    def step_async(self, image: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        """`RPOMulti.step_async` with every member's own rate: the table is refreshed (one [S, 4] copy on the current
        stream, in front of the step) when the epoch has advanced; the graph is captured once."""
        assert torch.cuda.current_device() == self.device.index, "set the trainer's device current (torch.cuda.set_device)"
        self._refresh_hyper()
        return super().step_async(image, label)

    def update_lr(self) -> None:
        self.epoch += 1
        self.lr = [lr_at_epoch(oc, self.epoch) for oc in self.optim_cfgs]

    def train(self, image_sets, max_epoch: Optional[int] = None, generators=None, directories: Optional[Sequence[str]] = None,
              verbose: bool = True) -> List[dict]:
        """`run_epoch` until `max_epoch` (default: the members' shared one); the last epoch's models are saved to
        `directories`.  One record per epoch: the members' mean losses (one read per epoch)."""
        max_epoch = self.optim_cfgs[0].max_epoch if max_epoch is None else max_epoch
        history = []
        while self.epoch < max_epoch:
            res = self.run_epoch(image_sets, generators)
            rec = {"epoch": self.epoch, "loss": res["loss"].mean(0).tolist()}
            if verbose:
                print("epoch [{}/{}] loss ".format(self.epoch, max_epoch) + " ".join(f"{v:.4f}" for v in rec["loss"]))
            history.append(rec)
        if directories:
            self.save_model(directories)
        return history

    # ------------------------------------------------------------------ evaluation of one member: the shared path, S = 1
    def _select(self, member: int) -> None:
        raise RuntimeError("RPOSweep evaluates a member through the shared prompt-row path with the member's own K "
                           "(model_inference / test); the single-run eval path averages over the engine's K")

    def _member_sides(self, member: int):
        if not 0 <= member < self.n_runs:
            raise IndexError(f"member {member} of {self.n_runs}")
        eng, rows = self.engine, self.cfg.n_cls * self.cfg.K
        text_f = eng.multi_text_features()[member * rows:(member + 1) * rows]
        return eng.m_img_prompt[member:member + 1], text_f, eng.m_k_used[member:member + 1]

    def _shared_sides(self):
        eng = self.engine
        return eng.m_img_prompt, eng.multi_text_features(), eng.m_k_used

    @torch.no_grad()
    def model_inference(self, image: torch.Tensor, member: int = 0) -> torch.Tensor:
        """logits [B, n_cls] of member `member`, averaged over its own K_s pairs."""
        return self._sides_logits(image, lambda: self._member_sides(member))[0]

    def test(self, image_set, member: int = 0, batch_size: int = 100, verbose: bool = True, per_class_result: bool = False,
             frozen=None):
        """Dassl's `test()` for member `member` (loop.EvalMixin._test_shared with that member alone)."""
        return self._test_shared(image_set, 1, lambda: self._member_sides(member), batch_size, frozen, verbose,
                                 per_class_result)[0]

    # ------------------------------------------------------------------ checkpoints: per member, a standalone RPO(K_s)'s files
    def save_model(self, directories: Sequence[str], epoch: Optional[int] = None, is_best: bool = False,
                   val_results: Optional[Sequence[Optional[float]]] = None) -> List[str]:
        """Per member, the file a standalone `RPO(cfg.K = K_s, optim_s).save_model(directories[s])` writes: prompts
        [K_s, d], momentum in its flat order, the member's own learning rate and optimiser settings."""
        if len(directories) != self.n_runs:
            raise ValueError(f"{len(directories)} directories for {self.n_runs} members")
        epoch = self.epoch if epoch is None else epoch
        p, m = self.engine.m_params.detach().cpu(), self.engine.m_mom.detach().cpu()
        out = []
        for s, d in enumerate(directories):
            ck = member_checkpoint(member_row_to_flat(p[s], *self._dims(s)), member_row_to_flat(m[s], *self._dims(s)),
                                   self.member_cfgs[s], epoch, self.optim_cfgs[s], self.lr[s], self._steps,
                                   None if val_results is None else val_results[s])
            if self._opt is not None and not _optim.is_plain_sgd(self.optim_cfgs[s]):
                ck["optimizer"] = self._opt.state_dict(_prompt_shapes(ck["state_dict"]), s=s, lr=self.lr[s],
                                                       gather=lambda row, s=s: member_row_to_flat(row, *self._dims(s)))
            out.append(write_checkpoint(d, ck, epoch, is_best))
        return out

    def load_model(self, directories: Sequence[str], epoch: Optional[int] = None) -> None:
        """Reads S files written by standalone `RPO(cfg.K = K_s)` runs (or by `save_model`).  One loop runs all members:
        files of different epochs are refused."""
        if len(directories) != self.n_runs:
            raise ValueError(f"{len(directories)} directories for {self.n_runs} members")
        got = [read_member_checkpoint(d, epoch, self.member_cfgs[s]) for s, d in enumerate(directories)]
        epochs = [int(ck.get("epoch", 0)) for _, _, ck in got]
        if any(e != epochs[0] for e in epochs):
            raise ValueError(f"RPOSweep.load_model: the checkpoints are of epochs {epochs}; one loop runs all members")
        moms = [m for _, m, _ in got]
        if self._opt is not None:
            # per member its own kind's state; a plain-SGD member's momentum is `moms[s]` as before
            shapes = [[(k, self.cfg.d_t), (k, self.cfg.d_v)] for k in self.member_K]
            plain = [_optim.is_plain_sgd(oc) for oc in self.optim_cfgs]
            have = [(moms[s] is not None) if plain[s] else
                    (_optim.rows_from_state_dict(self.optim_cfgs[s], got[s][2].get("optimizer"), shapes[s]) is not None)
                    for s in range(self.n_runs)]
            if any(have) != all(have):
                raise ValueError("RPOSweep.load_model: some checkpoints carry optimiser state and some do not")
            if all(have):
                for s, (_, _, ck) in enumerate(got):
                    self._opt.load_state_dict(ck.get("optimizer"), shapes[s], s=s, steps=ck.get("steps", 1),
                                              scatter=lambda d, r, s=s: d.copy_(flat_to_member_row(r, *self._dims(s))))
                self._steps = max(1, max(int(ck.get("steps", 1)) for _, _, ck in got))
            self._opt.epoch = None
            moms = [None] * self.n_runs
        if any(m is None for m in moms) != all(m is None for m in moms):
            raise ValueError("RPOSweep.load_model: some checkpoints carry momentum and some do not (one first-step flag "
                             "covers every member)")
        eng = self.engine
        eng.m_params.copy_(torch.stack([flat_to_member_row(p, *self._dims(s)) for s, (p, _, _) in enumerate(got)]))
        if moms[0] is not None:
            eng.m_mom.copy_(torch.stack([flat_to_member_row(m, *self._dims(s)) for s, m in enumerate(moms)]))
            self._steps = max(1, max(int(ck.get("steps", 1)) for _, _, ck in got))
        self.epoch = epochs[0]
        self.lr = [lr_at_epoch(oc, self.epoch) for oc in self.optim_cfgs]
        self._hyper_epoch = None
        if getattr(self, "_found_inf", None) is not None:       # the skip counts are the resumed run's own
            self._found_inf.zero_()
        eng.text_f_version = -1
