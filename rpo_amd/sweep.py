"""``RPOSweep``: the points of a hyper-parameter sweep as the members of ONE step on the shared frozen towers -- each
member with its own K, its own optimiser settings and schedule, and (amp) its own Inf / NaN verdict.

``RPOMulti`` (rpo_amd/multi.py) advances S runs of one recipe.  The sweeps of the method vary what it holds fixed: K is the
paper's ablated hyper-parameter (the reference ships configs/trainers/RPO/main_K4.yaml, main.yaml, main_K24.yaml), the
OPTIM block is tuned per dataset, PREC amp is one of the trainer's three precisions (trainers/rpo.py:298-304).  Nothing
reads a prompt, so prompt row i of a member depends on no other prompt row: a member that uses the
first K_s of the engine's K = max K_s rows IS a standalone K_s run as soon as the head averages over K_s pairs
(rpo_head_fwd_bwd_grouped_k) and the optimiser and the checkpoint see those rows only (rpo_sgd_step_sets, the gather /
scatter below).  The other rows ("inert") are zero, get zero gradients and ride along: a member costs what a K member costs.

The optimiser settings live in a device table [S, 4] = (lr, momentum, weight decay, grad_scale) that the members' optimiser
owns (`optim.PlainSGD` with `used`, `optim.sgd_hyper_table`; [S, 8] in `optim.OptimState` as soon as one member is not plain
SGD): a new epoch's learning rates are one small copy on the step's stream, and the step's HIP graph is captured ONCE
(`captures`).

The surface is ``RPOMulti``'s, whose step, epoch loop and shared evaluation this class inherits; evaluation of one member
goes through the shared prompt-row pass with that member's K, and a member's checkpoint is the file a standalone
``RPO`` with ``cfg.K = K_s`` writes and reads.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import members as _members
from . import optim as _optim
from .custom_clip import init_prompts, refuse_rn
from .multi import _WHY_NO_DP, RPOMulti
from .trainer import OptimConfig, lr_at_epoch, write_checkpoint


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


class RPOSweep(_members.MemberScheduleMixin, RPOMulti):
    _one_counter = ""

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
        _members.refuse_world_size("RPOSweep", world_size, _WHY_NO_DP)
        _shared(members, "batch_size", B, "batch size")
        act_dtype = _shared(members, "act_dtype", act_dtype, "storage mode (act_dtype)")
        for s, m in enumerate(members):
            if (m.get("seed") is None) == (m.get("prompts") is None):
                raise ValueError(f"RPOSweep: member {s} needs exactly one of seed= or prompts=(text_prompt, img_prompt)")
            if "K" not in m or int(m["K"]) < 1:
                raise ValueError(f"RPOSweep: member {s} has K = {m.get('K')}: every member names its own K >= 1")
            m["K"] = int(m["K"])
        self.optim_cfgs = _members.member_optim_configs("RPOSweep", members, OptimConfig, "the cosine schedule counts")
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
        self._build(cfg, state_dict, tokens, S, B, sweep_prompts(state_dict, members, cfg.d_t, cfg.d_v), device, act_dtype,
                    num_batches, use_graph, member_K=self.member_K)
        with torch.cuda.device(self.device):
            self._used = used_table(self.member_K, cfg.d_t, cfg.d_v).to(self.device)
            self._found_inf = torch.zeros(S, 2, dtype=torch.int32, device=self.device) if self.amp else None
            # one set per member: rpo_sgd_step_sets, or -- a member that is not plain SGD -- rpo_optim_step_sets for every
            # member (plain-SGD members keep their momentum in m_mom and get the bits of rpo_sgd_step_sets)
            self._opt = _optim.make_optimizer(self.optim_cfgs, self.engine.m_params.stride(0), cfg.K * cfg.d_t,
                                              cfg.K * cfg.d_v, self.device, s0=self.engine.m_mom, used=self._used)

    # ------------------------------------------------------------------ members' state
    def _dims(self, s: int):
        return self.cfg.K, self.member_K[s], self.cfg.d_t, self.cfg.d_v

    def _shapes(self, s: int):
        return [(self.member_K[s], self.cfg.d_t), (self.member_K[s], self.cfg.d_v)]

    def set_prompts(self, prompts: Sequence[tuple]) -> None:
        """Member s's (text_prompt [K_s, d_t], img_prompt [K_s, d_v]) into the leading rows of its row; the inert rows zero."""
        host = torch.stack([flat_to_member_row(torch.cat([torch.from_numpy(np.asarray(tp, dtype=np.float32)).reshape(-1),
                                                          torch.from_numpy(np.asarray(ip, dtype=np.float32)).reshape(-1)]),
                                               *self._dims(s)) for s, (tp, ip) in enumerate(prompts)])
        self.engine.m_params.copy_(host)
        self.engine.text_f_version = -1
        self._eval_member = None

    # ------------------------------------------------------------------ the step: `RPOMulti`'s (the rates are device data)
    def train(self, image_sets, max_epoch: Optional[int] = None, generators=None, directories: Optional[Sequence[str]] = None,
              verbose: bool = True) -> List[dict]:
        """`run_epoch` until `max_epoch` (default: the members' shared one); the last epoch's models are saved to
        `directories`.  One record per epoch: the members' mean losses (one read per epoch)."""
        history = self._train_members(max_epoch, lambda i: self.run_epoch(image_sets, generators), verbose=verbose)
        if directories:                               # (no validation, no per-epoch save: once, also when no epoch ran)
            self.save_model(directories)
        return history

    # ------------------------------------------------------------------ evaluation of one member: the shared path, S = 1
    def _select(self, member: int) -> None:
        raise RuntimeError("RPOSweep evaluates a member through the shared prompt-row path with the member's own K "
                           "(model_inference / test); the single-run eval path averages over the engine's K")

    def class_set(self, tokens, chunk=None):
        raise NotImplementedError("RPOSweep.class_set: evaluation on another class set is not built for members with their "
                                  "own K -- a class set's text features would be averaged over the engine's K, not the "
                                  "member's K_s; train the member as an RPO / RPOMulti run, or load its checkpoint into one")

    def _member_sides(self, member: int):
        self._check_member(member)
        eng, rows = self.engine, self.cfg.n_cls * self.cfg.K
        text_f = eng.multi_text_features()[member * rows:(member + 1) * rows]
        return eng.m_img_prompt[member:member + 1], text_f, eng.m_k_used[member:member + 1]

    def _shared_sides(self, classes=None):
        if classes is not None:
            self.class_set(None)                      # (test_all(classes=...): refuses, by name and with the reason)
        eng = self.engine
        return eng.m_img_prompt, eng.multi_text_features(), eng.m_k_used

    def test_all(self, image_set, batch_size: int = 100, frozen=None, verbose: bool = True, per_class_result: bool = False,
                 hook=None, classes=None, features=None) -> List[dict]:
        self._refuse_features(features, "test_all(features=...)")
        if classes is not None:
            self.class_set(None)                      # (refuses, by name and with the reason)
        return super().test_all(image_set, batch_size, frozen, verbose, per_class_result, hook)

    @torch.no_grad()
    def model_inference(self, image: torch.Tensor, member: int = 0, classes=None) -> torch.Tensor:
        """logits [B, n_cls] of member `member`, averaged over its own K_s pairs."""
        if classes is not None:
            self.class_set(None)                      # (refuses, by name and with the reason)
        return self._sides_logits(image, lambda: self._member_sides(member))[0]

    def test(self, image_set, member: int = 0, batch_size: int = 100, verbose: bool = True, per_class_result: bool = False,
             frozen=None, classes=None, features=None):
        """Dassl's `test()` for member `member` (loop.EvalMixin._test_shared with that member alone)."""
        self._refuse_features(features, "test(features=...)")
        if classes is not None:
            self.class_set(None)                      # (refuses, by name and with the reason)
        return self._test_shared(image_set, 1, lambda: self._member_sides(member), batch_size, frozen, verbose,
                                 per_class_result)[0]

    # ------------------------------------------------------------------ checkpoints: per member, a standalone RPO(K_s)'s files
    def save_model(self, directories: Sequence[str], epoch: Optional[int] = None, is_best: bool = False,
                   val_results: Optional[Sequence[Optional[float]]] = None) -> List[str]:
        """Per member, the file a standalone `RPO(cfg.K = K_s, optim_s).save_model(directories[s])` writes: prompts
        [K_s, d], momentum in its flat order, the member's own learning rate and optimiser settings."""
        self._check_directories(directories)
        epoch = self.epoch if epoch is None else epoch
        p = self.engine.m_params.detach().cpu()
        out = []
        for s, d in enumerate(directories):
            entry = self._opt.state_dict(self._shapes(s), s=s, lr=self.lr[s], steps=self._steps,
                                         gather=lambda row: member_row_to_flat(row, *self._dims(s)))
            ck = _members.member_checkpoint(member_row_to_flat(p[s], *self._dims(s)), None, self.member_cfgs[s], epoch,
                                            self.optim_cfgs[s], self.lr[s], self._steps,
                                            None if val_results is None else val_results[s], entry)
            out.append(write_checkpoint(d, ck, epoch, is_best))
        return out

    def load_model(self, directories: Sequence[str], epoch: Optional[int] = None) -> None:
        """Reads S files written by standalone `RPO(cfg.K = K_s)` runs (or by `save_model`).  One loop runs all members:
        files of different epochs are refused."""
        self._check_directories(directories)
        got = [_members.read_member_checkpoint(d, epoch, self.member_cfgs[s]) for s, d in enumerate(directories)]
        ep = self._files_epoch([ck for _, ck in got], "load_model")
        self._load_states(got, lambda s: dict(param_shapes=self._shapes(s), s=s,
                                              scatter=lambda d, r: d.copy_(flat_to_member_row(r, *self._dims(s)))))
        eng = self.engine
        eng.m_params.copy_(torch.stack([flat_to_member_row(p, *self._dims(s)) for s, (p, _) in enumerate(got)]))
        self.epoch = ep
        self.lr = [lr_at_epoch(oc, self.epoch) for oc in self.optim_cfgs]
        self._opt.set_epoch(self.epoch)
        if self._found_inf is not None:                         # the skip counts are the resumed run's own
            self._found_inf.zero_()
        eng.text_f_version = -1
