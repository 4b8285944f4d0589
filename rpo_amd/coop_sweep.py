"""``CoOpSweep``: the points of a CoOp sweep -- seeds, optimiser settings and context LENGTHS -- as the members of ONE step
on one shared image pass (rpo_amd/engine_coop_sweep.py).

The reference sweeps CoOp harder than any other trainer: scripts/coop/main.sh runs every dataset x shots x seed cell once
per NCTX (4 / 16), CSC and CTP, all through the same frozen towers.  For CoOp, as for the linear probe, the image feature
depends on nothing that is trained, so S members on the same batches need ONE plain image pass per step; for the text pass
a member is a replica of the class set with its own context (`coop_setup(replicas=S)`), behind it one grouped head call,
one text backward and one optimiser launch over the S rows (rates and step counters are device data: the step's HIP graph
is captured once).  A member may have its OWN n_ctx <= the trainer's: its prompts are the trainer's with the surplus
placeholders removed (`member_tokens`), built and reduced on the device by rpo_amd/csrc/coop_sets.hip.

Member s ends a step where a standalone ``CoOp(n_ctx=n_s)`` on `member_tokens(tokens, n_max, n_s)` with its context, config
and the same batches ends it -- the summation orders are the standalone run's; only the GEMM plans are those of the larger
row counts (S = 1 at n_s = n_max: bit for bit) -- and its checkpoint is the file that standalone run writes and reads.  The
members see the SAME batches (one set, one generator); per-member training accuracy is not reported (`_reports_acc`).
Generic contexts in front of the class name only.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import members as _members
from . import optim as _optim
from .config import RPOConfig
from .coop import _init_ctx
from .custom_clip import config_from_state_dict
from .engine_coop_sweep import MAX_MEMBERS, sweep_used
from .loop import LoopMixin
from .trainer import OptimConfig, lr_at_epoch

MEMBER_KEYS = {"seed", "ctx", "ctx_init", "n_ctx", "optim", "csc", "class_token_position"}


def default_optim() -> OptimConfig:
    return OptimConfig(lr=0.002, max_epoch=50)           # configs/trainers/CoOp/vit_b16_ep50.yaml, as ``CoOp``


def member_tokens(tokens: np.ndarray, n_max: int, n_s: int) -> np.ndarray:
    """The "X X .. name." prompts of n_s placeholders from those of n_max: the n_max - n_s surplus placeholders (positions
    1 + n_s .. n_max) removed, everything behind them moved up, zeros at the end.  Equals `synth.coop_tokens(base, n_s)`
    wherever `tokens == synth.coop_tokens(base, n_max)`; the prompt lengths shrink by n_max - n_s."""
    tokens = np.asarray(tokens, dtype=np.int64)
    n_max, n_s = int(n_max), int(n_s)
    if not 1 <= n_s <= n_max:
        raise ValueError(f"member_tokens: n_ctx = {n_s} of a member must be in 1 .. {n_max} (the trainer's n_ctx)")
    out = np.zeros_like(tokens)
    out[:, :1 + n_s] = tokens[:, :1 + n_s]
    out[:, 1 + n_s:tokens.shape[1] - (n_max - n_s)] = tokens[:, 1 + n_max:]
    return out


def _refuse_classes(what: str):
    raise NotImplementedError(f"CoOpSweep.{what}: evaluation on another class set (classes=...) is not built for the members "
                              "of a sweep -- the replicas of the text pass serve the class set the sweep was built with; "
                              "load the member's checkpoint into a CoOp (CoOp(n_ctx=n_s).load_model(directory)) and "
                              "evaluate it there with CoOp.class_set(tokens)")


def check_members(members: Sequence[dict], n_max: int) -> List[dict]:
    """The members as dicts with exactly one of `seed` (+ `ctx_init`) or `ctx`, their `n_ctx` (default n_max) filled in."""
    out = []
    for s, m in enumerate(members):
        m = dict(m)
        _members.check_member_dict("CoOpSweep", s, m, MEMBER_KEYS, ("ctx",), "ctx=[n_ctx, d_t]")
        if m.get("csc") or m.get("class_token_position", "end") != "end":
            raise ValueError(f"CoOpSweep: member {s} asks for csc={m.get('csc', False)!r}, class_token_position="
                             f"{m.get('class_token_position', 'end')!r}: the members of a sweep have a generic context at "
                             "the front of the name only (csc=False, class_token_position='end'); run the other settings "
                             "as standalone CoOp trainers")
        ns = n_max if m.get("n_ctx") is None else int(m["n_ctx"])
        if not 1 <= ns <= n_max:
            raise ValueError(f"CoOpSweep: member {s} has n_ctx = {ns}; a member's n_ctx must be in 1 .. {n_max} (the trainer's "
                             "n_ctx, whose placeholders the tokenized prompts carry)")
        m["n_ctx"] = ns
        out.append(m)
    return out


def member_start(m: dict, cfg: RPOConfig, n_cls: int, token_embedding) -> np.ndarray:
    """Member m's context [n_s, d_t]: given, or what ``CoOp(n_ctx=n_s)`` draws under ``torch.manual_seed(seed)``
    (`_init_ctx`: N(0, 0.02), or the CTX_INIT words, which draw nothing)."""
    ns = m["n_ctx"]
    if m.get("seed") is not None:
        torch.manual_seed(int(m["seed"]))
        ctx = _init_ctx(cfg, n_cls, ns, False, None, m.get("ctx_init"), token_embedding)
    else:
        ctx = np.asarray(m["ctx"], dtype=np.float32)
    if ctx.shape != (ns, cfg.d_t):
        raise ValueError(f"CoOpSweep: a member's ctx has shape {ctx.shape}, its n_ctx = {ns} needs {(ns, cfg.d_t)}")
    return np.ascontiguousarray(ctx, dtype=np.float32)


class CoOpSweep(_members.MemberCheckpointMixin, _members.MemberScheduleMixin, LoopMixin):
    """S CoOp runs on one frozen CLIP, advanced by one step on shared batches.

    members: per member dict(seed=int [, ctx_init=...]) or dict(ctx=[n_s, d_t]), each with an optional n_ctx=n_s (1 .. the
    trainer's `n_ctx`, the default) and optim=OptimConfig (default: the reference's yaml).  Kinds may differ; `max_epoch`
    is shared (one loop runs all members).  `tokenized_prompts`: the prompts with `n_ctx` placeholders.  `shared_prefix`:
    the shared-prefix text rows (every member at `n_ctx` only).  `amp`: every member has its own Inf / NaN verdict
    (`skipped_steps()`).  `forward_backward` returns {"loss": [S floats]}."""

    _reports_acc = False
    captures = 0                       # HIP graphs of the step captured so far (rates are device data: one)

    def __init__(self, state_dict: Dict[str, np.ndarray], tokenized_prompts: np.ndarray, members: Sequence[dict] = (),
                 n_ctx: int = 16, device: str | torch.device = "cuda:0", act_dtype: torch.dtype = torch.float16,
                 batch_size: int = 32, num_batches: int = 1, use_graph: bool = False, amp: bool = False,
                 shared_prefix: bool = False, cfg: Optional[RPOConfig] = None, max_batch: Optional[int] = None,
                 world_size: int = 1, csc: bool = False, class_token_position: str = "end", classes=None, class_set=None):
        # ---- refusals, before any device is touched
        _members.refuse_world_size("CoOpSweep", world_size, "data parallelism for the sweep is not built: the members share "
                                   "one image pass on one card")
        if classes is not None or class_set is not None:
            _refuse_classes("__init__(classes=... / class_set=...)")
        if csc or class_token_position != "end":
            raise ValueError(f"CoOpSweep: csc={csc!r}, class_token_position={class_token_position!r}: the members of a sweep "
                             "have a generic context at the front of the name only (csc=False, class_token_position='end'); "
                             "run the other settings as standalone CoOp trainers")
        S, n_max = len(members), int(n_ctx)
        if S < 1:
            raise ValueError("CoOpSweep: no members -- pass members=[dict(seed=1), dict(seed=2, n_ctx=4), ...], one per run")
        if S > MAX_MEMBERS:
            raise ValueError(f"CoOpSweep: {S} members; the text pass takes at most {MAX_MEMBERS} replicas (DESIGN.md "
                             "section 9p)")
        if n_max < 1:
            raise ValueError(f"CoOpSweep: n_ctx = {n_ctx}: must be >= 1")
        members = check_members(members, n_max)
        self.n_ctx_members: List[int] = [m["n_ctx"] for m in members]
        if shared_prefix and any(v != n_max for v in self.n_ctx_members):
            raise ValueError(f"CoOpSweep: shared_prefix=True with members of different n_ctx {self.n_ctx_members}: the prefix "
                             "length P = 1 + n_ctx is per pass, so the shared-prefix rows serve members of the trainer's "
                             f"n_ctx = {n_max} only; use the dense rows (shared_prefix=False) for a mix")
        self.optim_cfgs: List[OptimConfig] = _members.member_optim_configs("CoOpSweep", members, default_optim)
        tokens = np.asarray(tokenized_prompts, dtype=np.int64)
        if cfg is None:
            cfg = config_from_state_dict(state_dict, 1, tokens.shape[0])
        # ---- the members' starting contexts (host; a seed draws from torch's global generator as ``CoOp`` does)
        emb = state_dict["token_embedding.weight"]
        starts = [member_start(m, cfg, tokens.shape[0], emb) for m in members]
        # ---- the engine and the members' rows
        from . import engine as _engine
        self.cfg, self.n_runs, self.amp, self.n_ctx = cfg, S, bool(amp), n_max
        self.batch_size, self.num_batches = int(batch_size), num_batches
        if max_batch is None:
            max_batch = max(self.batch_size, S)                          # (coop_setup takes at most max_batch replicas)
        if max_batch < max(self.batch_size, S):
            raise ValueError(f"CoOpSweep: max_batch = {max_batch} is below max(batch_size, S) = {max(self.batch_size, S)}")
        self.engine = eng = _engine.make_engine(cfg, state_dict, tokens, torch.device(device), act_dtype, max_batch)
        self.device = eng.dev
        self.tokenized_prompts = tokens
        self._token_embedding = emb
        self.epoch = self.batch_idx = self._steps = 0
        self.lr = [lr_at_epoch(oc, 0) for oc in self.optim_cfgs]
        self.use_graph, self._graph = use_graph, None
        self.best_results = [-float("inf")] * S
        dt = cfg.d_t
        with torch.cuda.device(self.device):
            eng.coop_sweep_setup(S, self.n_ctx_members, shared_prefix, max_batch)
            rows = np.zeros((S, eng.cs_stride), dtype=np.float32)
            for s, c in enumerate(starts):
                rows[s, :c.size] = c.reshape(-1)
            eng.cs_params.copy_(torch.from_numpy(rows))
            self._found_inf = torch.zeros(S, 2, dtype=torch.int32, device=self.device) if self.amp else None
            # one optimiser over the S rows; `used`: member s updates its own n_s * d_t floats (and an all-plain-SGD sweep
            # reads its rates from the device table)
            used = torch.from_numpy(sweep_used(self.n_ctx_members, dt)).to(self.device)
            self._opt = _optim.make_optimizer(self.optim_cfgs, eng.cs_stride, n_max * dt, 0, self.device, s0=eng.cs_moms,
                                              used=used)

    # ------------------------------------------------------------------ members' state
    def _param_shapes(self, member: int):
        return [(self.n_ctx_members[member], self.cfg.d_t)]

    def named_parameters(self, member: int):
        """(name, device tensor) of member `member`'s trained tensor: ctx [n_s, d_t], a view of its row."""
        self._check_member(member)
        yield "ctx", self.engine.coop_sweep_member_ctx(member)

    def member_tokens(self, member: int) -> np.ndarray:
        """The tokenized prompts a standalone ``CoOp(n_ctx=n_s)`` of member `member` is built with."""
        self._check_member(member)
        return member_tokens(self.tokenized_prompts, self.n_ctx, self.n_ctx_members[member])

    # ------------------------------------------------------------------ the step (`LoopMixin.step_async` / `run_epoch`)
    def _enqueue(self, image: torch.Tensor, label: torch.Tensor) -> None:
        eng = self.engine
        eng.coop_sweep_forward_backward(image, label)
        self._opt.step(eng.cs_params, eng.cs_grads, self._found_inf, first_step=(self._steps == 0))

    def _loop_loss(self) -> torch.Tensor:
        return self.engine.cs_loss

    def _loop_new_losses(self, nb: int) -> torch.Tensor:
        return torch.zeros(nb, self.n_runs, dtype=torch.float32, device=self.device)

    def forward_backward(self, batch) -> Dict[str, List[float]]:
        """One step of every member on ONE Dassl-style batch: {"loss": [S floats]}; update_lr() after the last batch of an
        epoch.  (No "acc": per-member training accuracy is not reported.)"""
        with torch.cuda.device(self.device):
            image, label = self.parse_batch_train(batch)
            loss = self.step_async(image, label).tolist()                # D2H sync, as CoOp
        self._loop_advance()
        return {"loss": [float(v) for v in loss]}

    # ------------------------------------------------------------------ the training loop
    def train(self, train_set, max_epoch: Optional[int] = None, val_set=None, val_features=None,
              directories: Optional[Sequence[str]] = None, generator: Optional[torch.Generator] = None,
              test_batch_size: int = 100, verbose: bool = True, plans=None) -> List[dict]:
        """`run_epoch` until `max_epoch` (default: the members' shared one).  After each epoch, with a validation set,
        `test_all(val_set, features=val_features)` and per member Dassl's `after_epoch` bookkeeping: a member whose
        validation accuracy beats its own best so far is saved to its directory as `model-best`.  Without a validation set
        the last epoch's models are saved.  One record per epoch: the members' mean losses, and "val_acc" [S]."""
        self._check_val_features(val_set, val_features)
        return self._train_members(
            max_epoch, lambda i: self.run_epoch(train_set, generator, None if plans is None else plans[i]),
            None if val_set is None else lambda: self.test_all(val_set, test_batch_size, val_features, verbose=False),
            directories, verbose)

    # ------------------------------------------------------------------ evaluation: all members per image pass
    @torch.no_grad()
    def model_inference_all(self, image: torch.Tensor) -> torch.Tensor:
        """logits [S, B, n_cls] of every member for any number of images: one image pass per chunk of max_batch images and
        one text pass over the S replicas each (cloned)."""
        eng = self.engine
        with torch.cuda.device(self.device):
            image = image.to(device=self.device, dtype=torch.float32).contiguous()
            B, R = image.shape[0], eng.cs_B
            if B <= R:
                return eng.coop_sweep_forward_backward(image, None).clone()
            out = torch.empty(self.n_runs, B, self.cfg.n_cls, dtype=torch.float32, device=self.device)
            for b0 in range(0, B, R):
                out[:, b0:b0 + R].copy_(eng.coop_sweep_forward_backward(image[b0:b0 + R], None))
            return out

    @torch.no_grad()
    def model_inference(self, image: torch.Tensor, member: int = 0, classes=None) -> torch.Tensor:
        """logits [B, n_cls] of member `member`: `model_inference_all(image)[member]`."""
        if classes is not None:
            _refuse_classes("model_inference(classes=...)")
        self._check_member(member)
        return self.model_inference_all(image)[member]

    @torch.no_grad()
    def text_features(self) -> torch.Tensor:
        """The members' text features [S, n_cls, e] (un-normalised, cloned): ONE eval text pass over the S replicas."""
        with torch.cuda.device(self.device):
            return self.engine.coop_sweep_text_features().clone()

    @torch.no_grad()
    def test_all(self, image_set, batch_size: int = 100, features=None, verbose: bool = True,
                 per_class_result: bool = False, classes=None) -> List[dict]:
        """Dassl's `test()` for EVERY member: one eval text pass over the S replicas -> [S, n_cls, e] cosine classifiers, and
        the image features of the set -- `features`, an `ImageFeatures` of this engine and set, or built here by ONE image
        pass over the set -- classified by all of them in one fused launch, one read-back.  Returns S evaluator dicts
        (+ "confusion_matrix")."""
        from .features import ImageFeatures, classify_many
        if classes is not None:
            _refuse_classes("test_all(classes=...)")
        image_set.check_labels(self.cfg.n_cls)
        if features is None:
            features = ImageFeatures.build(self, image_set, batch_size)
        else:
            features.check(self.engine, image_set)
        return classify_many(features, self.text_features(), None, True, True, self.engine.logit_scale_exp, verbose=verbose,
                             per_class_result=per_class_result)

    def test(self, image_set, member: int = 0, batch_size: int = 100, verbose: bool = True, per_class_result: bool = False,
             classes=None, features=None) -> dict:
        """`test_all(...)[member]`."""
        if classes is not None:
            _refuse_classes("test(classes=...)")
        self._check_member(member)
        return self.test_all(image_set, batch_size, features, verbose, per_class_result)[member]

    def class_set(self, tokens, chunk=None):
        _refuse_classes("class_set")

    # ------------------------------------------------------------------ checkpoints: `MemberCheckpointMixin`, CoOp's files
    def _checkpoint_extra(self, member: int) -> Dict[str, torch.Tensor]:
        """The token_prefix / token_suffix buffers of the prompts a standalone ``CoOp(n_ctx=n_s)`` of this member has:
        those of `member_tokens(member)`."""
        ns = self.n_ctx_members[member]
        emb = np.asarray(self._token_embedding)[self.member_tokens(member)]                 # [n_cls, 77, d_t]
        return {"token_prefix": torch.from_numpy(np.ascontiguousarray(emb[:, :1])),
                "token_suffix": torch.from_numpy(np.ascontiguousarray(emb[:, 1 + ns:]))}

    def load_model(self, directories: Sequence[str], epoch: Optional[int] = None) -> List[dict]:
        """Reads S files written by standalone ``CoOp`` runs (or by `save_model`): weights only, as ``CoOp.load_model`` --
        optimiser state, epoch and learning rates stay what they were (token_prefix / token_suffix are dropped, as
        trainers/coop.py:315-320 drops them).  Returns the checkpoint dicts."""
        got = self._read(directories, epoch)
        self._load_weights(got)
        return got

    def resume_model(self, directories: Sequence[str], epoch: Optional[int] = None) -> int:
        """``CoOp.resume_model`` for every member: `load_model` plus the optimiser state, the epoch and the learning rates
        of the checkpoints.  One loop runs all members: files of different epochs are refused, and so is a mix of files
        with and without optimiser state.  Returns the epoch to continue from."""
        return self._resume(directories, epoch, "resume_model")
