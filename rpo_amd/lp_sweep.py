"""``LPSweep``: the points of a linear-probe sweep as the members of ONE step.

The linear probe (rpo_amd/lp.py) trains one e x e layer plus bias behind a frozen image feature; its initialisation is the
identity and needs no seed.  What varies between LP runs is the OPTIM block -- learning rate, weight decay, kind, schedule
-- and more than 95 % of a step is an image pass that depends on nothing LP trains.  So S optimiser settings on the same
data order share everything up to the image feature: ONE plain image pass per step, S layers behind it in the launches of
one (rpo_lp_head_fwd_bwd_grouped: the member is a grid dimension), one optimiser launch over the S rows
(rpo_amd/optim.py: rates and step counters are device data, so the step's HIP graph is captured once), and one fused launch
that evaluates all S classifiers on cached image features (features.lp_compose + classify_many).

Member s ends every step where a standalone ``LP(optim=that member's)`` on the same batches ends it, bit for bit, and its
checkpoint is the file that standalone run writes and reads.  The members see the SAME batches (one set, one generator);
per-member training accuracy is not reported (`_reports_acc` is False: the loop would need one evaluator launch per
member per step for a number the sweep is not judged by -- the validation accuracy of `test_all` is).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import members as _members
from . import optim as _optim
from .config import RPOConfig
from .custom_clip import config_from_state_dict
from .loop import LoopMixin
from .lp import LP_MODEL_NAME, _check_prec, lp_optim_config
from .trainer import OptimConfig, lr_at_epoch


def _refuse_classes(what: str):
    raise NotImplementedError(f"LPSweep.{what}: evaluation on another class set (classes=...) is not built for the members of "
                              "a sweep -- the grouped head and the composed classifiers serve the class set the sweep was "
                              "built with; load the member's checkpoint into an LP (LP.load_model(directory)) and evaluate "
                              "it there with LP.class_set(tokens)")


def member_optimizer(optim_cfgs: Sequence[OptimConfig], stride: int, device, s0: Optional[torch.Tensor] = None):
    """The members' ONE optimiser: a set per member, each row [W | b] its own floats in full.  `used` = (stride, 0) per
    member makes also an all-plain-SGD sweep read its rates from the device table (rpo_sgd_step_sets), so no learning rate
    is a kernel argument of the captured step; as soon as one member is not plain SGD all go through rpo_optim_step_sets
    (`kind` [S], `hyper` [S, 8], `step` [S] on the device)."""
    used = torch.tensor([[stride, 0]] * len(optim_cfgs), dtype=torch.int32).to(device)
    return _optim.make_optimizer(optim_cfgs, stride, stride, 0, device, s0=s0, used=used)


class LPSweep(_members.MemberCheckpointMixin, _members.MemberScheduleMixin, LoopMixin):
    """S linear probes with their own optimiser configs on one frozen CLIP, advanced by one step on shared batches.

    members: per member dict(optim=OptimConfig [, weight=[e, e], bias=[e]]); the default start is the reference's identity /
    zeros.  Any kind rpo_amd/optim.py accepts, mixed freely; `max_epoch` is shared (one loop runs all members).
    `prec` / `amp` / `act_dtype` as `LP`; with amp every member has its own Inf / NaN verdict (`skipped_steps()`).
    `forward_backward` returns {"loss": [S floats]}; there is no per-member training accuracy (see the module docstring)."""

    _reports_acc = False
    captures = 0                       # HIP graphs of the step captured so far (rates are device data: one)
    _checkpoint_name = LP_MODEL_NAME   # `MemberCheckpointMixin`: per member, a standalone ``LP``'s file

    def __init__(self, state_dict: Dict[str, np.ndarray], tokenized_prompts: np.ndarray, members: Sequence[dict] = (),
                 device: str | torch.device = "cuda:0", act_dtype: torch.dtype = torch.float32, batch_size: int = 32,
                 num_batches: int = 1, use_graph: bool = False, amp: bool = False, prec: Optional[str] = None,
                 max_batch: Optional[int] = None, cfg: Optional[RPOConfig] = None, world_size: int = 1):
        # ---- refusals, before any device is touched
        _members.refuse_world_size("LPSweep", world_size, "data parallelism for the sweep is not built: the members share "
                                   "one image pass on one card")
        _check_prec(prec)
        if prec == "fp32":
            act_dtype, amp = torch.float32, False
        elif prec == "amp":
            act_dtype, amp = torch.float16, True
        members = [dict(m) for m in members]
        S = len(members)
        if S < 1:
            raise ValueError("LPSweep: no members -- pass members=[dict(optim=OptimConfig(...)), ...], one per point of the sweep")
        if S > 1024:
            raise ValueError(f"LPSweep: {S} members; the grouped head and the fused evaluation take at most 1024")
        self.optim_cfgs: List[OptimConfig] = _members.member_optim_configs("LPSweep", members, lp_optim_config)
        tokens = np.asarray(tokenized_prompts, dtype=np.int64)
        if cfg is None:
            cfg = config_from_state_dict(state_dict, 1, tokens.shape[0])
        if cfg.is_rn:
            raise NotImplementedError(f"LPSweep on a ResNet ({cfg.name}) is not implemented: the probe at embed {cfg.embed} has "
                                      "not been built for this engine (ViT backbones only)")
        if cfg.embed != cfg.d_t:
            raise ValueError(f"the reference's lp_layer is nn.Linear(d_t, d_t) applied to the image feature: it needs "
                             f"embed == d_t, this model has embed {cfg.embed}, d_t {cfg.d_t}")
        e = cfg.embed
        starts = []
        for s, m in enumerate(members):
            w = np.eye(e, dtype=np.float32) if m.get("weight") is None else np.asarray(m["weight"], dtype=np.float32)
            b = np.zeros(e, dtype=np.float32) if m.get("bias") is None else np.asarray(m["bias"], dtype=np.float32)
            if w.shape != (e, e) or b.shape != (e,):
                raise ValueError(f"LPSweep: member {s}'s weight / bias are {w.shape} / {b.shape}; lp_layer is [{e}, {e}] / [{e}]")
            starts.append(np.concatenate([w.reshape(-1), b]))
        # ---- the engine and the members' rows
        from . import engine as _engine
        self.cfg, self.n_runs, self.amp = cfg, S, bool(amp)
        self.batch_size, self.num_batches = int(batch_size), num_batches
        if max_batch is None:
            max_batch = max(self.batch_size, 100)                       # the yaml's test batch, as LP
        self.engine = eng = _engine.make_engine(cfg, state_dict, tokens, torch.device(device), act_dtype, max_batch)
        self.device = eng.dev
        self.tokenized_prompts = tokens
        self.epoch = self.batch_idx = self._steps = 0
        self.lr = [lr_at_epoch(oc, 0) for oc in self.optim_cfgs]
        self.use_graph, self._graph = use_graph, None
        self.best_results = [-float("inf")] * S
        with torch.cuda.device(self.device):
            eng.lp_sweep_setup(S)
            eng.lps_params.copy_(torch.from_numpy(np.stack(starts)))
            stride = eng.lps_stride
            self._found_inf = torch.zeros(S, 2, dtype=torch.int32, device=self.device) if self.amp else None
            self._opt = member_optimizer(self.optim_cfgs, stride, self.device, eng.lps_moms)

    # ------------------------------------------------------------------ members' state
    def _param_shapes(self, member: int = 0):
        e = self.cfg.embed
        return [(e, e), (e,)]

    def named_parameters(self, member: int):
        """(name, device tensor) of member `member`'s lp_layer, in torch.optim's parameter order (weight, bias)."""
        self._check_member(member)
        yield "weight", self.engine.lps_w[member]
        yield "bias", self.engine.lps_b[member]

    # ------------------------------------------------------------------ the step (`LoopMixin.step_async` / `run_epoch`)
    def _enqueue(self, image: torch.Tensor, label: torch.Tensor) -> None:
        eng = self.engine
        eng.lp_sweep_forward_backward(image, label)
        self._opt.step(eng.lps_params, eng.lps_grads, self._found_inf, first_step=(self._steps == 0))

    def _loop_loss(self) -> torch.Tensor:
        return self.engine.lps_loss

    def _loop_new_losses(self, nb: int) -> torch.Tensor:
        return torch.zeros(nb, self.n_runs, dtype=torch.float32, device=self.device)

    def forward_backward(self, batch) -> Dict[str, List[float]]:
        """One step of every member on ONE Dassl-style batch: {"loss": [S floats]}; update_lr() after the last batch of an
        epoch.  (No "acc": per-member training accuracy is not reported.)"""
        with torch.cuda.device(self.device):
            image, label = self.parse_batch_train(batch)
            loss = self.step_async(image, label).tolist()                # D2H sync, as LP
        self._loop_advance()
        return {"loss": [float(v) for v in loss]}

    # ------------------------------------------------------------------ the training loop
    def train(self, train_set, max_epoch: Optional[int] = None, val_set=None, val_features=None,
              directories: Optional[Sequence[str]] = None, generator: Optional[torch.Generator] = None,
              test_batch_size: int = 100, verbose: bool = True, plans=None) -> List[dict]:
        """`run_epoch` until `max_epoch` (default: the members' shared one).  After each epoch, with a validation set,
        `test_all(val_set, features=val_features)` and per member Dassl's `after_epoch` bookkeeping: a member whose
        validation accuracy beats its own best so far is saved to its directory as `model-best`.  Without a validation set
        the last epoch's models are saved.  `plans`: per epoch of this call, per batch, the images' `SamplePlan`s.
        One record per epoch: the members' mean losses, and "val_acc" [S]."""
        self._check_val_features(val_set, val_features)
        return self._train_members(
            max_epoch, lambda i: self.run_epoch(train_set, generator, None if plans is None else plans[i]),
            None if val_set is None else lambda: self.test_all(val_set, test_batch_size, val_features, verbose=False),
            directories, verbose)

    # ------------------------------------------------------------------ evaluation: all members per image pass
    @torch.no_grad()
    def classifiers(self):
        """The members' probes composed with the text features into affine classifiers on the image feature
        (features.lp_compose per member): (M [S, C, e], c [S, C], scale)."""
        from .features import lp_compose
        eng = self.engine
        with torch.cuda.device(self.device):
            got = [lp_compose(eng.lp_text_f_n, eng.lps_w[s], eng.lps_b[s], eng.logit_scale_exp) for s in range(self.n_runs)]
            return torch.stack([g[0] for g in got]), torch.stack([g[1] for g in got]), eng.logit_scale_exp

    @torch.no_grad()
    def test_all(self, image_set, batch_size: int = 100, features=None, verbose: bool = True,
                 per_class_result: bool = False, classes=None) -> List[dict]:
        """Dassl's `test()` for EVERY member: the image features of the set -- `features`, an `ImageFeatures` of this
        engine and set, or built here by ONE image pass over the set in `ImageFeatures.build`'s chunks -- classified by all
        S composed classifiers in one fused launch, one read-back.  Returns S evaluator dicts (+ "confusion_matrix")."""
        from .features import ImageFeatures, classify_many
        if classes is not None:
            _refuse_classes("test_all(classes=...)")
        image_set.check_labels(self.cfg.n_cls)
        if features is None:
            features = ImageFeatures.build(self, image_set, batch_size)
        else:
            features.check(self.engine, image_set)
        M, c, scale = self.classifiers()
        return classify_many(features, M, c, False, False, scale, verbose=verbose, per_class_result=per_class_result)

    def test(self, image_set, member: int = 0, batch_size: int = 100, verbose: bool = True, per_class_result: bool = False,
             classes=None, features=None) -> dict:
        """`test_all(...)[member]`."""
        if classes is not None:
            _refuse_classes("test(classes=...)")
        self._check_member(member)
        return self.test_all(image_set, batch_size, features, verbose, per_class_result)[member]

    @torch.no_grad()
    def model_inference(self, image: torch.Tensor, member: int = 0, classes=None) -> torch.Tensor:
        """logits [B, n_cls] of member `member` for a test batch (up to max_batch images): the grouped head in eval mode."""
        if classes is not None:
            _refuse_classes("model_inference(classes=...)")
        self._check_member(member)
        with torch.cuda.device(self.device):
            image = image.to(device=self.device, dtype=torch.float32).contiguous()
            return self.engine.lp_sweep_forward_backward(image, None)[member].clone()

    def class_set(self, tokens, chunk=None):
        _refuse_classes("class_set")

    # ------------------------------------------------------------------ checkpoints: `MemberCheckpointMixin`, LP's files
    def load_model(self, directories: Sequence[str], epoch: Optional[int] = None) -> None:
        """Reads S files written by standalone `LP` runs (or by `save_model`): the layer, the optimiser state, the epoch and
        the learning rates (what `LP.resume_model` restores; `load_model` is this trainer's name for it).  One loop runs all
        members: files of different epochs are refused, and so is a mix of files with and without optimiser state, before
        anything is applied."""
        self._resume(directories, epoch, "load_model")
