"""``CoCoOpMulti``: S independent CoCoOp runs ("members") advanced by ONE batched step (rpo_amd/engine_cocoop_multi.py,
DESIGN.md section 9r).

The reference trains CoCoOp at batch 1 (configs/trainers/CoCoOp/vit_b16_c4_ep10_batch1*.yaml): every image needs its own
text pass, and at one image per step that step is launch latency.  For the text pass a CoCoOp image is a replica of the
class set with its own context; nothing stops a replica from being the image of ANOTHER run.  So S members of b images
share one image pass over S * b images, one text pass over S * b replicas, one grouped head call, one optimiser launch and
one HIP graph.  Each member has its own context, meta-net, optimiser config of any kind rpo_amd/optim.py accepts (rates and
step counters are device data), images and labels: the seeds of one recipe (each with its own few-shot set) and the
points of a sweep (the same set given S times) alike.

Member s ends a step where a standalone ``CoCoOp`` with its tensors, batch and config ends it -- the summation orders are
the standalone run's; only the GEMM plans are those of the larger row counts -- and its checkpoint is the file that
standalone run writes and reads.  Evaluation is per member through the standalone code: ``select_member`` copies the
member's row into the engine's single-run parameters.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import members as _members
from . import optim as _optim
from .config import RPOConfig
from .coop import CoCoOp, CoCoOpCustomCLIP, CoCoOpPromptLearner, _init_ctx
from .custom_clip import config_from_state_dict
from .engine_cocoop_multi import MAX_REPLICAS
from .evaluator import Classification
from .loop import EvalMixin
from .trainer import OptimConfig, lr_at_epoch

META_KEYS = ("w1", "b1", "w2", "b2")
PARAM_NAMES = ("ctx", "meta_net.linear1.weight", "meta_net.linear1.bias", "meta_net.linear2.weight", "meta_net.linear2.bias")


def default_optim() -> OptimConfig:
    return OptimConfig(lr=0.002, max_epoch=10)           # configs/trainers/CoCoOp/vit_b16_c4_ep10_batch1.yaml


def check_members(members: Sequence[dict]) -> List[dict]:
    """The members as dicts with exactly one of `seed` or (`ctx`, `meta`) each (+ `ctx_init` next to a seed, `optim`)."""
    out = []
    for s, m in enumerate(members):
        m = dict(m)
        given = _members.check_member_dict("CoCoOpMulti", s, m, ("seed", "ctx", "meta", "ctx_init", "optim"), ("ctx", "meta"),
                                           "(ctx=..., meta=...)")
        if given and (m.get("ctx") is None or m.get("meta") is None):
            raise ValueError(f"CoCoOpMulti: member {s} gives its tensors: both ctx [n_ctx, d_t] and meta "
                             f"{{{', '.join(META_KEYS)}}} are needed")
        out.append(m)
    return out


def member_start(m: dict, cfg: RPOConfig, n_cls: int, n_ctx: int, token_embedding) -> np.ndarray:
    """Member m's flat row [ctx | w1 | b1 | w2 | b2].  A seed gives what ``CoCoOpCustomCLIP`` draws under
    ``torch.manual_seed(seed)``: the context (nn.init.normal_(std=0.02), trainers/cocoop.py:83-84 -- or the CTX_INIT words,
    which draw nothing), then nn.Linear's default initialisation of linear1 and linear2 (:93-97), in that order."""
    e, dt = cfg.embed, cfg.d_t
    h = e // 16
    if m.get("seed") is not None:
        torch.manual_seed(int(m["seed"]))
        ctx = _init_ctx(cfg, n_cls, n_ctx, False, None, m.get("ctx_init"), token_embedding)
        l1, l2 = torch.nn.Linear(e, h), torch.nn.Linear(h, dt)
        meta = dict(w1=l1.weight.detach().numpy(), b1=l1.bias.detach().numpy(),
                    w2=l2.weight.detach().numpy(), b2=l2.bias.detach().numpy())
    else:
        ctx, meta = m["ctx"], m["meta"]
    parts = [np.asarray(ctx, dtype=np.float32)] + [np.asarray(meta[k], dtype=np.float32) for k in META_KEYS]
    shapes = [(n_ctx, dt), (h, e), (h,), (dt, h), (dt,)]
    for name, p, sh in zip(("ctx",) + META_KEYS, parts, shapes):
        if p.shape != sh:
            raise ValueError(f"CoCoOpMulti: a member's {name} has shape {p.shape}, this model needs {sh}")
    return np.concatenate([p.reshape(-1) for p in parts])


class _MemberCLIP(CoCoOpCustomCLIP):
    """``CoCoOpCustomCLIP`` on an engine that exists: `model(image)` evaluates the member `select_member` loaded."""

    def __init__(self, engine, cfg: RPOConfig, n_ctx: int, token_embedding, tokens: np.ndarray):
        self.cfg, self.engine = cfg, engine
        self.prompt_learner = CoCoOpPromptLearner(engine, n_ctx, token_embedding, tokens)
        self.tokenized_prompts = tokens


class CoCoOpMulti(_members.MemberCheckpointMixin, _members.MemberScheduleMixin, _members.MemberLoopMixin,
                  EvalMixin):
    """S CoCoOp runs on one frozen CLIP, advanced by one step.

    members: per member dict(seed=int [, ctx_init=...]) or dict(ctx=[n_ctx, d_t], meta={w1, b1, w2, b2}), each with an
    optional optim=OptimConfig (default: the reference's yaml).  Kinds may differ; `max_epoch` is shared (one loop runs all
    members).  `batch_size` is the members' own batch b (the reference: 1); a step takes S * b images, member-major.
    `amp`: every member has its own Inf / NaN verdict (`skipped_steps`)."""

    _reports_acc = False
    _loop_name = "CoCoOpMulti"         # `MemberLoopMixin`: parse_batch_train, run_epoch (one resident set and generator per member)
    _features_why_not = CoCoOp._features_why_not
    captures = 0                       # HIP graphs of the step captured so far (rates are device data: one)

    def __init__(self, state_dict: Dict[str, np.ndarray], tokenized_prompts: np.ndarray, members: Sequence[dict] = (),
                 n_ctx: int = 4, batch_size: int = 1, num_batches: int = 1, act_dtype: torch.dtype = torch.float16,
                 use_graph: bool = False, amp: bool = False, shared_prefix: bool = False, cfg: Optional[RPOConfig] = None,
                 device: str | torch.device = "cuda:0", world_size: int = 1):
        # ---- refusals, before any device is touched
        _members.refuse_world_size("CoCoOpMulti", world_size, "data parallelism for this trainer is not built: the members "
                                   "fill the step that data parallelism would split")
        tokens = np.asarray(tokenized_prompts, dtype=np.int64)
        if cfg is None:
            cfg = config_from_state_dict(state_dict, 1, tokens.shape[0])
        if cfg.is_rn:
            raise NotImplementedError(f"CoCoOpMulti on a ResNet ({cfg.name}) is not implemented: CoCoOp's meta-net at vis_dim "
                                      f"{cfg.embed} has not been built for this engine (ViT backbones only)")
        S, b = len(members), int(batch_size)
        if S < 1:
            raise ValueError("CoCoOpMulti: no members -- pass members=[dict(seed=1), dict(seed=2), ...], one per run")
        if b < 1:
            raise ValueError(f"CoCoOpMulti: batch_size = {batch_size}: must be >= 1")
        if S * b > MAX_REPLICAS:
            raise ValueError(f"CoCoOpMulti: S * b = {S} * {b} = {S * b} images per step; the text pass takes at most "
                             f"{MAX_REPLICAS} replicas (rpo_metanet_fwd's limit, DESIGN.md section 9p)")
        members = check_members(members)
        self.optim_cfgs: List[OptimConfig] = _members.member_optim_configs("CoCoOpMulti", members, default_optim)
        # ---- the members' starting rows (host; a seed draws from torch's global generator as the standalone trainer does)
        emb = state_dict["token_embedding.weight"]
        starts = np.stack([member_start(m, cfg, tokens.shape[0], n_ctx, emb) for m in members])
        # ---- the engine and the members' rows
        from . import engine as _engine
        self.cfg, self.n_runs, self.amp, self.n_ctx = cfg, S, bool(amp), int(n_ctx)
        self.batch_size, self.num_batches = b, num_batches
        self.engine = eng = _engine.make_engine(cfg, state_dict, tokens, torch.device(device), act_dtype, S * b)
        self.device = eng.dev
        self.tokenized_prompts = tokens
        self.epoch = self.batch_idx = self._steps = 0
        self.lr = [lr_at_epoch(oc, 0) for oc in self.optim_cfgs]
        self.use_graph, self._graph, self._warm = use_graph, None, False
        self.best_results = [-float("inf")] * S
        self._eval_member: Optional[int] = None
        with torch.cuda.device(self.device):
            eng.cocoop_multi_setup(S, b, self.n_ctx, shared_prefix=shared_prefix)
            assert starts.shape[1] == eng.cm_len
            eng.cm_params[:, :eng.cm_len].copy_(torch.from_numpy(starts))
            self._found_inf = torch.zeros(S, 2, dtype=torch.int32, device=self.device) if self.amp else None
            # one optimiser over the S rows; `used` makes also an all-plain-SGD set read its rates from the device table
            used = torch.tensor([[eng.cm_len, 0]] * S, dtype=torch.int32).to(self.device)
            self._opt = _optim.make_optimizer(self.optim_cfgs, eng.cm_stride, eng.cm_len, 0, self.device, s0=eng.cm_moms,
                                              used=used)
            self._image = torch.zeros(S * b, 3, cfg.image_size, cfg.image_size, device=self.device)
            self._label = torch.zeros(S * b, dtype=torch.int64, device=self.device)
        self.model = _MemberCLIP(eng, cfg, self.n_ctx, emb, tokens)

    # ------------------------------------------------------------------ members' state
    def _param_shapes(self, member: int = 0):
        e, dt = self.cfg.embed, self.cfg.d_t
        h = e // 16
        return [(self.n_ctx, dt), (h, e), (h,), (dt, h), (dt,)]

    def named_parameters(self, member: int):
        """(name, device tensor) of member `member`'s trained tensors, in torch.optim's parameter order: views of its row."""
        self._check_member(member)
        views = self.engine.cocoop_member_views(member)
        for name, k in zip(PARAM_NAMES, ("ctx",) + META_KEYS):
            yield name, views[k]

    skipped_steps = property(_members.MemberScheduleMixin.skipped_steps)     # (a property here, a method on the other three)

    # ------------------------------------------------------------------ the step: `MemberLoopMixin.step_async` enqueues these
    def _forward_backward(self, image: torch.Tensor, label: torch.Tensor) -> None:
        self.engine.cocoop_multi_forward_backward(image, label)

    def _enqueue(self, image: torch.Tensor, label: torch.Tensor) -> None:
        eng = self.engine
        self._forward_backward(image, label)
        self._opt.step(eng.cm_params, eng.cm_grads, self._found_inf, first_step=(self._steps == 0))

    def _loop_loss(self) -> torch.Tensor:
        return self.engine.cm_loss

    def forward_backward(self, batches: Sequence[dict]) -> List[Dict[str, float]]:
        """trainers/cocoop.py:255-275 for every member: S batches in, S {"loss"} out (no accuracy, as ``CoCoOp``)."""
        with torch.cuda.device(self.device):
            image, label = self.parse_batch_train(batches)
            loss = self.step_async(image, label).tolist()                # D2H sync, as the reference
        self._loop_advance()
        return [{"loss": float(v)} for v in loss]

    def train(self, image_sets, max_epoch: Optional[int] = None, val_set=None, directories: Optional[Sequence[str]] = None,
              generators: Optional[Sequence[Optional[torch.Generator]]] = None, test_batch_size: int = 100,
              verbose: bool = True) -> List[dict]:
        """`run_epoch` until `max_epoch` (default: the members' shared one).  After each epoch, with a validation set,
        `test_all(val_set)` and per member Dassl's `after_epoch` bookkeeping (a member that beats its own best is saved to
        its directory as `model-best`); without one the last epoch's models are saved.  One record per epoch."""
        return self._train_members(
            max_epoch, lambda i: self.run_epoch(image_sets, generators),
            None if val_set is None else lambda: self.test_all(val_set, test_batch_size, verbose=False), directories, verbose)

    # ------------------------------------------------------------------ evaluation: the standalone path, one member
    def select_member(self, member: int) -> None:
        self._check_member(member)
        if self._eval_member != member:
            with torch.cuda.device(self.device):
                self.engine.select_member(member)
            self._eval_member = member

    @torch.no_grad()
    def model_inference(self, image: torch.Tensor, member: int = 0, classes=None) -> torch.Tensor:
        """logits [B, n_cls] of member `member` for any number of images (walked in chunks of S * b, as ``CoCoOp`` walks a
        test batch); `classes`: a `ConditionalClassSet` (`conditional_class_set(tokens)`) -- logits [B, n'] against it."""
        self.select_member(member)
        with torch.cuda.device(self.device):
            image = image.to(device=self.device, dtype=torch.float32).contiguous()
            return (self.model(image) if classes is None else self._class_logits(image, classes)).clone()

    def _class_logits(self, image: torch.Tensor, classes) -> torch.Tensor:
        return self.engine.cocoop_class_logits(image, classes)

    def _test_chunk(self, batch_size: int, classes) -> int:
        return max(1, batch_size) if classes is not None else super()._test_chunk(batch_size, classes)

    def class_set(self, tokens, chunk=None):
        raise NotImplementedError(f"CoCoOpMulti.class_set: {self._features_why_not}; use conditional_class_set(tokens)")

    def conditional_class_set(self, tokens, images_per_pass: Optional[int] = None, row_budget: Optional[int] = None):
        """``CoCoOp.conditional_class_set``: a class set for `model_inference(image, member, classes=)`, `test(set, member,
        classes=)` and `evaluator.base_to_new`; it belongs to the tokens, not to a member."""
        with torch.cuda.device(self.device):
            return self.engine.conditional_class_set(tokens, images_per_pass, row_budget)

    def test(self, image_set, member: int = 0, batch_size: int = 100, verbose: bool = True, per_class_result: bool = False,
             classes=None, features=None):
        """Dassl's `test()` for member `member` (loop.EvalMixin.test); `classes`: against that conditional class set."""
        self._refuse_features(features, "test(features=...)")
        self.select_member(member)
        return super().test(image_set, batch_size, verbose, per_class_result, classes=classes)

    @torch.no_grad()
    def test_all(self, image_set, batch_size: int = 100, verbose: bool = True, per_class_result: bool = False) -> List[dict]:
        """Dassl's `test()` for EVERY member: each chunk of the set is transformed once, then evaluated member by member
        (every member runs its own image pass: sharing it at test time is not built).  Returns, per member, the dict
        `test(image_set, member=s)` returns."""
        from . import ops
        S, n, C = self.n_runs, len(image_set), self._n_classes(image_set, None)
        chunk = self._test_chunk(batch_size, None)
        evs = [Classification(C, per_class_result) for _ in range(S)]
        with torch.cuda.device(self.device):
            tf = self._loop_transform(False, chunk)
            size = self.cfg.image_size
            buf = torch.zeros(chunk, 3, size, size, dtype=torch.float32, device=self.device)
            counts = torch.zeros(S, 2, dtype=torch.int64, device=self.device)
            cmat = torch.zeros(S, C * C, dtype=torch.int32, device=self.device)
            for b0 in range(0, n, chunk):
                B = min(chunk, n - b0)
                image = tf.from_set(image_set, range(b0, b0 + B), out=buf[:B])
                for s in range(S):
                    self.select_member(s)
                    ops.eval_accumulate(self.model(image), image_set.labels_dev[b0:b0 + B], counts[s], cmat[s])
            counts_h, cmat_h = counts.cpu().numpy(), cmat.cpu().numpy()         # the one read-back
        out = []
        for s, ev in enumerate(evs):
            ev.process_counts(counts_h[s], cmat_h[s])
            res = ev.evaluate(verbose=verbose)
            res["confusion_matrix"] = ev.cmat.copy()
            out.append(res)
        return out

    # ------------------------------------------------------------------ checkpoints: `MemberCheckpointMixin`, CoCoOp's files
    def _checkpoint_extra(self, member: int) -> Dict[str, torch.Tensor]:
        pl = self.model.prompt_learner
        return {"token_prefix": pl.token_prefix.clone(), "token_suffix": pl.token_suffix.clone()}

    def _load_weights(self, got: Sequence[dict]) -> None:
        super()._load_weights(got)                   # (token_prefix / token_suffix are dropped, as trainers/cocoop.py:304-309)
        self._eval_member = None

    def load_model(self, directories: Sequence[str], epoch: Optional[int] = None) -> List[dict]:
        """Reads S files written by standalone ``CoCoOp`` runs (or by `save_model`): weights only, as ``CoCoOp.load_model``
        -- optimiser state, epoch and learning rates stay what they were.  Returns the checkpoint dicts."""
        got = self._read(directories, epoch)
        self._load_weights(got)
        return got

    def resume_model(self, directories: Sequence[str], epoch: Optional[int] = None) -> int:
        """``CoCoOp.resume_model`` for every member: `load_model` plus the optimiser state, the epoch and the learning
        rates of the checkpoints.  One loop runs all members: files of different epochs are refused, and so is a mix of
        files with and without optimiser state.  Returns the epoch to continue from."""
        return self._resume(directories, epoch, "resume_model")
