"""The linear probe (LP) on the HIP engine: the host-side mirror of `trainers/linear_prob.py` (CustomCLIP :61-95, the `LP`
trainer's build_model / forward_backward / load_model :111-225) -- the fifth trainer of the reference, the baseline of the
paper's tables that trains neither prompts nor contexts.

    text_features = normalise(encode_text("A photo of a {cls_name}"))          once (preprocess, :77-83)
    logits        = exp(logit_scale) * lp_layer(encode_image(image)) @ text_features.T      (:85-95)
    loss          = F.cross_entropy(logits, label);   only lp_layer (e x e weight + bias) is trained (:128-134)

The image feature is NOT normalised (:89 is commented out in the reference) and `lp_layer` starts as the identity
(weight = eye(512), bias = 0, :71-72).  The frozen towers are the plain ones ZeroshotCLIP and CoOp use; the head, its
gradient and the SGD step are rpo_lp_head_fwd_bwd + rpo_sgd_step on ONE flat [W | b] buffer (engine_lp.LpEngineMixin).

The caller provides the token ids of the "A photo of a {cls_name}" prompts (train.py:115's default for
TRAINER.LP.PROMPT: no trailing period, class names as given); the BPE tokenizer is out of scope.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np
import torch

from . import optim as _optim
from .config import RPOConfig
from .custom_clip import config_from_state_dict
from .dist import GradSync
from .engine import make_engine
from .loop import LoopMixin
from .trainer import OptimConfig, load_checkpoint_file, lr_at_epoch, write_checkpoint

LP_PROMPT = "A photo of a {cls_name}"            # train.py:115 (cfg.TRAINER.LP.PROMPT)
LP_MODEL_NAME = "lp_layer"                       # register_model("lp_layer", ...) (:143): the checkpoint sub-directory


def lp_optim_config() -> OptimConfig:
    """configs/trainers/LP/vit_b16_c4_ep10_batch1_ctxv1.yaml: SGD, LR 5e-4, 30 epochs, cosine, one constant warm-up epoch
    at 1e-5 (batch 32, test batch 100, PREC fp32); momentum / weight decay are Dassl's defaults."""
    return OptimConfig(lr=5e-4, max_epoch=30, lr_scheduler="cosine", warmup_epoch=1, warmup_type="constant",
                       warmup_cons_lr=1e-5)


def _check_prec(prec: Optional[str]) -> None:
    if prec is None or prec in ("fp32", "amp"):
        return
    if prec == "fp16":
        raise ValueError("LP with PREC fp16 is not supported: the reference keeps lp_layer in fp32 while CLIP's features are "
                         "fp16 (build_model skips clip_model.float() for fp16, trainers/linear_prob.py:117-119), so its "
                         "forward fails with a dtype error at :91.  Use prec='fp32' or 'amp', or act_dtype=torch.bfloat16 "
                         "for the 16-bit speed mode.")
    raise ValueError(f"prec must be 'fp32', 'amp' or 'fp16' (check_cfg, :108-109), not {prec!r}")


class LPCustomCLIP:
    """`trainers/linear_prob.py:CustomCLIP`: `model(image)` -> logits [B, n_cls] (fp32, on the device).  `weight` [e, e]
    (out x in) and `bias` [e] default to the reference's eye / zeros."""

    def __init__(self, state_dict: Dict[str, np.ndarray], tokenized_prompts: np.ndarray,
                 device: str | torch.device = "cuda:0", act_dtype: torch.dtype = torch.float32, max_batch: int = 100,
                 weight: Optional[np.ndarray] = None, bias: Optional[np.ndarray] = None, cfg: Optional[RPOConfig] = None):
        tokens = np.asarray(tokenized_prompts, dtype=np.int64)
        if cfg is None:
            cfg = config_from_state_dict(state_dict, 1, tokens.shape[0])     # one (unused) prompt row per image
        if cfg.is_rn:
            raise NotImplementedError(f"LP on a ResNet ({cfg.name}) is not implemented: the probe at embed {cfg.embed} has not "
                                      f"been built for this engine (ViT backbones only)")
        if cfg.embed != cfg.d_t:
            raise ValueError(f"the reference's lp_layer is nn.Linear(d_t, d_t) applied to the image feature (:69-72): it "
                             f"needs embed == d_t, this model has embed {cfg.embed}, d_t {cfg.d_t}")
        self.cfg = cfg
        self.engine = eng = make_engine(cfg, state_dict, tokens, torch.device(device), act_dtype, max_batch)
        e = cfg.embed
        with torch.cuda.device(eng.dev):
            eng.lp_setup()
            w = np.eye(e, dtype=np.float32) if weight is None else np.asarray(weight, dtype=np.float32)
            b = np.zeros(e, dtype=np.float32) if bias is None else np.asarray(bias, dtype=np.float32)
            assert w.shape == (e, e) and b.shape == (e,), "weight [e, e], bias [e]"
            eng.lp_w.copy_(torch.from_numpy(np.ascontiguousarray(w)))
            eng.lp_b.copy_(torch.from_numpy(np.ascontiguousarray(b)))
        self.tokenized_prompts = tokens

    @property
    def text_features(self) -> torch.Tensor:
        """The normalised text features the reference registers as a buffer (:83), [n_cls, e] fp32."""
        return self.engine.lp_text_f_n

    def named_parameters(self):
        """(name, device tensor) of lp_layer, in torch.optim.SGD's parameter order (nn.Linear: weight, bias)."""
        yield "weight", self.engine.lp_w
        yield "bias", self.engine.lp_b

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {n: t.detach().cpu().clone() for n, t in self.named_parameters()}

    def __call__(self, image: torch.Tensor) -> torch.Tensor:
        eng = self.engine
        with torch.cuda.device(eng.dev):
            image = image.to(device=eng.dev, dtype=torch.float32).contiguous()
            return eng.lp_forward_backward(image, None)


class LP(LoopMixin):
    """The trainer (trainers/linear_prob.py:111-225): forward -> cross-entropy -> backward -> SGD step on lp_layer, returning
    {"loss", "acc"}; per-epoch LR update.  `prec` as TRAINER.LP.PREC: "fp32" = the f32 engine, "amp" = f16 storage plus
    the skip of a step whose gradient holds Inf / NaN (what is left of GradScaler when the gradients are fp32, as
    `CoOp(amp=True)`), "fp16" raises (the reference itself cannot run it).  Without `prec`, `act_dtype` and `amp` choose;
    bf16 is the explicit speed mode.  Data parallel: one sum all-reduce of the flat [W | b] gradient through `sync`
    (GradSync), grad_scale 1 / world_size in the SGD step."""

    _reports_acc = True              # forward_backward reports "acc": run_epoch sums it on the device

    def __init__(self, state_dict: Dict[str, np.ndarray], tokenized_prompts: np.ndarray, optim: Optional[OptimConfig] = None,
                 device: str | torch.device = "cuda:0", act_dtype: torch.dtype = torch.float32, batch_size: int = 32,
                 num_batches: int = 1, use_graph: bool = False, amp: bool = False, prec: Optional[str] = None,
                 weight: Optional[np.ndarray] = None, bias: Optional[np.ndarray] = None, max_batch: Optional[int] = None,
                 sync: Optional[GradSync] = None, cfg: Optional[RPOConfig] = None):
        _check_prec(prec)                                               # (before anything touches a device)
        if prec == "fp32":
            act_dtype, amp = torch.float32, False
        elif prec == "amp":
            act_dtype, amp = torch.float16, True
        self.optim_cfg = optim or lp_optim_config()
        self.sync = sync or GradSync()
        if max_batch is None:
            max_batch = max(batch_size, 100)                            # the yaml's test batch (DATALOADER.TEST.BATCH_SIZE)
        self.model = LPCustomCLIP(state_dict, tokenized_prompts, device, act_dtype, max_batch, weight, bias, cfg)
        self.engine, self.cfg = self.model.engine, self.model.cfg
        self.device = self.engine.dev
        self.batch_size, self.num_batches = batch_size, num_batches
        self.epoch = self.batch_idx = self._steps = 0
        self.lr = lr_at_epoch(self.optim_cfg, 0)
        # (a gloo / RCCL collective between the head and the SGD step is issued eagerly: the step is captured only
        #  without data parallelism)
        self.use_graph = use_graph and not self.sync.enabled
        self._graph = None                               # (HIP graph of one step, the learning rate it was captured with)
        self.amp = amp
        self._found_inf = torch.zeros(2, dtype=torch.int32, device=self.device) if amp else None
        self.best_result = -float("inf")
        n = self.engine.lp_params.numel()                # the flat [W | b] buffer as one set
        with torch.cuda.device(self.device):
            self._opt = _optim.make_optimizer([self.optim_cfg], n, n, 0, self.device, s0=self.engine.lp_moms,
                                              grad_scale=self.sync.grad_scale)
        if self.sync.enabled:                            # identical layer on every rank
            with torch.cuda.device(self.device):
                self.sync.broadcast(self.engine.lp_params)

    def _enqueue(self, image: torch.Tensor, label: torch.Tensor) -> None:
        eng = self.engine
        eng.lp_forward_backward(image, label)
        if self.sync.enabled:
            self.sync.all_reduce_sum(eng.lp_grads)
        self._opt.step(eng.lp_params, eng.lp_grads, self._found_inf, first_step=(self._steps == 0))

    def _param_shapes(self):
        return [tuple(t.shape) for _, t in self.model.named_parameters()]

    @property
    def skipped_steps(self) -> int:
        """amp: steps GradScaler would have skipped so far (a device read)."""
        return int(self._found_inf[1].item()) if self.amp else 0

    def forward_backward(self, batch) -> Dict[str, float]:
        """trainers/linear_prob.py:151-184: {"loss", "acc"}; update_lr() after the last batch of an epoch."""
        eng = self.engine
        with torch.cuda.device(self.device):
            image, label = self.parse_batch_train(batch)
            self.step_async(image, label)
            logits = eng.logits[:image.shape[0]]
            acc = float((logits.argmax(1) == label).float().mean().item()) * 100.0      # compute_accuracy()[0]
            summary = {"loss": float(eng.loss.item()), "acc": acc}
        self._loop_advance()
        return summary

    @torch.no_grad()
    def model_inference(self, image: torch.Tensor, classes=None) -> torch.Tensor:
        """logits [B, n_cls] for a test batch (up to max_batch images: the yaml's 100); `classes`: a `ClassSet`
        (`class_set(tokens)`) -- logits [B, n'] against it."""
        if classes is None:
            return self.model(image)
        with torch.cuda.device(self.device):
            image = image.to(device=self.device, dtype=torch.float32).contiguous()
            return self._class_logits(image, classes).clone()

    @torch.no_grad()
    def classifier(self, classes=None):
        """lp_layer and the normalised text features (the trained classes', or a `ClassSet`'s) composed into ONE affine
        classifier on the un-normalised image feature (features.lp_compose): norms off, bias = scale T b."""
        from .features import lp_compose
        eng = self.engine
        with torch.cuda.device(self.device):
            if classes is None:
                T = eng.lp_text_f_n
            else:
                f = eng._cs_plain_current(eng._cs_check(classes))
                T = f / f.norm(dim=-1, keepdim=True)                                  # as Engine._cs_lp_forward
            M, c = lp_compose(T, eng.lp_w, eng.lp_b, eng.logit_scale_exp)
        return M, c, False, False, eng.logit_scale_exp

    def _class_logits(self, image: torch.Tensor, classes) -> torch.Tensor:
        """lp_layer on the image feature, then the class set's normalised text features (Engine._cs_lp_forward)."""
        return self.engine._cs_lp_forward(image, classes)

    # -- checkpoints in Dassl's layout (the reader: trainers/linear_prob.py:193-225) ----------------------------------------
    def checkpoint_dict(self, epoch: Optional[int] = None, val_result: Optional[float] = None) -> dict:
        """The dict Dassl's save_checkpoint pickles: `state_dict` (lp_layer's weight, bias), `epoch`, `optimizer`
        (the torch optimiser's own state-dict layout, param 0 = weight, 1 = bias), `scheduler`, `val_result`."""
        epoch = self.epoch if epoch is None else epoch
        optimizer = self._opt.state_dict(self._param_shapes(), lr=self.lr, steps=self._steps)
        return {"state_dict": self.model.state_dict(), "epoch": int(epoch),
                "optimizer": optimizer, "scheduler": {"last_epoch": int(epoch)},
                "val_result": val_result, "steps": int(self._steps)}

    def save_model(self, directory: str, epoch: Optional[int] = None, is_best: bool = False,
                   val_result: Optional[float] = None) -> str:
        """`<directory>/lp_layer/model.pth.tar-<epoch>` (+ `model-best.pth.tar`)."""
        ck = self.checkpoint_dict(epoch, val_result)
        return write_checkpoint(directory, ck, ck["epoch"], is_best, name=LP_MODEL_NAME)

    def load_model(self, directory: str, epoch: Optional[int] = None) -> Optional[dict]:
        """trainers/linear_prob.py:193-225: `model-best.pth.tar` unless an epoch is named; load_state_dict(strict=False)
        -- weights only: optimiser state, epoch and learning rate stay what they were (resuming is `resume_model`).
        Returns the checkpoint dict it read (None where the reference skips: no directory)."""
        if not directory:
            print("Note that load_model() is skipped as no pretrained model is given")
            return None
        model_file = "model-best.pth.tar" if epoch is None else f"model.pth.tar-{epoch}"
        model_path = os.path.join(directory, LP_MODEL_NAME, model_file)
        if not os.path.exists(model_path):
            raise FileNotFoundError(f'Model not found at "{model_path}"')
        ck = load_checkpoint_file(model_path)
        sd = dict(ck["state_dict"])
        for k in ("token_prefix", "token_suffix"):
            sd.pop(k, None)
        params = list(self.model.named_parameters())
        for name, p in params:                  # strict=False still refuses a tensor of another shape
            if name in sd and tuple(torch.as_tensor(sd[name]).shape) != tuple(p.shape):
                raise ValueError(f"{model_path}: {name} has shape {tuple(torch.as_tensor(sd[name]).shape)}, lp_layer "
                                 f"{tuple(p.shape)}")
        print(f'Loading weights to {LP_MODEL_NAME} from "{model_path}" (epoch = {ck["epoch"]})')
        with torch.no_grad():
            for name, p in params:
                if name in sd:
                    p.copy_(torch.as_tensor(sd[name]).to(p.dtype))
        self._graph = None
        return ck

    def resume_model(self, directory: str, epoch: Optional[int] = None) -> int:
        """Dassl's `resume_model_if_exist` for this trainer: `load_model` plus the momentum buffers, the epoch and the
        learning rate of the checkpoint.  Returns the epoch to continue from.  A checkpoint whose tensors do not have the
        layer's shapes is refused rather than half-applied."""
        ck = self.load_model(directory, epoch)
        if ck is None:
            raise ValueError("resume_model needs a checkpoint directory (load_model skipped: nothing was loaded)")
        params = list(self.model.named_parameters())
        sd = ck["state_dict"]
        if any(n not in sd for n, _ in params):
            raise ValueError("checkpoint lacks lp_layer's weight / bias: it was written by another trainer")
        opt_state = ck.get("optimizer")
        if (opt_state or {}).get("state"):                       # (a file with no state at all: epoch and rate only)
            if not self._opt.load_state_dict(opt_state, self._param_shapes(), steps=ck.get("steps", 1)):
                if not self._opt.table_driven:
                    for (name, p), sh in zip(params, _optim.state_shapes(self.optim_cfg, opt_state)):
                        if sh != tuple(p.shape):
                            raise ValueError(f"checkpoint momentum of {name} has shape {sh}, lp_layer {tuple(p.shape)}")
                raise ValueError(f"the checkpoint's optimiser state is not {self.optim_cfg.name}'s for lp_layer's shapes")
            self._steps = max(1, int(ck.get("steps", 1)))
        self.epoch = int(ck.get("epoch", 0))
        self.lr = lr_at_epoch(self.optim_cfg, self.epoch)
        self._graph = None
        return self.epoch
