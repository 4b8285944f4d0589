"""Dassl's optimisers beyond plain SGD on the HIP engine: the host side of rpo_optim_step_sets.

``OptimState`` owns what the kernel reads from the device -- `kind` [S], `hyper` [S, 8], `step` [S] -- and the fp32 state
rows of S sets, and offers the four operations a trainer needs: ``step``, ``set_epoch``, ``state_dict``,
``load_state_dict``.  A trainer builds one only when its config is NOT plain SGD (``is_plain_sgd``); plain SGD keeps
calling rpo_sgd_step* exactly as before.

The module-level functions are pure host code (no device): the hyper table, torch.optim's state-dict layout per kind in
both directions, and the refusals.  Dassl is not installed here: the names, the defaults and what `OPTIM.NAME` selects are
Dassl's `build_optimizer` as its source is remembered (dassl/optim/optimizer.py); the update rules are the installed
torch's.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

KINDS = {"sgd": 0, "adam": 1, "adamw": 2, "amsgrad": 3, "rmsprop": 4}       # include/rpo_amd.h RPO_OPT_*
EPS = 1e-8                                                                   # torch's default; Dassl has no knob for it


def validate(oc) -> None:
    """Refusals at construction of a trainer (before a device is touched)."""
    name = getattr(oc, "name", "sgd")
    if name == "radam":
        raise ValueError("OPTIM.NAME 'radam' is not supported: Dassl ships its own RAdam (dassl/optim/radam.py), which is "
                         "not torch.optim.RAdam, and Dassl is not available to pin an implementation against")
    if name not in KINDS:
        raise ValueError(f"OptimConfig.name = {name!r}: one of {' | '.join(KINDS)}")
    if not getattr(oc, "gamma", 0.1) >= 0.0:
        raise ValueError(f"OptimConfig.gamma = {oc.gamma}: the decay factor of single_step / multi_step must be >= 0")
    for f in ("sgd_dampening", "rmsprop_alpha", "adam_beta1", "adam_beta2"):
        v = getattr(oc, f, 0.0)
        if not 0.0 <= v <= 1.0:
            raise ValueError(f"OptimConfig.{f} = {v}: must lie in [0, 1]")
    if name == "sgd" and getattr(oc, "sgd_nesterov", False) and (oc.momentum <= 0 or oc.sgd_dampening != 0):
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")          # torch.optim.SGD's own refusal


def is_plain_sgd(oc) -> bool:
    """torch.optim.SGD with dampening 0 and no Nesterov: what rpo_sgd_step* implement."""
    return (getattr(oc, "name", "sgd") == "sgd" and getattr(oc, "sgd_dampening", 0.0) == 0.0
            and not getattr(oc, "sgd_nesterov", False))


def _lo(x: float) -> float:
    return float(x) - float(np.float32(x))


def hyper_row(oc, lr: float, grad_scale: float = 1.0) -> List[float]:
    """One row of `hyper` [8] as doubles (include/rpo_amd.h names the columns); `hyper_table` rounds it to float32."""
    name = getattr(oc, "name", "sgd")
    if name == "sgd":
        return [lr, grad_scale, oc.weight_decay, oc.momentum, oc.sgd_dampening, EPS, 1.0 if oc.sgd_nesterov else 0.0,
                _lo(oc.sgd_dampening)]
    if name == "rmsprop":
        return [lr, grad_scale, oc.weight_decay, oc.momentum, oc.rmsprop_alpha, EPS, 0.0, _lo(oc.rmsprop_alpha)]
    return [lr, grad_scale, oc.weight_decay, oc.adam_beta1, oc.adam_beta2, EPS, _lo(oc.adam_beta1), _lo(oc.adam_beta2)]


def hyper_table(optims: Sequence, epoch: int, grad_scale: float = 1.0) -> torch.Tensor:
    """float32 [S, 8] of the members' settings at `epoch` (each member's own schedule)."""
    from .trainer import lr_at_epoch
    return torch.tensor([hyper_row(oc, lr_at_epoch(oc, epoch), grad_scale) for oc in optims],
                        dtype=torch.float64).to(torch.float32)


def kind_table(optims: Sequence) -> torch.Tensor:
    return torch.tensor([KINDS[getattr(oc, "name", "sgd")] for oc in optims], dtype=torch.int32)


# ---- torch.optim's state-dict layout ------------------------------------------------------------------------------------
_ROWS = {"sgd": ("momentum_buffer",), "adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq"),
         "amsgrad": ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"), "rmsprop": ("momentum_buffer", "square_avg")}


def state_names(oc) -> tuple:
    """The per-parameter tensors of the kind, in the order of the state rows (s0, s1, s2) they are slices of."""
    return _ROWS[getattr(oc, "name", "sgd")]


def param_group(oc, lr: float, n_params: int) -> dict:
    """The one `param_groups` entry, with that torch optimiser's own keys (+ `initial_lr`, which a scheduler adds)."""
    name = getattr(oc, "name", "sgd")
    if name == "sgd":
        g = {"lr": lr, "momentum": oc.momentum, "dampening": oc.sgd_dampening if oc.sgd_dampening else 0,
             "weight_decay": oc.weight_decay, "nesterov": bool(oc.sgd_nesterov), "maximize": False, "foreach": None,
             "differentiable": False, "fused": None}
    elif name == "rmsprop":
        g = {"lr": lr, "momentum": oc.momentum, "alpha": oc.rmsprop_alpha, "eps": EPS, "centered": False,
             "weight_decay": oc.weight_decay, "capturable": False, "foreach": None, "maximize": False,
             "differentiable": False}
    else:
        g = {"lr": lr, "betas": (oc.adam_beta1, oc.adam_beta2), "eps": EPS, "weight_decay": oc.weight_decay,
             "amsgrad": name == "amsgrad", "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
             "fused": None, "decoupled_weight_decay": name == "adamw"}
    g["initial_lr"] = oc.lr
    g["params"] = list(range(n_params))
    return g


def torch_state_dict(oc, lr: float, rows: Sequence[torch.Tensor], step: int, param_shapes: Sequence[tuple]) -> dict:
    """`torch.optim.<kind>.state_dict()` of a run whose flat state rows (s0, s1, s2 as far as the kind has them; host
    tensors, the parameters back to back as in the trainer's flat buffer) are `rows` and which has applied `step` updates.
    The flat rows are sliced exactly as the SGD checkpoints slice `momentum_buffer`."""
    names = state_names(oc)
    name = getattr(oc, "name", "sgd")
    state: Dict[int, dict] = {}
    if step > 0:
        off = 0
        for i, shape in enumerate(param_shapes):
            n = int(np.prod(shape))
            st = {} if name == "sgd" else {"step": torch.tensor(float(step), dtype=torch.float32)}
            for nm, row in zip(names, rows):
                st[nm] = row[off:off + n].reshape(shape).clone()
            # torch's RMSprop keeps no momentum_buffer when momentum == 0 (the key is absent from its state dict)
            if name == "rmsprop" and not oc.momentum > 0:
                st.pop("momentum_buffer")
            if name == "rmsprop":          # torch's key order: step, square_avg, momentum_buffer
                st = {k: st[k] for k in ("step", "square_avg", "momentum_buffer") if k in st}
            state[i] = st
            off += n
    return {"state": state, "param_groups": [param_group(oc, lr, len(param_shapes))]}


def rows_from_state_dict(oc, opt_state: Optional[dict], param_shapes: Sequence[tuple]):
    """The inverse: (rows [flat fp32 host tensors in state-row order], step) or None when the file carries no state that
    matches this kind and these shapes (the caller then loads weights only)."""
    st = (opt_state or {}).get("state") or {}
    if not st:
        return None
    names = state_names(oc)
    name = getattr(oc, "name", "sgd")
    rows: List[List[torch.Tensor]] = [[] for _ in names]
    steps = []
    try:
        for i, shape in enumerate(param_shapes):
            e = st[i]
            for r, nm in zip(rows, names):
                if nm == "momentum_buffer" and name == "rmsprop" and nm not in e:
                    t = torch.zeros(tuple(shape))
                else:
                    t = torch.as_tensor(e[nm])
                if tuple(t.shape) != tuple(shape):
                    return None
                r.append(t.reshape(-1).float())
            if name != "sgd":
                steps.append(int(round(float(e["step"]))))
    except (KeyError, TypeError, IndexError):
        return None
    step = max(steps) if steps else 1
    return [torch.cat(r) for r in rows], step


class OptimState:
    """The device tables and state rows of S sets for rpo_optim_step_sets.

    optims: one config per set.  `s0` may be given (a trainer's existing momentum buffer, viewed [S, stride]): SGD sets
    then keep their momentum where the plain path keeps it.  `used` int32 [S, 2] (device) or None."""

    def __init__(self, optims: Sequence, set_stride: int, seg0: int, seg1: int, device, s0: Optional[torch.Tensor] = None,
                 used: Optional[torch.Tensor] = None, grad_scale: float = 1.0):
        for oc in optims:
            validate(oc)
        self.optims, self.S = list(optims), len(optims)
        self.stride, self.seg0, self.seg1 = int(set_stride), int(seg0), int(seg1)
        self.device, self.grad_scale, self.used = torch.device(device), float(grad_scale), used
        S, dev = self.S, self.device
        self.s0 = torch.zeros(S, self.stride, device=dev) if s0 is None else s0.view(S, self.stride)
        self.s1 = torch.zeros(S, self.stride, device=dev)
        self.needs_s2 = any(oc.name == "amsgrad" for oc in optims)
        self.s2 = torch.zeros(S, self.stride, device=dev) if self.needs_s2 else None
        self.kind = kind_table(optims).to(dev)
        self.hyper = torch.zeros(S, 8, dtype=torch.float32, device=dev)
        self.counter = torch.zeros(S, dtype=torch.int32, device=dev)
        self.epoch = None
        self.set_epoch(0)

    def set_epoch(self, epoch: int) -> None:
        """The rates of `epoch` into the device table: one small H2D copy on the current stream (nothing when the table
        already holds that epoch)."""
        if self.epoch != epoch:
            self.hyper.copy_(hyper_table(self.optims, epoch, self.grad_scale))
            self.epoch = epoch

    def step(self, p: torch.Tensor, g: torch.Tensor, found_inf: Optional[torch.Tensor] = None) -> None:
        from . import ops
        S = self.S
        ops.optim_step_sets(p.view(S, self.stride), g.view(S, self.stride), self.s0, self.s1, self.s2, self.kind, self.hyper,
                            self.counter, self.seg0, self.seg1, used=self.used,
                            found_inf=None if found_inf is None else found_inf.view(S, 2), needs_s2=self.needs_s2)

    def _rows(self, s: int):
        return [r[s].detach().cpu() for r in (self.s0, self.s1, self.s2)[:len(state_names(self.optims[s]))]]

    def steps(self) -> List[int]:
        """Per set, the number of updates applied so far (one D2H read)."""
        return [int(v) for v in self.counter.tolist()]

    def state_dict(self, param_shapes: Sequence[tuple], s: int = 0, lr: Optional[float] = None,
                   gather: Optional[Callable[[torch.Tensor], torch.Tensor]] = None) -> dict:
        """Set s's `optimizer` entry in torch's own layout.  `gather`: row -> the flat vector the shapes slice (a sweep
        member's own columns); default: the leading sum(numel) floats of the row."""
        from .trainer import lr_at_epoch
        oc = self.optims[s]
        n = sum(int(np.prod(sh)) for sh in param_shapes)
        rows = [gather(r) if gather is not None else r[:n] for r in self._rows(s)]
        lr = lr_at_epoch(oc, self.epoch or 0) if lr is None else lr
        return torch_state_dict(oc, lr, rows, self.steps()[s], param_shapes)

    def load_state_dict(self, opt_state: Optional[dict], param_shapes: Sequence[tuple], s: int = 0,
                        scatter: Optional[Callable[[torch.Tensor, torch.Tensor], None]] = None,
                        steps: Optional[int] = None) -> bool:
        """Restores set s's state rows and device counter from a torch-layout `optimizer` entry; False (nothing touched)
        when the entry has no state matching this kind and these shapes.  `steps`: the counter for kinds whose state
        carries none (SGD); `scatter(dst_row, flat)`: writes a file's flat vector into the set's row (default: its leading floats)."""
        got = rows_from_state_dict(self.optims[s], opt_state, param_shapes)
        if got is None:
            return False
        rows, step = got
        if self.optims[s].name == "sgd":
            step = max(1, int(steps if steps is not None else 1))
        for dst, r in zip((self.s0, self.s1, self.s2), rows):
            if scatter is not None:
                scatter(dst[s], r)
            else:
                dst[s, :r.numel()].copy_(r)
        self.counter[s:s + 1].copy_(torch.tensor([step], dtype=torch.int32))
        return True
