"""Every trainer's optimiser on the HIP engine: the host side of rpo_sgd_step* and rpo_optim_step_sets.

A trainer holds ONE optimiser object, built by ``make_optimizer`` from its configs: ``PlainSGD`` when every set's config is
plain SGD (``is_plain_sgd``) -- it issues rpo_sgd_step / rpo_sgd_step_guarded / rpo_sgd_step_sets on the trainer's own
momentum buffer -- and ``OptimState`` otherwise, which owns what rpo_optim_step_sets reads from the device -- `kind` [S],
`hyper` [S, 8], `step` [S] -- and the fp32 state rows of S sets.  Both offer the same surface, and nothing outside this
module knows which kernel steps a buffer: ``step``, ``set_epoch``, ``graph_key`` (what a captured step has baked in
besides addresses), ``splittable`` (whether ``step`` can update one part of the flat buffer), ``state_dict``,
``load_state_dict``, and ``table_driven`` (the rate and the step count are device data).

The module-level functions are pure host code (no device): the hyper tables, torch.optim's state-dict layout per kind in
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


def sgd_hyper_table(optims: Sequence, epoch: int, grad_scale: float = 1.0) -> torch.Tensor:
    """float32 [S, 4] for rpo_sgd_step_sets: (lr_at_epoch(optim_s, epoch), momentum, weight decay, grad_scale) per member,
    rounded to float32 as the scalar arguments of rpo_sgd_step are."""
    from .trainer import lr_at_epoch
    return torch.tensor([[lr_at_epoch(oc, epoch), oc.momentum, oc.weight_decay, grad_scale] for oc in optims],
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
                elif e[nm] is None:              # torch.optim.SGD with momentum 0 writes `momentum_buffer: None`
                    return None
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


def state_shapes(oc, opt_state: Optional[dict]) -> List[tuple]:
    """The shapes of the kind's first state tensor (SGD: `momentum_buffer`) per parameter of a torch-layout `optimizer`
    entry, as far as the file has them: what a refusal names when `load_state_dict` finds no match."""
    st, nm = (opt_state or {}).get("state") or {}, state_names(oc)[0]
    return [tuple(torch.as_tensor(st[i][nm]).shape) for i in sorted(st) if st[i].get(nm) is not None]


class _Sets:
    """What both optimisers share: the configs and the geometry of S sets, the first state row `s0` [S, stride], and
    torch's state-dict layout in both directions over the state rows `_state()` (each [S, stride])."""

    splittable = False             # `step(..., part=slice)` can update one part of the flat buffer
    table_driven = False           # the rate and the step count are device data: `graph_key()` is constant

    def __init__(self, optims: Sequence, set_stride: int, seg0: int, seg1: int, device, s0: Optional[torch.Tensor] = None,
                 used: Optional[torch.Tensor] = None, grad_scale: float = 1.0):
        for oc in optims:
            validate(oc)
        self.optims, self.S = list(optims), len(optims)
        self.stride, self.seg0, self.seg1 = int(set_stride), int(seg0), int(seg1)
        self.device, self.grad_scale, self.used = torch.device(device), float(grad_scale), used
        self.s0 = torch.zeros(self.S, self.stride, device=self.device) if s0 is None else s0.view(self.S, self.stride)
        self.epoch = None

    def state_dict(self, param_shapes: Sequence[tuple], s: int = 0, lr: Optional[float] = None,
                   gather: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, steps: Optional[int] = None) -> dict:
        """Set s's `optimizer` entry in torch's own layout.  `gather`: row -> the flat vector the shapes slice (a sweep
        member's own columns); default: the leading sum(numel) floats of the row.  `steps`: the trainer's count of updates,
        which a plain-SGD set's file carries (the kernels of plain SGD keep no device counter)."""
        from .trainer import lr_at_epoch
        oc = self.optims[s]
        n = sum(int(np.prod(sh)) for sh in param_shapes)
        rows = [r[s].detach().cpu() for r in self._state()[:len(state_names(oc))]]
        rows = [gather(r) if gather is not None else r[:n] for r in rows]
        lr = lr_at_epoch(oc, self.epoch or 0) if lr is None else lr
        return torch_state_dict(oc, lr, rows, self._count(s, steps), param_shapes)

    def load_state_dict(self, opt_state: Optional[dict], param_shapes: Sequence[tuple], s: int = 0,
                        scatter: Optional[Callable[[torch.Tensor, torch.Tensor], None]] = None,
                        steps: Optional[int] = None) -> bool:
        """Restores set s's state rows (and device counter) from a torch-layout `optimizer` entry; False (nothing touched)
        when the entry has no state matching this kind and these shapes.  `steps`: the counter for kinds whose state
        carries none (SGD); `scatter(dst_row, flat)`: writes a file's flat vector into the set's row (default: its leading floats)."""
        got = rows_from_state_dict(self.optims[s], opt_state, param_shapes)
        if got is None:
            return False
        rows, step = got
        for dst, r in zip(self._state(), rows):
            if scatter is not None:
                scatter(dst[s], r)
            else:
                dst[s, :r.numel()].copy_(r)
        self._restore_count(s, step, steps)
        return True


class PlainSGD(_Sets):
    """torch.optim.SGD with dampening 0 and no Nesterov on the trainer's own momentum buffer `s0`: rpo_sgd_step over the
    flat buffer (or one `part` of it), rpo_sgd_step_guarded when the step brings a `found_inf`, and -- with `used`, the
    sets of a sweep -- rpo_sgd_step_sets.  The first two take the rate as a kernel argument (`graph_key()` is the rate);
    the sets form reads (lr, momentum, weight decay, grad_scale) from a device table [S, 4]: every epoch's table is
    uploaded once, and a new epoch's rates are one device-side [S, 4] copy on the current stream."""

    def __init__(self, optims: Sequence, *args, **kw):
        super().__init__(optims, *args, **kw)
        self.splittable = self.used is None
        self.hyper = None
        if self.used is not None:
            self.hyper = torch.zeros(self.S, 4, dtype=torch.float32, device=self.device)
            self._hyper_epochs = torch.stack([sgd_hyper_table(optims, e, self.grad_scale)
                                              for e in range(optims[0].max_epoch + 1)]).to(self.device)
        elif self.S != 1:
            raise ValueError("PlainSGD: sets with their own configs need `used` (the kernel-argument forms step one set)")
        self.set_epoch(0)

    def _state(self):
        return (self.s0,)

    def _count(self, s: int, steps: Optional[int]) -> int:
        return int(steps or 0)

    def _restore_count(self, s: int, step: int, steps: Optional[int]) -> None:
        pass                                            # (the caller keeps the count: it is `first_step` of its next call)

    def set_epoch(self, epoch: int) -> None:
        if self.epoch == epoch:
            return
        if self.hyper is None:
            from .trainer import lr_at_epoch
            self.lr = lr_at_epoch(self.optims[0], epoch)
        elif 0 <= epoch < self._hyper_epochs.shape[0]:
            self.hyper.copy_(self._hyper_epochs[epoch])
        else:                                           # (past the schedule's end: the formula still gives a rate)
            self.hyper.copy_(sgd_hyper_table(self.optims, epoch, self.grad_scale))
        self.epoch = epoch

    def graph_key(self):
        return 0 if self.hyper is not None else self.lr

    def step(self, p: torch.Tensor, g: torch.Tensor, found_inf: Optional[torch.Tensor] = None, first_step: bool = False,
             part: Optional[slice] = None) -> None:
        from . import ops
        oc = self.optims[0]
        assert part is None or (self.splittable and found_inf is None), "only the ungated elementwise step takes a part"
        if self.hyper is not None:
            ops.sgd_step_sets(p, g, self.s0, self.hyper, self.seg0, self.seg1, first_step=first_step, used=self.used,
                              found_inf=found_inf)
        elif found_inf is not None:
            ops.sgd_step_guarded(p.view(-1), g.view(-1), self.s0.view(-1), self.lr, oc.momentum, oc.weight_decay,
                                 self.grad_scale, first_step=first_step, found_inf=found_inf)
        else:
            sl = slice(None) if part is None else part
            ops.sgd_step(p.view(-1)[sl], g.view(-1)[sl], self.s0.view(-1)[sl], self.lr, oc.momentum, oc.weight_decay,
                         self.grad_scale, first_step=first_step)


class OptimState(_Sets):
    """The device tables and state rows of S sets for rpo_optim_step_sets.

    optims: one config per set.  `s0` may be given (a trainer's existing momentum buffer, viewed [S, stride]): SGD sets
    then keep their momentum where the plain path keeps it.  `used` int32 [S, 2] (device) or None."""

    table_driven = True

    def __init__(self, optims: Sequence, *args, **kw):
        super().__init__(optims, *args, **kw)
        S, dev = self.S, self.device
        self.s1 = torch.zeros(S, self.stride, device=dev)
        self.needs_s2 = any(oc.name == "amsgrad" for oc in optims)
        self.s2 = torch.zeros(S, self.stride, device=dev) if self.needs_s2 else None
        self.kind = kind_table(optims).to(dev)
        self.hyper = torch.zeros(S, 8, dtype=torch.float32, device=dev)
        self.counter = torch.zeros(S, dtype=torch.int32, device=dev)
        self.set_epoch(0)

    def _state(self):
        return (self.s0, self.s1, self.s2)

    def set_epoch(self, epoch: int) -> None:
        """The rates of `epoch` into the device table: one small H2D copy on the current stream (nothing when the table
        already holds that epoch)."""
        if self.epoch != epoch:
            self.hyper.copy_(hyper_table(self.optims, epoch, self.grad_scale))
            self.epoch = epoch

    def graph_key(self):
        return 0

    def step(self, p: torch.Tensor, g: torch.Tensor, found_inf: Optional[torch.Tensor] = None, first_step: bool = False,
             part: Optional[slice] = None) -> None:
        """One launch steps every set and advances its counter (`first_step` is the kernel's own business; no `part`)."""
        from . import ops
        assert part is None, "one launch steps the set and advances its counter once"
        S = self.S
        ops.optim_step_sets(p.view(S, self.stride), g.view(S, self.stride), self.s0, self.s1, self.s2, self.kind, self.hyper,
                            self.counter, self.seg0, self.seg1, used=self.used,
                            found_inf=None if found_inf is None else found_inf.view(S, 2), needs_s2=self.needs_s2)

    def steps(self) -> List[int]:
        """Per set, the number of updates applied so far (one D2H read)."""
        return [int(v) for v in self.counter.tolist()]

    def _count(self, s: int, steps: Optional[int]) -> int:
        if steps is not None and is_plain_sgd(self.optims[s]):       # (a sweep's plain-SGD member beside other kinds)
            return int(steps)
        return self.steps()[s]

    def _restore_count(self, s: int, step: int, steps: Optional[int]) -> None:
        if self.optims[s].name == "sgd":
            step = max(1, int(steps if steps is not None else 1))
        self.counter[s:s + 1].copy_(torch.tensor([step], dtype=torch.int32))


def make_optimizer(optims: Sequence, set_stride: int, seg0: int, seg1: int, device, s0: Optional[torch.Tensor] = None,
                   used: Optional[torch.Tensor] = None, grad_scale: float = 1.0):
    """The trainer's optimiser: `PlainSGD` when every set's config is plain SGD, else `OptimState` for all of them (a sweep
    with one other member is table-driven as a whole; its plain-SGD members get the bits of rpo_sgd_step_sets)."""
    cls = PlainSGD if all(is_plain_sgd(oc) for oc in optims) else OptimState
    return cls(optims, set_stride, seg0, seg1, device, s0=s0, used=used, grad_scale=grad_scale)
