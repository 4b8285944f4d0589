"""``LogisticProbe``: CLIP's own linear-probe protocol on cached image features.

The "Linear probe CLIP" baseline of the few-shot CLIP literature is three steps: the frozen image features once, with the
evaluation transform; an L2-regularised multinomial logistic regression on them; the regularisation strength chosen on a
validation split.  (`LP` is something else: the reference's trainers/linear_prob.py, an e x e layer in front of the text
classifier trained by SGD on augmented images.)  `ImageFeatures.build` is the first step and `classify_many` the third;
this module is the fit -- S members at once, one per (l2, sample weights), over ONE feature matrix on the device:

    F    = ImageFeatures.build(engine, train_set)                       # one image pass
    lp   = LogisticProbe(F, n_cls, l2=[1e-6, 1e-4, 1e-2, 1.0])          # or LogisticProbe.from_set(engine, train_set, ...)
    info = lp.fit()                                                     # {"iters", "grad_inf", "loss", "converged"} per member
    s, res = lp.select(ImageFeatures.build(engine, val_set))            # the member that classifies the split best
    lp.test(F_test)[s]

Member s minimises  J_s(W, b) = (1/Omega_s) sum_i w_si CE(softmax(z_si.), y_i) + (l2[s]/2) |W|_F^2,
z_sic = a_i <f_i, W[c,:]> + b[c]  (a_i = 1/|f_i| with `norm_feat`), Omega_s = sum_i w_si: sklearn's
LogisticRegression(C = 1 / (l2 Omega)) objective divided by C; the bias is not penalised.  The solver is accelerated
gradient descent with the fixed step 1/L_s (L_s: the trace bound on the Hessian) and gradient restart, all of it on the
device (rpo_logreg_loss_grad_sets + rpo_logreg_step_sets); the host replays a captured chunk of `check_every` iterations
and reads the S "done" flags once per chunk.  A member stops at |grad J_s(y)|_inf <= tol, keeps y and is never written
again, so its result does not depend on S or on the other members.  The few-shot axis is a per-member sample mask
(`shots_mask`) over the same cached matrix.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .features import ImageFeatures, classify_many

MAX_CLASSES = 1024                         # rpo_logreg_loss_grad_sets' C and S (include/rpo_amd.h)
MAX_MEMBERS = 1024


def shots_mask(labels, shots: Sequence[int], generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """[len(shots), n] 0/1 fp32 sample weights: row j keeps, per class, the first shots[j] samples of ONE seeded
    permutation of the n samples (all of a class that has fewer) -- so the k-shot subsets are nested and one cached
    feature matrix serves the whole shots axis."""
    lab = torch.as_tensor(labels, dtype=torch.int64).reshape(-1).cpu()
    n = lab.numel()
    shots = [int(k) for k in shots]
    if n < 1 or not shots or min(shots) < 1:
        raise ValueError(f"shots_mask: needs at least one label and shots >= 1, got {n} labels, shots {shots}")
    perm = torch.randperm(n, generator=generator)
    rank = torch.empty(n, dtype=torch.int64)                # position of sample i among its class, in permutation order
    seen: Dict[int, int] = {}
    for i in perm.tolist():
        c = int(lab[i])
        rank[i] = seen.get(c, 0)
        seen[c] = rank[i] + 1
    return torch.stack([(rank < k).to(torch.float32) for k in shots])


class LogisticProbe:
    def __init__(self, features: ImageFeatures, n_cls: int, l2: Sequence[float], sample_weight=None, norm_feat: bool = False,
                 fit_bias: bool = True):
        n_cls = int(n_cls)
        if n_cls < 1 or n_cls > MAX_CLASSES:
            raise ValueError(f"LogisticProbe: n_cls must be 1 .. {MAX_CLASSES}, got {n_cls}")
        l2 = [float(v) for v in l2]
        if not l2 or len(l2) > MAX_MEMBERS:
            raise ValueError(f"LogisticProbe: 1 .. {MAX_MEMBERS} members (values of l2), got {len(l2)}")
        if any(not (v > 0.0) or v == float("inf") for v in l2):
            raise ValueError(f"LogisticProbe: every l2 must be a positive number, got {l2}")
        S, n = len(l2), len(features)
        w64 = None
        if sample_weight is not None:
            w64 = torch.as_tensor(sample_weight).detach().to("cpu", torch.float64)
            if tuple(w64.shape) != (S, n):
                raise ValueError(f"LogisticProbe: sample_weight must be [{S}, {n}] (members x samples), got {tuple(w64.shape)}")
            if not bool(torch.isfinite(w64).all()) or bool((w64 < 0).any()):
                raise ValueError("LogisticProbe: sample_weight has negative or non-finite entries")
            w64 = w64.to(torch.float32).to(torch.float64)          # the values the kernel reads
            empty = [s for s in range(S) if float(w64[s].sum()) == 0.0]
            if empty:
                raise ValueError(f"LogisticProbe: the sample weights of member(s) {empty} sum to 0")
        bad = [int(v) for v in features.labels if not 0 <= int(v) < n_cls]
        if bad:
            raise ValueError(f"LogisticProbe: {len(bad)} label(s) outside [0, {n_cls}), the first is {bad[0]}")
        dev = torch.device(features.device)
        if features.feat.device != dev or features.labels_dev.device != dev:
            raise ValueError(f"LogisticProbe: the features are on another device (feat {features.feat.device}, labels "
                             f"{features.labels_dev.device}, ImageFeatures.device {dev})")
        e = features.feat.shape[1]
        if e % 32 != 0 or e > 1024:
            raise ValueError(f"LogisticProbe: the embedding size must be a multiple of 32 up to 1024, got {e}")

        self.features, self.device = features, dev
        self.n_cls, self.l2, self.norm_feat, self.fit_bias = n_cls, l2, bool(norm_feat), bool(fit_bias)
        self.S, self.n, self.e = S, n, e
        self.count = n_cls * e + n_cls
        self.stride = (self.count + 3) // 4 * 4
        with torch.cuda.device(dev), torch.no_grad():
            f32 = dict(dtype=torch.float32, device=dev)
            self.weight = None if w64 is None else w64.to(**f32).contiguous()
            omega = torch.full((S,), float(n), dtype=torch.float64) if w64 is None else w64.sum(dim=1)
            self.omega = omega.to(dev)
            self.l2_dev = torch.tensor(l2, **f32)
            # L_s = 0.5 (1/Omega_s) sum_i w_si (a_i^2 |f_i|^2 + [fit_bias]) + l2[s]: once per fit object, float64
            q = features.feat.to(torch.float64).pow(2).sum(dim=1)
            if self.norm_feat:
                a = q.rsqrt().to(torch.float32).to(torch.float64)
                q = a * a * q
            h = q + (1.0 if self.fit_bias else 0.0)
            tr = h.sum().expand(S) if w64 is None else self.weight.to(torch.float64) @ h
            self.L = (0.5 * tr / self.omega + torch.tensor(l2, dtype=torch.float64, device=dev)).to(torch.float32)
            self.x = torch.zeros(S, self.stride, **f32)
            self.y = torch.zeros(S, self.stride, **f32)
            self.grads = torch.zeros(S, self.stride, **f32)
            self.loss = torch.zeros(S, **f32)
            self.t = torch.ones(S, **f32)
            self.tol = torch.zeros(S, **f32)
            self.grad_inf = torch.full((S,), float("inf"), **f32)
            self.done = torch.zeros(S, dtype=torch.int32, device=dev)
            self.iters = torch.zeros(S, dtype=torch.int32, device=dev)
            self.ws = torch.empty(ops.logreg_workspace_floats(n, n_cls, e, S), **f32)
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self._warm = False

    @classmethod
    def from_set(cls, trainer_or_engine, image_set, n_cls: Optional[int] = None, l2: Sequence[float] = (1.0,),
                 batch_size: int = 100, budget_bytes: Optional[int] = None, **kw) -> "LogisticProbe":
        """`ImageFeatures.build` over the set (eval transform, one image pass), then the probe on them.  n_cls defaults to
        the largest label + 1."""
        if n_cls is None:
            n_cls = max(int(v) for v in image_set.labels) + 1
        if int(n_cls) > MAX_CLASSES:
            raise ValueError(f"LogisticProbe: n_cls must be 1 .. {MAX_CLASSES}, got {int(n_cls)}")
        F = ImageFeatures.build(trainer_or_engine, image_set, batch_size=batch_size, budget_bytes=budget_bytes)
        return cls(F, n_cls, l2, **kw)

    # ---- the fit
    def _iteration(self, done) -> None:
        ops.logreg_loss_grad_sets(self.features.feat, self.features.labels_dev, self.weight, self.omega, self.l2_dev, self.y,
                                  self.n_cls, self.grads, self.loss, self.ws, self.norm_feat, self.fit_bias, done)
        ops.logreg_step_sets(self.x, self.y, self.grads, self.count, self.t, self.L, self.tol, done, self.iters,
                             self.grad_inf)

    @torch.no_grad()
    def fit(self, tol: float = 1e-4, max_iter: int = 20000, check_every: int = 50, use_graph: bool = True) -> dict:
        """Iterates until every member's |grad J_s(y)|_inf <= tol (sklearn's lbfgs default, on the same max-norm) or for
        `max_iter` iterations; members that have not converged are reported, not raised.  A second call continues from
        the current point.  -> {"iters" [S] (all calls), "grad_inf" [S], "loss" [S], "converged" [S]}."""
        tol, max_iter, check_every = float(tol), int(max_iter), int(check_every)
        if not tol > 0.0 or max_iter < 1 or check_every < 1:
            raise ValueError(f"LogisticProbe.fit: tol > 0, max_iter >= 1, check_every >= 1; got {tol}, {max_iter}, {check_every}")
        with torch.cuda.device(self.device):
            self.tol.fill_(tol)
            self.done.zero_()
            if not self._warm:                                   # every kernel once, every member skipped: writes nothing
                self._iteration(torch.ones_like(self.done))
                self._warm = True
            it = 0
            while it < max_iter:
                k = min(check_every, max_iter - it)
                if use_graph and k == check_every:
                    g = self._graphs.get(k)
                    if g is None:
                        torch.cuda.synchronize(self.device)
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g, capture_error_mode="thread_local"):
                            for _ in range(k):
                                self._iteration(self.done)
                        self._graphs[k] = g                      # (capture does not execute)
                    g.replay()
                else:
                    for _ in range(k):
                        self._iteration(self.done)
                it += k
                if bool(self.done.cpu().all()):                  # the one read per chunk
                    break
            return {"iters": self.iters.cpu().tolist(), "grad_inf": self.grad_inf.cpu().tolist(),
                    "loss": self.loss.cpu().tolist(), "converged": [bool(d) for d in self.done.cpu().tolist()]}

    @torch.no_grad()
    def reset(self) -> None:
        """Back to the zero start: the next `fit` begins from W = 0, b = 0 with the iteration counts at 0."""
        with torch.cuda.device(self.device):
            for v in (self.x, self.y, self.done, self.iters):
                v.zero_()
            self.t.fill_(1.0)

    def classifier(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(W [S, C, e], b [S, C]) on the device: the point y of every member (the one whose gradient was tested)."""
        C, e = self.n_cls, self.e
        return (self.y[:, :C * e].reshape(self.S, C, e).clone(), self.y[:, C * e:C * e + C].clone())

    def _check_features(self, features: ImageFeatures, what: str) -> None:
        if torch.device(features.device) != self.device or features.feat.device != self.device:
            raise ValueError(f"LogisticProbe.{what}: the features are on another device ({features.feat.device}), the probe "
                             f"is on {self.device}")
        if features.feat.shape[1] != self.e:
            raise ValueError(f"LogisticProbe.{what}: features of embedding size {features.feat.shape[1]}, the probe has {self.e}")

    def test(self, features: ImageFeatures, **kw) -> List[dict]:
        """The S members over cached features in one rpo_features_classify launch: `classify_many`'s dicts."""
        self._check_features(features, "test")
        W, b = self.classifier()
        return classify_many(features, W, b, norm_feat=self.norm_feat, norm_cls=False, scale=1.0, **kw)

    def select(self, val_features: ImageFeatures, **kw) -> Tuple[int, dict]:
        """(the member with the best accuracy on the split, its result); ties go to the larger l2."""
        res = self.test(val_features, **kw)
        best = max(range(self.S), key=lambda s: (res[s]["accuracy"], self.l2[s], -s))
        return best, res[best]

    def state_dict(self) -> dict:
        W, b = self.classifier()
        return {"weight": W.cpu(), "bias": b.cpu(), "l2": torch.tensor(self.l2, dtype=torch.float64),
                "norm_feat": self.norm_feat}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        W, b = torch.as_tensor(sd["weight"]), torch.as_tensor(sd["bias"])
        C, e = self.n_cls, self.e
        if tuple(W.shape) != (self.S, C, e) or tuple(b.shape) != (self.S, C):
            raise ValueError(f"LogisticProbe.load_state_dict: weight {tuple(W.shape)} / bias {tuple(b.shape)}, expected "
                             f"{(self.S, C, e)} / {(self.S, C)}")
        if [float(v) for v in sd["l2"]] != self.l2 or bool(sd["norm_feat"]) != self.norm_feat:
            raise ValueError("LogisticProbe.load_state_dict: l2 / norm_feat are not this probe's")
        with torch.cuda.device(self.device):
            for p in (self.x, self.y):                           # the restart point of the next fit
                p[:, :C * e].copy_(W.reshape(self.S, C * e).to(self.device, torch.float32))
                p[:, C * e:C * e + C].copy_(b.to(self.device, torch.float32))
            self.t.fill_(1.0)
            self.done.zero_()
