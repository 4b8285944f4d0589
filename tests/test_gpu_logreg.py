"""The logistic probe on the GPU (rpo_amd/csrc/logreg.hip, rpo_amd/logreg.py).  A float64 NumPy
restatement of the objective, written here, is the only oracle: the gradient kernel against it inside a budget computed
from the inputs; member isolation, repeatability and NaN containment bit for bit; the step kernel against the float64
recurrence; the fit certified by the float64 gradient at the point it returns, inside an iteration window pinned by the
float64 recurrence; an independent solver (SciPy) at the well-conditioned l2; the public path on a depth-2 synthetic ViT.
Kernel tests: tens of tiny launches per case; fits: a few thousand iterations of four tiny launches."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rpo_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def gamma(m):
    return m * U / (1.0 - m * U)


# ---- the float64 restatement (one member) -------------------------------------------------------------------------------

def row_scale(F, norm_feat):
    return 1.0 / np.sqrt((F * F).sum(1)) if norm_feat else np.ones(F.shape[0])


def oracle(F, y, w, l2, W, b, norm_feat, fit_bias, omega=None):
    """J, dJ/dW, dJ/db of section 1 in float64 (F [n, e], y int [n], w [n] >= 0, W [C, e], b [C]) and the pieces the
    budget needs.  A label outside [0, C) behaves as weight 0; `omega` overrides sum(w) (the caller's Omega)."""
    n, C = F.shape[0], W.shape[0]
    ok = (y >= 0) & (y < C)
    a = row_scale(F, norm_feat)
    AF = a[:, None] * F
    Z = AF @ W.T + b[None]
    m = Z.max(1, keepdims=True)
    E = np.exp(Z - m)
    s = E.sum(1, keepdims=True)
    P = E / s
    Y = np.zeros((n, C))
    Y[np.nonzero(ok)[0], y[ok]] = 1.0
    om = np.where(ok, w, 0.0) / (w.sum() if omega is None else omega)
    ce = np.where(ok, (m[:, 0] + np.log(s[:, 0])) - (Z * Y).sum(1), 0.0)
    reg = 0.5 * l2 * (W * W).sum()
    Rm = om[:, None] * (P - Y)
    gW = Rm.T @ AF + l2 * W
    gb = Rm.sum(0) if fit_bias else np.zeros(C)
    return dict(J=(om * ce).sum() + reg, gW=gW, gb=gb, Z=Z, P=P, Y=Y, om=om, AF=AF, ce=ce, reg=reg, a=a, l2=l2)


def budget(F, W, b, o):
    """Per element, from the inputs (u = 2^-24, gamma_m = m u / (1 - m u)):
      dz_ic <= gamma_{e+2} (sum_k |a_i f_ik W_ck| + |b_c|)         the fp32 dot product, the row scale, the bias fma
      dp_ic <= p_ic (2 max_c' dz_ic' + 4 u)                          the shifted exponent, expf, the division
      |dG_ck| <= sum_i om_i |a_i f_ik| dp_ic + gamma_{n+1} sum_i om_i |a_i f_ik r_ic| + u l2 |W_ck|      (r = p - [c == y])
      |dgb_c| <= sum_i om_i dp_ic + gamma_{n+1} sum_i om_i |r_ic|
      |dJ|    <= sum_i om_i (2 max_c dz_ic + 4 u) + gamma_{n+1} sum_i om_i ce_i + 2 u (l2/2)|W|^2
    The first two terms of dG are the data term's; the third is the penalty's share of the result's own rounding, which
    no fp32 output can avoid where l2 W_ck dominates the element (it vanishes with l2 or W).  The loss line has the same
    form: log-sum-exp moves by at most max_c dz, the label's logit by its own dz, and the penalty is rounded twice (as
    the fp32 it is kept in, and in the final sum)."""
    n, e = F.shape
    absAF = np.abs(o["AF"])
    dz = gamma(e + 2) * (absAF @ np.abs(W).T + np.abs(b)[None])
    dzmax = dz.max(1, keepdims=True)
    dp = o["P"] * (2.0 * dzmax + 4.0 * U)
    wAF = o["om"][:, None] * absAF
    absr = np.abs(o["P"] - o["Y"])
    dG = dp.T @ wAF + gamma(n + 1) * (absr.T @ wAF) + U * o["l2"] * np.abs(W)
    dgb = (o["om"][:, None] * dp).sum(0) + gamma(n + 1) * (o["om"][:, None] * absr).sum(0)
    dJ = (o["om"] * (2.0 * dzmax[:, 0] + 4.0 * U)).sum() + gamma(n + 1) * (o["om"] * o["ce"]).sum() + 2.0 * U * o["reg"]
    return dict(dz=dz, gW=dG, gb=dgb, J=dJ)


def lipschitz(F, w, l2, norm_feat, fit_bias):
    a = row_scale(F, norm_feat)
    h = a * a * (F * F).sum(1) + (1.0 if fit_bias else 0.0)
    return 0.5 * (w * h).sum() / w.sum() + l2


def recurrence(F, y, w, l2, C, norm_feat, fit_bias, tol, max_iter=20000):
    """Section 2 in float64 from a zero start -> (W, b, iterations applied before the stopping test passed)."""
    e = F.shape[1]
    L = lipschitz(F, w, l2, norm_feat, fit_bias)
    x = np.zeros(C * e + C)
    yk = x.copy()
    t = 1.0
    for it in range(max_iter + 1):
        o = oracle(F, y, w, l2, yk[:C * e].reshape(C, e), yk[C * e:], norm_feat, fit_bias)
        g = np.concatenate([o["gW"].reshape(-1), o["gb"]])
        if np.abs(g).max() <= tol:
            return yk[:C * e].reshape(C, e), yk[C * e:], it
        xn = yk - g / L
        if g @ (xn - x) > 0:
            t = 1.0
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        yk = xn + ((t - 1.0) / tn) * (xn - x)
        x, t = xn, tn
    return None, None, max_iter + 1


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def clustered(n, C, e, seed, unit=False, spread=0.5):
    """Gaussian class clusters: fp32 features [n, e], labels [n] with every class < min(C, n) present."""
    rng = np.random.default_rng(seed)
    y = (np.arange(n) % C).astype(np.int64)
    rng.shuffle(y)
    centres = rng.standard_normal((C, e))
    F = centres[y] + spread * rng.standard_normal((n, e))
    if unit:
        F = F / np.sqrt((F * F).sum(1, keepdims=True))
    return F.astype(np.float32), y


def trained_W(F, C, S, seed, norm_feat):
    """[S, C, e] and [S, C] fp32 with logits up to about 30 in magnitude."""
    rng = np.random.default_rng(seed)
    e = F.shape[1]
    W = rng.standard_normal((S, C, e))
    b = rng.standard_normal((S, C))
    a = row_scale(F.astype(np.float64), norm_feat)
    for s in range(S):
        z = np.abs((a[:, None] * F) @ W[s].T).max()
        W[s] *= 29.0 / z
    return W.astype(np.float32), b.astype(np.float32)


def weights(n, S, seed):
    """[S, n] fp32 >= 0 with exact zeros; member 0 zeroes the whole first row tile where there is a second one."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.0, 2.0, (S, n))
    w[rng.uniform(size=(S, n)) < 0.2] = 0.0
    if n > 32:
        w[0, :32] = 0.0
    w[:, -1] = 1.25                                             # (no member sums to 0)
    return w.astype(np.float32)


class Problem:
    """The device side of one loss_grad call."""

    def __init__(self, F, y, w, l2, C, norm_feat, fit_bias):
        n, e = F.shape
        S = len(l2)
        self.n, self.e, self.C, self.S, self.nf, self.fb = n, e, C, S, norm_feat, fit_bias
        self.count = C * e + C
        self.stride = (self.count + 3) // 4 * 4
        self.feat = torch.from_numpy(F).to(DEV)
        self.label = torch.from_numpy(y).to(DEV)
        self.weight = None if w is None else torch.from_numpy(w).to(DEV)
        om = np.full(S, float(n)) if w is None else w.astype(np.float64).sum(1)
        self.omega = torch.from_numpy(om).to(DEV)
        self.l2 = torch.tensor(l2, dtype=torch.float32, device=DEV)
        self.ws = torch.full((ops.logreg_workspace_floats(n, C, e, S),), float("nan"), device=DEV)
        self.grads = torch.full((S, self.stride), -7.0, device=DEV)
        self.loss = torch.full((S,), -7.0, device=DEV)

    def params(self, W, b):
        p = torch.zeros(self.S, self.stride, device=DEV)
        p[:, :self.C * self.e] = torch.from_numpy(W).to(DEV).reshape(self.S, -1)
        p[:, self.C * self.e:self.count] = torch.from_numpy(b).to(DEV)
        return p

    def run(self, p, done=None):
        ops.logreg_loss_grad_sets(self.feat, self.label, self.weight, self.omega, self.l2, p, self.C, self.grads, self.loss,
                                  self.ws, self.nf, self.fb, done)
        torch.cuda.synchronize()
        g = self.grads.cpu().numpy()
        Ce = self.C * self.e
        return g[:, :Ce].reshape(self.S, self.C, self.e), g[:, Ce:self.count], self.loss.cpu().numpy()


def worst_fraction(F, y, w, l2, W, b, nf, fb, gW, gb, J, what):
    """Asserts every element inside its budget; -> the largest fraction used."""
    worst = 0.0
    F64 = F.astype(np.float64)
    for s in range(len(l2)):
        ws_ = np.ones(F.shape[0]) if w is None else w[s].astype(np.float64)
        l2s = float(np.float32(l2[s]))
        o = oracle(F64, y, ws_, l2s, W[s].astype(np.float64), b[s].astype(np.float64), nf, fb)
        bud = budget(F64, W[s].astype(np.float64), b[s].astype(np.float64), o)
        for name, got, want, room in (("gW", gW[s], o["gW"], bud["gW"]), ("gb", gb[s], o["gb"], bud["gb"] if fb else 0.0),
                                      ("J", J[s], o["J"], bud["J"])):
            err = np.abs(got.astype(np.float64) - want)
            room = np.broadcast_to(room, err.shape)
            assert (err <= room).all(), (f"{what} member {s} {name}: error {err.max():.3e} at "
                                         f"{np.unravel_index(np.argmax(err - room), err.shape)}, its budget "
                                         f"{room[np.unravel_index(np.argmax(err - room), err.shape)]:.3e}")
            pos = room > 0
            if pos.any():
                worst = max(worst, float((err[pos] / room[pos]).max()))
    return worst


# ---- 1. the gradient kernel against float64 -------------------------------------------------------------------------------

SHAPES = [(1, 2, 32, 1), (33, 3, 32, 3), (65, 33, 64, 2), (40, 1, 32, 1), (64, 1000, 32, 1), (96, 5, 1024, 2),
          (1030, 5, 32, 2)]                                     # the last: a second row chunk of the gradient GEMM


@pytest.mark.parametrize("n,C,e,S", SHAPES)
def test_loss_and_gradient_against_float64(n, C, e, S):
    F, y = clustered(n, C, e, seed=n + C)
    l2 = [1e-30, 1e-1, 1e-3][:S]                                # (member 0: the data term alone, the budget's first two terms)
    worst = 0.0
    for weighted in (False, True):
        w = weights(n, S, seed=7) if weighted else None
        for nf in (False, True):
            Wt, bt = trained_W(F, C, S, seed=3, norm_feat=nf)
            for fb in (False, True):
                pr = Problem(F, y, w, l2, C, nf, fb)
                for rng_name, (W, b) in (("zeros", (np.zeros_like(Wt), np.zeros_like(bt))), ("trained", (Wt, bt))):
                    if not fb:
                        b = np.zeros_like(b)
                    gW, gb, J = pr.run(pr.params(W, b))
                    what = f"[n {n} C {C} e {e} S {S} weight {weighted} norm_feat {nf} fit_bias {fb} W {rng_name}]"
                    worst = max(worst, worst_fraction(F, y, w, l2, W, b, nf, fb, gW, gb, J, what))
                    if C == 1:                                   # one class: p = 1, the data terms are exactly 0
                        assert np.array_equal(gb, np.zeros_like(gb))
                        lam = np.array(l2, dtype=np.float32)[:, None, None]
                        assert np.array_equal(gW, lam * W), what
                        if rng_name == "zeros":
                            assert not gW.any() and not J.any(), what
                    if not fb:
                        assert not gb.any(), what
                    if weighted and 32 < n <= 1024:
                        # member 0's mask zeroes row tile 0: those rows contribute exact zeros, so the call without them
                        # (same Omega) has the same bits
                        sub = Problem(F[32:], y[32:], np.ascontiguousarray(w[:1, 32:]), l2[:1], C, nf, fb)
                        sub.omega.copy_(pr.omega[:1])
                        gW1, gb1, J1 = sub.run(sub.params(W[:1], b[:1]))
                        assert np.array_equal(gW1[0].view(np.int32), gW[0].view(np.int32)), what
                        assert np.array_equal(gb1[0].view(np.int32), gb[0].view(np.int32)), what
                        assert J1[0].view(np.int32) == J[0].view(np.int32), what
    print(f"\n[logreg_loss_grad n {n} C {C} e {e} S {S}] worst err / budget {worst:.4f}")


def test_label_outside_the_range_is_weight_zero():
    n, C, e = 40, 5, 32
    F, y = clustered(n, C, e, seed=11)
    y[3], y[35] = C, -1
    W, b = trained_W(F, C, 1, seed=4, norm_feat=False)
    pr = Problem(F, y, None, [1e-2], C, False, True)
    pr.omega.fill_(float(n - 2))                                 # the caller's Omega: the rows that count
    gW, gb, J = pr.run(pr.params(W, b))
    F64 = F.astype(np.float64)
    o = oracle(F64, y, np.ones(n), float(np.float32(1e-2)), W[0].astype(np.float64), b[0].astype(np.float64), False, True,
               omega=float(n - 2))
    bud = budget(F64, W[0].astype(np.float64), b[0].astype(np.float64), o)
    assert (np.abs(gW[0] - o["gW"]) <= bud["gW"]).all() and (np.abs(gb[0] - o["gb"]) <= bud["gb"]).all()
    assert abs(J[0] - o["J"]) <= bud["J"]


# ---- 2. isolation and repeatability ---------------------------------------------------------------------------------------

class Solver:
    """loss_grad + step on S members from given parameters."""

    def __init__(self, pr, p0, L, tol):
        S = pr.S
        self.pr = pr
        self.x, self.y = p0.clone(), p0.clone()
        self.t = torch.ones(S, device=DEV)
        self.L = torch.tensor(L, dtype=torch.float32, device=DEV)
        self.tol = torch.full((S,), tol, device=DEV)
        self.done = torch.zeros(S, dtype=torch.int32, device=DEV)
        self.iters = torch.zeros(S, dtype=torch.int32, device=DEV)
        self.ginf = torch.zeros(S, device=DEV)

    def iterate(self, k):
        pr = self.pr
        for _ in range(k):
            ops.logreg_loss_grad_sets(pr.feat, pr.label, pr.weight, pr.omega, pr.l2, self.y, pr.C, pr.grads, pr.loss, pr.ws,
                                      pr.nf, pr.fb, self.done)
            ops.logreg_step_sets(self.x, self.y, pr.grads, pr.count, self.t, self.L, self.tol, self.done, self.iters,
                                 self.ginf)
        torch.cuda.synchronize()
        return [bits(v) for v in (self.x, self.y, self.t, self.iters, pr.grads, pr.loss)]


def test_members_are_isolated_and_runs_repeat():
    n, C, e, S = 65, 33, 64, 3
    F, y = clustered(n, C, e, seed=21)
    w = weights(n, S, seed=5)
    l2 = [1e-1, 1e-2, 1e-3]
    W, b = trained_W(F, C, S, seed=9, norm_feat=True)
    W, b = 0.2 * W, 0.2 * b
    L = [lipschitz(F.astype(np.float64), w[s].astype(np.float64), l2[s], True, True) for s in range(S)]

    def whole(Wm):
        pr = Problem(F, y, w, l2, C, True, True)
        p = pr.params(Wm, b)
        gW, gb, J = pr.run(p)
        first = [bits(pr.grads[:, :pr.count]), bits(pr.loss)]
        return first, Solver(pr, p, L, 1e-30).iterate(20), pr.count

    first, after, count = whole(W)
    first2, after2, _ = whole(W)
    for a_, b_ in zip(first + after, first2 + after2):
        assert torch.equal(a_, b_), "two runs differ"
    assert int(after[3].min()) == 20
    for s in range(S):
        pr = Problem(F, y, w[s:s + 1], l2[s:s + 1], C, True, True)
        p = pr.params(W[s:s + 1], b[s:s + 1])
        pr.run(p)
        assert torch.equal(bits(pr.grads[:, :count]), first[0][s:s + 1]) and torch.equal(bits(pr.loss), first[1][s:s + 1])
        one = Solver(pr, p, L[s:s + 1], 1e-30).iterate(20)
        for k, name in enumerate(("x", "y", "t", "iters")):
            got = after[k][s:s + 1]
            want = one[k]
            if name in ("x", "y"):
                got, want = got[:, :count], want[:, :count]
            assert torch.equal(got, want), f"member {s} of the S = 3 call: {name} differs from the S = 1 call"
    Wn = W.copy()
    Wn[0, 1, 5] = np.nan
    firstn, aftern, _ = whole(Wn)
    for a_, b_ in zip(first + after, firstn + aftern):
        assert torch.equal(a_[1:], b_[1:]), "a NaN in member 0 reached another member"
    assert torch.isnan(firstn[1].view(torch.float32)[0])


# ---- 3. the step kernel ---------------------------------------------------------------------------------------------------

def _step_once(x, y, g, t, L, tol, done, iters):
    S, count = x.shape
    stride = (count + 3) // 4 * 4
    d = {}
    for name, v in (("x", x), ("y", y), ("g", g)):
        buf = torch.full((S, stride), 123.0, device=DEV)
        buf[:, :count] = torch.from_numpy(v).to(DEV)
        d[name] = buf
    d["t"] = torch.from_numpy(t).to(DEV)
    d["L"] = torch.from_numpy(L).to(DEV)
    d["tol"] = torch.from_numpy(tol).to(DEV)
    d["done"] = torch.from_numpy(done).to(DEV)
    d["iters"] = torch.from_numpy(iters).to(DEV)
    d["ginf"] = torch.full((S,), -3.0, device=DEV)
    ops.logreg_step_sets(d["x"], d["y"], d["g"], count, d["t"], d["L"], d["tol"], d["done"], d["iters"], d["ginf"])
    torch.cuda.synchronize()
    assert bool((d["x"][:, count:] == 123.0).all()) and bool((d["y"][:, count:] == 123.0).all())
    return {k: v.cpu().numpy() for k, v in d.items()}


def _step64(x, y, g, t, L):
    xn = y - g / L
    restart = float(g @ (xn - x)) > 0
    t0 = 1.0 if restart else t
    tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t0 * t0))
    beta = (t0 - 1.0) / tn
    return xn, xn + beta * (xn - x), tn, beta, restart


def test_step_against_the_float64_recurrence():
    """One iteration at a time from the kernel's own fp32 state, so the bound is one iteration's roundings: x+ is the
    rounded 1/L and one fma (<= 3 u on |y| + |g|/L), y+ one subtraction and one fma on top of it and the fp32 beta
    (<= 4 roundings of t): 4 u and 8 u (1 + beta) of |x| + |y| + |g|/L hold with room."""
    rng = np.random.default_rng(0)
    S, count = 3, 2 * 32 + 2 + 1027                             # more than one pass of the workgroup
    x = rng.standard_normal((S, count)).astype(np.float32)
    y = (x + 0.1 * rng.standard_normal((S, count))).astype(np.float32)
    t = np.array([1.0, 2.5, 4.0], dtype=np.float32)
    L = np.array([0.7, 1.3, 20.0], dtype=np.float32)
    tol = np.full(S, 1e-6, dtype=np.float32)
    done = np.zeros(S, dtype=np.int32)
    iters = np.array([0, 5, 9], dtype=np.int32)
    seen = set()
    for k in range(5):
        g = rng.standard_normal((S, count)).astype(np.float32)
        if k == 1:                                               # hand-made: y - x = 2 g / L -> <g, x+ - x> = |g|^2 / L > 0
            y[0] = (x[0].astype(np.float64) + 2.0 * g[0] / np.float64(L[0])).astype(np.float32)
        if k == 2:                                               # hand-made: y = x -> <g, x+ - x> = -|g|^2 / L < 0
            y[0] = x[0]
        out = _step_once(x, y, g, t, L, tol, done, iters)
        for s in range(S):
            xn, yn, tn, beta, restart = _step64(x[s].astype(np.float64), y[s].astype(np.float64), g[s].astype(np.float64),
                                                float(t[s]), float(L[s]))
            if s == 0 and k in (1, 2):
                assert restart == (k == 1)
                seen.add(restart)
            mag = np.abs(x[s]) + np.abs(y[s]) + np.abs(g[s]) / float(L[s])
            assert (np.abs(out["x"][s, :count] - xn) <= 4 * U * mag).all(), (k, s)
            assert (np.abs(out["y"][s, :count] - yn) <= 8 * U * (1 + beta) * mag).all(), (k, s)
            assert abs(out["t"][s] - tn) <= 4 * U * tn and out["iters"][s] == iters[s] + 1 and out["done"][s] == 0
            assert out["ginf"][s] == np.abs(g[s]).max()
            if restart:                                          # beta = 0: y+ is x+, bit for bit
                assert np.array_equal(out["y"][s, :count], out["x"][s, :count])
        x, y, t, iters = out["x"][:, :count].copy(), out["y"][:, :count].copy(), out["t"], out["iters"]
    assert seen == {True, False}
    # a member with done = 1 is not written, its counter and its tested norm included; a member inside tol stops and keeps y
    g = rng.standard_normal((S, count)).astype(np.float32)
    g[2] *= 1e-8
    done = np.array([0, 1, 0], dtype=np.int32)
    out = _step_once(x, y, g, t, L, tol, done, iters)
    assert np.array_equal(out["x"][1, :count], x[1]) and np.array_equal(out["y"][1, :count], y[1])
    assert out["t"][1] == t[1] and out["iters"][1] == iters[1] and out["ginf"][1] == -3.0 and out["done"][1] == 1
    assert out["done"][2] == 1 and out["iters"][2] == iters[2] and out["t"][2] == t[2]
    assert np.array_equal(out["x"][2, :count], x[2]) and np.array_equal(out["y"][2, :count], y[2])
    assert out["ginf"][2] == np.abs(g[2]).max() <= 1e-6
    assert out["done"][0] == 0 and out["iters"][0] == iters[0] + 1


# ---- 4. the fit -----------------------------------------------------------------------------------------------------------

FIT_L2 = (1e-1, 1e-2, 1e-3)
FIT_TOL = 1e-4
FIT_CASES = {"c3": (60, 3, 32, 40), "c33": (66, 33, 64, 41)}


def _features(F, y):
    from rpo_amd.features import ImageFeatures
    return ImageFeatures({"n_images": F.shape[0]}, torch.from_numpy(F).to(DEV), torch.from_numpy(y).to(DEV),
                         [int(v) for v in y], torch.device(DEV))


@functools.lru_cache(maxsize=None)
def _fit_case(name):
    """The inputs, the float64 recurrence's iteration counts (run once) and the fitted probe, shared by the tests below."""
    from rpo_amd.logreg import LogisticProbe
    n, C, e, seed = FIT_CASES[name]
    F, y = clustered(n, C, e, seed, unit=True)
    F64 = F.astype(np.float64)
    counts = [recurrence(F64, y, np.ones(n), float(np.float32(l2)), C, False, True, FIT_TOL)[2] for l2 in FIT_L2]
    probe = LogisticProbe(_features(F, y), C, FIT_L2)
    info = probe.fit(tol=FIT_TOL)
    return F, y, C, counts, probe, info


def certificate(F, y, w, l2, W, b, nf, fb, tol, what):
    """The float64 gradient at (W, b) is within tol + test 1's budget at that point, element by element."""
    F64 = F.astype(np.float64)
    o = oracle(F64, y, w, float(np.float32(l2)), W.astype(np.float64), b.astype(np.float64), nf, fb)
    bud = budget(F64, W.astype(np.float64), b.astype(np.float64), o)
    assert (np.abs(o["gW"]) <= tol + bud["gW"]).all(), f"{what}: |dJ/dW|_inf {np.abs(o['gW']).max():.3e}"
    assert (np.abs(o["gb"]) <= tol + bud["gb"]).all(), f"{what}: |dJ/db|_inf {np.abs(o['gb']).max():.3e}"
    return float(max(bud["gW"].max(), bud["gb"].max()))


@pytest.mark.parametrize("name", list(FIT_CASES))
def test_fit_converges_inside_the_window_and_is_certified(name):
    F, y, C, counts, probe, info = _fit_case(name)
    print(f"\n[logreg fit {name}] float64 recurrence {counts}, device {info['iters']}, |g|_inf {info['grad_inf']}")
    assert all(c <= 5000 for c in counts), counts
    assert all(info["converged"]), info
    W, b = (v.cpu().numpy() for v in probe.classifier())
    for s, l2 in enumerate(FIT_L2):
        assert 0.75 * counts[s] <= info["iters"][s] <= 1.25 * counts[s], (s, counts[s], info["iters"][s])
        assert info["grad_inf"][s] <= FIT_TOL
        certificate(F, y, np.ones(len(y)), l2, W[s], b[s], False, True, FIT_TOL, f"{name} member {s}")


def test_a_larger_tol_stops_earlier_and_a_second_fit_continues():
    from rpo_amd.logreg import LogisticProbe
    F, y, C, counts, probe, info = _fit_case("c3")
    p2 = LogisticProbe(_features(F, y), C, FIT_L2)
    early = p2.fit(tol=1e-2)
    assert all(early["converged"]) and all(a < b for a, b in zip(early["iters"], info["iters"])), (early, info)
    assert all(g <= 1e-2 for g in early["grad_inf"])
    W1 = p2.classifier()[0].clone()
    late = p2.fit(tol=FIT_TOL)
    # stopping wrote nothing, so the second fit walks on along the same trajectory: the iterations add up to the one
    # fit's, and the point is the same bits
    assert late["iters"] == info["iters"] and all(late["converged"])
    for a_, b_ in zip(p2.classifier(), probe.classifier()):
        assert torch.equal(bits(a_), bits(b_))
    assert not torch.equal(bits(W1), bits(p2.classifier()[0]))


def test_graph_replay_and_eager_give_equal_bits():
    from rpo_amd.logreg import LogisticProbe
    F, y, C, counts, probe, info = _fit_case("c3")
    eager = LogisticProbe(_features(F, y), C, FIT_L2)
    got = eager.fit(tol=FIT_TOL, use_graph=False)
    assert got["iters"] == info["iters"] and got["converged"] == info["converged"]
    assert np.array_equal(np.array(got["grad_inf"], np.float32).view(np.int32), np.array(info["grad_inf"], np.float32).view(np.int32))
    assert np.array_equal(np.array(got["loss"], np.float32).view(np.int32), np.array(info["loss"], np.float32).view(np.int32))
    for a_, b_ in zip(eager.classifier(), probe.classifier()):
        assert torch.equal(bits(a_), bits(b_))
    # max_iter ends the fit, unconverged members are reported
    short = LogisticProbe(_features(F, y), C, FIT_L2).fit(tol=FIT_TOL, max_iter=10, check_every=4)
    assert short["iters"] == [10, 10, 10] and short["converged"] == [False, False, False]


# ---- 5. against an independent solver -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FIT_CASES))
def test_against_lbfgs_at_the_well_conditioned_l2(name):
    opt = pytest.importorskip("scipy.optimize", reason="SciPy is not installed on this machine")
    F, y, C, counts, probe, info = _fit_case(name)
    F64, e = F.astype(np.float64), F.shape[1]
    l2 = float(np.float32(FIT_L2[0]))
    w = np.ones(len(y))

    def fun(v):
        o = oracle(F64, y, w, l2, v[:C * e].reshape(C, e), v[C * e:], False, True)
        return o["J"], np.concatenate([o["gW"].reshape(-1), o["gb"]])
    res = opt.minimize(fun, np.zeros(C * e + C), jac=True, method="L-BFGS-B",
                       options=dict(gtol=1e-12, ftol=0.0, maxiter=20000, maxfun=40000, maxcor=30))
    Wstar = res.x[:C * e].reshape(C, e)
    assert np.abs(fun(res.x)[1]).max() <= 1e-9, "L-BFGS-B did not reach its own optimum"
    W, b = (v.cpu().numpy() for v in probe.classifier())
    bud = certificate(F, y, w, FIT_L2[0], W[0], b[0], False, True, FIT_TOL, name)
    err = np.abs(W[0] - Wstar).max()
    room = (FIT_TOL + bud) * np.sqrt(C * e) / l2
    print(f"\n[logreg vs L-BFGS-B {name}] |W - W*|_inf {err:.3e}, bound {room:.3e}")
    assert err <= room


# ---- 6. the public path ---------------------------------------------------------------------------------------------------

PUB_L2 = (1.0, 1e-1, 1e-2)


@functools.lru_cache(maxsize=None)
def _public():
    from test_gpu_features import _decoded, _vit
    from rpo_amd.features import ImageFeatures
    from rpo_amd.input_pipeline import DeviceImageSet
    from rpo_amd.logreg import LogisticProbe
    from rpo_amd.zeroshot import ZeroshotCLIP
    cfg, sd = _vit()
    engine = ZeroshotCLIP(sd, device=DEV, act_dtype=torch.float32, max_batch=4).engine
    labels = [i % 3 for i in range(24)]
    train = DeviceImageSet(_decoded(24, 0), labels, DEV)
    val = DeviceImageSet(_decoded(12, 1), [(i + 1) % 3 for i in range(12)], DEV)
    probe = LogisticProbe.from_set(engine, train, n_cls=3, l2=PUB_L2, norm_feat=True, batch_size=4)
    info = probe.fit()
    return engine, train, probe, info, ImageFeatures.build(engine, val, batch_size=4)


def test_public_path_predicts_the_float64_argmax():
    engine, train, probe, info, F_val = _public()
    assert all(info["converged"]), info
    Ftr = probe.features
    assert len(Ftr) == 24 and Ftr.labels == [i % 3 for i in range(24)]
    pred = torch.full((3, 24), -1, dtype=torch.int32, device=DEV)
    res = probe.test(Ftr, pred_out=pred)
    assert len(res) == 3 and all(r["total"] == 24 for r in res)
    F64 = Ftr.feat.cpu().numpy().astype(np.float64)
    y = np.array(Ftr.labels)
    W, b = (v.cpu().numpy().astype(np.float64) for v in probe.classifier())
    for s in range(3):
        o = oracle(F64, y, np.ones(24), float(np.float32(PUB_L2[s])), W[s], b[s], True, True)
        dz = budget(F64, W[s], b[s], o)["dz"]
        order = np.argsort(-o["Z"], axis=1)
        top, second = order[:, 0], order[:, 1]
        rows = np.arange(24)
        gap = o["Z"][rows, top] - o["Z"][rows, second]
        keep = gap >= dz[rows, top] + dz[rows, second]
        assert keep.sum() >= 23, f"member {s}: {24 - keep.sum()} rows inside the logit budget"
        got = pred[s].cpu().numpy()
        assert np.array_equal(got[keep], top[keep]), f"member {s}"
        assert res[s]["correct"] == int((got == y).sum())


def test_select_returns_the_member_classify_many_ranks_first():
    from rpo_amd.features import classify_many
    engine, train, probe, info, F_val = _public()
    W, b = probe.classifier()
    res = classify_many(F_val, W, b, norm_feat=True, norm_cls=False, scale=1.0)
    acc = [r["accuracy"] for r in res]
    want = max(range(3), key=lambda s: (acc[s], PUB_L2[s]))
    best, got = probe.select(F_val)
    assert best == want and got["accuracy"] == acc[want] and got["total"] == 12
    if acc.count(max(acc)) > 1:
        assert PUB_L2[best] == max(l for l, a_ in zip(PUB_L2, acc) if a_ == max(acc))


def test_shots_members_equal_fits_on_the_gathered_rows():
    from rpo_amd.features import ImageFeatures
    from rpo_amd.logreg import LogisticProbe, shots_mask
    engine, train, probe, info, F_val = _public()
    Ftr = probe.features
    l2 = 1e-1
    mask = shots_mask(Ftr.labels, (1, 4), torch.Generator().manual_seed(3))
    assert mask.sum(1).tolist() == [3.0, 12.0]
    both = LogisticProbe(Ftr, 3, [l2, l2], sample_weight=mask, norm_feat=True)
    assert all(both.fit()["converged"])
    Wm, bm = (v.cpu().numpy() for v in both.classifier())
    F_all, y_all = Ftr.feat.cpu().numpy(), np.array(Ftr.labels)
    for s in range(2):
        idx = np.nonzero(mask[s].numpy())[0]
        sub = ImageFeatures({"n_images": len(idx)}, Ftr.feat[torch.from_numpy(idx).to(DEV)].contiguous(),
                            Ftr.labels_dev[torch.from_numpy(idx).to(DEV)].contiguous(), [int(y_all[i]) for i in idx], Ftr.device)
        one = LogisticProbe(sub, 3, [l2], norm_feat=True)
        assert all(one.fit()["converged"])
        W1, b1 = (v.cpu().numpy() for v in one.classifier())
        # both points are certified stationary points of the SAME objective (the gathered rows'), so they are as close as
        # strong convexity in W puts two such points
        bud_m = certificate(F_all[idx], y_all[idx], np.ones(len(idx)), l2, Wm[s], bm[s], True, True, 1e-4, f"mask member {s}")
        bud_1 = certificate(F_all[idx], y_all[idx], np.ones(len(idx)), l2, W1[0], b1[0], True, True, 1e-4, f"gathered fit {s}")
        certificate(F_all, y_all, mask[s].numpy().astype(np.float64), l2, W1[0], b1[0], True, True, 1e-4, f"gathered fit {s}, masked")
        room = (2e-4 + bud_m + bud_1) * np.sqrt(3 * F_all.shape[1]) / float(np.float32(l2))
        assert np.abs(Wm[s] - W1[0]).max() <= room


def test_state_dict_round_trips_to_equal_bits():
    from rpo_amd.logreg import LogisticProbe
    engine, train, probe, info, F_val = _public()
    sd = probe.state_dict()
    assert set(sd) == {"weight", "bias", "l2", "norm_feat"} and sd["norm_feat"] is True
    assert tuple(sd["weight"].shape) == (3, 3, probe.e) and tuple(sd["bias"].shape) == (3, 3)
    assert sd["l2"].tolist() == list(PUB_L2)
    other = LogisticProbe(probe.features, 3, PUB_L2, norm_feat=True)
    other.load_state_dict(sd)
    for a_, b_ in zip(other.classifier(), probe.classifier()):
        assert torch.equal(bits(a_), bits(b_))
    sd2 = other.state_dict()
    assert torch.equal(bits(sd2["weight"]), bits(sd["weight"])) and torch.equal(bits(sd2["bias"]), bits(sd["bias"]))
    a_, b_ = probe.test(F_val), other.test(F_val)
    assert [r["correct"] for r in a_] == [r["correct"] for r in b_]
    with pytest.raises(ValueError, match="l2 / norm_feat"):
        LogisticProbe(probe.features, 3, (1.0, 0.5, 0.25), norm_feat=True).load_state_dict(sd)
