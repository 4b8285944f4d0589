"""rpo_optim_step_sets and the trainers that use it, on the device (rpo_amd/csrc/optim.hip, rpo_amd/optim.py).

"Matches torch" everywhere below is ONE rule, with torch itself as the yardstick: for the same inputs torch.optim runs on
the CPU once in float32 and once in float64, E_ref = max |x32 - x64|, and the kernel's result must lie within
max(4 E_ref, 4 * 2^-24 * max |x64|) of the float64 run.  Nothing can be bit-identical to torch (fma contraction, the lerp
form); 4 allows a few rounding-order changes of the size of torch's own, the second term is the floor of one fp32
rounding.  E_ref comes from torch alone, never from the code under test.  Every comparison prints err / E_ref.
"""
import os

import numpy as np
import pytest
import torch

import test_gpu_multi as M
from helpers import workload
from rpo_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEG0, SEG1, STRIDE = 37, 29, 80                     # odd lengths, padded rows
N = SEG0 + SEG1
same, bits = M.same, M.bits


# ------------------------------------------------------------------------------------------------------------ helpers
def _oc(name="sgd", **kw):
    from rpo_amd.trainer import OptimConfig
    return OptimConfig(name=name, warmup_epoch=0, lr_scheduler="constant", **kw)


def _torch_opt(oc, params, lr):
    kw = dict(lr=lr, weight_decay=oc.weight_decay)
    if oc.name == "sgd":
        return torch.optim.SGD(params, momentum=oc.momentum, dampening=oc.sgd_dampening, nesterov=oc.sgd_nesterov, **kw)
    if oc.name == "rmsprop":
        return torch.optim.RMSprop(params, momentum=oc.momentum, alpha=oc.rmsprop_alpha, **kw)
    cls = torch.optim.AdamW if oc.name == "adamw" else torch.optim.Adam
    return cls(params, betas=(oc.adam_beta1, oc.adam_beta2), amsgrad=oc.name == "amsgrad", **kw)


class TorchPair:
    """torch.optim on the CPU over one flat parameter vector, in float32 and in float64, fed the same fp32 gradients."""

    def __init__(self, oc, p0: torch.Tensor, lr: float):
        self.oc = oc
        self.p = [torch.nn.Parameter(p0.detach().cpu().to(dt).clone()) for dt in (torch.float32, torch.float64)]
        self.opt = [_torch_opt(oc, [q], lr) for q in self.p]

    def step(self, g: torch.Tensor, lr=None):
        for q, o in zip(self.p, self.opt):
            if lr is not None:
                o.param_groups[0]["lr"] = lr
            q.grad = g.detach().cpu().to(q.dtype).clone()
            o.step()

    def state(self, key):
        out = []
        for q, o in zip(self.p, self.opt):
            st = o.state[q]
            out.append(st[key].detach() if key in st else torch.zeros_like(q))
        return out


def check(got: torch.Tensor, x32: torch.Tensor, x64: torch.Tensor, what: str, ratios=None) -> None:
    """The tolerance rule of the module docstring."""
    got, x32, x64 = got.detach().cpu().double().reshape(-1), x32.detach().double().reshape(-1), x64.detach().reshape(-1)
    e_ref = float((x32 - x64).abs().max())
    bound = max(4.0 * e_ref, 4.0 * 2.0 ** -24 * float(x64.abs().max()))
    err = float((got - x64).abs().max())
    ratio = err / e_ref if e_ref > 0 else (0.0 if err == 0 else float("inf"))
    print(f"[optim] {what}: err {err:.3e} E_ref {e_ref:.3e} err/E_ref {ratio:.2f} bound {bound:.3e}")
    if ratios is not None:
        ratios.append(ratio)
    assert torch.isfinite(got).all() and err <= bound, f"{what}: err {err:.3e} > bound {bound:.3e} (E_ref {e_ref:.3e})"


def _used_idx(u0, u1):
    return torch.cat([torch.arange(0, u0), torch.arange(SEG0, SEG0 + u1)])


class Sets:
    """Device buffers of `sets` sets of the odd shape, with per-set configs; NaN-free padding that must never change."""

    def __init__(self, ocs, lrs, gss, used=None, seed=0):
        from rpo_amd import optim
        S = self.S = len(ocs)
        g = torch.Generator().manual_seed(seed)
        self.ocs, self.lrs, self.gss = ocs, lrs, gss
        self.p = (0.1 * torch.randn(S, STRIDE, generator=g)).to(DEV)
        self.g = torch.zeros(S, STRIDE, device=DEV)
        self.s0, self.s1, self.s2 = (torch.zeros(S, STRIDE, device=DEV) for _ in range(3))
        self.kind = optim.kind_table(ocs).to(DEV)
        self.hyper = torch.tensor([optim.hyper_row(oc, lr, gs) for oc, lr, gs in zip(ocs, lrs, gss)],
                                  dtype=torch.float64).to(torch.float32).to(DEV)
        self.step = torch.zeros(S, dtype=torch.int32, device=DEV)
        self.used_host = used
        self.used = None if used is None else torch.tensor(used, dtype=torch.int32, device=DEV)
        self.p0 = self.p.clone()

    def idx(self, s):
        return _used_idx(*(self.used_host[s] if self.used_host is not None else (SEG0, SEG1)))

    def launch(self, found=None, g=None):
        from rpo_amd import ops
        ops.optim_step_sets(self.p, self.g if g is None else g, self.s0, self.s1, self.s2, self.kind, self.hyper, self.step,
                            SEG0, SEG1, used=self.used, found_inf=found, needs_s2=True)

    def untouched_outside_used(self):
        for s in range(self.S):
            mask = torch.ones(STRIDE, dtype=torch.bool)
            mask[self.idx(s)] = False
            assert same(self.p[s][mask], self.p0[s][mask]), f"set {s}: parameters outside the used ranges were written"
            for r in (self.s0, self.s1, self.s2):
                assert not bool(bits(r[s][mask]).any()), f"set {s}: a state row was written outside the used ranges"


def _grad(step, seed=0):
    """N(0, 1) scaled 1e-4 .. 1e2, cycling per step."""
    g = torch.Generator().manual_seed(1000 + 17 * step + seed)
    return torch.randn(4, STRIDE, generator=g) * 10.0 ** (-4 + step % 7)


KIND_CASES = {
    "sgd_nesterov": dict(name="sgd", sgd_nesterov=True),
    "sgd_dampening": dict(name="sgd", sgd_dampening=0.3),
    "adam": dict(name="adam"),
    "adamw": dict(name="adamw"),
    "amsgrad": dict(name="amsgrad"),
    "rmsprop_mom": dict(name="rmsprop", momentum=0.9),
    "rmsprop": dict(name="rmsprop", momentum=0.0),
}
STATE_KEYS = {"sgd": ("momentum_buffer", None, None), "adam": ("exp_avg", "exp_avg_sq", None),
              "adamw": ("exp_avg", "exp_avg_sq", None), "amsgrad": ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"),
              "rmsprop": ("momentum_buffer", "square_avg", None)}


def _per_set_configs(case, S):
    """A different `hyper` per set: rate, weight decay, momentum / betas / alpha, grad_scale (powers of two: gs * g is exact)."""
    base = KIND_CASES[case]
    lrs = [1e-3, 3e-3, 1e-2, 2e-3][:S]
    gss = [1.0, 0.5, 0.25, 1.0][:S]
    ocs = []
    for s in range(S):
        kw = dict(base, weight_decay=[0.0, 1e-3, 5e-4, 1e-2][s])
        if base["name"] in ("adam", "adamw", "amsgrad"):
            kw.update(adam_beta1=[0.9, 0.8, 0.95, 0.9][s], adam_beta2=[0.999, 0.99, 0.9995, 0.999][s])
        elif base["name"] == "rmsprop":
            kw.update(rmsprop_alpha=[0.99, 0.9, 0.95, 0.99][s])
            if base["momentum"] > 0:
                kw["momentum"] = [0.9, 0.5, 0.7, 0.9][s]
        else:
            kw["momentum"] = [0.9, 0.5, 0.7, 0.9][s]
            if base.get("sgd_dampening"):
                kw["sgd_dampening"] = [0.3, 0.1, 0.5, 0.3][s]
        ocs.append(_oc(**kw))
    return ocs, lrs, gss


# ---------------------------------------------------------------------------------------------- 1. matches torch, per kind
@pytest.mark.parametrize("form", ["elementwise", "guarded_used"])
@pytest.mark.parametrize("case", list(KIND_CASES))
def test_kernel_matches_torch_optim_per_kind(case, form):
    """12 steps, a different `hyper` per set, gradients N(0, 1) scaled 1e-4 .. 1e2 cycling per step, against torch.optim on
    the CPU by the tolerance rule: parameters and state rows (s2 for AMSGrad only).  elementwise: 3 sets, all elements;
    guarded_used: a 4th set with used = (20, 0), found_inf given.  Outside the used ranges nothing is written."""
    guarded = form == "guarded_used"
    S = 4 if guarded else 3
    ocs, lrs, gss = _per_set_configs(case, S)
    used = [[SEG0, SEG1]] * 3 + [[20, 0]] if guarded else None
    st = Sets(ocs, lrs, gss, used)
    found = torch.zeros(S, 2, dtype=torch.int32, device=DEV) if guarded else None
    refs = [TorchPair(ocs[s], st.p0[s].cpu()[st.idx(s)], lrs[s]) for s in range(S)]
    ratios = []
    for step in range(12):
        g = _grad(step)[:S]
        st.g.copy_(g)
        st.launch(found)
        for s in range(S):
            refs[s].step((g[s] * gss[s])[st.idx(s)])
    torch.cuda.synchronize()
    assert st.step.tolist() == [12] * S and (found is None or found.tolist() == [[0, 0]] * S)
    keys = STATE_KEYS[ocs[0].name]
    for s in range(S):
        ix = st.idx(s)
        check(st.p[s].cpu()[ix], refs[s].p[0], refs[s].p[1], f"{case} {form} set {s} p", ratios)
        for row, key in zip((st.s0, st.s1, st.s2), keys):
            if key is None or (key == "momentum_buffer" and ocs[s].name == "rmsprop" and ocs[s].momentum == 0):
                continue
            a32, a64 = refs[s].state(key)
            check(row[s].cpu()[ix], a32, a64, f"{case} {form} set {s} {key}", ratios)
    if ocs[0].name != "amsgrad":
        assert not bool(bits(st.s2).any()), "s2 belongs to AMSGrad alone"
    if ocs[0].name == "sgd":
        assert not bool(bits(st.s1).any()), "SGD has one state row"
    st.untouched_outside_used()
    print(f"[optim] {case} {form}: worst err / E_ref {max(ratios):.2f}")


# ------------------------------------------------------------------------------------------------ 2. SGD bit-identity
@pytest.mark.parametrize("guarded", [False, True], ids=["elementwise", "guarded"])
def test_plain_sgd_kind_is_rpo_sgd_step_sets_bit_for_bit(guarded):
    from rpo_amd import ops
    S = 4
    ocs = [_oc(momentum=m, weight_decay=w) for m, w in ((0.9, 5e-4), (0.8, 0.0), (0.0, 1e-3), (0.9, 1e-2))]
    lrs, gss = [0.01, 0.02, 0.005, 0.1], [1.0, 0.5, 1.0, 0.125]
    used = [[SEG0, SEG1], [20, 0], [SEG0, 11], [0, SEG1]]
    st = Sets(ocs, lrs, gss, used)
    p, buf = st.p0.clone(), torch.zeros_like(st.p0)
    hyper4 = torch.tensor([[lr, oc.momentum, oc.weight_decay, gs] for oc, lr, gs in zip(ocs, lrs, gss)],
                          dtype=torch.float64).to(torch.float32).to(DEV)
    f_new = torch.zeros(S, 2, dtype=torch.int32, device=DEV) if guarded else None
    f_old = torch.zeros(S, 2, dtype=torch.int32, device=DEV) if guarded else None
    for step in range(5):
        g = _grad(step).to(DEV)
        st.launch(f_new, g=g)
        ops.sgd_step_sets(p, g, buf, hyper4, SEG0, SEG1, first_step=(step == 0), used=st.used, found_inf=f_old)
        torch.cuda.synchronize()
        assert same(st.p, p) and same(st.s0, buf), f"step {step}"
    assert st.step.tolist() == [5] * S and not bool(bits(st.s1).any()) and not bool(bits(st.s2).any())
    assert not same(st.p, st.p0)
    st.untouched_outside_used()


# -------------------------------------------------------------------------------------------------- 3. skip semantics
def test_guarded_skip_is_per_set_and_leaves_the_counter():
    S = 3
    ocs, lrs, gss = _per_set_configs("adam", S)
    st = Sets(ocs, lrs, gss)
    found = torch.zeros(S, 2, dtype=torch.int32, device=DEV)
    refs = [TorchPair(ocs[s], st.p0[s].cpu()[st.idx(s)], lrs[s]) for s in range(S)]
    for step in range(6):
        g = _grad(step)[:S]
        if step == 2:                                              # the third launch: a NaN inside set 1's used range
            g[1, SEG0 + 5] = float("nan")
            before = [t.clone() for t in (st.p, st.s0, st.s1, st.step)]
        st.g.copy_(g)
        st.launch(found)
        torch.cuda.synchronize()
        for s in range(S):
            if not (step == 2 and s == 1):                         # torch: optimizer.step() is not called on a skipped step
                refs[s].step((g[s] * gss[s])[st.idx(s)])
        if step == 2:
            for now, was in zip((st.p, st.s0, st.s1), before):
                assert same(now[1], was[1]), "the skipped set was written"
                assert not same(now[0], was[0]) and not same(now[2], was[2]), "the other sets must step"
            assert st.step.tolist() == [3, 2, 3] and found.tolist() == [[0, 0], [1, 1], [0, 0]]
    assert st.step.tolist() == [6, 5, 6] and found.tolist() == [[0, 0], [0, 1], [0, 0]]
    for s in range(S):
        check(st.p[s].cpu()[st.idx(s)], refs[s].p[0], refs[s].p[1], f"skip: set {s} p")
        check(st.s1[s].cpu()[st.idx(s)], *refs[s].state("exp_avg_sq"), f"skip: set {s} exp_avg_sq")
    # ---- a NaN OUTSIDE the used range changes nothing and skips nothing
    used = [[SEG0, SEG1], [20, 0], [SEG0, SEG1]]
    runs = []
    for poison in (False, True):
        st = Sets(ocs, lrs, gss, used)
        found = torch.zeros(S, 2, dtype=torch.int32, device=DEV)
        for step in range(3):
            g = _grad(step)[:S]
            if poison:
                g[1, 25] = float("nan")                             # in segment 0 past used[1][0] = 20
                g[1, SEG0 + 3] = float("inf")                       # segment 1, of which set 1 uses nothing
                g[1, N + 2] = float("nan")                          # the row's padding
            st.g.copy_(g)
            st.launch(found)
        torch.cuda.synchronize()
        assert found.tolist() == [[0, 0]] * S and st.step.tolist() == [3] * S
        st.untouched_outside_used()
        runs.append((st.p.clone(), st.s0.clone(), st.s1.clone()))
    assert all(same(a, b) for a, b in zip(*runs))


# --------------------------------------------------------------------------------------- 4. device counter under a graph
def test_one_captured_launch_replayed_equals_eager_launches():
    """Elementwise Adam (no found_inf): the counter lives on the device, so ONE captured launch serves steps 1 .. 5.  The
    graph has one branch (the update, then the one-thread-per-set counter advance)."""
    S = 3
    ocs, lrs, gss = _per_set_configs("adam", S)
    eager, graph = Sets(ocs, lrs, gss), Sets(ocs, lrs, gss)
    grads = [_grad(step)[:S].to(DEV) for step in range(5)]
    for g in grads:
        eager.g.copy_(g)
        eager.launch()
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        graph.launch()
    assert graph.step.tolist() == [0] * S, "a capture does not execute"
    for g in grads:
        graph.g.copy_(g)
        cg.replay()
    torch.cuda.synchronize()
    assert graph.step.tolist() == eager.step.tolist() == [5] * S
    for a, b in ((graph.p, eager.p), (graph.s0, eager.s0), (graph.s1, eager.s1)):
        assert same(a, b)
    assert not same(graph.p, graph.p0)


# ----------------------------------------------------------------------------------------------------- 5. argument checks
def test_refused_arguments_return_their_codes_and_touch_nothing():
    from rpo_amd import _lib
    lib = _lib.load()
    S = 3
    ocs, lrs, gss = _per_set_configs("amsgrad", S)
    st = Sets(ocs, lrs, gss)
    st.g.copy_(_grad(0)[:S])
    found = torch.zeros(S, 2, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    keep = [t.clone() for t in (st.p, st.g, st.s0, st.s1, st.s2, st.step, found)]
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()

    def call(p=P(st.p), g=P(st.g), s0=P(st.s0), s1=P(st.s1), s2=P(st.s2), stride=STRIDE, sets=S, kind=P(st.kind),
             hyper=P(st.hyper), step=P(st.step), seg0=SEG0, seg1=SEG1, needs=1, fi=None):
        return lib.rpo_optim_step_sets(p, g, s0, s1, s2, stride, sets, kind, hyper, step, None, seg0, seg1, needs, fi, stream)

    BAD, SHAPE = _lib.E_BADARG, _lib.E_SHAPE
    for fi in (None, P(found)):
        for kw in (dict(p=None), dict(g=None), dict(s0=None), dict(s1=None), dict(kind=None), dict(hyper=None), dict(step=None),
                   dict(s2=None, needs=1), dict(sets=0), dict(sets=-1), dict(seg0=0, seg1=0), dict(seg0=-1), dict(seg1=-3)):
            assert call(fi=fi, **kw) == BAD, kw
        for kw in (dict(stride=N - 1), dict(sets=65536), dict(seg0=2 ** 62, seg1=2 ** 62, stride=2 ** 62)):
            assert call(fi=fi, **kw) == SHAPE, kw
    torch.cuda.synchronize()
    for now, was in zip((st.p, st.g, st.s0, st.s1, st.s2, st.step, found), keep):
        assert same(now, was)
    # an unknown kind cannot be seen by the host: the set is ignored on the device, the others step
    st.kind.copy_(torch.tensor([3, 77, -1], dtype=torch.int32))
    for fi in (None, found):
        st.launch(fi)
    torch.cuda.synchronize()
    assert st.step.tolist() == [2, 0, 0] and found.tolist() == [[0, 0]] * S
    for now, was in zip((st.p, st.s0, st.s1, st.s2), keep[:1] + keep[2:5]):
        assert not same(now[0], was[0]) and same(now[1:], was[1:])


# ----------------------------------------------------------------------------------------------------- 6. through RPO
def _rpo_batch(cfg, B, step):
    return (torch.from_numpy(synth.images(cfg, B, seed=1234 + 10 * step)).to(DEV),
            torch.from_numpy(synth.labels(cfg, B, seed=4321 + 10 * step)).to(DEV))


@pytest.mark.parametrize("amp", [False, True], ids=["plain", "amp_skip"])
@pytest.mark.parametrize("name", ["adam", "adamw", "rmsprop"])
def test_rpo_steps_follow_torch_optim_on_the_engines_gradients(name, amp):
    """Depth 1, K = 4, batch 2, f32: after each of 4 steps the gradients the engine produced go to a CPU torch.optim on a
    copy of the initial prompts; the prompts match by the tolerance rule at every step.  amp: step 2's image holds an Inf --
    the step is skipped, and the trajectory continues as torch's does without it."""
    from rpo_amd.trainer import RPO
    cfg, sd, toks, tp, ip, _, _ = workload("d1_k4_b2")
    oc = _oc(name, lr=2e-3, weight_decay=1e-3 if name != "rmsprop" else 5e-4)
    tr = RPO(cfg, sd, toks, oc, DEV, torch.float32, batch_size=2, num_batches=10 ** 9, prompts=(tp, ip), amp=amp)
    assert tr._opt is not None
    ref = TorchPair(oc, tr.engine.params.cpu(), oc.lr)
    applied = 0
    for step in range(4):
        image, label = _rpo_batch(cfg, 2, step)
        poisoned = amp and step == 1
        if poisoned:
            image[1, 0, 5, 7] = float("inf")
        before = tr.engine.params.clone()
        tr.step_async(image, label)
        tr._join_side()
        torch.cuda.synchronize()
        g = tr.engine.grads.cpu()
        if poisoned:
            assert not bool(torch.isfinite(g).all()) and same(tr.engine.params, before) and tr._found_inf.tolist() == [1, 1]
        else:
            assert bool(torch.isfinite(g).all()) and not same(tr.engine.params, before)
            ref.step(g)
            applied += 1
        check(tr.engine.params, ref.p[0], ref.p[1], f"RPO {name} amp={amp} step {step + 1}")
    assert tr._opt.steps() == [applied] and applied == (3 if amp else 4)


# --------------------------------------------------------------------------------------------------- 7. through RPOSweep
def test_mixed_sweep_members_equal_their_standalone_runs(tmp_path):
    """Members (sgd, adam, adamw, rmsprop) with their own rates, the same prompts and batches, f32, 3 steps over an epoch
    boundary of a multi_step schedule.  The SGD member equals an all-SGD sweep's member bit for bit; every other member
    equals a standalone RPO with its config under the criterion of tests/test_gpu_sweep.py (prompts within SGD_TOL, loss
    within 1e-6 in f32).  ONE graph capture.  Then the checkpoints: a member's file is its standalone run's (each kind in
    torch's layout), and a fresh sweep that loads them continues bit for bit."""
    from rpo_amd import optim
    from rpo_amd.sweep import RPOSweep
    from rpo_amd.trainer import RPO, OptimConfig
    K, B, S = 8, 2, 4
    cfg, sd, toks = M._workload(2, K)
    sched = dict(max_epoch=4, lr_scheduler="multi_step", stepsize=(1,), gamma=0.5, warmup_epoch=0)
    ocs = [OptimConfig(lr=0.01, **sched), OptimConfig(name="adam", lr=1e-3, **sched),
           OptimConfig(name="adamw", lr=2e-3, weight_decay=1e-2, **sched), OptimConfig(name="rmsprop", lr=5e-4, **sched)]
    all_sgd = [ocs[0], OptimConfig(lr=0.02, **sched), OptimConfig(lr=0.005, **sched), OptimConfig(lr=0.01, momentum=0.8, **sched)]
    prompts = M._member(cfg, sd, 0, B)[0]

    def sweep(optims):
        members = [dict(prompts=prompts, K=K, optim=oc) for oc in optims]
        return RPOSweep(cfg, sd, toks, members=members, batch_size=B, device=DEV, act_dtype=torch.float32, num_batches=2)

    mixed, plain = sweep(ocs), sweep(all_sgd)
    assert type(mixed._opt) is optim.OptimState and type(plain._opt) is optim.PlainSGD
    solos = [RPO(cfg, sd, toks, ocs[s], DEV, torch.float32, batch_size=B, num_batches=2, prompts=prompts) for s in range(1, S)]
    lrs = []
    for step in range(3):
        im, lb = M._member(cfg, sd, 0, B, step)[1:]
        im, lb = torch.from_numpy(im).to(DEV), torch.from_numpy(lb).to(DEV)
        image, label = im.repeat(S, 1, 1, 1).contiguous(), lb.repeat(S).contiguous()
        lrs.append(tuple(mixed.lr))
        loss = mixed.step_async(image, label).clone()
        mixed._loop_advance()
        plain.step_async(image, label)
        plain._loop_advance()
        torch.cuda.synchronize()
        assert same(mixed.engine.m_params[0], plain.engine.m_params[0]) and same(mixed.engine.m_mom[0], plain.engine.m_mom[0]), \
            f"step {step + 1}: the SGD member of a mixed sweep"
        assert float(loss[0]) == float(plain.engine.m_loss[0])
        for s, solo in enumerate(solos, start=1):
            assert solo.lr == lrs[-1][s]                          # (the rate this step runs at)
            l1 = solo.step_async(im, lb).clone()
            solo._join_side()
            solo._loop_advance()
            torch.cuda.synchronize()
            ep = float((mixed.engine.m_params[s] - solo.engine.params).abs().max())
            el = abs(float(loss[s]) - float(l1))
            print(f"[optim sweep] step {step + 1} member {s} ({ocs[s].name}): prompts err {ep:.2e} loss err {el:.2e}")
            assert ep <= M.SGD_TOL["f32"], f"step {step + 1} member {s}: prompts differ by {ep:.3e}"
            assert el <= 1e-6
    assert lrs[0] == lrs[1] and lrs[2] == tuple(0.5 * v for v in lrs[0]) and mixed.epoch == 1
    assert mixed.captures == 1
    assert mixed._opt.steps() == [3] * S
    # ---- checkpoints
    from rpo_amd.trainer import load_checkpoint_file
    dirs = [str(tmp_path / f"m{s}") for s in range(S)]
    paths = mixed.save_model(dirs)
    keys = [set(load_checkpoint_file(p)["optimizer"]["state"][0]) for p in paths]
    assert keys == [{"momentum_buffer"}, {"step", "exp_avg", "exp_avg_sq"}, {"step", "exp_avg", "exp_avg_sq"},
                    {"step", "square_avg", "momentum_buffer"}]
    for s, solo in enumerate(solos, start=1):                          # a standalone run reads its member's file
        solo.load_model(dirs[s], epoch=1)
        assert solo._opt.steps() == [3] and same(solo._opt.s0[0], mixed._opt.s0[s]) and same(solo._opt.s1[0], mixed._opt.s1[s])
    fresh = sweep(ocs)
    fresh.load_model(dirs, epoch=1)
    assert fresh.epoch == 1 and fresh.lr == mixed.lr and fresh._opt.steps() == [3] * S
    for tr in (mixed, fresh):
        tr.step_async(image, label)
    torch.cuda.synchronize()
    for k in ("m_params", "m_mom"):
        assert same(getattr(fresh.engine, k), getattr(mixed.engine, k)), k
    assert same(fresh._opt.s1, mixed._opt.s1)


# ------------------------------------------------------------------------------------------------ 8. through CoOp and LP
def test_coop_and_lp_adam_steps_follow_torch_optim():
    from rpo_amd.config import vit_b16
    from rpo_amd.coop import CoOp
    from rpo_amd.lp import LP
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    oc = _oc("adam", lr=2e-3, weight_decay=5e-4)
    # ---- CoOp: 4 generic context vectors
    g = dict(np.load(os.path.join(gold, "ref_coop_d2_b3_ctx4.npz")))
    cfg = vit_b16(layers_v=2, layers_t=2, K=1)
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    tr = CoOp(sd, g["tokenized_prompts"], 4, oc, DEV, torch.float32, batch_size=3, num_batches=10 ** 9, ctx=g["ctx"])
    ref = TorchPair(oc, tr.engine.coop_params.cpu(), oc.lr)
    for step in range(3):
        im, lb = synth.images(cfg, 3, seed=70 + step), synth.labels(cfg, 3, seed=80 + step)
        tr.forward_backward({"img": torch.from_numpy(im), "label": torch.from_numpy(lb)})
        torch.cuda.synchronize()
        ref.step(tr.engine.coop_grads.cpu())
        check(tr.engine.coop_params, ref.p[0], ref.p[1], f"CoOp adam step {step + 1}")
    assert tr._opt.steps() == [3]
    # ---- LP: lp_layer [e, e] + [e]
    gl = np.load(os.path.join(gold, "ref_lp_d2_b3.npz"))
    toks = gl["tokenized_prompts"]
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist(), logit_scale=float(np.log(100.0)))
    tr = LP(sd, toks, oc, DEV, torch.float32, batch_size=3, num_batches=10 ** 9, cfg=cfg, max_batch=3)
    ref = TorchPair(oc, tr.engine.lp_params.cpu(), oc.lr)
    for step in range(3):
        im, lb = synth.images(cfg, 3, seed=1000 + step), synth.labels(cfg, 3, seed=1100 + step)
        tr.forward_backward({"img": torch.from_numpy(im), "label": torch.from_numpy(lb)})
        torch.cuda.synchronize()
        ref.step(tr.engine.lp_grads.cpu())
        check(tr.engine.lp_params, ref.p[0], ref.p[1], f"LP adam step {step + 1}")
    assert tr._opt.steps() == [3]


# -------------------------------------------------------------------------------------------------------------- 9. resume
def test_rpo_adam_resume_is_the_uninterrupted_run_and_the_file_loads_into_torch(tmp_path):
    from rpo_amd.trainer import RPO, OptimConfig, load_checkpoint_file
    cfg, sd, toks, tp, ip, _, _ = workload("d1_k4_b2")
    oc = OptimConfig(name="adam", lr=2e-3, max_epoch=5, warmup_epoch=1, warmup_type="linear", lr_scheduler="cosine")
    mk = lambda: RPO(cfg, sd, toks, oc, DEV, torch.float32, batch_size=2, num_batches=2, prompts=(tp, ip))
    batch = lambda step: {"img": torch.from_numpy(synth.images(cfg, 2, seed=1234 + 10 * step)),
                          "label": torch.from_numpy(synth.labels(cfg, 2, seed=4321 + 10 * step))}
    a = mk()
    for step in range(4):                                           # 2 epochs of 2 steps
        a.forward_backward(batch(step))
    assert a.epoch == 2
    path, lr_saved = a.save_model(str(tmp_path)), a.lr
    for step in range(4, 6):
        a.forward_backward(batch(step))
    a._join_side()
    torch.cuda.synchronize()
    b = mk()
    b.load_model(str(tmp_path), epoch=2)
    assert b.epoch == 2 and b.lr == lr_saved and 0 < lr_saved < oc.lr and b._opt.steps() == [4]
    for step in range(4, 6):
        b.forward_backward(batch(step))
    b._join_side()
    torch.cuda.synchronize()
    assert same(a.engine.params, b.engine.params) and same(a._opt.s0, b._opt.s0) and same(a._opt.s1, b._opt.s1)
    assert a._opt.steps() == b._opt.steps() == [6]
    # ---- the file's optimizer entry is torch.optim.Adam's own
    ck = load_checkpoint_file(path)
    params = [torch.nn.Parameter(ck["state_dict"][k].clone()) for k in ("text_prompt", "img_prompt")]
    opt = torch.optim.Adam(params, lr=oc.lr, weight_decay=oc.weight_decay)
    opt.load_state_dict(ck["optimizer"])
    st = opt.state_dict()["state"]
    assert float(st[0]["step"]) == float(st[1]["step"]) == 4.0 and st[0]["step"].dtype == torch.float32
    assert tuple(st[0]["exp_avg"].shape) == (cfg.K, cfg.d_t) and tuple(st[1]["exp_avg_sq"].shape) == (cfg.K, cfg.d_v)
    assert opt.state_dict()["param_groups"][0]["betas"] == (0.9, 0.999)
    # a file without matching state (an SGD run's) loads weights only
    c = RPO(cfg, sd, toks, OptimConfig(lr=2e-3, max_epoch=5), DEV, torch.float32, batch_size=2, num_batches=2, prompts=(tp, ip))
    c.forward_backward(batch(0))
    c.save_model(str(tmp_path / "sgd"), epoch=0)
    d = mk()
    d.load_model(str(tmp_path / "sgd"), epoch=0)
    assert d._opt.steps() == [0] and not bool(bits(d._opt.s1).any()) and same(d.engine.params, c.engine.params)


# ------------------------------------------------------------------------- 10. RPOMulti, and resume of the other trainers
def test_multi_adam_members_equal_standalone_runs_and_resume_bit_for_bit(tmp_path):
    """RPOMulti with one shared Adam config (the flat buffer is one set): every member equals a standalone RPO with that
    config under the criterion of tests/test_gpu_multi.py (prompts within SGD_TOL in f32); ONE capture across an epoch
    boundary; save_model -> a fresh trainer's load_model -> one more step is the uninterrupted run bit for bit, and a
    member's file is a standalone RPO's (torch.optim.Adam's layout)."""
    from rpo_amd.multi import RPOMulti
    from rpo_amd.trainer import RPO, OptimConfig, load_checkpoint_file
    K, B, S = 8, 2, 2
    cfg, sd, toks = M._workload(2, K)
    oc = OptimConfig(name="adam", lr=1e-3, max_epoch=4, lr_scheduler="single_step", stepsize=(1,), gamma=0.5, warmup_epoch=0)
    prompts = [M._member(cfg, sd, s, B)[0] for s in range(S)]
    mk = lambda: RPOMulti(cfg, sd, toks, n_runs=S, batch_size=B, prompts=prompts, optim=oc, device=DEV,
                          act_dtype=torch.float32, num_batches=2)
    tr = mk()
    solos = [RPO(cfg, sd, toks, oc, DEV, torch.float32, batch_size=B, num_batches=2, prompts=prompts[s]) for s in range(S)]

    def batch(step):
        ims, lbs = zip(*[M._member(cfg, sd, s, B, step)[1:] for s in range(S)])
        return torch.from_numpy(np.concatenate(ims)).to(DEV), torch.from_numpy(np.concatenate(lbs)).to(DEV)

    for step in range(3):
        image, label = batch(step)
        tr.step_async(image, label)
        tr._loop_advance()
        for s, solo in enumerate(solos):
            solo.step_async(image[s * B:(s + 1) * B].contiguous(), label[s * B:(s + 1) * B].contiguous())
            solo._join_side()
            solo._loop_advance()
        torch.cuda.synchronize()
        for s, solo in enumerate(solos):
            ep = float((tr.engine.m_params[s] - solo.engine.params).abs().max())
            print(f"[optim multi] step {step + 1} member {s}: prompts err {ep:.2e}")
            assert ep <= M.SGD_TOL["f32"]
    assert tr.captures == 1 and tr.epoch == 1 and tr._opt.steps() == [3]
    dirs = [str(tmp_path / f"m{s}") for s in range(S)]
    paths = tr.save_model(dirs)
    ck = load_checkpoint_file(paths[1])
    st = ck["optimizer"]["state"]
    assert float(st[0]["step"]) == 3.0 and tuple(st[0]["exp_avg"].shape) == (K, cfg.d_t) and tuple(st[1]["exp_avg_sq"].shape) == (K, cfg.d_v)
    n, nt = tr.engine.m_params.shape[1], K * cfg.d_t
    assert same(st[1]["exp_avg_sq"].reshape(-1), tr._opt.s1[0, n + nt:2 * n])
    solos[1].load_model(dirs[1], epoch=1)                                   # a standalone RPO reads a member's file
    assert solos[1]._opt.steps() == [3] and same(solos[1]._opt.s0[0], tr._opt.s0[0, n:2 * n])
    image, label = batch(3)
    tr.step_async(image, label)
    b = mk()
    b.load_model(dirs, epoch=1)
    assert b.epoch == 1 and b.lr == tr.lr and b._opt.steps() == [3]
    b.step_async(image, label)
    torch.cuda.synchronize()
    assert same(b.engine.m_params, tr.engine.m_params) and same(b._opt.s0, tr._opt.s0) and same(b._opt.s1, tr._opt.s1)


def test_coop_and_lp_adam_resume_is_the_uninterrupted_run(tmp_path):
    from rpo_amd.config import vit_b16
    from rpo_amd.coop import CoOp
    from rpo_amd.lp import LP
    from rpo_amd.trainer import OptimConfig
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    oc = OptimConfig(name="amsgrad", lr=2e-3, max_epoch=5, lr_scheduler="multi_step", stepsize=(1, 2), gamma=0.5, warmup_epoch=0)
    cfg = vit_b16(layers_v=2, layers_t=2, K=1)
    g = dict(np.load(os.path.join(gold, "ref_coop_d2_b3_ctx4.npz")))
    sd = synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0)))
    gl = np.load(os.path.join(gold, "ref_lp_d2_b3.npz"))
    sd_lp = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(gl["tokenized_prompts"]).tolist(), logit_scale=float(np.log(100.0)))
    makers = {
        "coop": (lambda: CoOp(sd, g["tokenized_prompts"], 4, oc, DEV, torch.float32, batch_size=3, num_batches=1, ctx=g["ctx"]),
                 lambda t: t.engine.coop_params),
        "lp": (lambda: LP(sd_lp, gl["tokenized_prompts"], oc, DEV, torch.float32, batch_size=3, num_batches=1, cfg=cfg, max_batch=3),
               lambda t: t.engine.lp_params),
    }
    batch = lambda s: {"img": torch.from_numpy(synth.images(cfg, 3, seed=70 + s)), "label": torch.from_numpy(synth.labels(cfg, 3, seed=80 + s))}
    for name, (mk, params) in makers.items():
        a = mk()
        a.forward_backward(batch(0))
        a.forward_backward(batch(1))
        a.save_model(str(tmp_path / name))
        a.forward_backward(batch(2))
        b = mk()
        assert b.resume_model(str(tmp_path / name), epoch=2) == 2 and b.lr == oc.lr * 0.25 and b._opt.steps() == [2]
        b.forward_backward(batch(2))
        torch.cuda.synchronize()
        assert same(params(a), params(b)), name
        for r in ("s0", "s1", "s2"):
            assert same(getattr(a._opt, r), getattr(b._opt, r)), (name, r)
        assert a._opt.steps() == b._opt.steps() == [3]
