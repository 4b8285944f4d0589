"""rpo_lp_head_fwd_bwd_grouped (rpo_amd/csrc/lp_head.hip) against rpo_lp_head_fwd_bwd, bit for bit and group by group.

The ungrouped call is pinned to float64 stage by stage in tests/test_gpu_lp_ranges.py, in the probe's own regime (features
of norm about 10, W near the identity, scale 100); here the inputs are that test's, with a different layer per group, and
every group of the grouped call must give exactly the ungrouped call's bits on its slices -- so there is no tolerance.
The cases (S, B, C, e, row padding in floats) are the smallest that cross a 32-row tile (B = 33), a 32-class tile (C = 37,
65, 1000), a split-k wave with an empty range (e = 32), a padded row (4, 32) and the largest S (1024)."""
import math

import pytest
import torch

from test_gpu_lp_ranges import SCALE, _inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(1, 1, 1, 32, 0), (2, 33, 19, 32, 4), (3, 5, 65, 64, 0), (5, 32, 37, 512, 32), (2, 128, 1000, 512, 0),
         (1024, 2, 3, 32, 0)]
PAD = -3.0                                      # sentinel of everything the call must not write
GUARD = 64                                      # sentinel floats behind the small outputs


def _bits(t):
    return t.contiguous().view(torch.int32)


class Case:
    """Device inputs of one case: the shared img_f / text_f_n / label of _inputs(B, C, e), and S layers near the identity
    that DIFFER per group, in rows of `stride` = e e + e + pad floats whose padding is NaN (a read of it would show in the
    outputs), with one guard row behind the last group."""

    def __init__(self, S, B, C, e, pad):
        self.S, self.B, self.C, self.e, self.pad = S, B, C, e, pad
        self.n, self.stride = e * e + e, e * e + e + pad
        inp = _inputs(B, C, e)
        g = torch.Generator().manual_seed(S * 131 + B * 17 + C + e)
        f = lambda a: a.float().to(DEV).contiguous()
        self.x, self.t, self.label = f(inp["x"]), f(inp["t"]), inp["label"].to(DEV)
        w = inp["w"].float()[None] + 0.02 * torch.randn(S, e, e, generator=g) / math.sqrt(e)
        b = inp["bias"].float()[None] + 0.05 * torch.randn(S, e, generator=g)
        assert S == 1 or not torch.equal(w[0], w[-1])
        rows = torch.full((S + 1, self.stride), float("nan"))
        rows[:S, :e * e] = w.reshape(S, e * e)
        rows[:S, e * e:self.n] = b
        self.rows = rows.to(DEV)
        self.params = self.rows[:S]
        from rpo_amd import ops
        self.wsf = ops.lp_head_workspace_floats(B, C, e)

    def outputs(self):
        S, B, C, e = self.S, self.B, self.C, self.e
        full = lambda n: torch.full((n + GUARD,), PAD, device=DEV)
        o = dict(z=full(S * B * e), logits=full(S * B * C), loss=full(S), ws=full(S * self.wsf),
                 grads=torch.full((S + 1, self.stride), PAD, device=DEV))
        return o

    def views(self, o):
        S, B, C, e = self.S, self.B, self.C, self.e
        return (o["z"][:S * B * e].view(S, B, e), o["logits"][:S * B * C].view(S, B, C), o["loss"][:S], o["grads"][:S],
                o["ws"][:S * self.wsf])

    def grouped(self, label):
        from rpo_amd import ops
        o = self.outputs()
        z, logits, loss, grads, ws = self.views(o)
        ops.lp_head_fwd_bwd_grouped(self.x, self.params, self.t, label, SCALE, z, logits, None if label is None else loss,
                                    None if label is None else grads, ws)
        torch.cuda.synchronize()
        return o

    def ungrouped(self, label):
        """rpo_lp_head_fwd_bwd on every group's slices, written into tensors of the grouped call's shapes (computed once per
        label and shared by the checks)."""
        from rpo_amd import ops
        S, B, C, e, n = self.S, self.B, self.C, self.e, self.n
        z, logits = torch.full((S, B, e), PAD, device=DEV), torch.full((S, B, C), PAD, device=DEV)
        loss, g = torch.full((S,), PAD, device=DEV), torch.full((S, n), PAD, device=DEV)
        ws = torch.empty(self.wsf, device=DEV)
        for s in range(S):
            w, b = self.params[s, :e * e].view(e, e), self.params[s, e * e:n]
            if label is None:
                ops.lp_head_fwd_bwd(self.x, w, b, self.t, None, SCALE, z[s], logits[s], None, None, None, ws)
            else:
                ops.lp_head_fwd_bwd(self.x, w, b, self.t, label, SCALE, z[s], logits[s], loss[s:s + 1],
                                    g[s, :e * e].view(e, e), g[s, e * e:], ws)
        torch.cuda.synchronize()
        return z, logits, loss, g

    def untouched(self, o, what, train=True):
        """Padding floats, the guard row and the guards behind the small outputs keep their sentinels."""
        S, B, C, e, n = self.S, self.B, self.C, self.e, self.n
        for k, used in (("z", S * B * e), ("logits", S * B * C), ("loss", S if train else 0), ("ws", S * self.wsf)):
            assert bool((o[k][used:] == PAD).all()), f"{what}: {k} written past its end"
        gr = o["grads"]
        assert bool((gr[S] == PAD).all()), f"{what}: the guard row behind the last group's gradient was written"
        assert bool((gr[:S, n:] == PAD).all()), f"{what}: gradient padding written"
        if not train:
            assert bool((gr == PAD).all()), f"{what}: eval wrote a gradient"
        assert bool(torch.isnan(self.rows[S]).all() and torch.isnan(self.rows[:S, n:]).all()), f"{what}: params written"


def _equal_groups(case, o, ref, what, train=True):
    z, logits, loss, grads, _ = case.views(o)
    rz, rl, rloss, rg = ref
    e, n = case.e, case.n
    names = [("z", z, rz), ("logits", logits, rl)]
    if train:
        names += [("loss", loss, rloss), ("g_w", grads[:, :e * e], rg[:, :e * e]), ("g_bias", grads[:, e * e:n], rg[:, e * e:])]
    for name, a, b in names:
        same = (_bits(a) == _bits(b)).reshape(case.S, -1).all(1)
        assert bool(same.all()), f"{what}: {name} of groups {(~same).nonzero().flatten().tolist()[:8]} differ from rpo_lp_head_fwd_bwd"


@pytest.mark.parametrize("S,B,C,e,pad", CASES)
def test_every_group_has_the_bits_of_the_ungrouped_call(S, B, C, e, pad):
    """Training and eval: z, logits, loss, g_w, g_bias of every group `torch.equal` (as bits) to rpo_lp_head_fwd_bwd on that
    group's slices; padding, guard row and guards untouched; eval leaves loss and gradients alone; a second call repeats
    the bits; one label equal to C makes every group's loss NaN, with the ungrouped call's NaN mask in the gradients and
    its bits elsewhere."""
    case = Case(S, B, C, e, pad)
    what = f"S{S} B{B} C{C} e{e} pad{pad}"
    ref = case.ungrouped(case.label)
    assert bool(torch.isfinite(ref[2]).all()) and (S == 1 or C == 1 or not torch.equal(ref[1][0], ref[1][-1]))
    o = case.grouped(case.label)
    _equal_groups(case, o, ref, what)
    case.untouched(o, what)
    again = case.grouped(case.label)
    for k in ("z", "logits", "loss", "grads"):
        assert torch.equal(_bits(o[k]), _bits(again[k])), f"{what}: {k}: a second call gives other bits"
    # eval
    oe = case.grouped(None)
    _equal_groups(case, oe, case.ungrouped(None), what + " eval", train=False)
    case.untouched(oe, what + " eval", train=False)
    assert torch.equal(_bits(oe["z"]), _bits(o["z"])) and torch.equal(_bits(oe["logits"]), _bits(o["logits"]))
    # a bad label poisons every group (the labels are shared), as it poisons the ungrouped call
    bad = case.label.clone()
    bad[B - 1] = C
    rb = case.ungrouped(bad)
    ob = case.grouped(bad)
    _, lg, lossb, gb, _ = case.views(ob)
    assert bool(torch.isnan(lossb).all()) and bool(torch.isnan(rb[2]).all()), f"{what}: a bad label must give NaN losses"
    assert torch.equal(_bits(lg), _bits(rb[1]))
    gb = gb[:, :case.n]
    assert torch.equal(torch.isnan(gb), torch.isnan(rb[3])) and bool(torch.isnan(gb).any()), f"{what}: NaN masks"
    fin = ~torch.isnan(gb)
    assert torch.equal(_bits(gb)[fin], _bits(rb[3])[fin]), f"{what}: the finite rest of a poisoned gradient"
    case.untouched(ob, what + " bad label")


def test_replay_from_a_captured_graph_gives_the_eager_bits():
    """(2, 33, 19, 32, 4) captured on one stream and replayed twice over sentinel-filled outputs."""
    from rpo_amd import ops
    case = Case(2, 33, 19, 32, 4)
    eager = case.grouped(case.label)
    o = case.outputs()
    z, logits, loss, grads, ws = case.views(o)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        ops.lp_head_fwd_bwd_grouped(case.x, case.params, case.t, case.label, SCALE, z, logits, loss, grads, ws)
    for _ in range(2):
        for k in o:
            o[k].fill_(PAD)
        g.replay()
        torch.cuda.synchronize()
        for k in ("z", "logits", "loss", "grads"):
            assert torch.equal(_bits(o[k]), _bits(eager[k])), f"{k}: graph replay != eager"
        case.untouched(o, "replay")


def test_errors_give_their_codes_and_launch_nothing():
    """S = 0, S = 1025, set_stride = e e + e - 4 -> RPO_E_SHAPE; set_stride % 4 == 2, params off the 16-byte grid ->
    RPO_E_ALIGN; img_f NULL -> RPO_E_BADARG.  Every output keeps its sentinel.  (The buffers are large enough for every
    size asked for but S = 1025, which must be refused before anything is addressed.)"""
    from rpo_amd import _lib
    lib = _lib.load()
    S, B, C, e = 2, 4, 19, 32
    n = e * e + e
    case = Case(S, B, C, e, 8)
    o = case.outputs()
    z, logits, loss, grads, ws = case.views(o)
    st = torch.cuda.current_stream().cuda_stream

    def call(S=S, stride=case.stride, params=case.params.data_ptr(), img=case.x.data_ptr()):
        return lib.rpo_lp_head_fwd_bwd_grouped(img, params, stride, case.t.data_ptr(), case.label.data_ptr(), SCALE,
                                               z.data_ptr(), logits.data_ptr(), loss.data_ptr(), grads.data_ptr(), S, B, C, e,
                                               ws.data_ptr(), st)
    assert call(S=0) == _lib.E_SHAPE and call(S=1025) == _lib.E_SHAPE and call(stride=n - 4) == _lib.E_SHAPE
    assert call(stride=n + 2) == _lib.E_ALIGN and call(params=case.params.data_ptr() + 4) == _lib.E_ALIGN
    assert call(img=None) == _lib.E_BADARG
    torch.cuda.synchronize()
    for k, v in o.items():
        assert bool((v == PAD).all()), f"{k} was written by a refused call"
    assert call() == 0                                               # the same arguments, unbroken, do run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all())
