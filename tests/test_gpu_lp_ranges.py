"""rpo_lp_head_fwd_bwd (rpo_amd/csrc/lp_head.hip) in the linear probe's own regime, stage by stage against float64.

tests/test_gpu_lp.py draws N(0, 1) features and W = 0.01 I: logits are O(1) and the comparison is max |err| / max |ref|
over a whole tensor.  The probe itself runs on UN-normalised image features (norm about 10), W near the identity and a
logit scale of 100: logits reach the hundreds, every softmax row is one-hot and the loss m + log s - logit_label is a
difference of numbers in the hundreds.  Here every element of z, logits, dz, g_w and g_bias, and the loss, is held to a
budget of its own (helpers.assert_within), and each stage's float64 reference is formed from the kernel's own output
of the stage before, read back from the device, so a stage answers for its own roundings only.

Budgets: F32_OUT, U32 and FLOOR are test_gpu_ranges.py's.  The loss and dz budgets are written out in _loss_ref /
_dz_ref from the roundings lp_logits_kernel / lp_dz_kernel perform; with those of the library functions taken as
expf, logf <= 2 ulp = 4 U32 relative (the HIP math library documents 1 ulp for both)."""
import math

import pytest
import torch

from helpers import U32, assert_within
from test_gpu_ranges import F32_OUT, FLOOR

pytestmark = pytest.mark.gpu

SCALE = 100.0
LP_WAVES = 8                                   # split-k partials summed in wave order (lp_reduce)
ULP2 = 4 * U32                                 # a library function good to 2 ulp, relative
CASES = [(1, 1, 32), (3, 2, 96), (33, 33, 32), (128, 19, 512), (100, 1000, 1024), (5, 4097, 768), (128, 37, 1024)]
F0 = FLOOR["f32"]


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def _inputs(B, C, e, seed=0):
    """fp32 inputs as float64 (the values the kernel reads) and the labels.  The image rows lie along G = min(B, C / 2)
    directions; class c < 2 G has cosine +0.35 (c / G even) or -0.35 (odd) with the z of image c % G, so every image has
    a logit near +350 and, where C >= 2, one near -350; the other classes' cosines are uniform in +-0.3."""
    g = torch.Generator().manual_seed(seed * 7919 + B * 10007 + C * 31 + e)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    G = max(1, min(B, C // 2))
    dirs = _unit(rn(G, e))
    x = (10.0 * dirs[torch.arange(B) % G] + 0.3 * rn(B, e)).float().double()
    w = (torch.eye(e, dtype=torch.float64) + 0.02 * rn(e, e) / math.sqrt(e)).float().double()
    bias = (0.05 * rn(e)).float().double()
    zh = _unit(x @ w.t() + bias)
    c = torch.arange(C)
    a = torch.where(c < 2 * G, torch.where((c // G) % 2 == 0, 0.35, -0.35).double(),
                    torch.rand(C, generator=g, dtype=torch.float64) * 0.6 - 0.3)
    zc = zh[c % G]
    n = rn(C, e)
    n = _unit(n - (n * zc).sum(-1, keepdim=True) * zc)
    t = _unit(a[:, None] * zc + (1 - a * a).sqrt()[:, None] * n).float().double()
    logits = SCALE * ((x @ w.t() + bias) @ t.t())
    label = torch.randint(0, C, (B,), generator=g)
    b = torch.arange(B)
    label = torch.where(b % 3 == 0, logits.argmin(1), torch.where(b % 3 == 1, logits.argmax(1), label))
    loss = torch.nn.functional.cross_entropy(logits, label)
    # the regime, from float64 alone
    assert float(x.norm(dim=1).min()) > 9.0 and float(logits.abs().max()) > 200.0, (B, C, e)
    if B >= 3:
        assert float(loss) > 50.0, (B, C, e, float(loss))
    if C >= 2:
        assert float((torch.softmax(logits, 1).amax(1) > 0.99).double().mean()) > 0.5      # mostly one-hot rows
    return dict(x=x, w=w, bias=bias, t=t, label=label)


def _row_stats(L):
    """m, s = sum exp(L - m), d = m - L >= 0 of every row, and the relative budget rho of the kernel's s.  Class c
    enters s as expf(L - m_tile) (argument rounded: U32 (m_tile - L); expf: ULP2) times expf(m_tile - m) (argument:
    U32 (m - m_tile); expf: ULP2) with one rounding of the product: (2 ULP2 + U32 + U32 d_c) of its term, the two
    arguments adding up to d_c.  The terms are summed by a 5-level butterfly inside a tile and in order over the
    ceil(C / 32) tiles: (5 + tiles) U32 of s.  A term below 2^-126 may be flushed: C * FLOOR of s >= 1."""
    m = L.amax(1, keepdim=True)
    d = m - L
    ex = torch.exp(-d)
    s = ex.sum(1, keepdim=True)
    tiles = (L.shape[1] + 31) // 32
    rho = (ex * (2 * ULP2 + U32 + U32 * d)).sum(1, keepdim=True) / s + (5 + tiles) * U32 + L.shape[1] * F0
    return m, s, d, ex, rho


def _loss_ref(L, label):
    """Batch-mean cross-entropy of the device logits L (float64 of fp32) and its budget.  Row b: logf(s) errs by rho_b
    (the error of s, relative) + ULP2 |log s|; m + log s is rounded (U32 |m + log s|: an ulp of |m|, not of the loss) and
    so is the difference with logit_label (U32 |loss_b|, |loss_b| <= |m| + log s + |logit_label|).  The B rows are added
    in order ((B - 1) roundings of at most sum_b |loss_b|) and divided by B (one more)."""
    B = L.shape[0]
    m, s, _, _, rho = _row_stats(L)
    ll = L.gather(1, label[:, None])
    row = m + s.log() - ll
    e_row = rho + ULP2 * s.log().abs() + U32 * (m + s.log()).abs() + U32 * (m.abs() + s.log() + ll.abs())
    return row.mean(), float(e_row.sum() / B + B * U32 * row.abs().sum() / B)


def _dz_ref(L, t, label):
    """dz = G t, G = gmul (p - onehot), gmul = scale / B, from the device logits, with the budget of every element.
    p = expf(L - m) * (1 / s): expf ULP2 + its argument's rounding U32 d, the kernel's s (rho), the reciprocal and the
    product (2 U32): relative to p.  p - 1 on the label's class is rounded to an ulp of 1, not of the (e^-700) result:
    U32, absolute.  gmul is itself rounded and so is the product with it: 2 U32 |G|.  A p below 2^-126 may be flushed.
    The C-term sum: C roundings inside the waves' MFMA chains plus the LP_WAVES partials added in order."""
    B, C = L.shape
    _, s, d, ex, rho = _row_stats(L)
    p = ex / s
    onehot = torch.zeros_like(L)
    onehot[torch.arange(B), label] = 1.0
    gmul = SCALE / B
    G = gmul * (p - onehot)
    eG = gmul * (p * (ULP2 + U32 * d + rho + 2 * U32) + U32 * onehot + F0) + 2 * U32 * G.abs()
    return G @ t, eG @ t.abs() + (C + LP_WAVES) * U32 * (G.abs() @ t.abs()), G


def _check_stages(inp, z, logits, loss, dz, g_w, g_bias, what):
    """every stage against float64 of the stage before; returns {stage: worst err / budget}"""
    x, w, bias, t, label = (inp[k] for k in ("x", "w", "bias", "t", "label"))
    B = x.shape[0]
    worst = {}
    worst["z"] = assert_within(z, x @ w.t() + bias, F32_OUT * (x.abs() @ w.abs().t() + bias.abs()), what + " z")
    zd = z.double().cpu()
    worst["logits"] = assert_within(logits, SCALE * (zd @ t.t()), F32_OUT * SCALE * (zd.abs() @ t.abs().t()), what + " logits")
    Ld = logits.double().cpu()
    ref_loss, e_loss = _loss_ref(Ld, label)
    worst["loss"] = assert_within(loss, ref_loss.reshape(1), e_loss, what + " loss")
    ref_dz, e_dz, _ = _dz_ref(Ld, t, label)
    worst["dz"] = assert_within(dz, ref_dz, e_dz, what + " dz")
    dzd = dz.double().cpu()
    # k = b in order through the MFMA chain (g_w) or a scalar loop (g_bias): B roundings, doubled as the issue states it
    worst["g_w"] = assert_within(g_w, dzd.t() @ x, 2 * B * U32 * (dzd.abs().t() @ x.abs()), what + " g_w", floor=F0)
    worst["g_bias"] = assert_within(g_bias, dzd.sum(0), 2 * B * U32 * dzd.abs().sum(0), what + " g_bias", floor=F0)
    return worst


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("B,C,e", CASES)
def test_lp_head_stages_at_scale_100(B, C, e):
    """z, logits, loss, dz (the first B e workspace floats), g_w and g_bias, each against float64 of the device's previous
    stage, at |logit| up to ~400 and losses in the hundreds; every output and the workspace NaN-filled first.  e = 32
    leaves half of the split-k waves with an empty range, C = 1 / 2 leaves seven of the class waves empty, C = 4097
    has a last class tile of one class, B = 128 and e = 1024 are the contract's maxima.  Eval (label NULL) leaves loss
    and gradients alone; a second call repeats the bits; a bad label (-1, C, 2^40) on row B - 1 (and row 40) gives a NaN
    loss and all-NaN gradients.
    Measured worst err / budget (MI355X): z 0.010, logits 0.001, loss 0.146, dz 0.076, g_w 0.249, g_bias 0.125."""
    from rpo_amd import ops
    dev = torch.device("cuda:0")
    inp = _inputs(B, C, e)
    f = lambda a: a.float().to(dev).contiguous()
    xd, wd, bd, td, ld = f(inp["x"]), f(inp["w"]), f(inp["bias"]), f(inp["t"]), inp["label"].to(dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    nws = ops.lp_head_workspace_floats(B, C, e)
    assert nws == B * e + 2 * ((C + 31) // 32) * B

    def run(label):
        z, logits, ws = nan(B, e), nan(B, C), nan(nws)
        loss, g = torch.full((1,), -7.0, device=dev), torch.full((e * e + e,), -3.0, device=dev)
        if label is not None:
            loss.fill_(float("nan")); g.fill_(float("nan"))
        ops.lp_head_fwd_bwd(xd, wd, bd, td, label, SCALE, z, logits, loss, g[:e * e].view(e, e), g[e * e:], ws)
        torch.cuda.synchronize()
        return z, logits, loss, g, ws

    z0, l0, loss0, g0, _ = run(None)
    assert float(loss0) == -7.0 and bool((g0 == -3.0).all()), "eval wrote the loss or a gradient"
    z, logits, loss, g, ws = run(ld)
    assert torch.equal(_bits(z0), _bits(z)) and torch.equal(_bits(l0), _bits(logits)), "eval and training logits differ"
    worst = _check_stages(inp, z, logits, loss, ws[:B * e].view(B, e), g[:e * e].view(e, e), g[e * e:], f"lp B{B} C{C} e{e}")
    print(f"[lp head B{B} C{C} e{e}] loss {loss.item():.4f}; worst err / budget "
          + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    again = run(ld)
    for a, b, name in zip((z, logits, loss, g, ws[:B * e]), (again[0], again[1], again[2], again[3], again[4][:B * e]),
                          ("z", "logits", "loss", "g", "dz")):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: a second call gives other bits"
    rows = [B - 1] + ([40] if B > 40 else [])
    for row in rows:
        for badv in (-1, C, 2 ** 40):
            bad = ld.clone()
            bad[row] = badv
            _, lg, lossb, gb, _ = run(bad)
            assert torch.equal(_bits(lg), _bits(logits))
            assert torch.isnan(lossb).all() and torch.isnan(gb).all(), (row, badv, "the guarded step would not trip")


def test_lp_head_refusals():
    """e 16 / 48 / 1056, B 129 -> RPO_E_SHAPE; a z off the 16-byte grid -> RPO_E_ALIGN; nothing is written.  (The
    buffers are large enough for every size asked for.)"""
    from rpo_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    Bm, Cm, em = 129, 8, 1056
    x, w, bias, t = (torch.zeros(n, device=dev) for n in (Bm * em, em * em, em, Cm * em))
    label = torch.zeros(Bm, dtype=torch.int64, device=dev)
    outs = [torch.full((n,), 5.0, device=dev) for n in (Bm * em + 4, Bm * Cm, 1, em * em, em, Bm * em + 2 * Bm)]
    z, logits, loss, g_w, g_b, ws = outs

    def call(B, e, zoff=0):
        return lib.rpo_lp_head_fwd_bwd(x.data_ptr(), w.data_ptr(), bias.data_ptr(), t.data_ptr(), label.data_ptr(), SCALE,
                                       z.data_ptr() + zoff, logits.data_ptr(), loss.data_ptr(), g_w.data_ptr(),
                                       g_b.data_ptr(), B, Cm, e, ws.data_ptr(), s)
    for B, e in ((4, 16), (4, 48), (4, 1056), (129, 64)):
        assert call(B, e) == -2, (B, e)
    assert call(4, 64, zoff=4) == -4
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 5.0).all())
