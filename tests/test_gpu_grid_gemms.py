"""The image-tower GEMMs at the row counts of the patch grids beyond 14 x 14 / 16 x 16, on the MI355X.

ViT-B/32 has 50 frozen rows per image: with K = 24 prompt rows a row unit is 74 rows, a third of the 224-row tile of the
one-round kernels (gemm_w4g.inc, gemm_w4k.inc), so that four of a tile's seven 32-row MFMA blocks hold no valid row
and the prompt rows sit in blocks 1 .. 2.  ViT-L/14 at 336 px has 577 + K rows per image, above every row-unit geometry:
its GEMMs get no hint and choose by shape, at B = 7 the 288x256 geometry with equal-height contiguous tiles.

Every operand a kernel reads by row lies inside a NaN-filled allocation (tests/test_gpu_attn_long.py: guarded / put) and
every output is NaN before the launch: a row the tile does not own that is read after all poisons a checked value, a
row that is not written stays NaN, a store outside the matrix breaks a guard.

Tolerances are those of the tests these cases extend: tests/test_gpu_ops.py's `close` with its per-mode TOL (1e-4 for
fp32 results of 16-bit products, 2e-5 for the statistics, 1.5 TOL for the LayerNorm fold against the unfolded float64
path) and tests/test_gpu_ranges.py's elementwise budgets (assert_within: F32_OUT of the k-sum over absolute values --
K 2^-24 where K > 1024 --, GLN for the statistics, _check_qgelu for the fold's consumer against float64 of exactly
what it reads).  The worst error / budget ratio of every case is printed.
"""
import pytest
import torch

import test_gpu_ops as TO
import test_gpu_ranges as TR
from helpers import U32, assert_within
from test_gpu_attn_long import guarded, guards_intact, put

pytestmark = pytest.mark.gpu

from oracle import rows_oracle as R  # noqa: E402  (checker only)

DT = TO.DT
MODES = ["bf16", "f16"]

# (n0, n1, units) on the 224-row geometries: ViT-B/32 at K = 24 / 4 / 48, a partial round (224 tiles), two rounds; one
# MFMA row block exactly and no prompt rows, both segments across a block edge, one row each
UNITS_224 = [(50, 24, 32), (50, 4, 32), (50, 48, 32), (50, 24, 28), (50, 24, 64), (32, 0, 32), (33, 31, 32), (1, 1, 32)]
# ... and one short unit on each 288-row geometry
UNITS_288 = [(50, 24, 16)]
# the units the engine really offers (ViT-B/32, K = 24, B = 32 / 28): the heuristic itself must pick the one-round kernels
ENGINE_UNITS = {(50, 24, 32), (50, 24, 28)}
GEO = {224: dict(d=768, Nf=3072, grp=96), 288: dict(d=1024, Nf=4096, grp=64), "288n768": dict(d=768, grp=64)}
CFC_CASES = [(224,) + u for u in UNITS_224] + [(288,) + u for u in UNITS_288]
RESID_CASES = [(224, K) + u for u in UNITS_224 for K in (768, 3072)] + [(288, K) + u for u in UNITS_288 for K in (1024, 4096)]
# ViT-B/32 at B = 18 .. 21: 8 B tiles of 96 columns leave a round of the 224x96 geometry too empty, 12 B tiles of 64
# columns do not -- the engine's units then get the 288x64 geometry at N = 768 (64-column statistics, hi / lo stream)
RESID_CASES += [("288n768", K, 50, 24, 20) for K in (768, 3072)]


def dev():
    return torch.device("cuda:0")


def lib():
    from rpo_amd import _lib as L
    return L


def bits(t):
    """the raw bits of a tensor (NaN == NaN)"""
    return t.detach().contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same(x, y):
    return torch.equal(bits(x), bits(y))


def f32_out(K):
    """fp32 result of a K-term sum of 16-bit products, relative to the sum over absolute values (TR.F32_OUT covers
    K <= 1024: K 2^-24 roundings at most)"""
    return max(TR.F32_OUT, K * U32)


class Outs:
    """NaN-filled, guarded outputs of one launch"""
    def __init__(self):
        self.views, self.wholes = {}, {}

    def new(self, name, rows, cols, dtype):
        self.views[name], self.wholes[name] = guarded(rows, cols, dtype)
        return self.views[name]

    def __getitem__(self, name):
        return self.views[name]

    def check(self, what, unwritten=()):
        """guards intact; every element written (finite), except the named (output, rows) that must still be NaN"""
        torch.cuda.synchronize()
        for name, whole in self.wholes.items():
            assert guards_intact(whole), f"{what}: a guard element of {name} was overwritten"
            v = self.views[name]
            lo = dict(unwritten).get(name, 0)
            assert bool(torch.isnan(v[:lo].float()).all()), f"{what}: rows of {name} below {lo} were written"
            bad = ~torch.isfinite(v[lo:].float())
            assert not bool(bad.any()), \
                f"{what}: {name} has {int(bad.sum())} NaN / Inf in rows it must write, first at {tuple(bad.nonzero()[0].tolist())}"


# ------------------------------------------------------------------------------------------------------------------
# the split-k residual kernel (tile_config 11) with short units: out-proj (K = d) and c_proj (K = 4 d)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geo,K,n0,n1,units", RESID_CASES, ids=[f"g{c[0]}-K{c[1]}-u{c[2]}_{c[3]}_{c[4]}" for c in RESID_CASES])
def test_short_units_residual_gemm(mode, geo, K, n0, n1, units):
    """224x96 / 288x64 split-k tiles of units far shorter than the tile, in the three forms the engine issues: fp32
    residual (no hi / lo stream), fp32 residual in and halves out (block 0: c_row0 = first prompt row), halves in and out
    (not in place, so that the inputs keep their guards, and in place).  C, the 16-bit copy, the lo half and the
    tile-width statistics against float64; the forms agree bit for bit; C below c_row0 stays NaN; the heuristic's own
    launch, the prefetch hint and ten repeats give the same bits; the generic 64x128 tiles agree to fp32 summation order."""
    o, L = TO.ops(), lib()
    dt = DT[mode]
    d, grp = GEO[geo]["d"], GEO[geo]["grp"]
    seg1 = n0 * units
    M = seg1 + n1 * units
    hint = (n0, n1, seg1)
    a, w, bias = TO.rnd((M, K), 1, 0.5), TO.rnd((d, K), 2, K ** -0.5), TO.rnd((d,), 3)
    r32 = TO.rnd((M, d), 4, 2.0) + 0.4
    hi = r32.to(dt)
    lo = (r32 - hi.float()).to(dt)
    resid = hi.float() + lo.float()                 # exactly what the halves decode to
    assert o.gemm_stats_group(M, d, K, dt, hint) == grp and o.gemm_hilo_ok(M, d, K, dt, hint, grp)
    (ad, _), (hid, hi_whole), (lod, lo_whole) = put(a, mode), put(hi, mode), put(lo, mode)
    rd, r_whole = guarded(M, d, torch.float32)
    rd.copy_(resid)
    wd, bd = w.to(dev(), dt), bias.to(dev())
    nxt = torch.zeros(4 * d * d, dtype=dt, device=dev())           # what a prefetch hint names: the next GEMM's weight

    def run(form, cfg=11, prefetch=None, group=grp, units_hint=hint, inplace=None):
        outs = Outs()
        c = outs.new("C", M, d, torch.float32)
        st = outs.new("ln_stats", M, d // group * 2, torch.float32).view(M, d // group, 2)
        kw = dict(bias=bd, ln_stats=st, ln_group=group, tile_config=cfg, row_units=units_hint, prefetch=prefetch)
        if inplace is not None:
            kw.update(out2=inplace[0], out_lo=inplace[1])
        else:
            kw["out2"] = outs.new("out2", M, d, dt)
            if form != "fp32":
                kw["out_lo"] = outs.new("out_lo", M, d, dt)
        if form == "hilo":
            kw.update(resid_hi=hid if inplace is None else inplace[0], resid_lo=lod if inplace is None else inplace[1])
        else:
            kw["resid"] = rd
        if form != "fp32":
            kw["c_row0"] = seg1
        if cfg in (0, 11):
            assert o.gemm_nt_plan(ad, wd, c, L.EPI_BIAS_RESID, **kw) == 11, "the split-k kernel does not take these units"
        o.gemm_nt(ad, wd, c, L.EPI_BIAS_RESID, **kw)
        outs.check(f"{form} cfg {cfg}", unwritten=() if form == "fp32" else (("C", seg1),))
        return outs

    what = f"[short units {mode} {geo} K{K} {hint}]"
    f = run("fp32")
    a64, w64 = TO.q(a, mode), TO.q(w, mode)
    ref = a64 @ w64.t() + bias.double() + resid.double()
    TO.close(f["C"], ref, "f32", what + " C", tol=1e-4)
    worst = assert_within(f["C"], ref, f32_out(K) * (a64.abs() @ w64.abs().t() + bias.double().abs() + resid.double().abs()),
                          what + " C")
    assert torch.equal(f["out2"].cpu(), f["C"].cpu().to(dt)), "out2 must be the RNE act-dtype copy of C"
    c64 = f["C"].double().cpu()
    ref_st, mag = TR._stats64(c64, grp)
    st = f["ln_stats"].view(M, d // grp, 2)
    TO.close(st, ref_st, "f32", what + f" {grp}-column statistics", tol=2e-5)
    dmu = TR.GLN * mag
    worst = max(worst, assert_within(st[..., 0], ref_st[..., 0], dmu, what + " means"),
                assert_within(st[..., 1], ref_st[..., 1], TR.GLN * ref_st[..., 1] + 4 * grp * dmu ** 2, what + " M2", floor=1e-30))
    # block 0's form and the hi / lo form: the same bits, C on the prompt rows only
    first, h = run("first"), run("hilo")
    for name, g in (("first", first), ("hilo", h)):
        assert same(g["C"][seg1:], f["C"][seg1:]) and same(g["out2"], f["out2"]) and same(g["ln_stats"], f["ln_stats"]), \
            f"{what} {name}: differs from the fp32-residual launch"
    assert same(first["out_lo"], h["out_lo"])
    rec = h["out2"].float() + h["out_lo"].float()
    # (fp16: lo of a small value is a subnormal, resolution 6e-8)
    bound = f["C"].abs() * (2.0 ** -15 if mode == "bf16" else 2.0 ** -19) + (0.0 if mode == "bf16" else 6e-8)
    assert bool(((rec - f["C"]).abs() <= bound).all()), f"{what} hi + lo off by {((rec - f['C']).abs() - bound).max().item():.2e}"
    # in place: the halves of the input are overwritten by the halves of the output
    (hh, hh_whole), (ll, ll_whole) = put(hi, mode), put(lo, mode)
    ip = run("hilo", inplace=(hh, ll))
    assert same(hh, h["out2"]) and same(ll, h["out_lo"]) and same(ip["C"], h["C"]) and same(ip["ln_stats"], h["ln_stats"])
    for whole in (hh_whole, ll_whole, hi_whole, lo_whole, r_whole):
        assert guards_intact(whole), f"{what}: a guard of the residual was overwritten"
    assert same(hid, hi.to(dev())) and same(lod, lo.to(dev())), "the residual halves of the not-in-place launch changed"
    # the heuristic's own launch, the prefetch hint, repeats
    for name, g in (("heuristic", run("hilo", cfg=0)), ("prefetch", run("hilo", prefetch=nxt))) + \
            tuple((f"repeat {i}", run("hilo")) for i in range(10)):
        for k in ("C", "out2", "out_lo", "ln_stats"):
            assert same(g[k], h[k]), f"{what} {name}: {k} differs"
    # the generic tiles agree to fp32 summation-order noise (their statistics are over 64 columns)
    gen = run("fp32", cfg=6, group=64, units_hint=None)
    TO.close(gen["C"], c64, "f32", what + " 64x128 tiles vs the split-k tiles", tol=2e-5)
    print(f"\n{what} worst err / budget {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------
# the 224x384 / 288x256 kernel (tile_config 10) with short units: c_fc and the in-proj form
# ------------------------------------------------------------------------------------------------------------------
def _fold_inputs(M, d, Nf, grp, mode):
    """the consumer's operands as Engine._fold forms them, and the statistics of the fp32 rows its 16-bit A was cut from"""
    dt = DT[mode]
    x = TO.rnd((M, d), 11, 2.0) + 0.4
    st64, _ = TR._stats64(x.double(), grp)
    w, b = TO.rnd((Nf, d), 12, d ** -0.5), TO.rnd((Nf,), 13)
    gamma, beta = TO.rnd((d,), 14, 0.1) + 1.0, TO.rnd((d,), 15, 0.05)
    wq = (w.double() * gamma.double()[None, :]).float().to(dt)
    s = wq.double().sum(1).float()
    bq = (b.double() + w.double() @ beta.double()).float()
    return x, st64.float(), w, b, gamma, beta, wq, s, bq


def _fold_refs(x, st, w, b, gamma, beta, wq, s, bq, mode, rows=None):
    """(a) float64 of exactly what the consumer reads, with its fp32 budget (tests/test_gpu_ranges.py), and (b) float64 of
    the unfolded LayerNorm + GEMM; on a subset of the rows if given"""
    d = x.shape[1]
    sel = slice(None) if rows is None else rows
    xq, wq64 = TO.q(x, mode)[sel], wq.double()
    mu, rstd = TR._fold_from_stats(st.double()[sel], d, d // st.shape[1])
    pre_a = rstd * (xq @ wq64.t() - mu * s.double()[None, :]) + bq.double()
    du_a = rstd * f32_out(d) * (xq.abs() @ wq64.abs().t() + (mu * s.double()[None, :]).abs()) + f32_out(d) * bq.double().abs() \
        + 8 * U32 * (pre_a - bq.double()).abs()
    ln, _, _ = TR.ln64(x.double()[sel], gamma.double(), beta.double())
    pre_b = ln @ w.double().t() + b.double()
    return pre_a, du_a, pre_b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geo,n0,n1,units", CFC_CASES, ids=[f"g{c[0]}-u{c[1]}_{c[2]}_{c[3]}" for c in CFC_CASES])
def test_short_units_c_fc(mode, geo, n0, n1, units):
    """224x384 / 288x256 tiles of units far shorter than the tile.  c_fc as the engine issues it (LayerNorm fold over the
    geometry's statistics group, QuickGELU, the saved derivative of the prompt rows in the act dtype) against float64 of
    what it reads and of the unfolded path; the bits of the 128x128 tiles, of the heuristic's own launch, with and
    without the prefetch hint and over ten repeats; the saved derivative through the kernel's separate pass (odd row
    stride); BIAS_QGELU with fp32 saved pre-activations; the in-proj form (LN_BIAS with a skipped rectangle)."""
    o, L = TO.ops(), lib()
    dt = DT[mode]
    d, Nf, grp = GEO[geo]["d"], GEO[geo]["Nf"], GEO[geo]["grp"]
    seg1 = n0 * units
    M = seg1 + n1 * units
    hint = (n0, n1, seg1)
    what = f"[short units c_fc {mode} {geo} {hint}]"
    x, st, w, b, gamma, beta, wq, s, bq = _fold_inputs(M, d, Nf, grp, mode)
    pre_a, du_a, pre_b = _fold_refs(x, st, w, b, gamma, beta, wq, s, bq, mode)
    xb, _ = put(x, mode)
    std, _ = guarded(M, d // grp * 2, torch.float32)
    std.copy_(st.view(M, -1))
    std = std.view(M, d // grp, 2)
    wqd, sd, bqd = wq.to(dev()), s.to(dev()), bq.to(dev())
    nxt = torch.zeros(4 * d * d, dtype=dt, device=dev())
    # the engine saves the prompt rows' derivative; without prompt rows it passes no aux and aux_row0 = M
    row0 = seg1 if n1 else M

    def run(cfg, units_hint, prefetch=None, pad=0, epi=L.EPI_LN_BIAS_QGELU, skip=None):
        outs = Outs()
        y = outs.new("y", M, Nf, dt)
        kw = dict(bias=bqd, ln_stats=std, ln_colsum=sd, ln_group=grp, tile_config=cfg, row_units=units_hint, prefetch=prefetch)
        if n1 and epi == L.EPI_LN_BIAS_QGELU:
            if pad == 0:
                outs.new("aux", M - row0, Nf, dt)
            else:
                outs.views["aux"] = TR.nan((M - row0, Nf + pad), dt)[:, :Nf]
            kw.update(aux=outs["aux"], aux_row0=row0)
        elif epi == L.EPI_LN_BIAS_QGELU:
            kw["aux_row0"] = row0
        if skip is not None:
            kw.update(skip_row0=skip[0], skip_col0=skip[1])
        plan = o.gemm_nt_plan(xb, wqd, y, epi, **kw)
        if cfg:
            assert plan == cfg, f"{what}: tile_config {cfg} is not taken (plan {plan})"
        o.gemm_nt(xb, wqd, y, epi, **kw)
        torch.cuda.synchronize()
        if skip is None:
            outs.check(f"cfg {cfg}")
        return outs, plan

    u, _ = run(10, hint)
    worst = TR._check_qgelu(u["y"], None, pre_a, du_a, TR.ULP[mode], what + " (a)", True)
    TO.close(u["y"], R.qgelu(pre_b), mode, what + " against the unfolded path", tol=1.5 * TO.TOL[mode])
    if n1:
        worst = max(worst, TR._check_qgelu(u["y"][row0:], u["aux"], pre_a[row0:], du_a[row0:], TR.ULP[mode], what + " (a)", True))
        TO.close(u["aux"], R.qgelu_grad(pre_b[row0:]), mode, what + " saved derivative", tol=1.5 * TO.TOL[mode])
    # (whatever the heuristic picks for the shape -- tile_config 10 on the engine's own units -- has the same k-order)
    variants = [("128x128", run(2, None)), ("heuristic", run(0, hint)), ("prefetch", run(10, hint, prefetch=nxt))] + \
        [(f"repeat {i}", run(10, hint)) for i in range(10)]
    for name, (g, plan) in variants:
        if name == "heuristic" and hint in ENGINE_UNITS:
            assert plan == 10, f"{what}: the heuristic runs tile_config {plan} on the engine's own units"
        assert same(g["y"], u["y"]), f"{what} {name}: y differs"
        if n1:
            assert same(g["aux"], u["aux"]), f"{what} {name}: the saved derivative differs"
    if n1:
        # a row stride of the saved derivative that sends the kernel down its separate pass: the same bits
        g, _ = run(10, hint, pad=4)
        assert same(g["y"], u["y"]) and same(g["aux"], u["aux"]), f"{what}: separate saved-derivative pass differs"
    # BIAS_QGELU with the pre-activations saved in fp32 (tests/test_gpu_ops.py's row-unit case), rows [r0, M)
    r0 = seg1 if n1 else max(M - 300, 0)
    pre = TO.q(x, mode) @ wq.double().t() + bq.double()
    res = {}
    for name, cfg, uh in (("units", 10, hint), ("128x128", 2, None)):
        outs = Outs()
        y, aux = outs.new("y", M, Nf, dt), outs.new("aux", M - r0, Nf, torch.float32)
        o.gemm_nt(xb, wqd, y, L.EPI_BIAS_QGELU, bias=bqd, aux=aux, aux_row0=r0, tile_config=cfg, row_units=uh)
        outs.check(f"BIAS_QGELU {name}")
        res[name] = outs
    TO.close(res["units"]["y"], R.qgelu(pre), mode, what + " BIAS_QGELU")
    TO.close(res["units"]["aux"], pre[r0:], mode, what + " saved u", tol=1e-4)
    assert same(res["units"]["y"], res["128x128"]["y"]) and same(res["units"]["aux"], res["128x128"]["aux"]), \
        f"{what}: BIAS_QGELU differs from the 128x128 tiles"
    # the in-proj form: LN_BIAS, the K / V columns of the prompt rows may be skipped -- whatever a kernel does with the
    # rectangle, it writes the right value there or nothing, and everything outside it is the unskipped launch's bits
    full, _ = run(2, None, epi=L.EPI_LN_BIAS)
    worst = max(worst, assert_within(full["y"], pre_a, du_a + TR.ULP[mode] * pre_a.abs(), what + " (a) LN_BIAS"))
    if n1:
        g, _ = run(10, hint, epi=L.EPI_LN_BIAS, skip=(seg1, d))
        assert guards_intact(g.wholes["y"])
        assert same(g["y"][:seg1], full["y"][:seg1]) and same(g["y"][:, :d], full["y"][:, :d]), \
            f"{what}: in-proj form differs outside the skipped rectangle"
        rect, want = g["y"][seg1:, d:], full["y"][seg1:, d:]
        assert bool((torch.isnan(rect.float()) | (bits(rect) == bits(want))).all()), f"{what}: a wrong value in the skipped rectangle"
    else:
        g, _ = run(10, hint, epi=L.EPI_LN_BIAS)
        assert same(g["y"], full["y"])
    print(f"\n{what} worst err / budget {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------
# the 288x256 geometry without row units (ViT-L/14 at 336 px, B = 7: c_fc at M = 7 x 601)
# ------------------------------------------------------------------------------------------------------------------
# (M, K, what the heuristic runs): 15 tiles of 281 rows (the last one 273); 14 tiles of 268 rows (the last one 261) --
# there 15 x 16 tiles of 256x256 fill one round, so the heuristic itself prefers tile_config 8 and the geometry is
# reached with tile_config = 10 only; 16 tiles of exactly 288 rows
NO_UNIT_CASES = [(4207, 1024, 10), (3745, 128, 8), (4608, 256, 10)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,K,auto", NO_UNIT_CASES)
def test_gemm_288x256_without_row_units(mode, M, K, auto):
    """tile_config 10 at N = 4096 with no hint: equal-height contiguous tiles of the 288x256 geometry (with units it is
    tested at (257, 24, 16) only; the other no-unit cases have N a multiple of 384 and get the 224x384 geometry).  BIAS,
    BIAS_QGELU and LN_BIAS_QGELU (K = 1024: 16 statistics groups, the admission edge) with the saved operand, against
    float64 and the bits of the 128x128 tiles, with the race screen of test_gemm_one_round_224x384_..."""
    o, L = TO.ops(), lib()
    dt = DT[mode]
    N = 4096
    what = f"[288x256 no units {mode} M{M} K{K}]"
    a, w, bias = TO.rnd((M, K), 1, 0.5), TO.rnd((N, K), 2, K ** -0.5), TO.rnd((N,), 3)
    acc = TO.q(a, mode) @ TO.q(w, mode).t()
    ad, _ = put(a, mode)
    wd, bd = w.to(dev(), dt), bias.to(dev())
    row0 = max(M - 800, 0)

    def launch(epi, cfg, **kw):
        outs = Outs()
        y = outs.new("y", M, N, dt)
        if epi != L.EPI_BIAS:
            kw.update(aux=outs.new("aux", M - row0, N, dt if epi == L.EPI_LN_BIAS_QGELU else torch.float32), aux_row0=row0)
        plan = o.gemm_nt_plan(ad, wd, y, epi, tile_config=cfg, **kw)
        o.gemm_nt(ad, wd, y, epi, tile_config=cfg, **kw)
        outs.check(f"{what} epi {epi} cfg {cfg}")
        return outs, plan

    worst = 0.0
    for epi, ref in ((L.EPI_BIAS, acc + bias.double()), (L.EPI_BIAS_QGELU, R.qgelu(acc + bias.double()))):
        (g, plan), (g2, _), (_, plan0) = launch(epi, 10, bias=bd), launch(epi, 2, bias=bd), launch(epi, 0, bias=bd)
        assert plan == 10 and plan0 == auto, f"{what}: plan {plan0} (forced: {plan}), expected {auto}"
        TO.close(g["y"], ref, mode, f"{what} epi {epi}")
        assert same(g["y"], g2["y"]), f"{what}: 128x128 tiles differ from the 288x256 kernel"
        if epi == L.EPI_BIAS_QGELU:
            TO.close(g["aux"], (acc + bias.double())[row0:], mode, what + " saved u", tol=1e-4)
            assert same(g["aux"], g2["aux"])
        if epi == L.EPI_BIAS:
            for _ in range(25):
                out = torch.empty((M, N), dtype=dt, device=dev())
                o.gemm_nt(ad, wd, out, epi, tile_config=10, bias=bd)
                assert same(out, g["y"]), "288x256 kernel is not deterministic: LDS race"
    # the LayerNorm fold (c_fc of the model: d = K)
    # (float64 on the first and last row of every 288x256 row tile, every 32nd saved row and 256 seeded rows; the
    #  outputs are finite everywhere and every row is compared with the 128x128 tiles' bits)
    tm = (M + 287) // 288
    h = (M + tm - 1) // tm
    edges = [r for t in range(tm) for r in (t * h, min((t + 1) * h, M) - 1)]
    rows = torch.tensor(sorted(set(edges + list(range(row0, M, 32)) + [M - 1]
                                   + torch.randperm(M, generator=torch.Generator().manual_seed(M))[:256].tolist())))
    saved = rows[rows >= row0]
    x, st, w_, b_, gamma, beta, wq, s, bq = _fold_inputs(M, K, N, 64, mode)
    pre_a, du_a, pre_b = _fold_refs(x, st, w_, b_, gamma, beta, wq, s, bq, mode, rows=rows)
    xb, _ = put(x, mode)
    std, _ = guarded(M, K // 64 * 2, torch.float32)
    std.copy_(st.view(M, -1))
    kw = dict(bias=bq.to(dev()), ln_stats=std.view(M, K // 64, 2), ln_colsum=s.to(dev()))
    ad, wd = xb, wq.to(dev())
    (g, plan), (g2, _), (g0, plan0) = launch(L.EPI_LN_BIAS_QGELU, 10, **kw), launch(L.EPI_LN_BIAS_QGELU, 2, **kw), \
        launch(L.EPI_LN_BIAS_QGELU, 0, **kw)
    assert plan == 10 and plan0 == auto, f"{what} LN fold: plan {plan0} (forced: {plan}), expected {auto}"
    ys, sub = g["y"].cpu()[rows], rows >= row0
    worst = max(worst, TR._check_qgelu(ys, None, pre_a, du_a, TR.ULP[mode], what + " (a)", True),
                TR._check_qgelu(ys[sub], g["aux"].cpu()[saved - row0], pre_a[sub], du_a[sub], TR.ULP[mode], what + " (a)", True))
    TO.close(ys, R.qgelu(pre_b), mode, what + " against the unfolded path", tol=1.5 * TO.TOL[mode])
    for other in (g2, g0):
        assert same(g["y"], other["y"]) and same(g["aux"], other["aux"]), f"{what}: LN fold differs between the tilings"
    print(f"\n{what} worst err / budget (LN fold, (a)) {worst:.3f}")
