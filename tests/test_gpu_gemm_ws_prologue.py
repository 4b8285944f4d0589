"""rpo_gemm_ws: what its prologue decides -- which (m-tile, n-tile, k-split) a workgroup owns, which 64-deep k-chunks each
of its waves takes, where the operand rows and weight blocks lie -- against a float64 matmul of the same 16-bit inputs.

The launcher computes everything that is the same for every workgroup once per launch (tile counts and their reciprocals
for a division-free workgroup mapping, the start of every XCD's run, the chunk bounds of the k-splits, byte strides), so
the cases here aim at that arithmetic: grids that do not divide by the 8 XCDs, tile counts that are no powers of two,
partial last tiles on both sides, padded operands, every split factor at chunk counts that leave waves with 0, 1, 2 and
more chunks, and one small case per epilogue.  Tolerances are those of tests/test_gpu_ops.py for this kernel
(relative to max|ref|): 1e-4 for fp32 outputs, 1.5e-2 / 2e-3 for bf16 / f16 outputs, 1.5 x that behind the LayerNorm fold.

The last tests need no GPU: they re-state the launcher's integer formulas and check them against integer division."""
import math

import numpy as np
import pytest
import torch

from oracle import rows_oracle as R  # checker only

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
TOL = {"bf16": 1.5e-2, "f16": 2e-3}
F32TOL = 1e-4
SENTINEL = -1024.0                     # exact in fp32, bf16 and f16; the results are O(1)
GEOM = {110: (32, 32), 120: (32, 64), 220: (64, 64), 330: (96, 96)}     # tile_config -> (BM, BN)


def dev():
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


def close(got, ref, what, tol):
    got = got.detach().to(torch.float64).cpu()
    ref = ref.to(torch.float64)
    err = (got - ref).abs().max().item()
    den = max(ref.abs().max().item(), 1e-30)
    print(f"{what}: max err {err:.3e}, max ref {den:.3e}, rel {err / den:.2e} (limit {tol})")
    assert math.isfinite(err) and err <= tol * den, f"{what}: max err {err:.3e} vs max ref {den:.3e} (rel {err/den:.2e} > {tol})"


def ops():
    from rpo_amd import ops as o
    return o


def padded(t, dt, extra_cols):
    """`t` on the device as a view of a wider buffer (row stride > columns), the rest filled with NaN: nothing but the
    [M, K] rows may reach the result"""
    buf = torch.full((t.shape[0], t.shape[1] + extra_cols), float("nan"), dtype=dt, device=dev())
    buf[:, :t.shape[1]] = t.to(dev(), dt)
    return buf[:, :t.shape[1]]


def framed(M, N, dtype, lead=()):
    """an [.., M, N] view two rows and eight columns inside a sentinel-filled buffer, and the buffer"""
    buf = torch.full((*lead, M + 4, N + 16), SENTINEL, dtype=dtype, device=dev())
    return buf[..., 2:M + 2, 8:N + 8], buf


def check_frame(view, buf, what):
    """every element of the view written (no sentinel, no NaN), nothing outside it touched"""
    v = view.float()
    assert not torch.isnan(v).any().item(), f"{what}: NaN in the result"
    assert not (v == SENTINEL).any().item(), f"{what}: elements of the result were never written"
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    inside[..., 2:2 + view.shape[-2], 8:8 + view.shape[-1]] = True
    assert (buf.float()[~inside] == SENTINEL).all().item(), f"{what}: wrote outside [M, N]"


# (tile_config, M, N, K, split_k): workgroups = ceil(M / BM) x ceil(N / BN) x split_k
GRIDS = [
    (220, 290, 160, 128, 1),    # 5 x 3 = 15 (% 8 = 7); partial last m-tile (34 rows) and n-tile (32 of 64 columns)
    (110, 219, 32, 64, 1),      # 7 x 1 = 7 (% 8 = 7): fewer workgroups than XCDs
    (330, 70, 256, 128, 1),     # 1 x 3 = 3 (% 8 = 3); partial n-tile (64 of 96 columns)
    (330, 456, 160, 64, 1),     # 5 x 2 = 10 (% 8 = 2); partial n-tile (64 of 96), partial m-tile (72 of 96 rows)
    (120, 70, 160, 128, 1),     # 3 x 3 = 9 (% 8 = 1); partial n-tile (32 of 64), partial m-tile (6 rows)
    (220, 456, 64, 64, 1),      # 8 x 1 = 8 (% 8 = 0); partial m-tile (8 rows)
    (110, 33, 96, 192, 3),      # 2 x 3 x 3 = 18 (% 8 = 2): the k-split is the slowest index of the mapping
    (120, 33, 224, 256, 2),     # 2 x 4 x 2 = 16 (% 8 = 0); partial n-tile (32 of 64)
    (110, 456, 96, 64, 1),      # 15 x 3 = 45 (% 8 = 5): several workgroups per XCD, uneven runs
    (0, 456, 160, 128, 1),      # the launcher's own choice
    (0, 33, 64, 64, 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,M,N,K,split", GRIDS)
def test_uneven_grids_cover_the_output_exactly(cfg, M, N, K, split):
    """Every (m-tile, n-tile, k-split) is owned by exactly one workgroup: each element of [M, N] (of every slab) holds its
    reference value, nothing around the result is written, and a second call gives the same bits."""
    from rpo_amd import _lib as L
    o = ops()
    mode, dt = "bf16", torch.bfloat16
    a, w = rnd((M, K), 1, 0.5), rnd((N, K), 2, K ** -0.5)
    a64, w64 = a.to(dt).double(), w.to(dt).double()
    ad = padded(a, dt, 8)
    wp = o.gemm_ws_pack(w.to(dev(), dt))
    if cfg:
        bm, bn = GEOM[cfg]
        assert o.gemm_ws_plan(ad, wp, torch.empty(M, N, device=dev()), L.EPI_NONE, tile_config=cfg) == cfg
        print(f"grid {-(-M // bm)} x {-(-N // bn)} x {split} = {-(-M // bm) * -(-N // bn) * split} workgroups")
    if split == 1:
        out, buf = framed(M, N, torch.float32)
        o.gemm_ws(ad, wp, out, L.EPI_NONE, tile_config=cfg)
        check_frame(out, buf, "fp32 result")
        close(out, a64 @ w64.t(), "fp32 result", F32TOL)
        out16, buf16 = framed(M, N, dt)
        o.gemm_ws(ad, wp, out16, L.EPI_NONE, tile_config=cfg)
        check_frame(out16, buf16, "16-bit result")
        close(out16, a64 @ w64.t(), "16-bit result", TOL[mode])
        again, _ = framed(M, N, torch.float32)
        o.gemm_ws(ad, wp, again, L.EPI_NONE, tile_config=cfg)
        assert torch.equal(out, again)
    else:
        slabs, buf = framed(M, N, torch.float32, lead=(split,))
        o.gemm_ws(ad, wp, slabs, L.EPI_NONE, split_k=split, tile_config=cfg)
        check_frame(slabs, buf, "slabs")
        close(slabs.sum(0), a64 @ w64.t(), "sum of the slabs", F32TOL)
        again, _ = framed(M, N, torch.float32, lead=(split,))
        o.gemm_ws(ad, wp, again, L.EPI_NONE, split_k=split, tile_config=cfg)
        assert torch.equal(slabs, again)


SPLITS = [(K, S) for K in (64, 128, 192, 320, 768, 1536) for S in (1, 2, 3, 4) if S <= K // 64]


@pytest.mark.gpu
@pytest.mark.parametrize("K,split", SPLITS)
def test_split_k_chunk_ranges(K, split):
    """Slab s holds the product over the 64-deep chunks (K / 64) s / split_k .. (K / 64) (s + 1) / split_k, which the four
    waves of a workgroup divide again: K / 64 = 1, 2, 3, 5, 12, 24 chunks over 1 .. 4 slabs leave waves with 0, 1, 2 and
    3 .. 6 chunks, and 3, 5 are divisible neither by 2 nor by 4."""
    from rpo_amd import _lib as L
    o = ops()
    dt = torch.float16 if (K // 64 + split) % 2 else torch.bfloat16
    M, N = 70, 96
    a, w = rnd((M, K), 3, 0.5), rnd((N, K), 4, K ** -0.5)
    a64, w64 = a.to(dt).double(), w.to(dt).double()
    ad, wp = a.to(dev(), dt), o.gemm_ws_pack(w.to(dev(), dt))
    nch = K // 64
    for cfg in (110, 120, 220, 330):
        slabs, buf = framed(M, N, torch.float32, lead=(split,))
        o.gemm_ws(ad, wp, slabs if split > 1 else slabs[0], L.EPI_NONE, split_k=split, tile_config=cfg)
        check_frame(slabs, buf, f"cfg {cfg}")
        close(slabs.sum(0), a64 @ w64.t(), f"cfg {cfg}: sum of {split} slabs", F32TOL)
        for s in range(split):
            k0, k1 = 64 * (nch * s // split), 64 * (nch * (s + 1) // split)
            close(slabs[s], a64[:, k0:k1] @ w64[:, k0:k1].t(), f"cfg {cfg}: slab {s} = k {k0} .. {k1}", F32TOL)
        again, _ = framed(M, N, torch.float32, lead=(split,))
        o.gemm_ws(ad, wp, again if split > 1 else again[0], L.EPI_NONE, split_k=split, tile_config=cfg)
        assert torch.equal(slabs, again)


@pytest.mark.gpu
def test_more_slabs_than_the_table_holds_are_refused():
    """the k-split table of the argument block holds four slabs (the engine uses up to four); RPO_E_SHAPE beyond, which
    sends a caller to rpo_gemm_nt (ops.gemm_ws_try)"""
    from rpo_amd import _lib as L
    o = ops()
    assert o.gemm_ws_ok(456, 512, 2048, torch.bfloat16, torch.float32, L.EPI_NONE, split_k=4)
    assert not o.gemm_ws_ok(456, 512, 2048, torch.bfloat16, torch.float32, L.EPI_NONE, split_k=5)
    a = torch.zeros(64, 512, dtype=torch.bfloat16, device=dev())
    wp = o.gemm_ws_pack(torch.zeros(64, 512, dtype=torch.bfloat16, device=dev()))
    assert not o.gemm_ws_try(a, wp, torch.zeros(5, 64, 64, device=dev()), L.EPI_NONE, split_k=5)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("epi", ["NONE", "QGELU_BWD", "BIAS", "BIAS_QGELU", "LN_BIAS", "LN_BIAS_QGELU", "BIAS_RESID"])
def test_every_prompt_row_epilogue_at_a_small_ragged_shape(mode, epi):
    """One launch per epilogue the prompt rows use (its operands are requested by the prologue, clamped at the ragged
    edges): M = 33 rows (a second m-tile of one row), N = 64, K = 128 (two statistics groups), the launcher's geometry."""
    from rpo_amd import _lib as L
    o = ops()
    dt = DT[mode]
    M, N, K = 33, 64, 128
    a, w = rnd((M, K), 1, 0.5), rnd((N, K), 2, K ** -0.5)
    bias, resid, u = rnd((N,), 3), rnd((M, N), 4), rnd((M, N), 5)
    acc = a.to(dt).double() @ w.to(dt).double().t()
    ad, wd = padded(a, dt, 8), w.to(dev(), dt)
    wp = o.gemm_ws_pack(wd)
    bd = bias.to(dev())
    row0 = M // 3

    def run(out_dtype, e, **kw):
        out, buf = framed(M, N, out_dtype)
        o.gemm_ws(ad, wp, out, e, **kw)
        check_frame(out, buf, epi)
        again, _ = framed(M, N, out_dtype)
        o.gemm_ws(ad, wp, again, e, **kw)
        assert torch.equal(out, again), "the same call twice must give the same bits"
        return out

    if epi == "NONE":
        close(run(dt, L.EPI_NONE), acc, epi, TOL[mode])
        close(run(torch.float32, L.EPI_NONE), acc, epi + " fp32", F32TOL)
    elif epi == "QGELU_BWD":
        close(run(dt, L.EPI_QGELU_BWD, aux=u.to(dev())), acc * R.qgelu_grad(u.double()), epi, TOL[mode])
        d16 = R.qgelu_grad(u.double()).float().to(dev(), dt)
        close(run(dt, L.EPI_QGELU_BWD, aux=d16), acc * d16.double().cpu(), epi + " (16-bit derivative)", TOL[mode])
    elif epi == "BIAS":
        close(run(dt, L.EPI_BIAS, bias=bd), acc + bias.double(), epi, TOL[mode])
    elif epi == "BIAS_QGELU":
        pre = acc + bias.double()
        aux16 = torch.full((M - row0, N), float("nan"), dtype=dt, device=dev())
        close(run(dt, L.EPI_BIAS_QGELU, bias=bd, aux=aux16, aux_row0=row0), R.qgelu(pre), epi, TOL[mode])
        close(aux16, R.qgelu_grad(pre[row0:]), epi + " saved derivative", TOL[mode])
    elif epi == "BIAS_RESID":
        out2 = torch.full((M, N), float("nan"), dtype=dt, device=dev())
        stats = torch.full((M, N // 64, 2), float("nan"), device=dev())
        out = run(torch.float32, L.EPI_BIAS_RESID, bias=bd, resid=resid.to(dev()), out2=out2, ln_stats=stats)
        close(out, acc + bias.double() + resid.double(), epi, F32TOL)
        assert torch.equal(out2, out.to(dt)), "out2 must be the RNE act-dtype copy of C"
        grp = out.double().cpu().reshape(M, N // 64, 64)
        ref_stats = torch.stack([grp.mean(-1), ((grp - grp.mean(-1, keepdim=True)) ** 2).sum(-1)], -1)
        close(stats, ref_stats, epi + " partial row statistics", 2e-5)
    else:
        # LayerNorm fold, consumer side: A holds the 16-bit copy of x, the statistics are x's (64-column groups), the
        # weight carries gamma and the bias beta (tests/test_gpu_ops.py::test_gemm_ws_layernorm_fold)
        x = rnd((M, K), 6, 2.0) + 0.4
        gamma, beta = rnd((K,), 7, 0.1) + 1.0, rnd((K,), 8, 0.05)
        x64 = x.double()
        grp = x64.reshape(M, K // 64, 64)
        stats = torch.stack([grp.mean(-1), ((grp - grp.mean(-1, keepdim=True)) ** 2).sum(-1)], -1).float().contiguous().to(dev())
        wq = (w.double() * gamma.double()[None, :]).float().to(dt)
        s = wq.double().sum(1).float().to(dev())
        bq = (bias.double() + w.double() @ beta.double()).float().to(dev())
        mu = x64.mean(1, keepdim=True)
        rstd = (x64.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
        pre = ((x64 - mu) * rstd * gamma.double() + beta.double()) @ w.double().t() + bias.double()
        xb, wqp = padded(x, dt, 8), o.gemm_ws_pack(wq.to(dev()))
        tol = 1.5 * TOL[mode]
        for cfg in (0, 330):
            out, buf = framed(M, N, dt)
            if epi == "LN_BIAS":
                o.gemm_ws(xb, wqp, out, L.EPI_LN_BIAS, bias=bq, ln_stats=stats, ln_colsum=s, tile_config=cfg)
                check_frame(out, buf, epi)
                close(out, pre, f"{epi} cfg {cfg}", tol)
            else:
                aux16 = torch.full((M - row0, N), float("nan"), dtype=dt, device=dev())
                o.gemm_ws(xb, wqp, out, L.EPI_LN_BIAS_QGELU, bias=bq, aux=aux16, aux_row0=row0, ln_stats=stats, ln_colsum=s,
                          tile_config=cfg)
                check_frame(out, buf, epi)
                close(out, R.qgelu(pre), f"{epi} cfg {cfg}", tol)
                close(aux16, R.qgelu_grad(pre[row0:]), f"{epi} cfg {cfg} saved derivative", tol)


# ------------------------------------------------------------------------------------------
# The launcher's integer formulas, re-stated (csrc/gemm_ws.hip: ws_rcp / ws_divmod, the XCD runs, the chunk table)
def ws_rcp(d):
    return 0xFFFFFFFF if d <= 1 else (1 << 32) // d


def ws_divmod(x, d, rcp):
    """numpy uint64 arrays standing in for the device's 32-bit registers"""
    q = (x * np.uint64(rcp)) >> np.uint64(32)
    r = (x - q * np.uint64(d)) & np.uint64(0xFFFFFFFF)
    fix = r >= np.uint64(d)
    return q + fix, np.where(fix, r - np.uint64(d), r)


def test_reciprocal_division_is_exact():
    """mulhi(x, floor(2^32 / d)) + one compare-and-fix = x / d, x % d: exhaustively for every divisor up to 512 and every
    dividend below 2^16 (the tile counts and grids of any problem near the project's), and at the ends of the 32-bit range
    for small, odd, power-of-two and huge divisors (the bound the launcher relies on is the grid limit 2^31 - 1)"""
    x = np.arange(1 << 16, dtype=np.uint64)
    for d in range(1, 513):
        q, r = ws_divmod(x, d, ws_rcp(d))
        assert np.array_equal(q, x // np.uint64(d)) and np.array_equal(r, x % np.uint64(d)), d
    rng = np.random.default_rng(0)
    edge = np.concatenate([np.arange(0, 4096), (1 << 31) - 1 - np.arange(0, 4096), (1 << 32) - 1 - np.arange(0, 4096),
                           rng.integers(0, 1 << 32, 20000)]).astype(np.uint64)
    divisors = [1, 2, 3, 5, 7, 8, 15, 641, 4096, 65535, 65536, 65537, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
    divisors += rng.integers(1, 1 << 32, 200).tolist()
    for d in divisors:
        q, r = ws_divmod(edge, d, ws_rcp(d))
        assert np.array_equal(q, edge // np.uint64(d)) and np.array_equal(r, edge % np.uint64(d)), d


def test_xcd_runs_are_a_permutation_and_match_the_two_branch_form():
    """XCD x = bid % 8 starts at x (nwg / 8) + min(x, nwg % 8): the same workgroup order as the form with a branch on
    x < nwg % 8 that the kernel used before, and every workgroup exactly once"""
    for nwg in list(range(1, 600)) + [1000, 4095, 4097, 65537]:
        qd, rm = nwg >> 3, nwg & 7
        seen = []
        for bid in range(nwg):
            xcd = bid & 7
            old = (xcd * (qd + 1) if xcd < rm else rm * (qd + 1) + (xcd - rm) * qd) + (bid >> 3)
            new = xcd * qd + min(xcd, rm) + (bid >> 3)
            assert old == new
            seen.append(new)
        assert sorted(seen) == list(range(nwg)), nwg


def test_chunk_table_and_wave_ranges_partition_k():
    """kb[s] = (K / 64) s / split_k (the launcher's table; entries past split_k repeat the end) and the per-wave ranges
    wc0 + (n w) >> 2 .. wc0 + (n (w + 1)) >> 2 tile 0 .. K / 64 without gap or overlap"""
    for nch in range(1, 65):
        for split in range(1, min(4, nch) + 1):
            kb = [nch * min(s, split) // split for s in range(5)]
            assert kb[0] == 0 and kb[split] == nch and kb[split:] == [nch] * (5 - split)
            covered = []
            for ksl in range(split):
                wc0, wc1 = kb[0], kb[1]
                for s in range(1, 4):
                    if ksl >= s:
                        wc0, wc1 = kb[s], kb[s + 1]
                assert (wc0, wc1) == (nch * ksl // split, nch * (ksl + 1) // split)
                n = wc1 - wc0
                for wave in range(4):
                    covered += range(wc0 + ((n * wave) >> 2), wc0 + ((n * (wave + 1)) >> 2))
            assert covered == list(range(nch)), (nch, split)
