"""The RPO step at every batch size the image tower's GEMM heuristics distinguish.

The kernel an image-tower GEMM runs on is chosen from its row count M = B (N + K), so each batch size gets its own tile
families, row-unit tilings, LayerNorm-statistics group (64 / 96 columns) and residual-stream layout (fp32, or 16-bit hi /
lo halves).  This module

* asks the library which kernel a call would run (rpo_gemm_nt_plan / rpo_gemm_ws_plan) and checks the answer: forcing
  the reported tile_config gives the bits of the heuristic's own launch, and refused arguments get the call's own error;
* sweeps every batch size 1 .. max_batch through ONE engine per (model, mode) at depth 2, in a non-monotonic order that
  starts at max_batch, with every per-step image-side buffer filled with NaN before each call (a launch that reads rows
  past this batch's R would otherwise read the previous batch's plausible rows), against the CPU oracle run image by image;
* checks that batch composition does not change an image's result: bit for bit in f32, and between any two batch sizes
  whose image-tower GEMMs run the same plans in the 16-bit modes.

The sweeps cover ViT-B/16 and ViT-L/14 at 224 px and the two other patch grids: ViT-B/32, whose 74-row
units sit in 224-row (B = 26 .. 32) and 288-row (B = 18 .. 21) tiles, and ViT-L/14 at 336 px, which offers no units.
"""
import ctypes
import functools
import gc
import time

import numpy as np
import pytest
import torch

from helpers import BF16_GRAD_REL, BF16_LOGIT_ATOL, F16_GRAD_REL, F16_LOGIT_ATOL, TOL_F32
from rpo_amd import synth

pytestmark = pytest.mark.gpu

NAN = float("nan")
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def dev():
    return torch.device("cuda:0")


def ops():
    from rpo_amd import ops as o
    return o


def lib():
    from rpo_amd import _lib as L
    return L


def rnd(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev())


def nans(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=dev())


def bits(t):
    """the raw bits of a tensor (NaN == NaN), on the host"""
    return t.detach().contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()]).cpu()


# ------------------------------------------------------------------------------------------------------------------
# op level: the query tells the truth
# ------------------------------------------------------------------------------------------------------------------
def _gemm_case(M, N, K, epi, mode, units=None, ln_group=0, hilo=False, aux_rows=0, skip=None, seed=0):
    """(a, w, make_kw) of one image-tower-shaped rpo_gemm_nt call: make_kw() returns the keyword arguments with FRESH
    NaN-filled output buffers (out first), so that two launches can be compared bit for bit."""
    L = lib()
    dt = DT[mode]
    a, w = rnd((M, K), seed, 0.5, dt), rnd((N, K), seed + 1, K ** -0.5, dt)
    fixed = {}
    if epi in (L.EPI_BIAS, L.EPI_BIAS_QGELU, L.EPI_BIAS_RESID, L.EPI_LN_BIAS, L.EPI_LN_BIAS_QGELU):
        fixed["bias"] = rnd((N,), seed + 2, 0.1)
    if epi in (L.EPI_LN_BIAS, L.EPI_LN_BIAS_QGELU):
        g = ln_group or 64
        st = torch.empty(M, K // g, 2)
        st[..., 0] = torch.randn(M, K // g, generator=torch.Generator().manual_seed(seed + 3)) * 0.1
        st[..., 1] = g * (1.0 + torch.rand(M, K // g, generator=torch.Generator().manual_seed(seed + 4)))
        fixed.update(ln_stats=st.to(dev()), ln_colsum=rnd((N,), seed + 5), ln_group=ln_group)
    if epi == L.EPI_BIAS_RESID:
        if hilo:
            fixed.update(resid_hi=rnd((M, N), seed + 6, 1.0, dt), resid_lo=rnd((M, N), seed + 7, 1e-3, dt), c_row0=units[2])
        else:
            fixed["resid"] = rnd((M, N), seed + 6)
    if units is not None:
        fixed["row_units"] = units
    if skip is not None:
        fixed.update(skip_row0=skip[0], skip_col0=skip[1])
    out_dt = torch.float32 if epi == L.EPI_BIAS_RESID else dt

    def make_kw():
        kw = dict(fixed)
        kw["out"] = nans((M, N), out_dt)
        if epi == L.EPI_BIAS_RESID and mode != "f32":
            kw.update(out2=nans((M, N), dt), ln_stats=nans((M, N // (ln_group or 64), 2), torch.float32), ln_group=ln_group)
            if hilo:
                kw["out_lo"] = nans((M, N), dt)
        if aux_rows:
            kw.update(aux=nans((aux_rows, N), dt), aux_row0=M - aux_rows)
        return kw
    return a, w, make_kw


NB, NL = 197, 257         # frozen rows per image: ViT-B/16, ViT-L/14 (224 px)


def _units(n, k, B):
    return (n, k, B * n)


def _plan_cases():
    L = lib()
    r = lambda n, k, B: B * (n + k)
    cases = [
        # (id, M, N, K, epilogue, mode, extra, expected tile_config)
        ("b4_out_proj_64x64", r(NB, 24, 4), 768, 768, L.EPI_BIAS_RESID, "bf16", {}, 5),
        ("b8_c_fc_64x128", r(NB, 24, 8), 3072, 768, L.EPI_LN_BIAS_QGELU, "bf16", dict(aux_rows=8 * 24), 6),
        ("b12_c_proj_64x128", r(NB, 24, 12), 768, 3072, L.EPI_BIAS_RESID, "bf16", {}, 6),
        ("b12_in_proj_128x128", r(NB, 24, 12), 2304, 768, L.EPI_LN_BIAS, "bf16", dict(skip=(12 * NB, 768)), 2),
        ("b14_c_fc_256x256", r(NB, 24, 14), 3072, 768, L.EPI_LN_BIAS_QGELU, "bf16", dict(aux_rows=14 * 24), 8),
        ("b26_c_fc_224x384_partial", r(NB, 24, 26), 3072, 768, L.EPI_LN_BIAS_QGELU, "bf16",
         dict(units=_units(NB, 24, 26), ln_group=96, aux_rows=26 * 24), 10),
        ("b27_out_proj_224x96_partial_hilo", r(NB, 24, 27), 768, 768, L.EPI_BIAS_RESID, "f16",
         dict(units=_units(NB, 24, 27), ln_group=96, hilo=True), 11),
        ("k48_b32_out_proj_256x96", r(NB, 48, 32), 768, 768, L.EPI_BIAS_RESID, "bf16",
         dict(units=_units(NB, 48, 32), ln_group=96, hilo=True), 11),
        ("l14_b16_c_fc_288x256", r(NL, 24, 16), 4096, 1024, L.EPI_LN_BIAS_QGELU, "bf16",
         dict(units=_units(NL, 24, 16), ln_group=64, aux_rows=16 * 24), 10),
        ("l14_b13_out_proj_288x64_partial_hilo", r(NL, 24, 13), 1024, 1024, L.EPI_BIAS_RESID, "bf16",
         dict(units=_units(NL, 24, 13), ln_group=64, hilo=True), 11),
        ("f32_b4_out_proj_64x64", r(NB, 24, 4), 768, 768, L.EPI_BIAS_RESID, "f32", {}, 5),
        ("f32_b8_c_fc_64x128", r(NB, 24, 8), 3072, 768, L.EPI_BIAS_QGELU, "f32", dict(aux_rows=8 * 24), 6),
        ("f32_b12_c_fc_128x128", r(NB, 24, 12), 3072, 768, L.EPI_BIAS_QGELU, "f32", {}, 2),
    ]
    # the bench's own B = 32 shapes (ViT-B/16, K = 24): in-proj, c_fc, out-proj, c_proj
    R32, u32 = r(NB, 24, 32), _units(NB, 24, 32)
    cases += [
        ("bench_in_proj", R32, 2304, 768, L.EPI_LN_BIAS, "bf16", dict(ln_group=96, skip=(32 * NB, 768)), 8),
        ("bench_c_fc", R32, 3072, 768, L.EPI_LN_BIAS_QGELU, "bf16", dict(units=u32, ln_group=96, aux_rows=32 * 24), 10),
        ("bench_out_proj", R32, 768, 768, L.EPI_BIAS_RESID, "bf16", dict(units=u32, ln_group=96, hilo=True), 11),
        ("bench_c_proj", R32, 768, 3072, L.EPI_BIAS_RESID, "bf16", dict(units=u32, ln_group=96, hilo=True), 11),
    ]
    # the engine's own calls at the other patch grids.  ViT-B/32 (50 + 24 rows per image, max_batch 32):
    # row units a third of a 224-row tile high, 96-column statistics, hi / lo stream; in-proj gets no units and at
    # 2368 x 2304 fills neither 256x256 nor 224x384 rounds
    for B, tag in ((32, "b32_b32"), (28, "b32_b28_partial")):
        Rb, ub = r(NB32, 24, B), _units(NB32, 24, B)
        cases += [
            (f"{tag}_in_proj", Rb, 2304, 768, L.EPI_LN_BIAS, "bf16", dict(ln_group=96, skip=(B * NB32, 768)), 2),
            (f"{tag}_c_fc", Rb, 3072, 768, L.EPI_LN_BIAS_QGELU, "bf16", dict(units=ub, ln_group=96, aux_rows=B * 24), 10),
            (f"{tag}_out_proj", Rb, 768, 768, L.EPI_BIAS_RESID, "f16", dict(units=ub, ln_group=96, hilo=True), 11),
            (f"{tag}_c_proj", Rb, 768, 3072, L.EPI_BIAS_RESID, "bf16", dict(units=ub, ln_group=96, hilo=True), 11),
        ]
    # ViT-L/14 at 336 px (577 + 24 rows per image, max_batch 16): no units, the GEMMs choose by shape -- c_fc takes the
    # 288x256 geometry in equal-height contiguous tiles at B = 7 and 14, the residual GEMMs the 128x128 tiles from 8192 rows
    for B, (c_in, c_fc, c_res) in ((7, (8, 10, 6)), (8, (8, 2, 6)), (14, (2, 10, 2)), (16, (8, 2, 2))):
        Rl = r(NL336, 24, B)
        cases += [
            (f"l336_b{B}_in_proj", Rl, 3072, 1024, L.EPI_LN_BIAS, "bf16", dict(skip=(B * NL336, 1024)), c_in),
            (f"l336_b{B}_c_fc", Rl, 4096, 1024, L.EPI_LN_BIAS_QGELU, "bf16", dict(aux_rows=B * 24), c_fc),
            (f"l336_b{B}_out_proj", Rl, 1024, 1024, L.EPI_BIAS_RESID, "f16", {}, c_res),
            (f"l336_b{B}_c_proj", Rl, 1024, 4096, L.EPI_BIAS_RESID, "bf16", {}, c_res),
        ]
    return cases


NB32, NL336 = 50, 577     # ... ViT-B/32, ViT-L/14 at 336 px
_GRID_PLAN_IDS = [f"{t}_{g}" for t in ("b32_b32", "b32_b28_partial", "l336_b7", "l336_b8", "l336_b14", "l336_b16")
                  for g in ("in_proj", "c_fc", "out_proj", "c_proj")]
_PLAN_IDS =["b4_out_proj_64x64", "b8_c_fc_64x128", "b12_c_proj_64x128", "b12_in_proj_128x128", "b14_c_fc_256x256",
             "b26_c_fc_224x384_partial", "b27_out_proj_224x96_partial_hilo", "k48_b32_out_proj_256x96",
             "l14_b16_c_fc_288x256", "l14_b13_out_proj_288x64_partial_hilo", "f32_b4_out_proj_64x64",
             "f32_b8_c_fc_64x128", "f32_b12_c_fc_128x128", "bench_in_proj", "bench_c_fc", "bench_out_proj", "bench_c_proj"]


@pytest.mark.parametrize("case", _PLAN_IDS + _GRID_PLAN_IDS)
def test_gemm_nt_plan_names_the_launch_it_makes(case):
    """For one shape per tile family the heuristic picks (row-unit hints, 96-column statistics, hi / lo arguments and the
    bench's B = 32 shapes included): the query returns the family's code, and a launch forced to that code gives the bits
    of the heuristic's own launch in every output (C, the 16-bit copy, the lo half, the statistics, the saved derivative)."""
    o = ops()
    cid, M, N, K, epi, mode, extra, want = next(c for c in _plan_cases() if c[0] == case)
    a, w, make_kw = _gemm_case(M, N, K, epi, mode, **extra)
    kw0 = make_kw()
    out0 = kw0.pop("out")
    got = o.gemm_nt_plan(a, w, out0, epi, **kw0)
    assert got == want, f"{case}: plan {got}, expected {want}"
    o.gemm_nt(a, w, out0, epi, **kw0)
    kw1 = make_kw()
    out1 = kw1.pop("out")
    assert o.gemm_nt_plan(a, w, out1, epi, tile_config=got, **kw1) == got
    o.gemm_nt(a, w, out1, epi, tile_config=got, **kw1)
    torch.cuda.synchronize()
    assert torch.isfinite(out0[kw0.get("c_row0", 0):]).all() or "skip_row0" in kw0
    assert torch.equal(bits(out0), bits(out1)), f"{case}: tile_config {got} differs from the heuristic's launch"
    for name in ("out2", "out_lo", "ln_stats", "aux"):
        if name in kw0:
            assert torch.equal(bits(kw0[name]), bits(kw1[name])), f"{case}: {name} differs under tile_config {got}"


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K,epi_name", [(884, 2304, 768, "EPI_LN_BIAS"), (884, 768, 768, "EPI_BIAS_RESID"),
                                             (884, 3072, 768, "EPI_LN_BIAS_QGELU"), (768, 768, 3072, "EPI_BIAS_RESID")])
def test_gemm_ws_plan_names_the_launch_it_makes(mode, M, N, K, epi_name):
    """rpo_gemm_ws at the small-batch image forward's shapes (B = 4: every wide launch; 768 rows: the last block's prompt
    rows at B = 32): the query returns a geometry code, and forcing it gives the bits of the kernel's own choice."""
    o, L = ops(), lib()
    epi = getattr(L, epi_name)
    dt = DT[mode]
    a, w = rnd((M, K), 1, 0.5, dt), rnd((N, K), 2, K ** -0.5, dt)
    pw = o.gemm_ws_pack(w)
    kw = dict(bias=rnd((N,), 3, 0.1))
    if epi == L.EPI_BIAS_RESID:
        kw["resid"] = rnd((M, N), 4)
    if epi in (L.EPI_LN_BIAS, L.EPI_LN_BIAS_QGELU):
        st = torch.empty(M, K // 64, 2)
        st[..., 0], st[..., 1] = 0.05, 64.0
        kw.update(ln_stats=st.to(dev()), ln_colsum=rnd((N,), 5))
    out_dt = torch.float32 if epi == L.EPI_BIAS_RESID else dt

    def run(cfg):
        out = nans((M, N), out_dt)
        extra = {}
        if epi == L.EPI_BIAS_RESID:
            extra = dict(out2=nans((M, N), dt), ln_stats=nans((M, N // 64, 2), torch.float32))
        if epi == L.EPI_LN_BIAS_QGELU:
            extra = dict(aux=nans((M // 4, N), dt), aux_row0=M - M // 4)
        code = o.gemm_ws_plan(a, pw, out, epi, tile_config=cfg, **kw, **extra)
        o.gemm_ws(a, pw, out, epi, tile_config=cfg, **kw, **extra)
        return code, [out] + list(v for v in extra.values() if isinstance(v, torch.Tensor))
    code, outs0 = run(0)
    assert code in (110, 120, 220, 330), code
    code1, outs1 = run(code)
    assert code1 == code
    torch.cuda.synchronize()
    for x, y in zip(outs0, outs1):
        assert torch.equal(bits(x), bits(y)), f"rpo_gemm_ws geometry {code} differs from the kernel's own choice"


def _raw(fn, plan, a, w, out, epi, **kw):
    """(what the call returns, what the query returns) for the same arguments"""
    o = ops()
    wv = o._WView(w) if isinstance(w, o.PackedWeight) else w
    args = o.gemm_args(a, wv, out, epi, **kw)
    rc = int(fn(ctypes.byref(args), o._stream()))
    torch.cuda.synchronize()
    return rc, int(plan(ctypes.byref(args)))


def test_refused_arguments_get_the_calls_error():
    """The queries return the negative RPO_E_* the call itself returns, for arguments each entry point refuses."""
    o, L = ops(), lib()
    lb = L.load()
    bf, f32 = torch.bfloat16, torch.float32
    a, w = rnd((884, 768), 1, 1.0, bf), rnd((768, 768), 2, 0.03, bf)
    bias, resid = rnd((768,), 3), rnd((884, 768), 4)
    hi, lo = rnd((884, 768), 5, 1.0, bf), rnd((884, 768), 6, 1e-3, bf)
    nt_cases = [
        # tile_config 11 without the row-unit hint it needs
        (a, w, nans((884, 768), f32), L.EPI_BIAS_RESID, dict(bias=bias, resid=resid, tile_config=11), L.E_SHAPE),
        # 96-column statistics where no 96-column geometry applies
        (a, w, nans((884, 768), f32), L.EPI_BIAS_RESID,
         dict(bias=bias, resid=resid, out2=nans((884, 768), bf), ln_stats=nans((884, 8, 2), f32), ln_group=96), L.E_SHAPE),
        # hi / lo residual halves on a shape the one-round kernels do not take
        (a, w, nans((884, 768), f32), L.EPI_BIAS_RESID,
         dict(bias=bias, resid_hi=hi, resid_lo=lo, out2=nans((884, 768), bf), out_lo=nans((884, 768), bf), c_row0=788),
         L.E_SHAPE),
        # a LayerNorm-fold consumer with an fp32 output
        (a, w, nans((884, 768), f32), L.EPI_LN_BIAS,
         dict(bias=bias, ln_stats=nans((884, 12, 2), f32), ln_colsum=bias), L.E_BADARG),
        # a 16-bit output of the other 16-bit format
        (a, w, nans((884, 768), torch.float16), L.EPI_BIAS, dict(bias=bias), L.E_DTYPE),
        # K not a multiple of the k-tile
        (rnd((64, 96), 7, 1.0, bf), rnd((64, 96), 8, 1.0, bf), nans((64, 64), bf), L.EPI_NONE, {}, L.E_SHAPE),
    ]
    for i, (aa, ww, out, epi, kw, want) in enumerate(nt_cases):
        rc, plan = _raw(lb.rpo_gemm_nt, lb.rpo_gemm_nt_plan, aa, ww, out, epi, **kw)
        assert rc == want and plan == rc, f"rpo_gemm_nt case {i}: call {rc}, plan {plan}, expected {want}"
    pw = o.gemm_ws_pack(w)
    pw32 = o.PackedWeight(torch.zeros(768 * 768, device=dev()), 768, 768)
    ws_cases = [
        (a, pw, nans((884, 768), f32), L.EPI_BIAS_RESID, dict(bias=bias, resid=resid, row_units=(197, 24, 788)), L.E_SHAPE),
        (a, pw, nans((884, 768), bf), L.EPI_BIAS_RESID, dict(bias=bias, resid=resid), L.E_DTYPE),
        (a, pw, nans((884, 768), f32), L.EPI_BIAS, dict(bias=bias), L.E_DTYPE),
        (a, pw, nans((884, 768), bf), L.EPI_NONE, dict(tile_config=230), L.E_SHAPE),
        (a.float(), pw32, nans((884, 768), f32), L.EPI_NONE, {}, L.E_DTYPE),
        (a, pw, nans((884, 768), f32), L.EPI_BIAS_RESID,
         dict(bias=bias, resid=resid, out2=nans((884, 768), bf), ln_stats=nans((884, 8, 2), f32), ln_group=96), L.E_SHAPE),
    ]
    for i, (aa, ww, out, epi, kw, want) in enumerate(ws_cases):
        rc, plan = _raw(lb.rpo_gemm_ws, lb.rpo_gemm_ws_plan, aa, ww, out, epi, **kw)
        assert rc == want and plan == rc, f"rpo_gemm_ws case {i}: call {rc}, plan {plan}, expected {want}"


# ------------------------------------------------------------------------------------------------------------------
# model level: a batch-size sweep against the CPU oracle
# ------------------------------------------------------------------------------------------------------------------
SWEEPS = {                       # id -> (model, K, max_batch)
    "b16_k24_mb32": ("ViT-B/16", 24, 32),
    "b16_k24_mb4": ("ViT-B/16", 24, 4),
    "b16_k4_mb32": ("ViT-B/16", 4, 32),
    "b16_k48_mb32": ("ViT-B/16", 48, 32),
    "l14_k24_mb16": ("ViT-L/14", 24, 16),
    "b32_k24_mb32": ("ViT-B/32", 24, 32),
    "l14_336_k24_mb16": ("ViT-L/14@336px", 24, 16),
}
SWEEP_CASES = [("b16_k24_mb32", "f32"), ("b16_k24_mb32", "bf16"), ("b16_k24_mb32", "f16"),
               ("b16_k24_mb4", "bf16"), ("b16_k24_mb4", "f16"), ("b16_k4_mb32", "bf16"), ("b16_k48_mb32", "bf16"),
               ("l14_k24_mb16", "bf16"), ("l14_k24_mb16", "f16"),
               ("b32_k24_mb32", "f32"), ("b32_k24_mb32", "bf16"), ("b32_k24_mb32", "f16"),
               ("l14_336_k24_mb16", "bf16"), ("l14_336_k24_mb16", "f16")]
BOUNDS = {"f32": (TOL_F32, TOL_F32), "bf16": (BF16_LOGIT_ATOL, BF16_GRAD_REL), "f16": (F16_LOGIT_ATOL, F16_GRAD_REL)}

# Per-step image-side buffers: everything a step writes before it reads it.  Persistent state -- parameters, gradients,
# momentum, packed weights, the text K / V cache, the text features between eval calls -- is left alone.
STEP_BUFFERS = ("x_pre", "x", "xm", "h", "h_lo", "ln_stats", "qkv", "att", "g", "u", "y_post", "img_f", "im2col",
                "logits", "head_ws", "d_img_f", "d_img_f_a", "dy_v", "dxa_v", "dxb_v", "dxc_v", "du_v", "da_v", "dq_v")


@functools.lru_cache(maxsize=None)
def _workload(model, K):
    from rpo_amd.config import vit_b16, vit_b32, vit_l14, vit_l14_336
    make = {"ViT-B/16": vit_b16, "ViT-L/14": vit_l14, "ViT-B/32": vit_b32, "ViT-L/14@336px": vit_l14_336}[model]
    cfg = make(layers_v=2, layers_t=2, K=K)
    toks = synth.oxford_pets_base_tokens()
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
    tp, ip = synth.prompts(cfg, sd, seed=7)
    n = max(mb for m, k, mb in SWEEPS.values() if (m, k) == (model, K))
    return cfg, toks, sd, tp, ip, synth.images(cfg, n), synth.labels(cfg, n)


_ORACLE = {}


def _oracle(model, K):
    """Per-image (logits, loss, g_text, g_img) of the CPU oracle: one single-image run per image, shared by every mode
    and max_batch of the model.  The mean-CE gradient of a batch is the mean of these per-image gradients."""
    from oracle.rpo_oracle import OracleRPO
    key = (model, K)
    if key not in _ORACLE:
        t0 = time.time()
        cfg, toks, sd, tp, ip, img, lab = _workload(model, K)
        o = OracleRPO(sd, toks, cfg.K, cfg.patch)
        o.set_prompts(tp, ip)
        res = [o.loss_and_grads(img[i:i + 1], lab[i:i + 1]) for i in range(img.shape[0])]
        _ORACLE[key] = (np.stack([r[0].logits.detach().numpy()[0] for r in res]),
                        np.array([float(r[0].loss.item()) for r in res]),
                        np.stack([r[1].numpy() for r in res]), np.stack([r[2].numpy() for r in res]))
        print(f"[oracle {model} K={K}] {img.shape[0]} single-image runs: {time.time() - t0:.1f} s")
    return _ORACLE[key]


def _poison(eng):
    for name in STEP_BUFFERS:
        v = getattr(eng, name)
        for t in (v if isinstance(v, (list, tuple)) else [v]):
            t.fill_(NAN)


class _PlanLog:
    """Records the plan of every GEMM the image forward issues: ("nt", tile_config, ln_group) / ("ws", code)."""
    def __init__(self, monkeypatch, eng):
        o = ops()
        self.want, self.active, self.log, self.ws_rows = False, False, [], []
        real_nt, real_ws, real_fwd = o.gemm_nt, o.gemm_ws_try, eng._image_forward

        def gemm_nt(a, w, out, epilogue=0, **kw):
            if self.active:
                self.log.append(("nt", o.gemm_nt_plan(a, w, out, epilogue, **kw), kw.get("ln_group", 0) or 64))
            return real_nt(a, w, out, epilogue, **kw)

        def gemm_ws_try(a, w, out, epilogue=0, **kw):
            if self.active:
                code = o.gemm_ws_plan(a, w, out, epilogue, **kw)
                if code > 0:                       # (RPO_E_SHAPE: the engine sends the call to gemm_nt, recorded there)
                    self.log.append(("ws", code))
                    self.ws_rows.append(a.shape[0])
            return real_ws(a, w, out, epilogue, **kw)

        def image_forward(*args, **kw):
            self.active = self.want
            try:
                return real_fwd(*args, **kw)
            finally:
                self.active = False
        monkeypatch.setattr(o, "gemm_nt", gemm_nt)
        monkeypatch.setattr(o, "gemm_ws_try", gemm_ws_try)
        eng._image_forward = image_forward


def _order(mb):
    """max_batch first, then the rest in a fixed non-monotonic order"""
    return [mb] + (np.random.default_rng(mb).permutation(np.arange(1, mb)) if mb > 1 else np.arange(0)).tolist()


def _regimes(plans):
    """compact plan table: consecutive batch sizes with the same set of plans share a line"""
    def fam(p):
        nt = sorted({c for c in p if c[0] == "nt"})
        ws = sorted({c[1] for c in p if c[0] == "ws"})
        return " ".join(f"{c[1]}" + ("/96" if c[2] == 96 else "") for c in nt) + (f" | ws {ws}" if ws else "")
    lines, run = [], None
    for B in sorted(plans):
        f = fam(plans[B])
        if run and run[2] == f and run[1] == B - 1:
            run[1] = B
        else:
            run = [B, B, f]
            lines.append(run)
    return "\n".join(f"    B {b0:2d}-{b1:2d}: nt {f}" for b0, b1, f in lines)


@pytest.mark.parametrize("sweep,mode", SWEEP_CASES, ids=[f"{s}-{m}" for s, m in SWEEP_CASES])
def test_every_batch_size_against_oracle(sweep, mode, monkeypatch):
    """Every B in 1 .. max_batch through one engine (depth 2 in both towers: the hi / lo stream needs more than one image
    block), first B images: eager eval == graph replay == the train step's logits (bits); no NaN / Inf; per-image logits,
    the loss and the prompt gradients against the oracle at the bounds of tests/test_gpu_model.py; an image's logits and
    features are the same bits at every B (f32) or at every B with the same GEMM plans (16-bit modes)."""
    from rpo_amd.engine import make_engine
    t0 = time.time()
    model, K, mb = SWEEPS[sweep]
    cfg, toks, sd, tp, ip, img_np, lab_np = _workload(model, K)
    o_logits, o_loss, o_gt, o_gi = _oracle(model, K)
    la, gr = BOUNDS[mode]
    # (a captured graph must not be destroyed while another one is being captured: whatever earlier tests left for the
    #  cycle collector goes now, not at some allocation inside this engine's captures)
    gc.collect()
    eng = make_engine(cfg, sd, toks, dev(), DT[mode], mb)
    try:
        _sweep(eng, sweep, mode, monkeypatch, t0)
    finally:
        eng.__dict__.pop("_image_forward", None)       # (the plan log's wrapper: a reference cycle through the engine)
        eng._eval_graphs.clear()
        torch.cuda.synchronize()
        del eng
        gc.collect()


def _sweep(eng, sweep, mode, monkeypatch, t0):
    model, K, mb = SWEEPS[sweep]
    cfg, toks, sd, tp, ip, img_np, lab_np = _workload(model, K)
    o_logits, o_loss, o_gt, o_gi = _oracle(model, K)
    la, gr = BOUNDS[mode]
    with torch.no_grad():
        eng.text_prompt.copy_(torch.from_numpy(tp))
        eng.img_prompt.copy_(torch.from_numpy(ip))
    eng.params_version += 1
    rec = _PlanLog(monkeypatch, eng)
    img = torch.from_numpy(img_np[:mb]).to(dev())
    lab = torch.from_numpy(lab_np[:mb]).to(dev())
    e = cfg.embed
    plans, rows, worst = {}, {}, dict(logits=0.0, loss=0.0, g_text=0.0, g_img=0.0)
    for B in _order(mb):
        im, lb = img[:B], lab[:B]
        _poison(eng)
        rec.want, rec.log = True, []
        le = eng.forward_eval(im, use_graph=False).clone()
        rec.want = False
        fe = eng.img_f[:B * K].clone()
        plans[B] = tuple(rec.log)
        _poison(eng)
        lg = eng.forward_eval(im).clone()
        fg = eng.img_f[:B * K].clone()
        _poison(eng)
        eng.forward_backward(im, lb)
        torch.cuda.synchronize()
        lt, loss, grads = eng.logits[:B].clone(), eng.loss.clone(), eng.grads.clone()
        for name, t in (("eval logits", le), ("eval img_f", fe), ("train logits", lt), ("loss", loss), ("grads", grads)):
            assert torch.isfinite(t).all(), f"B={B}: {name} not finite"
        assert torch.equal(le, lg) and torch.equal(fe, fg), f"B={B}: graph replay differs from eager eval"
        assert torch.equal(lt, le), f"B={B}: the train step's logits differ from eval's"
        # against the oracle: per image, and the batch means (mean CE -> mean of per-image gradients)
        el = float(np.abs(le.cpu().numpy() - o_logits[:B]).max())
        ce = torch.nn.functional.cross_entropy(lt.double().cpu(), lb.cpu()).item()
        assert abs(ce - loss.item()) <= 1e-5 * max(1.0, abs(ce)), f"B={B}: loss {loss.item()} vs CE of its logits {ce}"
        eo = abs(loss.item() - float(o_loss[:B].mean()))
        nt = cfg.K * cfg.d_t
        g = grads.cpu().numpy()
        gt_ref, gi_ref = o_gt[:B].mean(0).reshape(-1), o_gi[:B].mean(0).reshape(-1)
        rt = float(np.abs(g[:nt] - gt_ref).max() / np.abs(gt_ref).max())
        ri = float(np.abs(g[nt:] - gi_ref).max() / np.abs(gi_ref).max())
        for k, v in (("logits", el), ("loss", eo), ("g_text", rt), ("g_img", ri)):
            worst[k] = max(worst[k], v)
        assert el <= la and eo <= la and rt <= gr and ri <= gr, \
            f"B={B} [{mode}]: logits err {el:.3e}, loss err {eo:.3e} (bound {la}); g_text rel {rt:.3e}, g_img rel {ri:.3e} (bound {gr})"
        rows[B] = (le.cpu(), fe.view(B, K, e).cpu())
    # batch composition must not change an image's result
    pairs = 0
    first_of = {}
    for B in _order(mb):
        ref = mb if mode == "f32" else first_of.setdefault(plans[B], B)
        if ref == B:
            continue
        n = min(B, ref)
        same = torch.equal(rows[B][0][:n], rows[ref][0][:n]) and torch.equal(rows[B][1][:n], rows[ref][1][:n])
        assert same, f"[{mode}] images 0..{n - 1}: logits / img_f at B={B} differ from B={ref}" + \
            ("" if mode == "f32" else " although every image-tower GEMM runs the same plan")
        pairs += 1
    # coverage is asserted, not assumed
    nt_codes = {c[1] for p in plans.values() for c in p if c[0] == "nt"}
    has_ws = any(c[0] == "ws" for p in plans.values() for c in p)
    row_unit_partial = [B for B in plans if B < mb and {10, 11} <= {c[1] for c in plans[B] if c[0] == "nt"}]
    if (sweep, mode) == ("b16_k24_mb32", "bf16"):
        assert {5, 6, 2, 8, 10, 11} <= nt_codes and has_ws, (sorted(nt_codes), has_ws)
        assert row_unit_partial, "no batch size below 32 runs the row-unit kernels in a partial round"
    if sweep == "l14_k24_mb16":
        assert {10, 11} <= nt_codes, sorted(nt_codes)
        # (N = 4096 / 1024 admit only the 288-row geometries; their residual GEMMs write 64-column statistics)
        assert all(c[2] == 64 for p in plans.values() for c in p if c[0] == "nt" and c[1] == 11)
        assert row_unit_partial, "no batch size below 16 runs the 288-row kernels in a partial round"
    if sweep == "b16_k24_mb4":
        assert all(any(c[0] == "ws" for c in plans[B]) for B in plans)
    if sweep == "b32_k24_mb32" and mode != "f32":
        # (74-row units in 224-row tiles: both one-round kernels, below B = 32 in a partial round, the split-k one with its
        #  96-column statistics)
        assert {10, 11} <= nt_codes, sorted(nt_codes)
        assert row_unit_partial, "no batch size below 32 runs the row-unit kernels in a partial round"
        assert all(any(c[:2] == ("nt", 11) and c[2] == 96 for c in plans[B]) for B in row_unit_partial + [mb])
    if sweep == "l14_336_k24_mb16":
        # (601 rows per image: no row units; c_fc on the 288x256 geometry in contiguous tiles, 64-column statistics
        #  throughout, rpo_gemm_ws for the prompt rows only)
        assert {2, 8, 10} <= nt_codes and 11 not in nt_codes, sorted(nt_codes)
        assert all(c[2] == 64 for p in plans.values() for c in p if c[0] == "nt")
        assert all(n <= 1024 for n in rec.ws_rows), f"rpo_gemm_ws at {max(rec.ws_rows)} rows"
    print(f"\n[{sweep} {mode}] plan table (tile_config[/96-column statistics] of the image-forward GEMMs):\n{_regimes(plans)}")
    print(f"[{sweep} {mode}] worst vs oracle: logits {worst['logits']:.3e} loss {worst['loss']:.3e} "
          f"g_text {worst['g_text']:.3e} g_img {worst['g_img']:.3e}; {pairs} bit-identity pairs; {time.time() - t0:.1f} s")
