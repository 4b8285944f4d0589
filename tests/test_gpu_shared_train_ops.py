"""rpo_attn_prompt_bwd, the backward twin of rpo_attn_prompt_fwd (the shared-batch sweep step), at op level.

Against float64 (oracle.rows_oracle.attn_rows_bwd per (set, image)) at tests/test_gpu_ops.py's TOL relative to the
reference's maximum, in the three storage modes; K / V inside a packed in-proj matrix (first_image = NULL, ldkv = 3 d) and
inside a cache (first_image = 1, ldkv = 2 d); ldq / ldda / lddq that are not d, guard elements around dq and its padding
columns untouched; set s of a multi-set launch bit for bit the launch of that set alone; a second launch the same bits.
"""
import math

import pytest
import torch

from test_gpu_ops import DT, TOL as OP_TOL

pytestmark = pytest.mark.gpu

from oracle import rows_oracle as R  # noqa: E402  (checker only)

DEV = torch.device("cuda:0")
GUARD = 64

SHAPES = [(3, 2, 2, 197, 24),
          (8, 1, 2, 50, 7),            # tiles mix sets
          (2, 3, 1, 257, 48),
          (1, 1, 1, 5, 1),
          (3, 1, 2, 224, 40),
          (2, 1, 1, 225, 24),          # the first NT = 9 shape
          (1, 2, 1, 288, 33),          # the limit
          (12, 1, 1, 33, 24)]          # 9 query tiles for 8 waves: a wave takes a second tile


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


def _same(a, b):
    return bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def _guarded(rows, ld, dtype):
    whole = torch.full((rows * ld + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + rows * ld].view(rows, ld)


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("sets,B,H,N,Kp", SHAPES)
def test_attn_prompt_bwd_against_float64(mode, sets, B, H, N, Kp):
    from rpo_amd import ops
    dt, d = DT[mode], 64 * H
    Rq = sets * B * Kp
    ldq, ldda, lddq = d + 8, d + 24, d + 16
    q_dev = (_rnd((Rq, ldq), 41) * 1.5).to(DEV, dt)                 # sharper softmax, as the forward's test
    da_dev = _rnd((Rq, ldda), 42).to(DEV, dt)
    q64, da64 = q_dev.cpu().to(torch.float64)[:, :d], da_dev.cpu().to(torch.float64)[:, :d]
    packed = _rnd((B * (N + Kp), 3 * d), 43)
    cache = _rnd((4 * N, 2 * d), 44)
    first = torch.tensor([1], dtype=torch.int32, device=DEV)
    layouts = [("packed", packed.to(DEV, dt), d, None, 0), ("cache", cache.to(DEV, dt), 0, first, 1)]
    for name, kv, c0, fi, f0 in layouts:
        k, v = kv[:, c0:c0 + d], kv[:, c0 + d:c0 + 2 * d]
        kv64 = kv.cpu().to(torch.float64)
        whole, dq = _guarded(Rq, lddq, dt)
        ops.attn_prompt_bwd(q_dev, k, v, da_dev, dq, B, H, N, Kp, sets, first_image=fi)
        torch.cuda.synchronize()
        ref = torch.empty(Rq, d, dtype=torch.float64)
        for s in range(sets):
            for b in range(B):
                rows = slice((s * B + b) * Kp, (s * B + b + 1) * Kp)
                fr = slice((f0 + b) * N, (f0 + b + 1) * N)
                ref[rows] = R.attn_rows_bwd(q64[rows], kv64[fr, c0:c0 + d], kv64[fr, c0 + d:c0 + 2 * d], da64[rows], H)
        got = dq[:, :d].to(torch.float64).cpu()
        err, den = (got - ref).abs().max().item(), max(ref.abs().max().item(), 1e-30)
        what = f"attn prompt bwd {name} sets{sets} B{B} H{H} N{N} K{Kp}"
        print(f"{what} [{mode}]: max err {err:.3e} vs max ref {den:.3e} (rel {err / den:.2e}, bound {OP_TOL[mode]})")
        assert math.isfinite(err) and err <= OP_TOL[mode] * den, f"{what} [{mode}]: rel {err / den:.2e} > {OP_TOL[mode]}"
        w = whole.float().cpu()
        assert bool(torch.isnan(w[:GUARD]).all()) and bool(torch.isnan(w[-GUARD:]).all()), f"{name}: guard elements written"
        assert bool(torch.isnan(dq[:, d:].float()).all()), f"{name}: padding columns of dq written"
        # a second launch: the same bits
        _, again = _guarded(Rq, lddq, dt)
        ops.attn_prompt_bwd(q_dev, k, v, da_dev, again, B, H, N, Kp, sets, first_image=fi)
        assert _same(again[:, :d], dq[:, :d]), f"{name}: a second launch gave other bits"
        # each set alone: the same bits
        if sets > 1:
            for s in range(sets):
                rows = slice(s * B * Kp, (s + 1) * B * Kp)
                _, one = _guarded(B * Kp, lddq, dt)
                ops.attn_prompt_bwd(q_dev[rows], k, v, da_dev[rows], one, B, H, N, Kp, 1, first_image=fi)
                assert _same(one[:, :d], dq[rows, :d]), f"{name}: set {s} of {sets} != its own launch"
            assert not _same(dq[:B * Kp, :d], dq[B * Kp:2 * B * Kp, :d])          # (the sets really differ)
