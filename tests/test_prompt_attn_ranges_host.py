"""The budgets of tests/test_gpu_prompt_attn_ranges.py are attainable: a float32 emulation of the two arrangements of
rpo_attn_prompt_fwd / rpo_attn_prompt_bwd lies within them, on the CPU, for every shape and storage mode of that module.

The emulation is written from attn_prompt_fwd_kernel / attn_prompt_bwd_kernel (rpo_amd/csrc/attn_image.hip), plain
PyTorch in float32, one query row per row:
  forward   online softmax over 32-key tiles in ascending order: mn = max(m, tile maximum), alpha = exp((m - mn) scale),
            p = exp((s - mn) scale), l = l alpha + sum p, o = o alpha + p . V with p rounded to the storage type in the
            16-bit modes (the sum l takes the unrounded p), out = o (1 / l) rounded to the storage type.  The 16-bit
            modes exponentiate as exp2(fma(s, c, -(m c))) with c = scale log2 e, the f32 mode as expf((s - m) scale).
  backward  pass 1 carries m, l and dsum = sum p o dP online (dsum = dsum alpha + sum p dP, dP = da . V^T), delta = dsum / l;
            pass 2 recomputes p with the FINAL m, forms dS = (p / l)(dP - delta) in fp32, rounds it ONCE to the storage
            type (16-bit modes) and contracts it with K; dq = scale (dS . K) rounded to the storage type.
So a GPU failure of a budget points at the kernel, not at the budget.  Inputs, float64 reference, budgets, tolerances and
floors are those of the GPU module (test_gpu_ranges.attn64, TOL, FLOOR); no number is set here.
"""
import math

import pytest
import torch

import test_gpu_prompt_attn_ranges as P
from helpers import assert_within
from test_gpu_ranges import DT, FLOOR, HD, SCALE

LOG2E = 1.4426950408889634


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def _heads(x, H):
    return x.reshape(x.shape[0], H, HD).transpose(0, 1).contiguous()


def _rows(x):
    return x.transpose(0, 1).reshape(x.shape[1], -1)


class Emulation:
    """one image: qh / dah [H, R, 64], kh / vh [H, N, 64], float32 copies of the stored values"""

    def __init__(self, mode):
        self.mode, self.dt = mode, DT[mode]
        self.scale = _f32(SCALE)
        self.c = self.scale * _f32(LOG2E)

    def rt(self, x):
        return x if self.mode == "f32" else x.to(self.dt).to(torch.float32)

    def p_of(self, sc, m):
        if self.mode == "f32":
            return torch.exp((sc - m) * self.scale)
        mc = m * self.c                                               # fma(s, c, -mc): one rounding
        return torch.exp2((sc.double() * self.c.double() - mc.double()).to(torch.float32))

    def alpha_of(self, dm):
        return torch.exp(dm * self.scale) if self.mode == "f32" else torch.exp2(dm * self.scale * _f32(LOG2E))

    def tiles(self, n):
        return [slice(32 * t, min(32 * t + 32, n)) for t in range((n + 31) // 32)]

    def fwd(self, qh, kh, vh):
        H, R, _ = qh.shape
        m, l, o = torch.full((H, R, 1), -math.inf), torch.zeros(H, R, 1), torch.zeros(H, R, HD)
        for t in self.tiles(kh.shape[1]):
            sc = qh @ kh[:, t].transpose(1, 2)
            mn = torch.maximum(m, sc.amax(-1, keepdim=True))
            alpha = self.alpha_of(m - mn)                             # first tile: exp(-inf) = 0
            p = self.p_of(sc, mn)
            l = l * alpha + p.sum(-1, keepdim=True)
            o = o * alpha + self.rt(p) @ vh[:, t]
            m = mn
        return self.rt(o * (1.0 / l))

    def bwd(self, qh, kh, vh, dah):
        H, R, _ = qh.shape
        m, l, dsum = torch.full((H, R, 1), -math.inf), torch.zeros(H, R, 1), torch.zeros(H, R, 1)
        for t in self.tiles(kh.shape[1]):                             # pass 1
            sc = qh @ kh[:, t].transpose(1, 2)
            dp = dah @ vh[:, t].transpose(1, 2)
            mn = torch.maximum(m, sc.amax(-1, keepdim=True))
            alpha = self.alpha_of(m - mn)
            p = self.p_of(sc, mn)
            l = l * alpha + p.sum(-1, keepdim=True)
            dsum = dsum * alpha + (p * dp).sum(-1, keepdim=True)
            m = mn
        inv = 1.0 / l
        delta = dsum * inv
        u = torch.zeros(H, R, HD)
        for t in self.tiles(kh.shape[1]):                             # pass 2: the final m
            p = self.p_of(qh @ kh[:, t].transpose(1, 2), m)
            dp = dah @ vh[:, t].transpose(1, 2)
            u = u + self.rt((p * inv) * (dp - delta)) @ kh[:, t]
        return self.rt(self.scale * u)


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("shape", P.SHAPES, ids=P.IDS)
def test_emulated_arrangements_lie_within_the_float64_budgets(shape, mode):
    sets, B, H, N, Kp = shape
    d = HD * H
    stored = lambda t: t.to(DT[mode]).to(torch.float32)
    qr, kv, da = (stored(t) for t in P.inputs(shape))
    ref = P.reference(shape, mode)
    em = Emulation(mode)
    out, dq = torch.empty(sets * B * Kp, d), torch.empty(sets * B * Kp, d)
    for b in range(B):
        rows = P.image_rows(sets, B, Kp, b)
        qh, dah, kh, vh = _heads(qr[rows], H), _heads(da[rows], H), _heads(kv[b, :, :d], H), _heads(kv[b, :, d:], H)
        out[rows], dq[rows] = _rows(em.fwd(qh, kh, vh)), _rows(em.bwd(qh, kh, vh, dah))
    what = f"emulated attn prompt {mode} " + "x".join(map(str, shape))
    wf = assert_within(out, ref["out"], ref["b_out"], what + " fwd", floor=FLOOR[mode])
    wb = assert_within(dq, ref["dq"], ref["b_dq"], what + " bwd", floor=FLOOR[mode])
    print(f"[{what}] worst err / budget fwd {wf:.3f} bwd {wb:.3f}")
