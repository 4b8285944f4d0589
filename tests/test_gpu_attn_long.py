"""The image tower's read-only attention above 288 frozen tokens (attn_fwd_long_kernel / attn_bwd_long_kernel: the keys
in chunks of C = 256 under an online softmax; ViT-L/14 at 336 px has N = 577) against float64, on the MI355X.

Tolerances are tests/test_gpu_ops.py's for the same ops (`close`: the mode default for the forward, 3e-2 in the 16-bit
modes for the backward); the sharp-score cases use tests/test_gpu_ranges.py's generators and per-element budgets.
Every N > 288 case fails on a library without the long kernels with RPO_E_SHAPE.
"""
import hashlib
import json
import os

import pytest
import torch

import test_gpu_ops as TO
import test_gpu_ranges as TR
from helpers import GOLDEN, assert_within

pytestmark = pytest.mark.gpu

from oracle import rows_oracle as R  # noqa: E402  (checker only)

DT = TO.DT
C = 256                 # keys per chunk (csrc/attn_image.hip: LONG_NT * 32)
LIMIT = 1025            # include/rpo_amd.h: N <= 1025
GUARD = 4096            # elements of NaN in front of and behind every buffer (a multiple of 64: 16-byte alignment holds)
MODES = ["f32", "bf16", "f16"]

# (N, B, H, Kp): the first sizes past the old limit, the chunk size and its neighbours (C and C + 1 still run the old
# kernels), one / two / three chunks with a last chunk of 1, 32 k and 32 k + 1 keys, ViT-L/14@336 and the upper limit
SHAPES = [(289, 2, 3, 24), (320, 1, 2, 0), (321, 2, 1, 33), (C, 1, 2, 24), (C + 1, 1, 1, 48), (2 * C - 1, 1, 3, 1),
          (2 * C, 2, 2, 48), (2 * C + 1, 1, 2, 24), (577, 2, 3, 24), (577, 1, 1, 33), (LIMIT, 1, 2, 48), (LIMIT, 2, 1, 0)]


def dev():
    return torch.device("cuda:0")


def guarded(rows, cols, dtype):
    """A [rows, cols] view in the middle of a NaN-filled allocation, and the allocation."""
    whole = torch.full((2 * GUARD + rows * cols,), float("nan"), dtype=dtype, device=dev())
    return whole[GUARD:GUARD + rows * cols].view(rows, cols), whole


def guards_intact(whole):
    w = whole.float()
    return bool(torch.isnan(w[:GUARD]).all()) and bool(torch.isnan(w[-GUARD:]).all())


def put(t, mode):
    """`t` on the device inside a NaN-filled allocation (a read outside the matrix poisons the result)."""
    view, whole = guarded(t.shape[0], t.shape[1], DT[mode])
    view.copy_(t.to(DT[mode]))
    return view, whole


def make_qkv(B, H, N, Kp, seed, sharp=1.5):
    """[B (N + Kp), 3d] in the engine's row layout.  The K / V columns of the prompt rows are NaN: nothing may read them
    (the read-only mask, trainers/rpo.py:154-156)."""
    d = 64 * H
    qkv = TO.rnd((B * (N + Kp), 3 * d), seed)
    qkv[:, :d] *= sharp
    qkv[B * N:, d:] = float("nan")
    return qkv


def fwd_ref(q64, B, H, N, Kp):
    d = 64 * H
    ref = torch.empty(B * (N + Kp), d, dtype=torch.float64)
    for b in range(B):
        fr, pr = slice(b * N, (b + 1) * N), slice(B * N + b * Kp, B * N + (b + 1) * Kp)
        k, v = q64[fr, d:2 * d], q64[fr, 2 * d:]
        ref[fr] = R.attn_rows_fwd(q64[fr, :d], k, v, H)
        if Kp:
            ref[pr] = R.attn_rows_fwd(q64[pr, :d], k, v, H)
    return ref


def bwd_ref(q64, da64, B, H, N, Kp):
    d, Rf = 64 * H, B * N
    ref = torch.empty(B * Kp, d, dtype=torch.float64)
    for b in range(B):
        fr, pr = slice(b * N, (b + 1) * N), slice(Rf + b * Kp, Rf + (b + 1) * Kp)
        ref[b * Kp:(b + 1) * Kp] = R.attn_rows_bwd(q64[pr, :d], q64[fr, d:2 * d], q64[fr, 2 * d:], da64[b * Kp:(b + 1) * Kp], H)
    return ref


def run_fwd(t, B, H, N, Kp, mode, q_first=0):
    d = 64 * H
    out, whole = guarded(B * (N + Kp), d, DT[mode])
    TO.ops().attn_readonly_fwd(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], out, B, H, N, Kp, q_first=q_first)
    torch.cuda.synchronize()
    return out, whole


def run_bwd(t, da, B, H, N, Kp, mode):
    d, Rf = 64 * H, B * N
    dq, whole = guarded(B * Kp, d, DT[mode])
    TO.ops().attn_readonly_bwd(t[Rf:, :d], t[:Rf, d:2 * d], t[:Rf, 2 * d:], da, dq, B, H, N, Kp)
    torch.cuda.synchronize()
    return dq, whole


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,B,H,Kp", SHAPES)
def test_attn_long_fwd_against_float64(mode, N, B, H, Kp):
    qkv = make_qkv(B, H, N, Kp, 31)
    t, _ = put(qkv, mode)
    out, whole = run_fwd(t, B, H, N, Kp, mode)
    assert guards_intact(whole), "a guard element was overwritten"
    assert not torch.isnan(out.float()).any(), "a row was not written, or something read outside its image's keys"
    TO.close(out, fwd_ref(TO.q(qkv, mode), B, H, N, Kp), mode, f"attn fwd B{B} H{H} N{N} K{Kp}")
    if Kp:                                  # the last block's form: the prompt rows alone, same bits, nothing else written
        part, pw = run_fwd(t, B, H, N, Kp, mode, q_first=N)
        assert guards_intact(pw) and torch.isnan(part[:B * N].float()).all(), "q_first = N wrote a frozen row"
        assert torch.equal(part[B * N:], out[B * N:]), "q_first = N: prompt rows differ from the full launch"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,B,H,Kp", [s for s in SHAPES if s[3] > 0])
def test_attn_long_bwd_against_float64(mode, N, B, H, Kp):
    qkv, da = make_qkv(B, H, N, Kp, 32, sharp=1.0), TO.rnd((B * Kp, 64 * H), 33)
    t, _ = put(qkv, mode)
    dad, _ = put(da, mode)
    dq, whole = run_bwd(t, dad, B, H, N, Kp, mode)
    assert guards_intact(whole), "a guard element was overwritten"
    assert not torch.isnan(dq.float()).any()
    TO.close(dq, bwd_ref(TO.q(qkv, mode), TO.q(da, mode), B, H, N, Kp), mode, f"attn bwd B{B} H{H} N{N} K{Kp}",
             tol=None if mode == "f32" else 3e-2)


@pytest.mark.parametrize("mode", MODES)
def test_attn_long_refuses_above_the_limit_and_writes_nothing(mode):
    from rpo_amd._lib import E_SHAPE, RPOLibraryError
    B, H, N, Kp = 1, 1, LIMIT + 1, 24
    qkv, da = make_qkv(B, H, N, Kp, 34), TO.rnd((B * Kp, 64 * H), 35)
    t, _ = put(qkv, mode)
    dad, _ = put(da, mode)
    out, whole = guarded(B * (N + Kp), 64 * H, DT[mode])
    dq, dwhole = guarded(B * Kp, 64 * H, DT[mode])
    d = 64 * H
    with pytest.raises(RPOLibraryError, match=f"code {E_SHAPE}"):
        TO.ops().attn_readonly_fwd(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], out, B, H, N, Kp)
    with pytest.raises(RPOLibraryError, match=f"code {E_SHAPE}"):
        TO.ops().attn_readonly_fwd(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], out, B, H, N, Kp, q_first=N)
    with pytest.raises(RPOLibraryError, match=f"code {E_SHAPE}"):
        TO.ops().attn_readonly_bwd(t[N:, :d], t[:N, d:2 * d], t[:N, 2 * d:], dad, dq, B, H, N, Kp)
    torch.cuda.synchronize()
    assert torch.isnan(whole.float()).all() and torch.isnan(dwhole.float()).all(), "a refused call wrote something"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,B,H,Kp", [(577, 2, 3, 24), (2 * C + 1, 2, 2, 33)])
def test_attn_long_bits_do_not_depend_on_the_batch_or_the_call(mode, N, B, H, Kp):
    """A whole-batch launch gives the bits of image-by-image launches, and a second call the bits of the first (fixed
    summation order, no atomics)."""
    d, Rf, S = 64 * H, B * N, N + Kp
    qkv, da = make_qkv(B, H, N, Kp, 36), TO.rnd((B * Kp, d), 37)
    t, _ = put(qkv, mode)
    dad, _ = put(da, mode)
    out, _ = run_fwd(t, B, H, N, Kp, mode)
    dq, _ = run_bwd(t, dad, B, H, N, Kp, mode)
    for b in range(B):
        one, _ = put(torch.cat([qkv[b * N:(b + 1) * N], qkv[Rf + b * Kp:Rf + (b + 1) * Kp]]), mode)
        o1, _ = run_fwd(one, 1, H, N, Kp, mode)
        assert torch.equal(o1[:N], out[b * N:(b + 1) * N]) and torch.equal(o1[N:], out[Rf + b * Kp:Rf + (b + 1) * Kp]), b
        d1, _ = run_bwd(one, dad[b * Kp:(b + 1) * Kp], 1, H, N, Kp, mode)
        assert torch.equal(d1, dq[b * Kp:(b + 1) * Kp]), b
    assert torch.equal(run_fwd(t, B, H, N, Kp, mode)[0], out)
    assert torch.equal(run_bwd(t, dad, B, H, N, Kp, mode)[0], dq)


# ---- N <= 288: the kernels and the bits of the parent commit ---------------------------------------------------------
PARENT_CASES = [(197, 2, 3, 24), (257, 1, 2, 33)]
PARENT_BITS = os.path.join(GOLDEN, "attn_parent_bits.json")


def short_bits(mode, N, B, H, Kp):
    """sha256 of the forward output and of the backward dq at one N <= 288 shape (tools/capture_attn_bits.py records
    them with a library built from the parent commit, on the same device type)."""
    qkv, da = make_qkv(B, H, N, Kp, 38), TO.rnd((B * Kp, 64 * H), 39)
    t, _ = put(qkv, mode)
    dad, _ = put(da, mode)
    out, _ = run_fwd(t, B, H, N, Kp, mode)
    dq, _ = run_bwd(t, dad, B, H, N, Kp, mode)
    h = lambda x: hashlib.sha256(x.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
    return {"fwd": h(out), "bwd": h(dq)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,B,H,Kp", PARENT_CASES)
def test_attn_up_to_288_tokens_keeps_the_parent_commits_bits(mode, N, B, H, Kp):
    want = json.load(open(PARENT_BITS))["bits"][f"{mode}_N{N}_B{B}_H{H}_K{Kp}"]
    assert short_bits(mode, N, B, H, Kp) == want


# ---- sharp scores across the chunks ------------------------------------------------------------------------------------
def sharp_qkv(B, H, N, Kp, seed):
    """tests/test_gpu_ranges.py's score patterns, head h following PATTERNS[h % 6]: a sink key 45 above the rest, a peak
    at the LAST key with every earlier chunk 110 below (the rescale factor underflows to 0), a peak in the first chunk
    (exact zeros afterwards), near-uniform rows at +80 and at -200 -- and, for "ties", exactly equal maxima in two
    DIFFERENT chunks (the generator's second tie key is copied into the second chunk, other lane half)."""
    d = TR.HD * H
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * (N + Kp), 3 * d, generator=g)
    for b in range(B):
        rows = TR._image_rows(B, N, Kp, b)
        for h in range(H):
            pattern = TR.PATTERNS[h % len(TR.PATTERNS)]
            qh, kh = torch.empty(N + Kp, TR.HD), torch.empty(N, TR.HD)
            TR._fill(qh, kh, pattern, g)
            if pattern == "ties":
                kh[C + 36] = kh[TR._tie_keys(N)[0]]
            qkv[rows, h * TR.HD:(h + 1) * TR.HD] = qh
            qkv[b * N:(b + 1) * N, d + h * TR.HD:d + (h + 1) * TR.HD] = kh
    return qkv


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", [577, 2 * C])
def test_attn_long_fwd_sharp_scores(mode, N):
    B, H, Kp = 1, 6, 24
    d, dt = TR.HD * H, DT[mode]
    qkv = sharp_qkv(B, H, N, Kp, 41)
    t, _ = put(qkv, mode)
    out, whole = run_fwd(t, B, H, N, Kp, mode)
    assert guards_intact(whole)
    q64 = TR.q(qkv, mode)
    r = TR.attn64(q64[:, :d], q64[:N, d:2 * d], q64[:N, 2 * d:], H, TR.TOL[mode])
    assert TR._max_weight(r["p"]) > 0.999                           # the rows are as sharp as intended
    w = assert_within(out, r["out"], r["b_out"], f"attn long fwd {mode} N{N}", floor=TR.FLOOR[mode])
    print(f"[attn long fwd {mode} N{N}] worst err / budget {w:.3f}")
    part, _ = run_fwd(t, B, H, N, Kp, mode, q_first=N)
    assert torch.equal(part[N:], out[N:])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,Kp", [(577, 24), (2 * C, 33)])
def test_attn_long_bwd_sharp_scores(mode, N, Kp):
    B, H = 1, 6
    d = TR.HD * H
    qkv, da = sharp_qkv(B, H, N, Kp, 42), TR.rnd((B * Kp, d), 43)
    t, _ = put(qkv, mode)
    dad, _ = put(da, mode)
    dq, whole = run_bwd(t, dad, B, H, N, Kp, mode)
    assert guards_intact(whole)
    q64, da64 = TR.q(qkv, mode), TR.q(da, mode)
    r = TR.attn64(q64[N:, :d], q64[:N, d:2 * d], q64[:N, 2 * d:], H, TR.TOL[mode], do=da64)
    w = assert_within(dq, r["dq"], r["b_dq"], f"attn long bwd {mode} N{N} K{Kp}", floor=TR.FLOOR[mode])
    print(f"[attn long bwd {mode} N{N} K{Kp}] worst err / budget {w:.3f}")
