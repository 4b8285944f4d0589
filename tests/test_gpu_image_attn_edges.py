"""The image tower's attention up to 288 frozen tokens (rpo_amd/csrc/attn_image.hip) at its edge shapes, per element
against float64.

tests/test_gpu_image_attn_bits.py pins 136 cases to the bits of an earlier commit: that shows that nothing changed, not
that the earlier commit was right.  Here every pinned shape with N <= 288, and the shapes around every tile remainder, is
held to tests/test_gpu_ranges.attn64 with its elementwise budgets (TOL, GAM, FLOOR as they stand; for the folded out-proj
the dp_rel = ULP and do_abs terms of test_attn_image_bwd_sharp_scores).  No tolerance is introduced here.

Inputs ("edge peaks", `inputs`).  The edge keys of an image of N keys are key 0, key N - 1 and, for every 32-key tile
boundary inside N, the keys 32 t - 1 and 32 t: the keys a wrong `nfull`, `rem`, tile skip or mask loses or gains first.
Edge key number i (in ascending order) holds 45 in column 1 + i of its K row and zeros in the other edge columns; a query
that is to peak at it holds 8 there (score 45 above the rest); everything else is N(0, 0.5^2), V and d_out are N(0, 1).
The query slots of a case, counted over (set, image, head, row), rotate over a list of jobs (`plan`):
  * with at least two slots per edge key: one dominant query per edge key, and one tie per edge key -- a query that is zero
    outside the columns of that key and of a partner in ANOTHER key tile (where N has more than one), so that the two scores
    are exactly equal (8 * 45 / 8, every other product an exact zero).  A one-hot row has dS ~ 0 and says little in the
    backward; a tie has dS = (dP_a - dP_b) / 4 on both keys.
  * with fewer slots (Kp = 1 cases): every query is an exact tie over ceil(edge keys / slots) (at least two) edge keys,
    and the tied keys' dP alternate in sign (+-8 in column 0 of their V rows, 8 in column 0 of d_out; see `inputs`).
    Such a case cannot give every edge key 0.4 of a row (288 / 1 at B = 1, H = 2 has two queries for 18 edge keys); what
    it must give is stated with `min_edge_weight`, and the mutants of the host test are what counts.
The layout is test_gpu_attn_long's: NaN in the K / V columns of the prompt rows, every buffer inside a NaN-filled
allocation, every output pre-filled with NaN.  The row after an image's keys is the next image's key 0 -- a peak key -- or,
after the last image, NaN: one key too many is a gross error.

tests/test_image_attn_edges_host.py shows on the CPU that the tables reach every path the dispatch distinguishes, that the
float64 result rounded to the storage type uses at most half of each budget, and that a reference with one defect (an edge
key dropped, key N read, a query row shifted, a set reading set 0's queries) leaves the budget by a factor of at least 4.
"""
import functools

import pytest
import torch

import test_gpu_attn_long as TL
import test_gpu_image_attn_bits as TB
import test_gpu_ops as TO
import test_gpu_ranges as TR
from helpers import assert_within

pytestmark = pytest.mark.gpu

MODES, HALF, HD = TL.MODES, TB.HALF, TR.HD
PEAK_K, PEAK_Q = 45.0, 8.0
CUS_ASSUMED = 256                 # the host test's device: an MI355X (the GPU tests read the real count)
# ---- case tables ---------------------------------------------------------------------------------------------------------
# rpo_attn_readonly_fwd_rows, (N, B, H, Kp, q_first): the pinned cases, then N in {1, 31, 32, 33, 64, 224, 225} with Kp in
# {0, 1, 31, 32, 33} so that S = N + Kp lands on a multiple of 32 (32, 64, 256), one below (31, 95) and one above (33, 97,
# 257: S > 256, a wave's second query tile, at NT = 7 and NT = 9).  B >= 2: the row after image 0's keys is a peak key.
FWD = list(TB.FWD) + [(1, 3, 2, 0, 0), (1, 2, 1, 31, 0), (31, 2, 2, 0, 0), (31, 2, 1, 1, 0), (32, 2, 1, 0, 0), (32, 2, 2, 1, 0),
                      (33, 2, 2, 31, 0), (64, 2, 1, 31, 0), (64, 2, 3, 33, 0), (224, 2, 2, 32, 0), (224, 2, 1, 33, 0),
                      (225, 2, 2, 31, 0), (225, 2, 1, 32, 0), (256, 2, 1, 0, 0)]      # (256: rem == 0 with a tile skipped at NT = 9)
# q_first anywhere in [0, N + Kp): one NT = 7 shape, one NT = 9 shape, one long shape; (N, B, H, Kp)
QFIRST_SHAPES = [(197, 2, 2, 24), (257, 2, 1, 33), (321, 2, 1, 33)]
# the two-phase kernel, (N, Kp, q_first) at H = 12 and B = CUs // 12 + 1
FWD_2PHASE = list(TB.FWD_2PHASE)
# rpo_attn_readonly_bwd, (N, B, H, Kp): the pinned cases up to 288 keys; one to four query tiles and their remainders at
# NT = 7 and NT = 9; one key, one full tile, one full tile and a key, three full tiles, three and a key
BWD = [c for c in TB.BWD if c[0] <= 288] \
    + [(197, 1 + (kp == 33), 2 - (kp == 33), kp) for kp in (31, 32, 33, 64, 65, 96, 97, 128)] \
    + [(257, 1 + (kp == 65), 2 - (kp == 65), kp) for kp in (31, 32, 33, 64, 65, 96, 97, 128)] \
    + [(1, 2, 2, 5), (32, 2, 2, 5), (33, 2, 1, 24), (96, 2, 2, 7), (97, 2, 1, 33)]
# rpo_attn_readonly_bwd_proj (16-bit; H = d / 64 in {8, 12, 16}), (N, B, H, Kp): the pinned cases; Kp on, over and at twice
# the query tile for every d; the NT switch
BWD_PROJ = list(TB.BWD_PROJ) + [(197, 1, h, kp) for h in (8, 12, 16) for kp in (32, 33, 64)] + [(224, 2, 8, 24), (225, 2, 8, 24)]
# rpo_attn_prompt_fwd / _bwd, (N, B, H, Kp, sets, first): the pinned cases (first as there), then first = "all" (no pointer,
# device scalar 0, device scalar 1 over a 3-image cache with ldkv = 2 d, which must agree bit for bit): Q = sets Kp in
# {31, 32, 33, 256, 257} with sets >= 2 (31 and 257 are prime: Kp = 1) and N in {1, 32, 224, 225, 288}
_pinned_prompt = list(dict.fromkeys(TB.PFWD + TB.PBWD))
PROMPT = _pinned_prompt + [(197, 2, 2, 1, 31, "all"), (32, 2, 1, 16, 2, "all"), (1, 2, 2, 11, 3, "all"),
                           (224, 1, 2, 32, 8, "all"), (225, 2, 1, 1, 257, "all"), (288, 2, 1, 5, 3, "all")]


def ident(p):
    return "_".join(str(x) for x in p)


# ---- the generator -----------------------------------------------------------------------------------------------------
def edge_keys(N):
    e = {0, N - 1}
    for t in range(1, (N - 1) // 32 + 1):
        e.update((32 * t - 1, 32 * t))
    return sorted(e)


def _partner(E, i):
    """index of another edge key, in a different 32-key tile if there is one"""
    n = len(E)
    for o in range(2, n + 2):
        j = (i + o) % n
        if j != i and E[j] // 32 != E[i] // 32:
            return j
    return (i + 1) % n


def plan(N, slots):
    """the jobs the query slots rotate over: tuples of edge-key indices a query peaks at (more than one: an exact tie)"""
    E = edge_keys(N)
    n = len(E)
    if n == 1:
        return [(0,)]
    if slots >= 2 * n:
        return [(i,) for i in range(n)] + [(i, _partner(E, i)) for i in range(n)]
    stride = _wide_tie_stride(N, slots)
    return [tuple(range(i, n, stride)) for i in range(stride)]


def _wide_tie_stride(N, slots):
    """fewer than two slots per edge key: every query ties edge keys i, i + stride, ... (at least two, ceil(n / slots) if
    that is more); None where `plan` has a dominant query and a two-key tie for every edge key"""
    n = len(edge_keys(N))
    if n == 1 or slots >= 2 * n:
        return None
    g = max(2, -(-n // slots))
    return -(-n // g)


def min_edge_weight(N, slots):
    """what every edge key must carry of some row's softmax weight: 0.4 wherever the case has a slot per two edge keys (a
    tie of two gives 1/2 each, less the e^-45-ish weight of the other keys), else 0.8 / g for the g-way ties of `plan`"""
    n = len(edge_keys(N))
    return 0.4 if 2 * slots >= n else 0.8 / max(2, -(-n // slots))


@functools.lru_cache(maxsize=8)
def inputs(N, B, H, R, sets=1):
    """float32, built once per shape and never changed: q / da [sets, B, R, d] (R query rows per image and set), k / v
    [B, N, d]"""
    d = HD * H
    g = torch.Generator().manual_seed(100003 * N + 1009 * R + 101 * B + 11 * H + sets)
    E = edge_keys(N)
    n = len(E)
    qh = torch.randn(sets, B, R, H, HD, generator=g) * 0.5
    kh = torch.randn(B, N, H, HD, generator=g) * 0.5
    v = torch.randn(B, N, d, generator=g)
    da = torch.randn(sets, B, R, d, generator=g)
    cols = [1 + i for i in range(n)]
    kh[:, E, :, 1:1 + n] = 0.0
    kh[:, E, :, cols] = PEAK_K
    jobs = plan(N, sets * B * H * R)
    J = torch.zeros(len(jobs), n, dtype=torch.bool)
    for j, keys in enumerate(jobs):
        J[j, list(keys)] = True
    s_, b_, r_, h_ = torch.meshgrid(torch.arange(sets), torch.arange(B), torch.arange(R), torch.arange(H), indexing="ij")
    slot = ((s_ * B + b_) * H + h_) * R + r_ + s_     # rotates over (set, image, head, row); + s: row j differs between sets
    member = J[slot % len(jobs)]                                          # [sets, B, R, H, n]
    qh[member.sum(-1) > 1] = 0.0
    qh[..., 1:1 + n] = member.float() * PEAK_Q
    stride = _wide_tie_stride(N, sets * B * H * R)
    if stride is not None:
        # A wide tie shows a dropped key e in the backward through dS_e = P_e (dP_e - delta) alone, by the factor
        # |dP_e - delta| / (TOL (|dP_e| + sum P |dP|)): with N(0, 1) draws alone that is small wherever dP_e happens to lie
        # next to delta.  So the tied keys' dP alternate in sign: +-8 in column 0 of their V rows, 8 in column 0 of d_out
        # (dP_e = +-64 +- 8, delta near 0)
        sign = torch.tensor([(-1.0) ** (i // stride) for i in range(n)])
        v.view(B, N, H, HD)[:, E, :, 0:1] = (PEAK_Q * sign).view(1, n, 1, 1)
        da.view(sets, B, R, H, HD)[..., 0] = PEAK_Q
    return qh.reshape(sets, B, R, d), kh.reshape(B, N, d), v, da


def _seeded(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def packed(qr, k, v, Kp):
    """[B (N + Kp), 3 d] in the engine's row layout from qr [B, R, d] (R = N + Kp: every row's query; R = Kp: the prompt
    rows', the frozen rows' q columns are noise), k / v [B, N, d]; NaN in the K / V columns of the prompt rows"""
    B, N, d = k.shape
    t = _seeded((B * (N + Kp), 3 * d), 7)
    t[:B * N, d:2 * d], t[:B * N, 2 * d:] = k.reshape(B * N, d), v.reshape(B * N, d)
    t[B * N:, d:] = float("nan")
    if qr.shape[1] == N + Kp:
        t[:B * N, :d] = qr[:, :N].reshape(B * N, d)
    t[B * N:, :d] = qr[:, qr.shape[1] - Kp:].reshape(B * Kp, d)
    return t


def unpack(out, B, N, Kp):
    """[B (N + Kp), d] in the engine's row layout -> [B, N + Kp, d]"""
    return torch.stack([out[TR._image_rows(B, N, Kp, b)] for b in range(B)])


def w_out_of(H):
    d = HD * H
    return TR.rnd((d, d), 15 + H, d ** -0.5)


@functools.lru_cache(maxsize=6)
def reference(mode, N, B, H, R, sets=1, proj=False):
    """float64 on the values the kernels read in `mode`: out / dq [sets, B, R, d] with attn64's budgets, the softmax
    weights' maximum per edge key, and the rows' maximum.  proj: d_out = the act-dtype rounding of dx . W_out (dx =
    inputs' da), budgets with the dp_rel = ULP and do_abs = |dx| . |W_out| terms of test_attn_image_bwd_sharp_scores."""
    d = HD * H
    q, k, v, da = (TR.q(t, mode) for t in inputs(N, B, H, R, sets))
    kw = {}
    if proj:
        w = TR.q(w_out_of(H), mode)
        kw = dict(dp_rel=TR.ULP[mode], do_abs=(da.abs() @ w.abs()))
        da = TR.q((da @ w).float(), mode)
    r = {n_: torch.empty(sets, B, R, d, dtype=torch.float64) for n_ in ("out", "b_out", "dq", "b_dq")}
    E = edge_keys(N)
    wmax = torch.zeros(len(E), dtype=torch.float64)
    for b in range(B):
        extra = {k_: v_[:, b].reshape(sets * R, d) for k_, v_ in kw.items() if torch.is_tensor(v_)}
        a = TR.attn64(q[:, b].reshape(sets * R, d), k[b], v[b], H, TR.TOL[mode], do=da[:, b].reshape(sets * R, d),
                      dp_rel=kw.get("dp_rel", 0.0), **extra)
        for n_ in r:
            r[n_][:, b] = a[n_].reshape(sets, R, d)
        wmax = torch.maximum(wmax, a["p"][:, :, E].amax((0, 1)))
    r["edge_weight"] = wmax
    return r


# ---- launches ------------------------------------------------------------------------------------------------------------
def _check(got, ref, bnd, what, mode):
    w = assert_within(got, ref, bnd, what, floor=TR.FLOOR[mode])
    print(f"[{what}] worst err / budget {w:.3f}")
    return w


def _fwd(mode, qr, k, v, Kp, q_first=0):
    """one forward launch; returns out [B, N + Kp, d] after checking the guards"""
    B, N, d = k.shape
    H = d // HD
    t, _ = TL.put(packed(qr, k, v, Kp), mode)
    out, whole = TL.run_fwd(t, B, H, N, Kp, mode, q_first=q_first)
    assert TL.guards_intact(whole), "a guard element was overwritten"
    return unpack(out, B, N, Kp)


def _bwd(mode, qr, k, v, da, Kp):
    """one rpo_attn_readonly_bwd launch; returns dq [B, Kp, d]"""
    B, N, d = k.shape
    t, _ = TL.put(packed(qr, k, v, Kp), mode)
    dad, _ = TL.put(da.reshape(B * Kp, d), mode)
    dq, whole = TL.run_bwd(t, dad, B, d // HD, N, Kp, mode)
    assert TL.guards_intact(whole), "a guard element was overwritten"
    return dq.view(B, Kp, d)


def _bwd_proj(mode, qr, k, v, dx, Kp, two_launch=False):
    """rpo_attn_readonly_bwd_proj, or the GEMM + rpo_attn_readonly_bwd pair it replaces; returns dq [B, Kp, d]"""
    from rpo_amd import _lib as L
    B, N, d = k.shape
    H, Rf, o = d // HD, B * N, TO.ops()
    t, _ = TL.put(packed(qr, k, v, Kp), mode)
    dxd, _ = TL.put(dx.reshape(B * Kp, d), mode)
    w_t, _ = TL.put(w_out_of(H).t().contiguous(), mode)                   # [in, out]: the dX-GEMM packing
    dq, whole = TL.guarded(B * Kp, d, TL.DT[mode])
    if two_launch:
        da, _ = TL.guarded(B * Kp, d, TL.DT[mode])
        o.gemm_nt(dxd, w_t, da, L.EPI_NONE)
        o.attn_readonly_bwd(t[Rf:, :d], t[:Rf, d:2 * d], t[:Rf, 2 * d:], da, dq, B, H, N, Kp)
    else:
        o.attn_readonly_bwd_proj(t[Rf:, :d], t[:Rf, d:2 * d], t[:Rf, 2 * d:], dxd, w_t, dq, B, H, N, Kp)
    torch.cuda.synchronize()
    assert TL.guards_intact(whole), "a guard element was overwritten"
    return dq.view(B, Kp, d)


def _prompt(mode, q, k, v, da, first, sets=None):
    """rpo_attn_prompt_fwd and _bwd of q / da [sets, B, Kp, d] over k / v [B, N, d]; first: None = no pointer, 0 = device
    scalar 0 (both over the packed in-proj layout), "dev1" = device scalar 1 over a 3-image cache [3 N, 2 d] whose other
    images repeat image 0 (so the row after the launch's last image is a peak key, or the end of the allocation).
    Returns (out, dq) [sets, B, Kp, d]."""
    B, N, d = k.shape
    sets = q.shape[0] if sets is None else sets
    H, Kp, o, dt = d // HD, q.shape[2], TO.ops(), TL.DT[mode]
    qd, _ = TL.put(q.reshape(-1, d), mode)
    dad, _ = TL.put(da.reshape(-1, d), mode)
    if first == "dev1":
        assert B <= 2
        imgs = [0] + list(range(B)) + [0] * (2 - B)
        kv, _ = TL.put(torch.cat([torch.cat([k[i], v[i]], 1) for i in imgs]), mode)
        kd, vd, fi = kv[:, :d], kv[:, d:], torch.tensor([1], dtype=torch.int32, device=TL.dev())
    else:
        t, _ = TL.put(packed(q[0], k, v, Kp), mode)
        kd, vd = t[:, d:2 * d], t[:, 2 * d:]
        fi = None if first is None else torch.tensor([first], dtype=torch.int32, device=TL.dev())
    out, w1 = TL.guarded(sets * B * Kp, d, dt)
    dq, w2 = TL.guarded(sets * B * Kp, d, dt)
    o.attn_prompt_fwd(qd, kd, vd, out, B, H, N, Kp, sets, first_image=fi)
    o.attn_prompt_bwd(qd, kd, vd, dad, dq, B, H, N, Kp, sets, first_image=fi)
    torch.cuda.synchronize()
    assert TL.guards_intact(w1) and TL.guards_intact(w2), "a guard element was overwritten"
    return out.view(sets, B, Kp, d), dq.view(sets, B, Kp, d)


# ---- rpo_attn_readonly_fwd_rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", FWD, ids=ident)
def test_fwd_edge_peaks_against_float64(case, mode):
    N, B, H, Kp, q_first = case
    qr, k, v, _ = inputs(N, B, H, N + Kp)
    out = _fwd(mode, qr[0], k, v, Kp, q_first)
    assert torch.isnan(out[:, :q_first].float()).all(), "a row below q_first was written"
    ref = reference(mode, N, B, H, N + Kp)
    _check(out[:, q_first:], ref["out"][0][:, q_first:], ref["b_out"][0][:, q_first:], f"edges fwd {mode} {ident(case)}", mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", QFIRST_SHAPES, ids=ident)
def test_fwd_any_q_first_keeps_the_bits_and_writes_no_other_row(shape, mode):
    """include/rpo_amd.h: any q_first in [0, N + Kp), and a query's bits do not depend on it"""
    N, B, H, Kp = shape
    qr, k, v, _ = inputs(N, B, H, N + Kp)
    full = _fwd(mode, qr[0], k, v, Kp)
    ref = reference(mode, N, B, H, N + Kp)
    _check(full, ref["out"][0], ref["b_out"][0], f"edges fwd {mode} {ident(shape)}", mode)
    for q_first in (1, 31, 32, 33, N - 1, N, N + 1, N + Kp - 1):
        part = _fwd(mode, qr[0], k, v, Kp, q_first)
        assert torch.isnan(part[:, :q_first].float()).all(), f"q_first = {q_first}: a row below it was written"
        assert torch.equal(part[:, q_first:], full[:, q_first:]), f"q_first = {q_first}: bits differ from the full launch"


@pytest.mark.parametrize("mode", HALF)
@pytest.mark.parametrize("case", FWD_2PHASE, ids=ident)
def test_fwd_two_phase_edge_peaks_against_float64(case, mode):
    """attn_fwd16_kernel on every image; image 0 and the last image launched alone take attn_fwd_kernel, whose arithmetic
    per query row is the same: the two kernels agree bit for bit (measured with this test; asserted)."""
    (N, Kp, q_first), H = case, 12
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = cus // H + 1
    assert B * H > cus and N <= 224, "this case must take the two-phase kernel"
    qr, k, v, _ = inputs(N, B, H, N + Kp)
    out = _fwd(mode, qr[0], k, v, Kp, q_first)
    assert torch.isnan(out[:, :q_first].float()).all(), "a row below q_first was written"
    ref = reference(mode, N, B, H, N + Kp)
    what = f"edges fwd two-phase {mode} {ident(case)}"
    _check(out[:, q_first:], ref["out"][0][:, q_first:], ref["b_out"][0][:, q_first:], what, mode)
    for b in (0, B - 1):
        one = _fwd(mode, qr[0, b:b + 1], k[b:b + 1], v[b:b + 1], Kp, q_first)
        _check(one[:, q_first:], ref["out"][0][b:b + 1, q_first:], ref["b_out"][0][b:b + 1, q_first:], f"{what} image {b} alone", mode)
        same = torch.equal(one[0, q_first:], out[b, q_first:])
        print(f"[{what}] image {b}: one-barrier kernel bit-identical to the two-phase kernel: {same}")
        assert same, f"image {b}: the one-barrier and the two-phase kernel differ"


# ---- rpo_attn_readonly_bwd / _bwd_proj -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", BWD, ids=ident)
def test_bwd_edge_peaks_against_float64(case, mode):
    N, B, H, Kp = case
    qr, k, v, da = inputs(N, B, H, Kp)
    dq = _bwd(mode, qr[0], k, v, da[0], Kp)
    ref = reference(mode, N, B, H, Kp)
    _check(dq, ref["dq"][0], ref["b_dq"][0], f"edges bwd {mode} {ident(case)}", mode)


@pytest.mark.parametrize("mode", HALF)
@pytest.mark.parametrize("case", BWD_PROJ, ids=ident)
def test_bwd_proj_edge_peaks_against_float64(case, mode):
    """the folded out-proj against float64, against the GEMM + rpo_attn_readonly_bwd pair it replaces (each per element
    within the same float64 budgets; against each other as test_attn_readonly_bwd_with_out_proj_folded_in holds them),
    and twice to equal bits"""
    N, B, H, Kp = case
    qr, k, v, dx = inputs(N, B, H, Kp)
    dq = _bwd_proj(mode, qr[0], k, v, dx[0], Kp)
    ref = reference(mode, N, B, H, Kp, proj=True)
    what = f"edges bwd_proj {mode} {ident(case)}"
    _check(dq, ref["dq"][0], ref["b_dq"][0], what, mode)
    dq2 = _bwd_proj(mode, qr[0], k, v, dx[0], Kp, two_launch=True)
    _check(dq2, ref["dq"][0], ref["b_dq"][0], what + " (GEMM + attn bwd)", mode)
    TO.close(dq, dq2.double().cpu(), mode, what + " fused vs GEMM + attn bwd", tol=3e-2)
    assert torch.equal(_bwd_proj(mode, qr[0], k, v, dx[0], Kp), dq), "a second launch gave other bits"


# ---- rpo_attn_prompt_fwd / _bwd -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", PROMPT, ids=ident)
def test_prompt_edge_peaks_against_float64(case, mode):
    N, B, H, Kp, sets, first = case
    q, k, v, da = inputs(N, B, H, Kp, sets)
    ref = reference(mode, N, B, H, Kp, sets)
    got = []
    for f in ((None, 0, "dev1") if first == "all" else (first,)):
        out, dq = _prompt(mode, q, k, v, da, f)
        what = f"edges prompt {mode} {ident(case)} first {f}"
        _check(out, ref["out"], ref["b_out"], what + " fwd", mode)
        _check(dq, ref["dq"], ref["b_dq"], what + " bwd", mode)
        got.append((out, dq))
    for out, dq in got[1:]:
        assert torch.equal(out, got[0][0]) and torch.equal(dq, got[0][1]), "the forms of first_image differ"
    if first == "all":
        for s in sorted({0, 1, sets // 2, sets - 1}):                     # (first, a middle and the last set)
            o1, g1 = _prompt(mode, q[s:s + 1], k, v, da[s:s + 1], None)
            assert torch.equal(o1[0], got[0][0][s]) and torch.equal(g1[0], got[0][1][s]), f"set {s} of {sets} != its own launch"


# ---- layouts the entry points accept ------------------------------------------------------------------------------------
def _wide(t, pad, dtype, off=0):
    """t [R, c] as columns off .. off + c of a NaN-filled [R, c + pad] device matrix inside a guarded allocation"""
    view, whole = TL.guarded(t.shape[0], t.shape[1] + pad, dtype)
    view[:, off:off + t.shape[1]] = t.to(dtype)
    return view[:, off:off + t.shape[1]], view, whole


def _only_the_view_written(view, whole, off, c):
    keep = torch.ones(view.shape[1], dtype=torch.bool, device=view.device)
    keep[off:off + c] = False
    return TL.guards_intact(whole) and bool(torch.isnan(view[:, keep].float()).all())


@pytest.mark.parametrize("mode", MODES)
def test_padded_leading_dimensions_and_offset_outputs(mode):
    """q / k / v as column views of a buffer wider than 3 d; out / dq as a column view 4 elements into a wider NaN buffer
    (8 bytes in the 16-bit modes: the least the alignment check allows): the bits of the plain layout, nothing outside the
    view written"""
    o, dt = TO.ops(), TL.DT[mode]
    N, B, H, Kp = 225, 2, 2, 33
    d, Rf = HD * H, B * N
    qr, k, v, _ = inputs(N, B, H, N + Kp)
    plain = _fwd(mode, qr[0], k, v, Kp)
    t, _, _ = _wide(packed(qr[0], k, v, Kp), 8, dt)
    out, ov, ow = _wide(torch.full((B * (N + Kp), d), float("nan")), 8, dt, off=4)
    o.attn_readonly_fwd(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], out, B, H, N, Kp)
    torch.cuda.synchronize()
    assert _only_the_view_written(ov, ow, 4, d), "fwd wrote outside the view"
    assert torch.equal(unpack(out, B, N, Kp), plain), "fwd: padded layout, other bits"
    # the backward and the prompt entry points: sets = 2 over the same keys
    sets = 2
    q, k, v, da = inputs(N, B, H, Kp, sets)
    dq_plain = _bwd(mode, q[0], k, v, da[0], Kp)
    p_out, p_dq = _prompt(mode, q, k, v, da, None)
    t, _, _ = _wide(packed(q[0], k, v, Kp), 8, dt)
    kd, vd = t[:Rf, d:2 * d], t[:Rf, 2 * d:]
    qd, _, _ = _wide(q.reshape(-1, d), 8, dt)
    dad, _, _ = _wide(da.reshape(-1, d), 16, dt)
    nanrows = lambda r: torch.full((r, d), float("nan"))
    dq, dv, dw = _wide(nanrows(B * Kp), 8, dt, off=4)
    o.attn_readonly_bwd(t[Rf:, :d], kd, vd, dad[:B * Kp], dq, B, H, N, Kp)
    torch.cuda.synchronize()
    assert _only_the_view_written(dv, dw, 4, d) and torch.equal(dq.reshape(B, Kp, d), dq_plain), "bwd: padded layout"
    po, pv, pw = _wide(nanrows(sets * B * Kp), 8, dt, off=4)
    pg, gv, gw = _wide(nanrows(sets * B * Kp), 8, dt, off=4)
    o.attn_prompt_fwd(qd, kd, vd, po, B, H, N, Kp, sets)
    o.attn_prompt_bwd(qd, kd, vd, dad, pg, B, H, N, Kp, sets)
    torch.cuda.synchronize()
    assert _only_the_view_written(pv, pw, 4, d) and torch.equal(po.reshape(sets, B, Kp, d), p_out), "prompt fwd: padded layout"
    assert _only_the_view_written(gv, gw, 4, d) and torch.equal(pg.reshape(sets, B, Kp, d), p_dq), "prompt bwd: padded layout"
    if mode == "f32":
        return
    Hp = 8
    d = HD * Hp
    q, k, v, dx = inputs(N, B, Hp, Kp)
    plain = _bwd_proj(mode, q[0], k, v, dx[0], Kp)
    t, _, _ = _wide(packed(q[0], k, v, Kp), 8, dt)
    dxd, _, _ = _wide(dx.reshape(-1, d), 8, dt)
    w_t, _, _ = _wide(w_out_of(Hp).t().contiguous(), 8, dt)
    dq, dv, dw = _wide(nanrows(B * Kp), 8, dt, off=4)
    o.attn_readonly_bwd_proj(t[Rf:, :d], t[:Rf, d:2 * d], t[:Rf, 2 * d:], dxd, w_t, dq, B, Hp, N, Kp)
    torch.cuda.synchronize()
    assert _only_the_view_written(dv, dw, 4, d) and torch.equal(dq.reshape(B, Kp, d), plain), "bwd_proj: padded layout"


# ---- invariances at one edge shape per kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_bits_do_not_depend_on_the_batch_or_the_call(mode):
    """a second launch gives equal bits; each image launched alone gives the bits it has in the batch"""
    N, B, H, Kp, sets = 225, 3, 2, 33, 2
    qr, k, v, _ = inputs(N, B, H, N + Kp)
    out = _fwd(mode, qr[0], k, v, Kp)
    assert torch.equal(_fwd(mode, qr[0], k, v, Kp), out), "fwd: second launch"
    q, kb, vb, da = inputs(N, B, H, Kp, sets)
    dq = _bwd(mode, q[0], kb, vb, da[0], Kp)
    assert torch.equal(_bwd(mode, q[0], kb, vb, da[0], Kp), dq), "bwd: second launch"
    p_out, p_dq = _prompt(mode, q, kb, vb, da, None)
    o2, g2 = _prompt(mode, q, kb, vb, da, None)
    assert torch.equal(o2, p_out) and torch.equal(g2, p_dq), "prompt: second launch"
    for b in range(B):
        s = slice(b, b + 1)
        assert torch.equal(_fwd(mode, qr[0, s], k[s], v[s], Kp)[0], out[b]), f"fwd: image {b} alone"
        assert torch.equal(_bwd(mode, q[0, s], kb[s], vb[s], da[0, s], Kp)[0], dq[b]), f"bwd: image {b} alone"
        o1, g1 = _prompt(mode, q[:, s], kb[s], vb[s], da[:, s], None)
        assert torch.equal(o1[:, 0], p_out[:, b]) and torch.equal(g1[:, 0], p_dq[:, b]), f"prompt: image {b} alone"
    if mode == "f32":
        return
    Hp = 12
    q, kb, vb, dx = inputs(N, 2, Hp, Kp)
    dq = _bwd_proj(mode, q[0], kb, vb, dx[0], Kp)
    for b in range(2):
        s = slice(b, b + 1)
        assert torch.equal(_bwd_proj(mode, q[0, s], kb[s], vb[s], dx[0, s], Kp)[0], dq[b]), f"bwd_proj: image {b} alone"


# ---- refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_refusals_write_nothing(mode):
    """N = 289 for the folded out-proj and the prompt entry points, Kp = 129 for the backward: RPO_E_SHAPE, nothing
    launched"""
    from rpo_amd._lib import E_SHAPE, RPOLibraryError
    o, dt = TO.ops(), TL.DT[mode]
    B, H, N, Kp = 1, 8, 289, 8
    d = HD * H
    t, _ = TL.put(TL.make_qkv(B, H, N, 129, 61), mode)
    rows, _ = TL.put(TO.rnd((129, d), 62), mode)
    w_t, _ = TL.put(TO.rnd((d, d), 63, d ** -0.5), mode)
    qd, kd, vd = t[N:, :d], t[:N, d:2 * d], t[:N, 2 * d:]
    outs = [TL.guarded(129, d, dt) for _ in range(4)]
    refused = pytest.raises(RPOLibraryError, match=f"code {E_SHAPE}")
    if mode != "f32":
        with refused:
            o.attn_readonly_bwd_proj(qd, kd, vd, rows, w_t, outs[0][0], B, H, N, Kp)
    with refused:
        o.attn_prompt_fwd(qd, kd, vd, outs[1][0], B, H, N, Kp, 1)
    with refused:
        o.attn_prompt_bwd(qd, kd, vd, rows, outs[2][0], B, H, N, Kp, 1)
    with refused:
        o.attn_readonly_bwd(qd, kd[:288], vd[:288], rows, outs[3][0], B, H, 288, 129)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(w.float()).all()) for _, w in outs), "a refused call wrote something"
