"""rpo_text_attn_fwd / rpo_text_attn_bwd (and their _shared forms) across the seam between their two kernels.

One entry point stands in front of two unrelated kernels (include/rpo_amd.h: "same meaning either way"):

  one-wave MFMA kernel  text_attn_wave_kernel (rpo_amd/csrc/attn_image.hip): 16-bit storage, causal = 0, rows <= 64,
                        Lmax <= 96, q / da 16-byte aligned with a 16-byte row pitch, out / dq 8-byte aligned with an 8-byte
                        row pitch.  NKT = 1 / 2 / 3 key tiles for Lmax <= 32 / <= 64 / <= 96, query tiles of 32 rows.
  fp32 VALU kernel      text_attn_kernel (rpo_amd/csrc/attn_text.hip): everything else -- f32 storage, the causal pass,
                        rows > 64, Lmax 97 .. 128, any unaligned q / da / out view.  Keys lane and lane + 64 in two score
                        sets; 2 * Lmax * 65 * 4 bytes of dynamic LDS, more than 64 KB from Lmax = 127 on.

The cases sit ON the switch points (CASE_TABLE), every class list holds the tile edges, one class's len exceeds Lmax (it
must read as Lmax) and the cache rows past a class's keys are NaN.  The reference is float64 on the values the kernel sees
(test_gpu_ops.q).  Every bound is one the project already uses for this operation: test_gpu_ops.TOL["f32"] and 8e-3 in the
16-bit modes with test_gpu_ops.close (test_text_attn_fwd_bwd), test_gpu_ranges.attn64's budgets with TOL / FLOOR
(test_text_attn_fwd_bwd_sharp_scores).  Every comparison prints its worst err / bound.

`expected_kernel` restates the dispatch from the header comment.  It labels the cases and lets
tests/test_text_attn_seam_host.py prove what the table covers; no assertion here depends on it.  Importing this module
does not touch the device.
"""
import functools
import math

import pytest
import torch

from helpers import assert_within
from oracle import rows_oracle as R  # noqa: E402  (checker only)
from test_gpu_ops import DT, TOL, close, q, rnd
from test_gpu_ranges import FLOOR, PATTERNS, _text_qkv, attn64
from test_gpu_ranges import TOL as RANGE_TOL

pytestmark = pytest.mark.gpu

MODES = ("f32", "bf16", "f16")
H, D, SCALE = 2, 128, 0.125
GUARD = 64                     # NaN elements in front of and behind out / dq
NAN = float("nan")
EDGES = (31, 32, 33, 63, 64, 65, 95, 96, 97)
BITS = {"f32": torch.int32, "bf16": torch.int16, "f16": torch.int16}


def tol_of(mode):
    """test_text_attn_fwd_bwd's bound (close: max |err| <= tol * max |ref|)"""
    return TOL["f32"] if mode == "f32" else 8e-3


# ------------------------------------------------------------------------------------------------------------------
# the dispatch, from the comments of rpo_text_attn_fwd (include/rpo_amd.h) and rpo_text_attn_wave (attn_image.hip)
# ------------------------------------------------------------------------------------------------------------------
def expected_kernel(mode, rows, Lmax, aligned):
    """The kernel a causal = 0 call runs ("aligned": views_aligned below)."""
    if mode == "f32" or rows > 64 or Lmax > 96 or not aligned:
        return "valu"
    return "wave1" if Lmax <= 32 else "wave2" if Lmax <= 64 else "wave3"


def valu_lds_bytes(Lmax):
    return 2 * Lmax * 65 * 4


# element offset of a view inside its allocation and the padding columns behind its d = 128 columns
LAYOUTS = {
    # test 1: row pitches d + 8 / 16 / 24 / 32 (multiples of 8 elements: a 16-bit call keeps its kernel)
    "pitched": dict(q=(0, 8), out=(GUARD, 16), da=(0, 24), dq=(GUARD, 32)),
    # test 2
    "aligned": dict(q=(0, 0), out=(GUARD, 0), da=(0, 0), dq=(GUARD, 0)),
    "q+2B": dict(q=(1, 0), out=(GUARD, 0), da=(0, 0), dq=(GUARD, 0)),
    "q_pitch_d+4": dict(q=(0, 4), out=(GUARD, 0), da=(0, 0), dq=(GUARD, 0)),
    "out+4B_da+2B": dict(q=(0, 0), out=(GUARD + 2, 0), da=(1, 0), dq=(GUARD + 2, 0)),
    "da+2B": dict(q=(0, 0), out=(GUARD, 0), da=(1, 0), dq=(GUARD, 0)),          # backward only
}
FWD_UNALIGNED = ("q+2B", "q_pitch_d+4", "out+4B_da+2B")
BWD_UNALIGNED = FWD_UNALIGNED + ("da+2B",)


def views_aligned(layout, bwd, esz=2):
    """What rpo_text_attn_wave asks of the views of a 16-bit call (the allocations themselves are 16-byte aligned)."""
    lay = LAYOUTS[layout]
    ok16 = lambda off, pad: (off * esz) % 16 == 0 and ((D + pad) * esz) % 16 == 0
    ok8 = lambda off, pad: (off * esz) % 8 == 0 and ((D + pad) * esz) % 8 == 0
    if bwd:
        return ok16(*lay["q"]) and ok16(*lay["da"]) and ok8(*lay["dq"])
    return ok16(*lay["q"]) and ok8(*lay["out"])


# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------
def case_lens(Lmax):
    """Lmax, 1, every tile edge up to Lmax, and one len above Lmax (reads as Lmax).  Twelve classes at most: the edge rule
    outweighs a shorter list."""
    return [Lmax, 1] + [e for e in EDGES if e < Lmax] + [Lmax + 5]


CASE_TABLE = [  # (id, Lmax, rows, what it crosses)
    ("L31_r7", 31, 7, "NKT 1 with one query tile, the key tile one short of full (added: the table's only other NKT 1 "
                      "case has two query tiles)"),
    ("L32_r45", 32, 45, "NKT 1, two query tiles (product shape K + Lmax = 77)"),
    ("L33_r44", 33, 44, "NKT 1 to 2, key 32 alone in tile 1"),
    ("L64_r13", 64, 13, "NKT 2 full; VALU second score set empty"),
    ("L65_r12", 65, 12, "NKT 2 to 3; VALU key 64 alone in the second set"),
    ("L77_r32", 77, 32, "exactly one full query tile"),
    ("L77_r33", 77, 33, "second query tile with one live row"),
    ("L77_r64", 77, 64, "last row count of the wave kernel"),
    ("L77_r65", 77, 65, "first row count of the VALU kernel; gridDim.y = 17, last chunk one row"),
    ("L96_r24", 96, 24, "last key count of the wave kernel, third tile full"),
    ("L97_r24", 97, 24, "first key count that sends 16-bit to the VALU kernel"),
    ("L126_r5", 126, 5, "largest LDS under 64 KB"),
    ("L127_r5", 127, 5, "first LDS over 64 KB"),
    ("L128_r24", 128, 24, "the limit; both VALU score sets full"),
    ("L128_r1", 128, 1, "one row: three idle waves per workgroup"),
]
IDS = [c[0] for c in CASE_TABLE]
CASES = {cid: (Lmax, rows, case_lens(Lmax)) for cid, Lmax, rows, _ in CASE_TABLE}
# test 2: the cases a 16-bit call runs on the wave kernel when its views are aligned
UNALIGNED_IDS = [cid for cid in IDS if CASES[cid][1] <= 64 and CASES[cid][0] <= 96]
SHARED_IDS = ["L33_r44", "L77_r65", "L96_r24", "L97_r24", "L128_r24"]
# test 3: (Lmax, Kr, mode)
SHARP = [(96, 24, "bf16"), (96, 24, "f16"), (97, 24, "bf16"), (97, 24, "f16"), (128, 24, "f32"), (128, 24, "bf16"),
         (128, 24, "f16"), (33, 44, "bf16"), (33, 44, "f16")]
CAUSAL_LMAX = (96, 127, 128)


def sharp_lens(Lmax):
    """Lmax, 1, 33, 65 (those a cache of Lmax rows per class can hold: _text_qkv sizes it by max(lens)) and a short class"""
    return [Lmax, 1] + [e for e in (33, 65) if e < Lmax] + [20]


# ------------------------------------------------------------------------------------------------------------------
# one problem: inputs and the float64 reference, computed once per (case, mode) and never written to
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(cid, mode):
    Lmax, rows, lens = CASES[cid]
    n = len(lens)
    kv = rnd((n * Lmax, 2 * D), 21)
    qr, da = rnd((n * rows, D), 22, 1.5), rnd((n * rows, D), 23)
    kv64, q64, da64 = q(kv, mode), q(qr, mode), q(da, mode)
    rf, rb = torch.empty(n * rows, D, dtype=torch.float64), torch.empty(n * rows, D, dtype=torch.float64)
    kv = kv.clone()
    for c, Lc in enumerate(lens):
        L = min(Lc, Lmax)
        k, v = kv64[c * Lmax:c * Lmax + L, :D], kv64[c * Lmax:c * Lmax + L, D:]
        sl = slice(c * rows, (c + 1) * rows)
        rf[sl] = R.attn_rows_fwd(q64[sl], k, v, H)
        rb[sl] = R.attn_rows_bwd(q64[sl], k, v, da64[sl], H)
        kv[c * Lmax + L:(c + 1) * Lmax] = NAN                  # nothing may read a cache row past the class's keys
    return dict(kv=kv, qr=qr, da=da, rf=rf, rb=rb)


# ------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------
def dev():
    return torch.device("cuda:0")


def lib():
    from rpo_amd import _lib
    return _lib.load()


def codes():
    from rpo_amd import _lib
    return _lib


def alloc(nrows, off, pad, mode):
    """A NaN-filled allocation and a [nrows, D] view of it: `off` elements in, row pitch D + pad, GUARD elements behind."""
    pitch = D + pad
    whole = torch.full((off + nrows * pitch + GUARD,), NAN, dtype=DT[mode], device=dev())
    assert whole.data_ptr() % 16 == 0
    return whole[off:off + nrows * pitch].view(nrows, pitch)[:, :D], whole


def put(t, mode, off, pad):
    view, _ = alloc(t.shape[0], off, pad, mode)
    view.copy_(t.to(DT[mode]))
    return view


def only_the_view_written(view, whole):
    """every element of the allocation outside the view's [rows, D] -- guards and padding columns -- is still NaN"""
    off = (view.data_ptr() - whole.data_ptr()) // whole.element_size()
    nrows, pitch = view.shape[0], view.stride(0)
    outside = torch.ones(whole.numel(), dtype=torch.bool, device=whole.device)
    outside[off:off + nrows * pitch].view(nrows, pitch)[:, :D] = False
    return bool(torch.isnan(whole[outside].float()).all())


def bits(t, mode):
    return t.contiguous().view(BITS[mode]).cpu()


def stream():
    return torch.cuda.current_stream().cuda_stream


def call_fwd(qv, kc, vc, out, len_ptr, n_cls, rows, Lmax, mode, heads=H, causal=0, n_kv=None):
    a = (qv.data_ptr(), qv.stride(0), kc.data_ptr(), vc.data_ptr(), kc.stride(0), out.data_ptr(), out.stride(0),
         _code(mode), len_ptr, n_cls)
    if n_kv is None:
        return lib().rpo_text_attn_fwd(*a, rows, Lmax, heads, causal, SCALE, stream())
    return lib().rpo_text_attn_fwd_shared(*a, n_kv, rows, Lmax, heads, SCALE, stream())


def call_bwd(qv, kc, vc, dav, dq, len_ptr, n_cls, rows, Lmax, mode, heads=H, n_kv=None):
    a = (qv.data_ptr(), qv.stride(0), kc.data_ptr(), vc.data_ptr(), kc.stride(0), dav.data_ptr(), dav.stride(0),
         dq.data_ptr(), dq.stride(0), _code(mode), len_ptr, n_cls)
    if n_kv is None:
        return lib().rpo_text_attn_bwd(*a, rows, Lmax, heads, SCALE, stream())
    return lib().rpo_text_attn_bwd_shared(*a, n_kv, rows, Lmax, heads, SCALE, stream())


def _code(mode):
    c = codes()
    return {"f32": c.RPO_F32, "bf16": c.RPO_BF16, "f16": c.RPO_F16}[mode]


class OnDevice:
    """A problem's inputs on the device in one layout; fwd / bwd launch all classes, or class `only` alone on its own
    slices of the same tensors, into fresh NaN-filled outputs."""

    def __init__(self, cid, mode, layout):
        p = problem(cid, mode)
        self.mode, self.lay = mode, LAYOUTS[layout]
        self.Lmax, self.rows, lens = CASES[cid]
        self.n = len(lens)
        self.q, self.da = put(p["qr"], mode, *self.lay["q"]), put(p["da"], mode, *self.lay["da"])
        self.kv = p["kv"].to(DT[mode]).to(dev())
        self.len = torch.tensor(lens, dtype=torch.int32, device=dev())

    def _slices(self, only):
        cs = slice(0, self.n) if only is None else slice(only, only + 1)
        return cs, slice(cs.start * self.rows, cs.stop * self.rows), slice(cs.start * self.Lmax, cs.stop * self.Lmax)

    def fwd(self, only=None):
        cs, rs, ks = self._slices(only)
        out, whole = alloc(rs.stop - rs.start, *self.lay["out"], self.mode)
        rc = call_fwd(self.q[rs], self.kv[ks, :D], self.kv[ks, D:], out, self.len[cs].data_ptr(), cs.stop - cs.start,
                      self.rows, self.Lmax, self.mode)
        assert rc == 0, f"rpo_text_attn_fwd returned {rc}"
        return out, whole

    def bwd(self, only=None):
        cs, rs, ks = self._slices(only)
        dq, whole = alloc(rs.stop - rs.start, *self.lay["dq"], self.mode)
        rc = call_bwd(self.q[rs], self.kv[ks, :D], self.kv[ks, D:], self.da[rs], dq, self.len[cs].data_ptr(),
                      cs.stop - cs.start, self.rows, self.Lmax, self.mode)
        assert rc == 0, f"rpo_text_attn_bwd returned {rc}"
        return dq, whole


def per_class(got, ref, cid, mode, what):
    """close() of every class's rows against its own max |ref|; prints and returns the worst err / bound first"""
    Lmax, rows, lens = CASES[cid]
    got64 = got.detach().to(torch.float64).cpu()
    worst = 0.0
    for c in range(len(lens)):
        sl = slice(c * rows, (c + 1) * rows)
        den = max(ref[sl].abs().max().item(), 1e-30)
        err = (got64[sl] - ref[sl]).abs().max().item()
        worst = max(worst, err / (tol_of(mode) * den)) if math.isfinite(err) else math.inf
    print(f"[{what}] worst err / bound {worst:.3f}")
    for c, Lc in enumerate(lens):
        sl = slice(c * rows, (c + 1) * rows)
        close(got[sl], ref[sl], mode, f"{what} class {c} (len {Lc})", tol=tol_of(mode))
    return worst


# ------------------------------------------------------------------------------------------------------------------
# 1
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cid", IDS)
def test_forward_and_backward_against_float64(cid, mode):
    """Padded row pitches for all four views, NaN guards around and NaN padding inside out / dq, NaN cache rows past every
    class's keys, a class with len > Lmax: float64 parity per class, nothing written outside the views, the same bits from
    a second launch and from every class launched alone."""
    p = problem(cid, mode)
    Lmax, rows, lens = CASES[cid]
    g = OnDevice(cid, mode, "pitched")
    assert views_aligned("pitched", False) and views_aligned("pitched", True)
    tag = f"seam {cid} {mode} {expected_kernel(mode, rows, Lmax, True)}"
    out, out_w = g.fwd()
    dq, dq_w = g.bwd()
    per_class(out, p["rf"], cid, mode, tag + " fwd")
    per_class(dq, p["rb"], cid, mode, tag + " bwd")
    assert torch.isfinite(out.float()).all() and torch.isfinite(dq.float()).all()
    assert only_the_view_written(out, out_w), "forward wrote outside its [rows, d] view"
    assert only_the_view_written(dq, dq_w), "backward wrote outside its [rows, d] view"
    out2, out2_w = g.fwd()
    dq2, dq2_w = g.bwd()
    assert torch.equal(bits(out, mode), bits(out2, mode)), "forward: a second launch gives other bits"
    assert torch.equal(bits(dq, mode), bits(dq2, mode)), "backward: a second launch gives other bits"
    assert only_the_view_written(out2, out2_w) and only_the_view_written(dq2, dq2_w)
    for c, Lc in enumerate(lens):
        sl = slice(c * rows, (c + 1) * rows)
        o1, o1_w = g.fwd(only=c)
        d1, d1_w = g.bwd(only=c)
        assert torch.equal(bits(o1, mode), bits(out[sl], mode)), f"forward: class {c} (len {Lc}) alone gives other bits"
        assert torch.equal(bits(d1, mode), bits(dq[sl], mode)), f"backward: class {c} (len {Lc}) alone gives other bits"
        assert only_the_view_written(o1, o1_w) and only_the_view_written(d1, d1_w)


# ------------------------------------------------------------------------------------------------------------------
# 2
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("cid", UNALIGNED_IDS)
def test_unaligned_views_take_the_other_kernel_with_the_same_meaning(cid, mode):
    """The same values through aligned views and through views rpo_text_attn_wave does not take: every variant within
    test 1's bound of the same float64 reference, the unaligned ones bit-identical to each other (one fp32 arithmetic on
    the same values), the aligned one within the sum of the two bounds of them.  An unaligned CACHE is refused."""
    p = problem(cid, mode)
    Lmax, rows, lens = CASES[cid]
    n = len(lens)
    res = {}
    for layout in ("aligned",) + BWD_UNALIGNED:
        g = OnDevice(cid, mode, layout)
        tag = f"seam views {cid} {mode} {layout}"
        if layout == "aligned" or layout in FWD_UNALIGNED:
            out, out_w = g.fwd()
            per_class(out, p["rf"], cid, mode, tag + " fwd")
            assert only_the_view_written(out, out_w), f"{tag}: forward wrote outside its view"
            res["fwd", layout] = out
        dq, dq_w = g.bwd()
        per_class(dq, p["rb"], cid, mode, tag + " bwd")
        assert only_the_view_written(dq, dq_w), f"{tag}: backward wrote outside its view"
        res["bwd", layout] = dq
    for which, layouts, ref in (("fwd", FWD_UNALIGNED, p["rf"]), ("bwd", BWD_UNALIGNED, p["rb"])):
        first = res[which, layouts[0]]
        for layout in layouts[1:]:
            assert torch.equal(bits(first, mode), bits(res[which, layout], mode)), \
                f"{which}: unaligned variants {layouts[0]} and {layout} differ in bits"
        a64, u64 = res[which, "aligned"].to(torch.float64).cpu(), first.to(torch.float64).cpu()
        worst = 0.0
        for c in range(n):
            sl = slice(c * rows, (c + 1) * rows)
            den = max(ref[sl].abs().max().item(), 1e-30)
            worst = max(worst, (a64[sl] - u64[sl]).abs().max().item() / den)
        print(f"[seam views {cid} {mode} {which}] aligned vs unaligned: max |diff| / max |ref| {worst:.3e} "
              f"(allowed {2 * tol_of(mode):.1e})")
        assert worst <= 2 * tol_of(mode), f"{which}: aligned and unaligned results differ by {worst:.3e} of max |ref|"
    # kc (then vc) two bytes off the 16-byte grid: RPO_E_ALIGN, nothing written
    g = OnDevice(cid, mode, "aligned")
    off_w = torch.zeros(1 + n * Lmax * 2 * D, dtype=DT[mode], device=dev())
    off = off_w[1:].view(n * Lmax, 2 * D)
    for kc, vc in ((off[:, :D], g.kv[:, D:]), (g.kv[:, :D], off[:, D:])):
        out, out_w = alloc(n * rows, GUARD, 0, mode)
        dq, dq_w = alloc(n * rows, GUARD, 0, mode)
        assert call_fwd(g.q, kc, vc, out, g.len.data_ptr(), n, rows, Lmax, mode) == codes().E_ALIGN
        assert call_bwd(g.q, kc, vc, g.da, dq, g.len.data_ptr(), n, rows, Lmax, mode) == codes().E_ALIGN
        assert torch.isnan(out_w.float()).all() and torch.isnan(dq_w.float()).all(), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------------------------
# 3
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lmax,Kr,mode", SHARP, ids=[f"L{c[0]}_r{c[1]}_{c[2]}" for c in SHARP])
def test_sharp_scores_at_the_new_key_counts(Lmax, Kr, mode):
    """test_gpu_ranges.test_text_attn_fwd_bwd_sharp_scores at the key counts on both sides of the wave / VALU switch, at the
    limit and at key 32 alone in a tile: the "late" heads peak at key len - 1, the key a wrong tile count or a short
    staging loop loses."""
    from rpo_amd import ops as o
    heads = 8
    assert "late" in PATTERNS[:heads]
    lens = sharp_lens(Lmax)
    assert max(lens) == Lmax
    n, d, dt = len(lens), 64 * heads, DT[mode]
    qr, kv = _text_qkv(lens, Kr, heads, 21)
    da = rnd((n * Kr, d), 22)
    kvd = kv.to(dev(), dt)
    len_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    out = torch.full((n * Kr, d), NAN, dtype=dt, device=dev())
    dq = torch.full((n * Kr, d), NAN, dtype=dt, device=dev())
    o.text_attn_fwd(qr.to(dev(), dt), kvd[:, :d], kvd[:, d:], out, len_d, n, Kr, Lmax, heads, causal=False)
    o.text_attn_bwd(qr.to(dev(), dt), kvd[:, :d], kvd[:, d:], da.to(dev(), dt), dq, len_d, n, Kr, Lmax, heads)
    kv64, q64, da64 = q(kv, mode), q(qr, mode), q(da, mode)
    rf, bf, rb, bb = (torch.empty((n * Kr, d), dtype=torch.float64) for _ in range(4))
    for c, L in enumerate(lens):
        sl = slice(c * Kr, (c + 1) * Kr)
        r = attn64(q64[sl], kv64[c * Lmax:c * Lmax + L, :d], kv64[c * Lmax:c * Lmax + L, d:], heads, RANGE_TOL[mode],
                   do=da64[sl])
        rf[sl], bf[sl], rb[sl], bb[sl] = r["out"], r["b_out"], r["dq"], r["b_dq"]
    what = f"seam sharp L{Lmax} r{Kr} {mode} {expected_kernel(mode, Kr, Lmax, True)}"
    w1 = assert_within(out, rf, bf, what + " fwd", floor=FLOOR[mode])
    w2 = assert_within(dq, rb, bb, what + " bwd", floor=FLOOR[mode])
    print(f"[{what}] worst err / budget fwd {w1:.3f} bwd {w2:.3f}")


# ------------------------------------------------------------------------------------------------------------------
# 4
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Lmax", CAUSAL_LMAX)
def test_causal_pass_at_the_key_limit(Lmax, mode):
    """The causal pass over packed [n * Lmax, 3d] class rows (always the VALU kernel) with rows = Lmax: row t of class c
    reads keys [0, min(t + 1, len[c])), the rows past len[c] included; their K / V columns are NaN."""
    lens = [Lmax, 1] + [e for e in (33, 64, 65, 96, 97) if e < Lmax] + [Lmax + 5]
    n, dt = len(lens), DT[mode]
    qkv = rnd((n * Lmax, 3 * D), 24)
    q3 = q(qkv, mode)
    for c, Lc in enumerate(lens):
        qkv[c * Lmax + min(Lc, Lmax):(c + 1) * Lmax, D:] = NAN
    t = qkv.to(dev(), dt)
    len_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    outc, whole = alloc(n * Lmax, GUARD, 8, mode)
    rc = call_fwd(t[:, :D], t[:, D:2 * D], t[:, 2 * D:], outc, len_d.data_ptr(), n, Lmax, Lmax, mode, causal=1)
    assert rc == 0, f"rpo_text_attn_fwd (causal) returned {rc}"
    got64 = outc.to(torch.float64).cpu()
    refs, worst = [], 0.0
    for c, Lc in enumerate(lens):
        L = min(Lc, Lmax)
        sl, keys = slice(c * Lmax, (c + 1) * Lmax), slice(c * Lmax, c * Lmax + L)
        ref = R.attn_causal_fwd(q3[sl, :D], q3[keys, D:2 * D], q3[keys, 2 * D:], H,
                                torch.arange(1, Lmax + 1).clamp(max=L))
        refs.append(ref)
        err = (got64[sl] - ref).abs().max().item()
        worst = max(worst, err / (tol_of(mode) * ref.abs().max().item())) if math.isfinite(err) else math.inf
    print(f"[seam causal L{Lmax} {mode} valu] worst err / bound {worst:.3f}")
    for c, Lc in enumerate(lens):
        close(outc[c * Lmax:(c + 1) * Lmax], refs[c], mode, f"text causal attn L{Lmax} class {c} (len {Lc})",
              tol=tol_of(mode))
    assert only_the_view_written(outc, whole), "the causal pass wrote outside its view"


# ------------------------------------------------------------------------------------------------------------------
# 5
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cid", SHARED_IDS)
def test_shared_cache_at_the_seam(cid, mode):
    """S = 2 prompt sets on a cache of n_kv = 3 classes: the bits of the plain calls on the cache and len replicated."""
    Lmax, rows, _ = CASES[cid]
    n_kv, S, dt = 3, 2, DT[mode]
    lens = [Lmax + 5, 1, max(e for e in EDGES if e < Lmax)]
    n = n_kv * S
    kv = rnd((n_kv * Lmax, 2 * D), 41)
    for c, Lc in enumerate(lens):
        kv[c * Lmax + min(Lc, Lmax):(c + 1) * Lmax] = NAN
    kvd = kv.to(dev(), dt)
    rep = kvd.repeat(S, 1)
    len_d = torch.tensor(lens, dtype=torch.int32, device=dev())
    len_rep = len_d.repeat(S)
    # rows of 7 classes: the refused n_cls = 7 call below must find nothing to write even if it ran
    qv, dav = put(rnd((7 * rows, D), 42, 1.5), mode, 0, 8), put(rnd((7 * rows, D), 43), mode, 0, 24)
    got, want = {}, {}
    for name, res, cache, ln, kw in (("shared", got, kvd, len_d, dict(n_kv=n_kv)), ("plain", want, rep, len_rep, {})):
        res["out"], res["out_w"] = alloc(7 * rows, GUARD, 16, mode)
        res["dq"], res["dq_w"] = alloc(7 * rows, GUARD, 32, mode)
        rc = call_fwd(qv, cache[:, :D], cache[:, D:], res["out"], ln.data_ptr(), n, rows, Lmax, mode, **kw)
        assert rc == 0, f"{name} forward returned {rc}"
        rc = call_bwd(qv, cache[:, :D], cache[:, D:], dav, res["dq"], ln.data_ptr(), n, rows, Lmax, mode, **kw)
        assert rc == 0, f"{name} backward returned {rc}"
    live = slice(0, n * rows)
    for k in ("out", "dq"):
        assert torch.isfinite(got[k][live].float()).all(), f"{k}: non-finite on the shared cache"
        assert torch.equal(bits(got[k][live], mode), bits(want[k][live], mode)), \
            f"{k}: the shared cache gives other bits than the replicated one"
        assert only_the_view_written(got[k], got[k + "_w"]), f"{k}: written outside the view on the shared cache"
        assert torch.isnan(got[k][n * rows:].float()).all(), f"{k}: rows behind the last virtual class written"
        s0, s1 = got[k][:n_kv * rows], got[k][n_kv * rows:n * rows]
        assert not torch.equal(s0, s1), f"{k}: the two prompt sets give the same rows"
    out, out_w = alloc(7 * rows, GUARD, 16, mode)
    dq, dq_w = alloc(7 * rows, GUARD, 32, mode)
    E = codes().E_SHAPE
    assert call_fwd(qv, kvd[:, :D], kvd[:, D:], out, len_d.data_ptr(), 7, rows, Lmax, mode, n_kv=n_kv) == E
    assert call_bwd(qv, kvd[:, :D], kvd[:, D:], dav, dq, len_d.data_ptr(), 7, rows, Lmax, mode, n_kv=n_kv) == E
    assert torch.isnan(out_w.float()).all() and torch.isnan(dq_w.float()).all(), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------------------------
# 6
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_refusals_write_nothing(mode):
    """Lmax = 129: RPO_E_SHAPE from all four entry points; rows = 0, n_cls = 0, a null len: RPO_E_BADARG; the outputs stay
    NaN.  (The tensors are sized for the refused shapes.)"""
    n, rows, Lmax, dt = 3, 8, 129, DT[mode]
    kvd = rnd((n * Lmax, 2 * D), 51).to(dev(), dt)
    qv, dav = put(rnd((n * rows, D), 52), mode, 0, 0), put(rnd((n * rows, D), 53), mode, 0, 0)
    len_d = torch.tensor([129, 5, 64], dtype=torch.int32, device=dev())
    out, out_w = alloc(n * rows, GUARD, 0, mode)
    dq, dq_w = alloc(n * rows, GUARD, 0, mode)
    kc, vc, lp = kvd[:, :D], kvd[:, D:], len_d.data_ptr()
    c = codes()

    def four(n_cls, r, L, len_ptr):
        return [call_fwd(qv, kc, vc, out, len_ptr, n_cls, r, L, mode),
                call_bwd(qv, kc, vc, dav, dq, len_ptr, n_cls, r, L, mode),
                call_fwd(qv, kc, vc, out, len_ptr, n_cls, r, L, mode, n_kv=max(n_cls, 1)),
                call_bwd(qv, kc, vc, dav, dq, len_ptr, n_cls, r, L, mode, n_kv=max(n_cls, 1))]

    assert four(n, rows, 129, lp) == [c.E_SHAPE] * 4
    assert four(n, 0, 128, lp) == [c.E_BADARG] * 4
    assert four(0, rows, 128, lp) == [c.E_BADARG] * 4
    assert four(n, rows, 128, None) == [c.E_BADARG] * 4
    torch.cuda.synchronize()
    assert torch.isnan(out_w.float()).all() and torch.isnan(dq_w.float()).all(), "a refused call wrote something"
