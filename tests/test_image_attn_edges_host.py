"""tests/test_gpu_image_attn_edges.py would notice: shown on the CPU, with that module's tables, generator and float64
reference (nothing is re-derived or loosened here).

  * coverage   a small mirror of the dispatch in rpo_amd/csrc/attn_image.hip (`features`) names every combination the code
               distinguishes -- N -> NT 7 / 9 / long, the two-phase predicate and its phases, `nfull` and `rem` in the
               16-bit and the f32 form, the query tiles of a wave, the workgroups per (image, head) and the W_out chunks of
               the folded out-proj, the set-major clamp -- and every one is reached by a case in every storage mode.  Every
               pinned case of test_gpu_image_attn_bits.SPECS with N <= 288 is in the tables.
  * inputs     every edge key carries `min_edge_weight` of some row's softmax weight; the float64 result rounded to the
               storage type uses at most half of every element's budget.
  * mutants    the float64 reference with ONE defect leaves the budget by a factor >= 4 at some element, per case and mode:
               each edge key dropped in turn; the row after the image's keys read as key N; query row r given row r - 1's
               query; for the prompt entry points, set s reading set 0's queries.  Where a result cannot depend on the
               defect it is not asked to: N = 1 has one weight, 1, whatever the query (out = V[0], dq = 0), so only the
               extra key shows there; a case with a single query has no neighbouring row; the extra key needs a second image (after the last image the row is NaN, which
               assert_within refuses).
  * oracle     attn64's out and dq agree with oracle.rows_oracle to 1e-12.
"""
import math

import pytest
import torch

import test_gpu_image_attn_bits as TB
import test_gpu_image_attn_edges as E
import test_gpu_ranges as TR
from oracle import rows_oracle as R

MODES = E.MODES
B_2PHASE = E.CUS_ASSUMED // 12 + 1

# (kind, case): everything the GPU module compares with float64 (the q_first sweep at q_first = 0: its other launches
# are held to that launch's bits)
CASES = [("fwd", c) for c in E.FWD] + [("fwd", s + (0,)) for s in E.QFIRST_SHAPES] \
    + [("fwd2phase", c) for c in E.FWD_2PHASE] + [("bwd", c) for c in E.BWD] + [("bwdproj", c) for c in E.BWD_PROJ] \
    + [("prompt", c) for c in E.PROMPT]


def modes_of(kind):
    return E.HALF if kind in ("fwd2phase", "bwdproj") else MODES


def geometry(kind, case):
    """(N, B, H, R, sets, q_first, Kp) of a case: the arguments of E.inputs / E.reference"""
    if kind == "fwd":
        N, B, H, Kp, qf = case
        return N, B, H, N + Kp, 1, qf, Kp
    if kind == "fwd2phase":
        N, Kp, qf = case
        return N, B_2PHASE, 12, N + Kp, 1, qf, Kp
    if kind == "prompt":
        N, B, H, Kp, sets, _ = case
        return N, B, H, Kp, sets, 0, Kp
    N, B, H, Kp = case
    return N, B, H, Kp, 1, 0, Kp


# ---- the dispatch, mirrored ------------------------------------------------------------------------------------------------
def _key_walk(mode, N, NT, tag):
    """fwd_walk_keys over the staged tiles: 16-bit = nfull full tiles, the partial tile of rem keys, tiles past N skipped;
    f32 = all NT tiles masked against N"""
    if mode == "f32":
        return {f"{tag}: f32 masked"} | ({f"{tag}: f32 tile without a key"} if 32 * (NT - 1) >= N else set())
    nfull = min(N >> 5, NT)
    rem = N - 32 * nfull if nfull < NT else 0
    f = {f"{tag}: nfull " + ("0" if nfull == 0 else "NT" if nfull == NT else "between"), f"{tag}: rem " + (">0" if rem else "0")}
    if nfull + (rem > 0) < NT:
        f.add(f"{tag}: tiles past N skipped")
    return f


def features(kind, mode, case):
    N, B, H, R, sets, q_first, Kp = geometry(kind, case)
    NT = 7 if N <= 224 else 9
    nt = "long" if N > 288 else f"nt{NT}"
    if kind in ("fwd", "fwd2phase"):
        two_phase = NT == 7 and N <= 288 and mode != "f32" and B * H > E.CUS_ASSUMED
        assert two_phase == (kind == "fwd2phase"), "the case takes the other forward kernel"
        S = N + Kp
        tiles = ((S + 31) >> 5) - (q_first >> 5)
        f = {f"{nt}: q_first " + ("0" if q_first == 0 else "inside a tile" if q_first % 32 else "on a tile"),
             f"{nt}: " + ("a wave's second query tile" if tiles > 8 else "a wave without a query tile" if tiles < 8 else "8 query tiles"),
             f"{nt}: last query tile " + ("clamped" if S % 32 else "full")}
        if nt == "long":
            return f
        if not two_phase:
            return f | _key_walk(mode, N, NT, nt)
        nfull = min(N >> 5, NT)
        rem = N - 32 * nfull
        nA = min(nfull, 4)
        f = {"2phase: " + x.split(": ")[1] for x in f}
        f.add(f"2phase: phase A " + ("no tile" if nA == 0 else "4 tiles" if nA == 4 else "1-3 tiles"))
        f.add("2phase: phase B " + ("full tiles + partial" if nfull > nA and rem else "partial only" if rem else "full only"
                                    if nfull > nA else "nothing"))
        return f
    if kind == "bwd":
        nqt, nkt = (Kp + 31) // 32, (N + 31) // 32
        return {nt, f"{nt}: {nqt} query tiles", f"{nt}: last query tile " + ("clamped" if Kp % 32 else "full"),
                f"{nt}: " + ("a wave without a key" if nkt < 4 else "every wave holds keys"),
                f"{nt}: last key tile " + ("partial" if N % 32 else "full")}
    if kind == "bwdproj":
        ncw, wgs = H // 4, (Kp + 31) // 32
        assert ncw in (2, 3, 4) and wgs <= 2
        return {f"{nt} ncw{ncw}", f"{wgs} workgroups per (image, head)", f"{nt}: last key tile " + ("partial" if N % 32 else "full"),
                "a wave without a key" if (N + 31) // 32 < 4 else "every wave holds keys"}
    Q = sets * Kp
    first = case[5]
    f = {f"{nt}: " + ("a wave's second query tile" if (Q + 31) // 32 > 8 else "at most one query tile per wave"),
         "last query tile " + ("clamped" if Q % 32 else "full"),
         "a query tile mixes sets" if sets > 1 and Kp % 32 else "query tiles of one set"}
    f |= {"first: " + str(x) for x in ((None, 0, "dev1") if first == "all" else (first,))}
    return f | _key_walk(mode, N, NT, nt)


_WALK16 = ["nfull 0", "nfull between", "nfull NT", "rem 0", "rem >0", "tiles past N skipped"]
REQUIRED = {
    "fwd": {"16": [f"nt7: {x}" for x in _WALK16] + [f"nt9: {x}" for x in _WALK16 if x != "nfull 0"],
            "f32": ["nt7: f32 masked", "nt7: f32 tile without a key", "nt9: f32 masked", "nt9: f32 tile without a key"],
            "all": [f"{nt}: {x}" for nt in ("nt7", "nt9", "long") for x in ("q_first 0", "q_first inside a tile", "q_first on a tile")]
            + [f"{nt}: {x}" for nt in ("nt7", "nt9") for x in ("a wave's second query tile", "a wave without a query tile",
                                                               "8 query tiles", "last query tile clamped", "last query tile full")]},
    "fwd2phase": {"16": ["2phase: phase A no tile", "2phase: phase A 1-3 tiles", "2phase: phase A 4 tiles",
                         "2phase: phase B full tiles + partial", "2phase: phase B partial only", "2phase: a wave's second query tile",
                         "2phase: a wave without a query tile", "2phase: q_first inside a tile", "2phase: q_first 0"]},
    "bwd": {"all": [f"{nt}: {x}" for nt in ("nt7", "nt9") for x in
                    ("1 query tiles", "2 query tiles", "3 query tiles", "4 query tiles", "last query tile clamped",
                     "last query tile full", "every wave holds keys", "last key tile partial", "last key tile full")]
            + ["nt7: a wave without a key"]},
    "bwdproj": {"16": [f"nt{n} ncw{c}" for n in (7, 9) for c in (2, 3, 4)]
                + ["1 workgroups per (image, head)", "2 workgroups per (image, head)", "a wave without a key", "every wave holds keys",
                   "nt7: last key tile full", "nt7: last key tile partial", "nt9: last key tile full", "nt9: last key tile partial"]},
    "prompt": {"16": ["nt7: nfull 0", "nt7: nfull between", "nt7: nfull NT", "nt7: rem 0", "nt7: rem >0", "nt7: tiles past N skipped",
                      "nt9: nfull between", "nt9: nfull NT", "nt9: rem >0", "nt9: tiles past N skipped"],
               "f32": ["nt7: f32 masked", "nt7: f32 tile without a key", "nt9: f32 masked", "nt9: f32 tile without a key"],
               "all": ["nt7: a wave's second query tile", "nt9: a wave's second query tile", "nt7: at most one query tile per wave",
                       "nt9: at most one query tile per wave", "last query tile clamped", "last query tile full",
                       "a query tile mixes sets", "query tiles of one set", "first: None", "first: 0", "first: dev1"]},
}


def _swept():
    """the q_first sweep's launches count as forward cases of the mirror"""
    return [("fwd", s + (qf,)) for s in E.QFIRST_SHAPES for qf in (1, 31, 32, 33, s[0] - 1, s[0], s[0] + 1, s[0] + s[3] - 1)]


@pytest.mark.parametrize("kind", list(REQUIRED))
def test_every_path_of_the_dispatch_is_reached_in_every_mode(kind):
    for mode in modes_of(kind):
        hit = set()
        for k_, case in CASES + _swept():
            if k_ == kind:
                hit |= features(kind, mode, case)
        want = REQUIRED[kind].get("all", []) + REQUIRED[kind].get("f32" if mode == "f32" else "16", [])
        missing = [w for w in want if w not in hit]
        assert not missing, f"{kind} {mode}: no case reaches {missing}"


def test_every_pinned_case_up_to_288_keys_is_in_the_tables():
    table = {"fwd": E.FWD, "fwd2phase": E.FWD_2PHASE, "pfwd": E.PROMPT, "pbwd": E.PROMPT, "bwd": E.BWD, "bwdproj": E.BWD_PROJ}
    n = 0
    for name, (kind, mode, p) in TB.SPECS.items():
        if p[0] <= 288:
            assert tuple(p) in table[kind], f"{name} is not compared with float64"
            n += 1
    assert n >= 100


# ---- inputs, the reference alone, the mutants ----------------------------------------------------------------------------------
def _attn(mode, H, q, k, v, da, mask=None):
    a = TR.attn64(q, k, v, H, TR.TOL[mode], mask=mask, do=da)
    return {"out": a["out"], "dq": a["dq"]}


def _factor(mut, ref, lim):
    r = (mut - ref).abs() / lim
    return math.inf if not bool(torch.isfinite(r).all()) else float(r.max())


WEAKEST = {}


@pytest.mark.parametrize("kind,case", CASES, ids=[f"{k_}_{E.ident(c)}" for k_, c in CASES])
def test_inputs_load_the_edges_and_mutants_leave_the_budget(kind, case):
    N, B, H, R, sets, q_first, Kp = geometry(kind, case)
    d = E.HD * H
    outs = {"fwd": ("out",), "fwd2phase": ("out",), "bwd": ("dq",), "bwdproj": ("dq",), "prompt": ("out", "dq")}[kind]
    edges = E.edge_keys(N)
    for mode in modes_of(kind):
        ref = E.reference(mode, N, B, H, R, sets, proj=kind == "bwdproj")
        need = E.min_edge_weight(N, sets * B * H * R)
        assert float(ref["edge_weight"].min()) >= need, f"{mode}: an edge key carries {float(ref['edge_weight'].min()):.3f} < {need:.3f}"
        q, k, v, da = (TR.q(t, mode) for t in E.inputs(N, B, H, R, sets))
        if kind == "bwdproj":
            da = TR.q((da @ TR.q(E.w_out_of(H), mode)).float(), mode)
        rows = slice(q_first, R)
        lim = {o: ref["b_" + o][:, :, rows] + TR.FLOOR[mode] for o in outs}
        want = {o: ref[o][:, :, rows] for o in outs}
        for o in outs:
            stored = want[o].to(TR.DT[mode]).double()
            w = _factor(stored, want[o], lim[o])
            assert w <= 0.5, f"{mode} {o}: the float64 result rounded to {mode} uses {w:.2f} of its budget"

        def run(b, qm=None, km=None, vm=None, mask=None):
            """image b with a defect: {out/dq: [sets, rows, d]}"""
            qb = (q if qm is None else qm)[:, b].reshape(sets * R, d)
            a = _attn(mode, H, qb, k[b] if km is None else km, v[b] if vm is None else vm, da[:, b].reshape(sets * R, d), mask)
            return {o: a[o].reshape(sets, R, d)[:, rows] for o in outs}

        def killed(name, mutant, images):
            """worst factor per output over the images, stopping at the first image where every output leaves by >= 4"""
            best = {o: 0.0 for o in outs}
            for b in images:
                got = mutant(b)
                for o in outs:
                    best[o] = max(best[o], _factor(got[o], want[o][:, b], lim[o][:, b]))
                if min(best.values()) >= 4:
                    break
            for o in outs:
                key = (kind, o, mode)
                if best[o] < WEAKEST.get(key, (math.inf,))[0]:
                    WEAKEST[key] = (best[o], f"{E.ident(case)}: {name}")
                assert best[o] >= 4, f"{mode} {o}: {name} stays within {best[o]:.2f} of the budget"

        if N > 1:
            for e in edges:
                mask = torch.ones(sets * R, N, dtype=torch.bool)
                mask[:, e] = False
                killed(f"edge key {e} dropped", lambda b: run(b, mask=mask), range(B))
            if sets * B * R > 1:                                          # (in the buffer's row order; a lone query has no neighbour)
                shifted = torch.roll(q.reshape(sets * B * R, d), 1, dims=0).reshape(q.shape)
                killed("query row r given row r - 1's query", lambda b: run(b, qm=shifted), range(B))
            if sets > 1:
                killed("every set reading set 0's queries", lambda b: run(b, qm=q[:1].expand_as(q)), range(B))
        if B > 1:
            killed("the row after the keys read as key N",
                   lambda b: run(b, km=torch.cat([k[b], k[b + 1, :1]]), vm=torch.cat([v[b], v[b + 1, :1]])), range(B - 1))


def test_report_the_weakest_mutants():
    """(runs after the cases above in file order; prints what DESIGN.md quotes)"""
    for key, (w, what) in sorted(WEAKEST.items()):
        print(f"[edges host] weakest mutant {key}: {w:.1f}x the budget ({what})")


def test_attn64_agrees_with_the_rows_oracle():
    N, B, H, Kp = 97, 2, 1, 33
    q, k, v, da = (t.double() for t in E.inputs(N, B, H, Kp))
    for b in range(B):
        a = TR.attn64(q[0, b], k[b], v[b], H, 0.0, do=da[0, b])
        assert (a["out"] - R.attn_rows_fwd(q[0, b], k[b], v[b], H)).abs().max() <= 1e-12
        assert (a["dq"] - R.attn_rows_bwd(q[0, b], k[b], v[b], da[0, b], H)).abs().max() <= 1e-12
