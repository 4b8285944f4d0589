#!/usr/bin/env python3
"""Generates rpo_amd/csrc/gemm_w4g_asm.inc and gemm_w4k_asm.inc: the k-loops of the one-round, one-wave-per-SIMD row-unit
GEMM kernels (gemm_w4g.inc: the four waves side by side along N; gemm_w4k.inc: the four waves split the contraction),
each as one inline-asm string, with the operand list that goes with it.

Why a generator: a loop is a hand schedule of MFMAs, fragment reads and LDS-DMA pieces per 64-deep k-tile with counted
waits; writing the counts by hand is where such loops go wrong, so they are DERIVED here from the issue order, and the
text is emitted.  The output is committed; re-run after editing (an optional argument names the output directory).

What the two kernels share (class Geo): TM x TN accumulators of 16 registers, MFMA j = accumulator [j / TM][j % TM] =
operand %j.  Which accumulators are AGPR tuples ("+a") and which VGPR tuples ("+v") is data of the geometry
(Geo.VGPR_ACC): the first 16 operands are AGPR tuples and the rest VGPR tuples, except in the 7 x 3 geometry of w4g,
where the five VGPR tuples are %0, %1, %7, %8 and %14 (acc[0][0..1], acc[1][0..1], acc[2][0]).  Fragment sets a / b: W fragments (TN) then X fragments (TM), 4 VGPRs each, the last 8 * (TM + TN)
VGPRs below v256.  Scratch: the four VGPRs below them (two DMA offsets of the W pieces, the W / X read addresses); s63
loop counter, s64 k byte offset of the tile being fetched, s71.. = i * 32 W rows; the A pieces take one offset operand
each (%[offa0] ..): the rows of a tile may come from two row segments.

Per geometry G (7X3, 9X2, 8X3) of kernel K (W4G, W4K) the output holds
  K_LOOP_G(OP)   the loop; OP is the MFMA mnemonic, a string literal
  K_CLOBBERS_G   its clobber list
  K_OPERANDS_G   the whole operand list of the asm statement; names the kernel body's acc, offa, offw, aw0, ax0, srda,
                 srdw, lds_w, nloop, rsw and, where the loop has entry positions, entry
and once per kernel K_KLOOP(CF, IS_F16): the asm statement of the geometry CF, with the MFMA of the dtype.

The two schedules:
w4g (w4g_loop)  two LDS slots, four 16-deep phases per tile.  Geometries (see gemm_w4g.inc for the reasoning):
  7X3  tile 224 (M, 7 x 32) x 384 (N): each wave 224 x 96 = 7 x 3 MFMA tiles -- ViT-B/16, 197 + K <= 224 rows/image
  9X2  tile 288 (M, 9 x 32) x 256 (N): each wave 288 x 64 = 9 x 2 MFMA tiles -- ViT-L/14, 257 + K <= 288 rows/image
  s60 slot of the current tile, s61 DMA destination, s62 the other slot.  The lgkmcnt waits are derived in w4g_phase.
w4k (w4k_loop)  ALL four waves compute the whole workgroup tile, wave w over k-step w (16 of the 64 k's) of every 64-deep
  k-tile; the accumulators are reduced across the waves by the epilogue.  Geometries (see gemm_w4k.inc):
  7X3  tile 224 (7 x 32) x 96 (3 x 32), LDS ring of 4 slots -- ViT-B/16 (197 + K <= 224 rows, 768 = 8 x 96)
  9X2  tile 288 (9 x 32) x 64 (2 x 32), LDS ring of 3 slots -- ViT-L/14 (257 + K <= 288 rows, 1024 = 16 x 64)
  8X3  tile 256 (8 x 32) x 96 (3 x 32), LDS ring of 3 slots -- ViT-B/16 with 225 .. 256 rows per image (K = 48)
  LDS: ring of R slots x (BM + BN) rows x 128 B.  Iteration t: wait for the wave's own fragment reads of tile t (issued
  during iteration t-1) and its own DMA pieces of tile t+1, barrier -- now every wave holds tile t in registers and tile
  t+1 is complete in LDS, so slot t % R is dead -- then the MFMAs on the fragments of tile t (set t % 2), the fragment
  reads of tile t+1 (other set) behind the first MFMAs and the wave's DMA pieces of tile t+R into slot t % R behind the
  later ones.  A tile has R-1 iterations to land; R-1 tiles are in flight per CU: inside a training step the operands
  come from HBM / MALL, not from a warm L2 (a two-iteration version of the 4-slot loop ran 37 us in a warm loop and 46 us
  in the step).
  Slot numbers and fragment sets are compile-time: the body is unrolled U = lcm(R, 2) times.  The number of fetching
  iterations, nk - R, need not be a multiple of U: the loop is ENTERED at position s = (-(nk - R)) mod U, with a prologue
  generated for every s the launcher admits (R = 4: nk % 4 == 0, s = 0; R = 3: nk % 6 in {0, 4}, s in {3, 5}).
  W4K_READ_AFTER / W4K_DMA_AFTER (environment, comma-separated MFMA indices) move the reads / DMA pieces of the 7X3
  geometry for experiments.
"""
import os
import sys
from math import gcd


class Geo:
    """What the emitters below need to know of a geometry; nw = W pieces per wave and k-tile."""

    def __init__(self, kernel, tm, tn, nw, vgpr_acc=None):
        self.kernel, self.name = kernel, f"{tm}X{tn}"
        self.TM, self.TN = tm, tn
        self.cond = f"CF::TM == {tm} && CF::TN == {tn}"   # the Cfg this geometry's loop is for
        self.NA, self.NW = tm, nw                        # DMA pieces per wave and k-tile: A (32 TM rows / 8 / 4 waves), W
        self.A_BYTES = 32 * tm * 128
        self.SLOT = (self.NA + self.NW) * 4096
        setsz = 4 * (tm + tn)
        self.FB = 256 - setsz
        self.FA = self.FB - setsz
        self.V0 = self.FA - 4                            # scratch: V0, V0+1 DMA offsets; V0+2 / V0+3 read addresses
        self.READ_ORDER = [("w", 0)] + [("x", i) for i in range(tm)] + [("w", i) for i in range(1, tn)]  # order of first use
        self.VGPR_ACC = set(range(16, tm * tn) if vgpr_acc is None else vgpr_acc)

    # ---- the shared emitter core ------------------------------------------------------------------------------------
    def frag(self, setname, kind, i):
        base = {"a": self.FA, "b": self.FB}[setname] + (0 if kind == "w" else 4 * self.TN) + 4 * i
        return f"v[{base}:{base + 3}]"

    def rd(self, setname, kind, i):
        addr = f"v{self.V0 + 2}" if kind == "w" else f"v{self.V0 + 3}"
        return f'"ds_read_b128 {self.frag(setname, kind, i)}, {addr} offset:{4096 * i}\\n\\t"'

    def mfma(self, j, cur):
        tn, tm = divmod(j, self.TM)
        return f'OP " %{j}, {self.frag(cur, "w", tn)}, {self.frag(cur, "x", tm)}, %{j}\\n\\t"'

    def dma(self, kind, i, base, slot_off=0):
        """piece i of the A / W rows of a k-tile -> LDS at `base` (an SGPR or operand) + slot_off"""
        lds = slot_off + 4096 * i + (0 if kind == "a" else self.A_BYTES)
        if kind == "a":                                  # per-piece offsets: the rows of a tile need not be contiguous
            return f'"s_add_u32 m0, {base}, {lds}\\n\\ts_nop 0\\n\\tbuffer_load_dwordx4 %[offa{i}], %[srda], s64 offen lds\\n\\t"'
        tmp = f"v{self.V0}" if i % 2 else f"v{self.V0 + 1}"
        pre = f"v_add_u32 {tmp}, s{70 + i}, %[offw]\\n\\t" if i > 0 else ""
        vo = tmp if i > 0 else "%[offw]"
        return f'"{pre}s_add_u32 m0, {base}, {lds}\\n\\ts_nop 0\\n\\tbuffer_load_dwordx4 {vo}, %[srdw], s64 offen lds\\n\\t"'

    def w_row_offsets(self):
        return ['"s_mov_b32 s71, %[rsw]\\n\\t"'] + [f'"s_add_u32 s{71 + i}, s{70 + i}, %[rsw]\\n\\t"' for i in range(1, self.NW - 1)]

    def operands(self, entry):
        acc = [f'"+{"v" if j in self.VGPR_ACC else "a"}"(acc[{j // self.TM}][{j % self.TM}])' for j in range(self.TM * self.TN)]
        ins = [f'[offa{i}] "v"(offa[{i}])' for i in range(self.NA)] + (['[entry] "s"(entry)'] if entry else [])
        ins += ['[offw] "v"(offw)', '[aw] "v"(aw0)', '[ax] "v"(ax0)', '[srda] "s"(srda)', '[srdw] "s"(srdw)',
                '[ldsw] "s"(lds_w)', '[nloop] "s"(nloop)', '[rsw] "s"(rsw)']

        def rows(items, per):
            return [", ".join(items[i:i + per]) for i in range(0, len(items), per)]
        return [": " + ", \\\n        ".join(rows(acc, 6)), ": " + ", \\\n        ".join(rows(ins, 5)),
                f": {self.kernel}_CLOBBERS_{self.name}"]


def write_inc(path, kernel, loops):
    """loops: (geo, lines of the loop, clobbered registers, has an entry operand) per geometry"""
    with open(path, "w") as f:
        f.write("// GENERATED by tools/gen_gemm_w4.py -- do not edit; the schedule and its wait counts are derived there.\n")
        f.write(f"// {kernel}_LOOP_<geometry>(OP): OP is the MFMA mnemonic; {kernel}_KLOOP(CF, IS_F16) picks loop, operands and mnemonic.\n")
        for geo, lines, clob, entry in loops:
            f.write(f"#define {kernel}_LOOP_{geo.name}(OP) \\\n")
            f.write(" \\\n".join("      " + l for l in lines))
            f.write("\n")
            f.write(f"#define {kernel}_CLOBBERS_{geo.name} " + ", ".join(f'"{c}"' for c in clob) + "\n")
            f.write(f"#define {kernel}_OPERANDS_{geo.name} \\\n      " + " \\\n      ".join(geo.operands(entry)) + "\n")
        f.write(f"#define {kernel}_ASM(IS_F16, LOOP, OPERANDS) \\\n"
                '  do { if constexpr (IS_F16) asm volatile(LOOP("v_mfma_f32_32x32x16_f16") OPERANDS); \\\n'
                '       else asm volatile(LOOP("v_mfma_f32_32x32x16_bf16") OPERANDS); } while (0)\n')
        f.write(f"#define {kernel}_KLOOP(CF, IS_F16) \\\n")
        for geo, _, _, _ in loops:
            f.write(f"  if constexpr ({geo.cond}) {kernel}_ASM(IS_F16, {kernel}_LOOP_{geo.name}, {kernel}_OPERANDS_{geo.name}); else \\\n")
        f.write('  static_assert(CF::TM < 0, "no generated k-loop for this geometry")\n')


# ---- w4g: two slots, four phases per tile ----------------------------------------------------------------------------
class GeoG(Geo):
    def __init__(self, tm, tn, vgpr_acc=None):
        super().__init__("W4G", tm, tn, 4 * tn, vgpr_acc)
        n_mfma, n_rd = tm * tn, tm + tn
        if 2 * n_rd <= n_mfma + 1:
            self.EVEN = list(range(0, 2 * n_rd, 2))      # reads after MFMA 0, 2, ..
        else:                                            # more reads than even gaps: the first odd gaps take one too
            self.EVEN = sorted(list(range(0, n_mfma, 2)) + list(range(1, 2 * (n_rd - (n_mfma + 1) // 2), 2)))
        self.FRONT = list(range(0, n_rd))                # the phase before the barrier: reads after MFMA 0 .. n_rd-1
        self.P3 = [("a", i) for i in range(self.NA)]                     # start of tile t+2 -> this slot
        self.P0 = [("w", i) for i in range(0, self.NW // 2)]             # rest of tile t+1 -> the other slot
        self.P1 = [("w", i) for i in range(self.NW // 2, self.NW)]


def w4g_phase(G, cur, nxt, read_gaps, dmas):
    """16-deep k-step: TM*TN MFMAs from set `cur`; the reads of set `nxt` after the MFMAs listed in read_gaps (or no
    reads); DMA pieces in the gaps that carry no read.  lgkmcnt: LDS reads return in order, so before an MFMA that first
    needs old read number q the wave may leave (last - q) old reads plus every new read issued so far in flight."""
    lines = []
    need = {}                                       # MFMA index -> highest old read index it needs for the first time
    seen = set()
    nm = G.TM * G.TN
    for j in range(nm):
        tn, tm = divmod(j, G.TM)
        for op in (("w", tn), ("x", tm)):
            if op not in seen:
                seen.add(op)
                need[j] = max(need.get(j, -1), G.READ_ORDER.index(op))
    issued = 0
    dq = list(dmas)
    if read_gaps is None:
        lines.append('"s_waitcnt lgkmcnt(0)\\n\\t"')
    for j in range(nm):
        if read_gaps is not None and j in need:
            lines.append(f'"s_waitcnt lgkmcnt({(len(G.READ_ORDER) - 1 - need[j]) + issued})\\n\\t"')
        lines.append(G.mfma(j, cur))
        if read_gaps is not None and j in read_gaps:
            kind, i = G.READ_ORDER[issued]
            lines.append(G.rd(nxt, kind, i))
            issued += 1
        elif dq and (read_gaps is None or j % 2 == 1 or j > max(read_gaps)):
            lines.append(G.dma(*dq.pop(0), "s61"))
    assert read_gaps is None or issued == len(G.READ_ORDER), issued
    while dq:                                       # more pieces than free gaps (9 x 2): the rest behind the last MFMA
        lines.append(G.dma(*dq.pop(0), "s61"))
    return lines


def w4g_addr(G, ks, sreg):
    vw, vx = f"v{G.V0 + 2}", f"v{G.V0 + 3}"
    if ks == 0:
        return [f'"v_add_u32 {vw}, {sreg}, %[aw]\\n\\tv_add_u32 {vx}, {sreg}, %[ax]\\n\\t"']
    return [f'"v_xor_b32 {vw}, {32 * ks}, %[aw]\\n\\tv_xor_b32 {vx}, {32 * ks}, %[ax]\\n\\t"',
            f'"v_add_u32 {vw}, {sreg}, {vw}\\n\\tv_add_u32 {vx}, {sreg}, {vx}\\n\\t"']


def w4g_tile(G, p0, p1, p3, read_next=True):
    L = [f'"s_sub_u32 s62, {G.SLOT}, s60\\n\\t"']
    L += w4g_addr(G, 1, "s60") + ['"s_add_u32 s61, s62, %[ldsw]\\n\\t"']
    L += w4g_phase(G, "a", "b", G.EVEN, p0)
    L += w4g_addr(G, 2, "s60") + w4g_phase(G, "b", "a", G.EVEN, p1)
    L += w4g_addr(G, 3, "s60") + w4g_phase(G, "a", "b", G.FRONT, [])
    if read_next:
        L += ['"s_waitcnt lgkmcnt(0)\\n\\ts_waitcnt vmcnt(0)\\n\\ts_barrier\\n\\t"', '"s_add_u32 s64, s64, 128\\n\\t"']
        L += w4g_addr(G, 0, "s62") + ['"s_add_u32 s61, s60, %[ldsw]\\n\\t"']
        L += w4g_phase(G, "b", "a", G.EVEN, p3)
        L += ['"s_mov_b32 s60, s62\\n\\t"']
    else:
        L += w4g_phase(G, "b", "a", None, [])
    return L


def w4g_loop(G):
    L = ['"s_mov_b32 s60, 0\\n\\ts_mov_b32 s64, 0\\n\\ts_mov_b32 s63, %[nloop]\\n\\t"']
    L += G.w_row_offsets()
    # prologue: tile 0 into slot 0, the A pieces of tile 1 into slot 1; tile 0 retired, published, its first reads issued
    L += ['"s_mov_b32 s61, %[ldsw]\\n\\t"'] + [G.dma("a", i, "s61") for i in range(G.NA)] + [G.dma("w", i, "s61") for i in range(G.NW)]
    L += [f'"s_add_u32 s64, s64, 128\\n\\ts_add_u32 s61, s61, {G.SLOT}\\n\\t"'] + [G.dma("a", i, "s61") for i in range(G.NA)]
    L += [f'"s_waitcnt vmcnt({G.NA})\\n\\ts_barrier\\n\\t"'] + w4g_addr(G, 0, "s60")
    L += [G.rd("a", k, i) for k, i in G.READ_ORDER]
    L += ['"s_cmp_eq_u32 s63, 0\\n\\ts_cbranch_scc1 2f\\n\\t"', '"1:\\n\\t"']
    L += w4g_tile(G, G.P0, G.P1, G.P3)
    L += ['"s_sub_u32 s63, s63, 1\\n\\ts_cmp_lg_u32 s63, 0\\n\\ts_cbranch_scc1 1b\\n\\t"', '"2:\\n\\t"']
    L += w4g_tile(G, G.P0, G.P1, [])                 # tile nk-2: the rest of tile nk-1 is the last fetch
    L += w4g_tile(G, [], [], [], read_next=False)    # tile nk-1
    L += ['"s_nop 15\\n\\ts_nop 15\\n\\t"']          # MFMA results -> compiler-generated readers
    clob = ["memory", "scc"] + [f"s{i}" for i in range(60, 82)] + [f"v{i}" for i in range(G.V0, 256)]
    return G, L, clob, False


# ---- w4k: ring of R slots, one k-step per wave, entry positions ------------------------------------------------------
class GeoK(Geo):
    def __init__(self, tm, tn, ring, entries, knobs=False):
        super().__init__("W4K", tm, tn, tn)
        self.RING = ring
        self.cond += f" && CF::RING == {ring}"
        self.P = self.NA + self.NW
        self.U = ring * 2 // gcd(ring, 2)
        self.entries = entries                       # admitted loop-entry positions s
        n_rd, n_mfma = tm + tn, tm * tn
        env_r, env_d = os.environ.get("W4K_READ_AFTER"), os.environ.get("W4K_DMA_AFTER")
        self.READ_AFTER = [int(x) for x in env_r.split(",")] if env_r and knobs else list(range(n_rd))
        if env_d and knobs:
            self.DMA_AFTER = [int(x) for x in env_d.split(",")]
        else:                                        # behind the reads; if the gaps run out, the last gap takes the rest
            self.DMA_AFTER = list(range(n_rd - 1, n_mfma - 1)) if n_mfma - n_rd < self.P else list(range(n_rd, n_rd + self.P))

    def pieces(self, slot):
        return [("a", i, "%[ldsw]", slot * self.SLOT) for i in range(self.NA)] + \
               [("w", i, "%[ldsw]", slot * self.SLOT) for i in range(self.NW)]


def w4k_phase(G, cur, nxt, reads, dmas):
    """The MFMAs of one iteration from set `cur` (whose reads have all returned: lgkmcnt(0) at the top of the iteration);
    if `reads`, the reads of set `nxt` after the MFMAs READ_AFTER; the DMA pieces after the MFMAs DMA_AFTER."""
    lines = []
    issued = 0
    dq = list(dmas)
    for j in range(G.TM * G.TN):
        lines.append(G.mfma(j, cur))
        if reads and j in G.READ_AFTER:
            kind, i = G.READ_ORDER[issued]
            lines.append(G.rd(nxt, kind, i))
            issued += 1
        if dq and j in G.DMA_AFTER:
            lines.append(G.dma(*dq.pop(0)))
    assert not reads or issued == len(G.READ_ORDER), issued
    while dq:
        lines.append(G.dma(*dq.pop(0)))
    return lines


def w4k_addr(G, slot):
    return [f'"v_add_u32 v{G.V0 + 2}, {slot * G.SLOT}, %[aw]\\n\\tv_add_u32 v{G.V0 + 3}, {slot * G.SLOT}, %[ax]\\n\\t"']


def w4k_iteration(G, j, fetch=True, wait=None, read_next=True):
    """iteration at unrolled position j: slot of tile t is j % R, its fragment set j % 2"""
    cur, nxt = ("a", "b") if j % 2 == 0 else ("b", "a")
    if wait is None:
        wait = (G.RING - 2) * G.P                    # younger than tile t+1: the tiles t+2 .. t+R-1
    L = []
    if read_next:
        L += [f'"s_waitcnt lgkmcnt(0)\\n\\ts_waitcnt vmcnt({wait})\\n\\ts_barrier\\n\\t"'] + w4k_addr(G, (j + 1) % G.RING)
    else:
        L += ['"s_waitcnt lgkmcnt(0)\\n\\t"']
    if fetch:
        L += ['"s_add_u32 s64, s64, 128\\n\\t"']
    L += w4k_phase(G, cur, nxt, read_next, G.pieces(j % G.RING) if fetch else [])
    return L


def w4k_prologue(G, s):
    """tiles 0 .. R-1 into the slots of positions s .. s+R-1; tile 0 retired, published, its fragments requested"""
    L = ['"s_mov_b32 s64, 0\\n\\t"']
    for t in range(G.RING):
        L += [G.dma(*p) for p in G.pieces((s + t) % G.RING)]
        if t < G.RING - 1:
            L += ['"s_add_u32 s64, s64, 128\\n\\t"']
    L += [f'"s_waitcnt vmcnt({(G.RING - 1) * G.P})\\n\\ts_barrier\\n\\t"'] + w4k_addr(G, s % G.RING)
    L += [G.rd("a" if s % 2 == 0 else "b", k, i) for k, i in G.READ_ORDER]
    return L


def w4k_loop(G):
    L = ['"s_mov_b32 s63, %[nloop]\\n\\t"'] + G.w_row_offsets()
    if G.entries == [0]:
        L += w4k_prologue(G, 0)
        L += ['"s_cmp_eq_u32 s63, 0\\n\\ts_cbranch_scc1 2f\\n\\t"', '"1:\\n\\t"']
        for j in range(G.U):
            L += w4k_iteration(G, j)
    else:
        for s in G.entries[:-1]:
            L += [f'"s_cmp_lg_u32 %[entry], {s}\\n\\ts_cbranch_scc1 {30 + s}f\\n\\t"'] + w4k_prologue(G, s)
            L += [f'"s_branch {10 + s}f\\n\\t"', f'"{30 + s}:\\n\\t"']
        s = G.entries[-1]
        L += w4k_prologue(G, s) + [f'"s_branch {10 + s}f\\n\\t"']
        L += ['"1:\\n\\t"']
        for j in range(G.U):
            if j in G.entries:
                L += [f'"{10 + j}:\\n\\t"']
            L += w4k_iteration(G, j)
    L += ['"s_sub_u32 s63, s63, 1\\n\\ts_cmp_lg_u32 s63, 0\\n\\ts_cbranch_scc1 1b\\n\\t"', '"2:\\n\\t"']
    for i in range(G.RING):                          # the last R iterations fetch nothing; position 0 again
        last = i == G.RING - 1
        L += w4k_iteration(G, i, fetch=False, wait=None if last else (G.RING - 2 - i) * G.P, read_next=not last)
    L += ['"s_nop 15\\n\\ts_nop 15\\n\\t"']          # MFMA results -> compiler-generated readers
    clob = ["memory", "scc"] + ["s63", "s64"] + [f"s{71 + i}" for i in range(max(G.NW - 1, 1))] + \
           [f"v{i}" for i in range(G.V0, 256)]
    return G, L, clob, G.entries != [0]


def main():
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rpo_amd", "csrc")
    if len(sys.argv) > 1:                            # tests regenerate into a scratch directory and compare
        out = sys.argv[1]
    for kernel, inc, loops in (
            ("W4G", "gemm_w4g_asm.inc", [w4g_loop(GeoG(7, 3, vgpr_acc=[0, 1, 7, 8, 14])), w4g_loop(GeoG(9, 2))]),
            ("W4K", "gemm_w4k_asm.inc", [w4k_loop(GeoK(7, 3, 4, [0], knobs=True)), w4k_loop(GeoK(9, 2, 3, [3, 5])),
                                         w4k_loop(GeoK(8, 3, 3, [3, 5]))])):
        write_inc(os.path.join(out, inc), kernel, loops)
        print("wrote", os.path.join(out, inc), *(f"{g.name}: {len(L)} lines" for g, L, _, _ in loops))


if __name__ == "__main__":
    main()
