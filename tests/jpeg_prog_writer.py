"""A PROGRESSIVE JPEG stream writer for tests, on top of tests/jpeg_writer.py (numpy only).  Never imported by the product.

Pillow's encoder writes one scan script (ten scans for YCbCr, six for gray) with optimised tables; this writer takes the
quantised coefficient blocks `jpeg_writer.forward` makes and writes them under ANY scan script, restart interval and table
set, and the baseline file of the same blocks through `jpeg_writer.write_jpeg` -- the two must decode to the same bits.

    scans = [Scan([0, 1, 2], 0, 0, 0, 1), Scan([0], 1, 5, 0, 2), ..., Scan([0], 1, 63, 1, 0, dri=3, dht=[[(1, 0, bits, vals)]])]
    data = write_progressive(width, height, blocks, comps, dqt, scans, fill=2, tail=b"...")
    twin = write_baseline(width, height, blocks, comps, dqt)

`Scan(comps, ss, se, ah, al)`: indices into `comps`, the band and the successive-approximation bits.  Per scan, in front of
its SOS: `dht` = DHT segments (lists of (class, id, bits, vals)) and `dri` = a DRI segment with that interval (restart
intervals count MCUs in an interleaved scan, blocks otherwise, and hold until the next DRI); `td` / `ta` override the table
ids of the components; `segments` = other (marker, payload) segments.  Without any `dht` the file starts with universal
tables: DC id 0 = 12 categories at 4 bits, AC id 0 = all 256 symbols at 8 and 9 bits.  `symbols(...)` returns what each scan uses,
to build tight tables (`jpeg_writer.spread_table`) for it.  The coding is T.81 Annex G's (figures G.3 - G.7): EOB runs up to
32767 cut at restarts, correction bits buffered behind the symbol they follow.

Tokens of a unit (one restart interval of one scan): ("sym", class, symbol, scan component), ("bits", value, nbits).
`hook(scan_index, unit_index, tokens) -> tokens` rewrites them (corrupt streams).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

import jpeg_writer as JW

ZZ = [int(v) for v in JW.ZIGZAG]


@dataclass
class Scan:
    comps: List[int]
    ss: int
    se: int
    ah: int
    al: int
    dht: list = field(default_factory=list)
    dri: Optional[int] = None
    td: Optional[List[int]] = None
    ta: Optional[int] = None
    segments: list = field(default_factory=list)
    ncomp_byte: Optional[int] = None          # refused headers: lie in the SOS


def universal_dht():
    ac = JW.table_from_lengths({s: 8 if s < 128 else 9 for s in range(256)})      # a DHT count is one byte: 128 + 128
    return [[(0, 0) + tuple(JW.flat_table(JW.DC_SYMBOLS)), (1, 0) + tuple(ac)]]


def pillow_script(nc: int) -> List[Scan]:
    """The script Pillow (libjpeg's jpeg_simple_progression) writes."""
    if nc == 1:
        return [Scan([0], 0, 0, 0, 1), Scan([0], 1, 5, 0, 2), Scan([0], 6, 63, 0, 2), Scan([0], 1, 63, 2, 1),
                Scan([0], 0, 0, 1, 0), Scan([0], 1, 63, 1, 0)]
    return [Scan([0, 1, 2], 0, 0, 0, 1), Scan([0], 1, 5, 0, 2), Scan([2], 1, 63, 0, 1), Scan([1], 1, 63, 0, 1),
            Scan([0], 6, 63, 0, 2), Scan([0], 1, 63, 2, 1), Scan([0, 1, 2], 0, 0, 1, 0), Scan([2], 1, 63, 1, 0),
            Scan([1], 1, 63, 1, 0), Scan([0], 1, 63, 1, 0)]


def _shift(v: int, al: int) -> int:
    """the point transform of an AC coefficient: magnitude shifted, sign kept"""
    return (abs(v) >> al) * (1 if v >= 0 else -1)


class _Unit:
    """Token stream of one restart interval, with the EOB run and the buffered correction bits of T.81 G.1.2.3."""

    def __init__(self):
        self.toks: List[tuple] = []
        self.eobrun = 0
        self.be: List[int] = []               # correction bits of the blocks inside the EOB run

    def sym(self, tc, s, ci=0):
        self.toks.append(("sym", tc, s, ci))

    def bits(self, v, n):
        if n:
            self.toks.append(("bits", v, n))

    def flush_eobrun(self):
        if self.eobrun:
            r = self.eobrun.bit_length() - 1
            self.sym(1, r << 4)
            self.bits(self.eobrun - (1 << r), r)
            self.eobrun = 0
        for b in self.be:
            self.bits(b, 1)
        self.be = []


def _walk(width, height, comps, sc: Scan):
    """-> (blocks per unit list of (scan component index, by, bx)), restart interval applied by the caller"""
    nc = len(comps)
    hs, vs = (comps[0].h, comps[0].v) if nc == 3 else (1, 1)
    mx, my = -(-width // (8 * hs)), -(-height // (8 * vs))
    if len(sc.comps) > 1:
        mcus = []
        for m in range(mx * my):
            yy, xx = divmod(m, mx)
            one = []
            for i, c in enumerate(sc.comps):
                h, v = (hs, vs) if (c == 0 and nc == 3) else (1, 1)
                one += [(i, yy * v + j // h, xx * h + j % h) for j in range(h * v)]
            mcus.append(one)
        return mcus
    c = sc.comps[0]
    h, v = (hs, vs) if (c == 0 and nc == 3) else (1, 1)
    bw, bh = -(-(-(-width * h // hs)) // 8), -(-(-(-height * v // vs)) // 8)
    return [[(0, by, bx)] for by in range(bh) for bx in range(bw)]


def _encode_block(u: _Unit, sc: Scan, blk, pred: list, ci: int):
    zz = [int(blk[z]) for z in ZZ]
    if sc.se == 0:
        if sc.ah == 0:
            v = zz[0] >> sc.al                                    # arithmetic shift (G.1.2.1)
            d = v - pred[ci]
            pred[ci] = v
            s = JW._size(d)
            u.sym(0, s, ci)
            u.bits(JW._bits_of(d, s), s)
        else:
            u.bits((zz[0] >> sc.al) & 1, 1)
        return
    if sc.ah == 0:
        r = 0
        for k in range(sc.ss, sc.se + 1):
            v = _shift(zz[k], sc.al)
            if v == 0:
                r += 1
                continue
            u.flush_eobrun()
            while r > 15:
                u.sym(1, 0xF0)
                r -= 16
            s = JW._size(v)
            u.sym(1, (r << 4) | s)
            u.bits(JW._bits_of(v, s), s)
            r = 0
        if r > 0:
            u.eobrun += 1
            if u.eobrun == 0x7FFF:
                u.flush_eobrun()
        return
    # AC refinement
    mags = [abs(zz[k]) >> sc.al for k in range(64)]
    eob = max((k for k in range(sc.ss, sc.se + 1) if mags[k] == 1), default=-1)
    r, br = 0, []                                                 # br: correction bits of this block not yet written
    for k in range(sc.ss, sc.se + 1):
        t = mags[k]
        if t == 0:
            r += 1
            continue
        while r > 15 and k <= eob:
            u.flush_eobrun()
            u.sym(1, 0xF0)
            r -= 16
            for b in br:
                u.bits(b, 1)
            br = []
        if t > 1:
            br.append(t & 1)
            continue
        u.flush_eobrun()
        u.sym(1, (r << 4) | 1)
        u.bits(0 if zz[k] < 0 else 1, 1)
        for b in br:
            u.bits(b, 1)
        br, r = [], 0
    if r > 0 or br:
        u.eobrun += 1
        u.be += br
        if u.eobrun == 0x7FFF:
            u.flush_eobrun()


def scan_units(width, height, blocks, comps, sc: Scan, ri: int) -> List[List[tuple]]:
    """The token lists of the scan's units."""
    mcus = _walk(width, height, comps, sc)
    ri = ri or len(mcus)
    out = []
    for lo in range(0, len(mcus), ri):
        u, pred = _Unit(), [0, 0, 0]
        for one in mcus[lo:lo + ri]:
            for ci, by, bx in one:
                _encode_block(u, sc, blocks[sc.comps[ci]][by, bx], pred, ci)
        u.flush_eobrun()                                          # an EOB run never crosses a restart
        out.append(u.toks)
    return out


def symbols(width, height, blocks, comps, scans: Sequence[Scan]) -> List[Tuple[set, set]]:
    """Per scan: (DC symbols, AC symbols) it is coded with."""
    out, ri = [], 0
    for sc in scans:
        ri = ri if sc.dri is None else sc.dri
        dc, ac = set(), set()
        for toks in scan_units(width, height, blocks, comps, sc, ri):
            for t in toks:
                if t[0] == "sym":
                    (dc, ac)[t[1]].add(t[2])
        out.append((dc, ac))
    return out


def write_progressive(width: int, height: int, blocks, comps: Sequence[JW.Comp], dqt, scans: Sequence[Scan], *,
                      dht=None, jfif: bool = True, adobe: Optional[int] = None, fill: int = 0, tail: bytes = b"",
                      eoi: bool = True, sof: int = 0xC2, segments: Sequence[Tuple[int, bytes]] = (),
                      hook: Optional[Callable] = None, scan_offsets: Optional[list] = None) -> bytes:
    """See the module docstring.  `dht`: the DHT segments in front of the first scan (default: the universal tables, unless
    the first scan brings its own).  `fill`: FF bytes in front of every marker behind the frame header.  `scan_offsets`
    receives (first byte, end) of every scan's entropy-coded data."""
    nc = len(comps)
    out = bytearray(b"\xff\xd8")
    head: List[Tuple[int, bytes]] = []
    if jfif:
        head.append(JW.jfif_segment())
    if adobe is not None:
        head.append(JW.adobe_segment(adobe))
    head += list(segments)
    for seg in dqt:
        head.append((0xDB, b"".join(bytes([tid]) + bytes(int(x) for x in np.asarray(tab).reshape(64)[JW.ZIGZAG]) for tid, tab in seg)))
    head.append((sof, bytes([8, height >> 8, height & 255, width >> 8, width & 255, nc]) +
                 b"".join(bytes([c.id, (c.h << 4) | c.v, c.tq]) for c in comps)))
    for marker, payload in head:
        out += JW._segment(marker, payload)
    codes: Dict[Tuple[int, int], Dict[int, Tuple[int, int]]] = {}
    fillb = b"\xff" * fill

    def put_dht(segs):
        nonlocal out
        for seg in segs:
            payload = b""
            for tc, th, bits, vals in seg:
                payload += bytes([(tc << 4) | th]) + bytes(int(x) for x in bits[1:17]) + bytes(int(x) for x in vals)
                codes[(tc, th)] = JW._codes(bits, vals)
            out += fillb + JW._segment(0xC4, payload)
    put_dht(dht if dht is not None else ([] if scans and scans[0].dht else universal_dht()))
    ri = 0
    for si, sc in enumerate(scans):
        put_dht(sc.dht)
        for marker, payload in sc.segments:
            out += fillb + JW._segment(marker, payload)
        if sc.dri is not None:
            ri = sc.dri
            out += fillb + JW._segment(0xDD, bytes([ri >> 8, ri & 255]))
        td = sc.td or [comps[c].td for c in sc.comps]
        ta = [sc.ta if sc.ta is not None else comps[c].ta for c in sc.comps]
        ns = len(sc.comps) if sc.ncomp_byte is None else sc.ncomp_byte
        out += fillb + JW._segment(0xDA, bytes([ns]) + b"".join(bytes([comps[c].id, (td[i] << 4) | ta[i]])
                                                                for i, c in enumerate(sc.comps)) +
                                   bytes([sc.ss, sc.se, (sc.ah << 4) | sc.al]))
        first = len(out)
        units = scan_units(width, height, blocks, comps, sc, ri)
        for ui, toks in enumerate(units):
            if hook is not None:
                toks = hook(si, ui, toks)
            if ui:
                out += fillb + bytes([0xFF, 0xD0 + (ui - 1) % 8])
            bw = JW._BitWriter()
            for t in toks:
                if t[0] == "sym":
                    bw.put(*codes[(1, ta[0]) if t[1] else (0, td[t[3]])][t[2]])
                else:
                    bw.put(t[1], t[2])
            bw.flush()
            out += bw.out
        if scan_offsets is not None:
            scan_offsets.append((first, len(out)))
    if eoi:
        out += fillb + b"\xff\xd9"
    return bytes(out + tail)


def write_baseline(width, height, blocks, comps, dqt, restart_interval: int = 0) -> bytes:
    """The baseline file of the same quantised blocks (universal tables)."""
    comps = [JW.Comp(c.id, c.h, c.v, c.tq, 0, 0) for c in comps]
    return JW.write_jpeg(width, height, blocks, comps, dqt, universal_dht(), restart_interval=restart_interval)


# ---- fixtures written by tools/make_jpeg_progressive.py ------------------------------------------------------------------

def load_progressive(path: str):
    """tests/golden/jpeg_progressive.npz -> (streams, refused): streams = [{file, rgb (Pillow's decode), tag, twin (the
    baseline file of the same blocks, writer-made streams only, else None)}], refused = [{file, code, tag}].  Everything is
    packed into a few arrays, because a zip entry costs more than a small stream."""
    g = np.load(path)

    def split(flat, lens):
        o = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
        return [flat[o[k]:o[k + 1]] for k in range(len(lens))]
    files, twins = split(g["files"], g["file_len"]), split(g["twins"], g["twin_len"])
    shape = g["shape"].astype(np.int64)
    rgbs = split(g["rgb"], 3 * shape[:, 0] * shape[:, 1])
    streams = [{"file": files[k].tobytes(), "rgb": rgbs[k].reshape(shape[k, 0], shape[k, 1], 3), "tag": str(g["tags"][k]),
                "twin": twins[k].tobytes() if len(twins[k]) else None} for k in range(len(files))]
    refused = [{"file": f.tobytes(), "code": int(c), "tag": str(t)}
               for f, c, t in zip(split(g["refused_files"], g["refused_len"]), g["refused_code"], g["refused_tags"])]
    return streams, refused


def eob_runs(toks) -> List[int]:
    """the lengths of the EOB runs in a unit's tokens"""
    out = []
    for i, t in enumerate(toks):
        if t[0] == "sym" and t[1] == 1 and (t[2] & 15) == 0 and (t[2] >> 4) < 15:
            r = t[2] >> 4
            out.append((1 << r) + (toks[i + 1][1] if r else 0))
    return out


# ---- corrupt streams, built live -------------------------------------------------------------------------------------------

def corrupt_streams():
    """[(what, file, the status word the device must leave)]: gray 32x32 (16 blocks) under Pillow's script, complete and
    consistent headers, each wrong in one known place of the entropy-coded data.  All of them go through
    tests/host/jpeg_prog_host_decode.cpp (tests/test_jpeg_progressive_host.py) before a GPU test decodes them."""
    S = JW.STATUS
    rng = np.random.default_rng(78)
    px = np.clip(np.kron(rng.integers(0, 256, (8, 8)), np.ones((4, 4))) + rng.normal(0, 10, (32, 32)), 0, 255).astype(np.uint8)
    i, j = np.mgrid[0:8, 0:8]
    q = (2 + i + j).reshape(64)
    blocks = JW.forward(px, 1, 1, (q,))

    def write(hook=None, ri=None, offsets=None):
        scans = pillow_script(1)
        scans[0].dri = ri
        return write_progressive(32, 32, blocks, [JW.Comp(1)], [[(0, q)]], scans, hook=hook, scan_offsets=offsets)

    def at(scan, fn):
        return lambda si, ui, toks: fn(toks) if si == scan and ui == 0 else toks
    offs: list = []
    good = write(offsets=offs)
    first, end = offs[5]                                                    # the last scan: AC refinement 1 -> 0
    assert end - first >= 16
    out = [("the final scan cut in the middle", good[:first + (end - first) // 2], S["TRUNCATED"]),
           # 9 one-bits: the universal AC table has no code that starts with them
           ("a code that is no code in an AC refinement scan", write(at(3, lambda t: t[:6] + [("bits", 0xFFFF, 16)] + t[6:])),
            S["BAD_CODE"]),
           # five times (run 15, size 1) from k = 1 lands on 80 > Se = 5
           ("a run past Se", write(at(1, lambda t: [("sym", 1, 0xF1, 0), ("bits", 1, 1)] * 5 + t)), S["BAD_INDEX"])]
    rst = write(ri=1)
    marks = [k for k in range(len(rst) - 1) if rst[k] == 0xFF and 0xD0 <= rst[k + 1] <= 0xD7]
    assert len(marks) == 6 * 15
    out.append(("one RSTn removed from the third scan", rst[:marks[37]] + rst[marks[37] + 2:], S["NO_RESTART"]))
    noise = bytes(int(v) for v in rng.integers(0, 255, end - first))        # no FF: the marker structure stays intact
    import jpeg_prog_oracle as PO
    out.append(("random bytes as the final scan", good[:first] + noise + good[end:], PO.decode_coefficients(good[:first] + noise + good[end:])[2]))
    assert out[-1][2] != 0
    return out
