"""CPU restatement (pure Python + numpy) of the PROGRESSIVE coefficient decode (ITU T.81 Annex G: spectral selection and
successive approximation, Huffman coded), the checker of the progressive half of rpo_amd/csrc/jpeg.hip.  It walks the file
by itself, decodes scan after scan into the quantised coefficient planes `jpeg_oracle.decode_coefficients` would give for the
baseline file of the same blocks, and hands them to `jpeg_oracle.idct` / `upsample` / `ycc_to_rgb`.  Never imported by the
product; pure Python, so only small images (tests use it up to 10 000 pixels).

    rgb = decode(file_bytes)                 # uint8 [H, W, 3]; raises Corrupt(status) with the device's status word
    planes, prog = decode_coefficients(file_bytes)
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

import jpeg_oracle as J

ZIGZAG = [int(v) for v in J.ZIGZAG]
OK, TRUNCATED, BAD_CODE, BAD_INDEX, NO_RESTART = range(5)          # include/rpo_amd.h RPO_JPEG_*


class Corrupt(J.Corrupt):
    def __init__(self, status: int):
        super().__init__(f"device status {status}")
        self.status = status


@dataclass
class Scan:
    comps: List[int]
    ss: int
    se: int
    ah: int
    al: int
    ri: int
    dc: list                              # per scan component: (derived, vals) or None
    ac: object
    starts: List[int] = field(default_factory=list)   # per restart interval found: first byte


@dataclass
class Prog:
    width: int = 0
    height: int = 0
    components: int = 0
    h_samp: int = 1
    v_samp: int = 1
    quant: List[np.ndarray] = field(default_factory=list)
    scans: List[Scan] = field(default_factory=list)

    @property
    def mcus_x(self) -> int:
        return -(-self.width // (8 * self.h_samp))

    @property
    def mcus_y(self) -> int:
        return -(-self.height // (8 * self.v_samp))


def parse(data: bytes) -> Prog:
    """The markers of a well-formed SOF2 file (what the device refuses is the business of rpo_jpeg_prog_probe's tests)."""
    n = len(data)
    assert data[:2] == b"\xff\xd8"
    pos, g, qt, ht, frame, ri = 2, Prog(), {}, {}, None, 0
    while pos + 2 <= n:
        assert data[pos] == 0xFF, pos
        m = data[pos + 1]
        pos += 2
        if m == 0xFF:
            pos -= 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            break
        L = (data[pos] << 8) | data[pos + 1]
        seg = data[pos + 2:pos + L]
        pos += L
        if m == 0xC2:
            assert seg[0] == 8
            g.height, g.width, g.components = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            frame = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(g.components)]
            if g.components == 3:
                g.h_samp, g.v_samp = frame[0][1], frame[0][2]
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                t = np.zeros(64, np.int64)
                t[J.ZIGZAG] = np.frombuffer(seg[p + 1:p + 65], np.uint8)
                qt[seg[p] & 15] = t
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                bits = np.zeros(17, np.int64)
                bits[1:] = np.frombuffer(seg[p + 1:p + 17], np.uint8)
                cnt = int(bits.sum())
                vals = np.frombuffer(seg[p + 17:p + 17 + cnt], np.uint8).astype(np.int64)
                ht[(seg[p] >> 4, seg[p] & 15)] = (J._derive(bits, vals), vals)
                p += 17 + cnt
        elif m == 0xDD:
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            ns = seg[0]
            ids = [f[0] for f in frame]
            comps = [ids.index(seg[1 + 2 * i]) for i in range(ns)]
            ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            sc = Scan(comps, ss, se, ah, al, ri,
                      [ht.get((0, seg[2 + 2 * i] >> 4)) if ss == 0 and ah == 0 else None for i in range(ns)],
                      ht.get((1, seg[2] & 15)) if ss > 0 else None, [pos])
            while pos < n:                                   # to the marker that ends the scan
                if data[pos] != 0xFF:
                    pos += 1
                elif pos + 1 >= n:
                    pos = n
                elif data[pos + 1] == 0:
                    pos += 2
                elif data[pos + 1] == 0xFF:
                    pos += 1
                elif 0xD0 <= data[pos + 1] <= 0xD7:
                    pos += 2
                    sc.starts.append(pos)
                else:
                    break
            if not g.quant:
                g.quant = [qt[f[3]] for f in frame]
            g.scans.append(sc)
    return g


def _bit(br) -> int:
    return br.get(1)


def _refine(br, blk, z, p1):
    if _bit(br):
        v = int(blk[z])
        if (v & p1) == 0:                                    # Python's & on a negative int is two's complement, as int16's
            blk[z] = v + p1 if v >= 0 else v - p1


def _block(br, sc: Scan, ci: int, blk, st) -> None:
    """One block of one scan; st = {"pred": [..], "eobrun": n}.  Raises Corrupt."""
    p1 = 1 << sc.al
    if sc.se == 0:
        if sc.ah == 0:
            try:
                s = J._huff(br, sc.dc[ci])
            except J.Corrupt:
                raise Corrupt(BAD_CODE)
            if s > 11:
                raise Corrupt(BAD_CODE)
            if s:
                st["pred"][ci] += J._extend(br.get(s), s)
            blk[0] = J._wrap(st["pred"][ci] << sc.al, 16)
        elif _bit(br):
            blk[0] = J._wrap(int(blk[0]) | p1, 16)
        return
    if sc.ah == 0:
        if st["eobrun"] > 0:
            st["eobrun"] -= 1
            return
        k = sc.ss
        while k <= sc.se:
            try:
                rs = J._huff(br, sc.ac)
            except J.Corrupt:
                raise Corrupt(BAD_CODE)
            r, s = rs >> 4, rs & 15
            if s:
                k += r
                if k > sc.se:
                    raise Corrupt(BAD_INDEX)
                blk[ZIGZAG[k]] = J._wrap(J._extend(br.get(s), s) << sc.al, 16)
                k += 1
            elif r == 15:
                k += 16
            else:
                st["eobrun"] = (1 << r) + (br.get(r) if r else 0) - 1
                break
        return
    k = sc.ss
    if st["eobrun"] == 0:
        while k <= sc.se:
            try:
                rs = J._huff(br, sc.ac)
            except J.Corrupt:
                raise Corrupt(BAD_CODE)
            r, s = rs >> 4, rs & 15
            val = 0
            if s:
                if s != 1:
                    raise Corrupt(BAD_CODE)
                val = p1 if _bit(br) else -p1
            elif r != 15:
                st["eobrun"] = (1 << r) + (br.get(r) if r else 0)
                break
            while k <= sc.se:
                z = ZIGZAG[k]
                if blk[z] != 0:
                    _refine(br, blk, z, p1)
                else:
                    r -= 1
                    if r < 0:
                        break
                k += 1
            if s:
                if k > sc.se:
                    raise Corrupt(BAD_INDEX)
                blk[ZIGZAG[k]] = val
            k += 1
    if st["eobrun"] > 0:
        while k <= sc.se:
            z = ZIGZAG[k]
            if blk[z] != 0:
                _refine(br, blk, z, p1)
            k += 1
        st["eobrun"] -= 1


def decode_coefficients(data: bytes) -> Tuple[List[np.ndarray], Prog, int]:
    """-> (planes as jpeg_oracle.decode_coefficients lays them out, the parsed file, the device's status word: the largest
    over the units, each unit stopping at its first error)"""
    g = parse(data)
    nc = g.components
    samp = [(g.h_samp, g.v_samp), (1, 1), (1, 1)] if nc == 3 else [(1, 1)]
    planes = [np.zeros((g.mcus_y * v, g.mcus_x * h, 64), np.int64) for h, v in samp]
    status = OK
    for sc in g.scans:
        if len(sc.comps) > 1:
            total, walk = g.mcus_x * g.mcus_y, None
        else:
            c = sc.comps[0]
            bw = -(-(-(-g.width * samp[c][0] // g.h_samp)) // 8)
            bh = -(-(-(-g.height * samp[c][1] // g.v_samp)) // 8)
            total = bw * bh
        ri = sc.ri or total
        for unit in range(-(-total // ri)):
            if unit >= len(sc.starts):
                status = max(status, NO_RESTART)
                continue
            br = J._Bits(data, sc.starts[unit])
            st = {"pred": [0, 0, 0], "eobrun": 0}
            try:
                for m in range(unit * ri, min((unit + 1) * ri, total)):
                    if len(sc.comps) == 1:
                        _block(br, sc, 0, planes[c][m // bw, m % bw], st)
                        if br.overrun():
                            raise Corrupt(TRUNCATED)
                        continue
                    my, mx = divmod(m, g.mcus_x)
                    for i, cc in enumerate(sc.comps):
                        h, v = samp[cc]
                        for j in range(h * v):
                            _block(br, sc, i, planes[cc][my * v + j // h, mx * h + j % h], st)
                            if br.overrun():
                                raise Corrupt(TRUNCATED)
            except Corrupt as e:
                status = max(status, e.status)
    return planes, g, status


def decode(data: bytes) -> np.ndarray:
    coefs, g, status = decode_coefficients(data)
    if status:
        raise Corrupt(status)
    planes = [J.idct(c, q) for c, q in zip(coefs, g.quant)]
    H, W = g.height, g.width
    if g.components == 1:
        y = planes[0][:H, :W]
        return np.stack([y, y, y], -1)
    cw, ch = -(-W // g.h_samp), -(-H // g.v_samp)
    cb = J.upsample(planes[1], cw, ch, g.h_samp, g.v_samp)[:H, :W]
    cr = J.upsample(planes[2], cw, ch, g.h_samp, g.v_samp)[:H, :W]
    return J.ycc_to_rgb(planes[0][:H, :W], cb, cr)
