"""CPU restatement (numpy only) of the baseline JPEG decode the reference's dataset loader ends in: Dassl's `read_image`
is `PIL.Image.open(path).convert("RGB")`, and Pillow decodes through libjpeg(-turbo) with its defaults -- the "islow"
integer IDCT, "fancy" (triangle) chroma upsampling and 16.16 fixed-point YCbCr -> RGB.  This file restates that path from
its conventional, published statement (ITU T.81 for the entropy coding, the Independent JPEG Group's documented
arithmetic for the rest); it is the checker of rpo_amd/csrc/jpeg.hip and is never imported by the product.

Pinned by tests/test_jpeg_host.py: bit-identical to the committed fixtures (tests/golden/jpeg_*.npz, written with Pillow
by tools/make_jpeg_golden.py) and, where Pillow is importable, to Pillow itself on freshly encoded files.

    rgb = decode(file_bytes)                 # uint8 [H, W, 3]
    hdr = parse(file_bytes)                  # Header; raises Unsupported(reason) for what the device refuses too
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Unsupported(ValueError):
    """A well-formed file of a kind the device decoder refuses (reason = the C ABI's reason name)."""

    def __init__(self, reason: str):
        super().__init__(reason)
        self.reason = reason


class Corrupt(ValueError):
    pass


@dataclass
class Header:
    width: int = 0
    height: int = 0
    components: int = 0
    h_samp: int = 1                       # luma sampling factors: 1x1 (4:4:4, gray), 2x1 (4:2:2), 2x2 (4:2:0)
    v_samp: int = 1
    restart_interval: int = 0
    scan_offset: int = 0                  # first entropy-coded byte
    quant: List[np.ndarray] = field(default_factory=list)            # per component, natural order, int64 [64]
    dc: List[Tuple[np.ndarray, np.ndarray]] = field(default_factory=list)   # per component (bits[17], vals)
    ac: List[Tuple[np.ndarray, np.ndarray]] = field(default_factory=list)

    @property
    def mcus_x(self) -> int:
        return -(-self.width // (8 * self.h_samp))

    @property
    def mcus_y(self) -> int:
        return -(-self.height // (8 * self.v_samp))


def parse(data: bytes) -> Header:
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise Corrupt("not a JPEG")
    pos = 2
    qt: Dict[int, np.ndarray] = {}
    ht: Dict[Tuple[int, int], Tuple[np.ndarray, np.ndarray]] = {}
    h = Header()
    frame = None
    jfif = False
    adobe = None
    while True:
        if pos + 2 > n:
            raise Corrupt("truncated")
        if data[pos] != 0xFF:
            raise Corrupt("marker expected")
        m = data[pos + 1]
        pos += 2
        if m == 0xFF:
            pos -= 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise Corrupt("no scan")
        if pos + 2 > n:
            raise Corrupt("truncated")
        L = (data[pos] << 8) | data[pos + 1]
        if L < 2 or pos + L > n:
            raise Corrupt("truncated")
        seg = data[pos + 2:pos + L]
        pos += L
        if m in (0xC2, 0xC6, 0xCA, 0xCE):
            raise Unsupported("progressive")
        if m in (0xC9, 0xCB, 0xCD, 0xCF, 0xCC):
            raise Unsupported("arithmetic")
        if m in (0xC3, 0xC5, 0xC7):
            raise Unsupported("lossless")
        if m in (0xC0, 0xC1):
            if frame is not None or len(seg) < 6:
                raise Corrupt("frame")
            if seg[0] != 8:
                raise Unsupported("precision")
            h.height, h.width, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if len(seg) != 6 + 3 * nc or h.height == 0 or h.width == 0:
                raise Corrupt("frame")
            if nc not in (1, 3):
                raise Unsupported("components")
            frame = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
            h.components = nc
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                pq, tq = seg[p] >> 4, seg[p] & 15
                if tq > 3:
                    raise Corrupt("DQT")
                if pq:
                    raise Unsupported("quant16")
                if p + 65 > len(seg):
                    raise Corrupt("DQT")
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(seg[p + 1:p + 65], np.uint8)
                qt[tq] = t
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                if p + 17 > len(seg):
                    raise Corrupt("DHT")
                tc, th = seg[p] >> 4, seg[p] & 15
                bits = np.zeros(17, np.int64)
                bits[1:] = np.frombuffer(seg[p + 1:p + 17], np.uint8)
                cnt = int(bits.sum())
                if tc > 1 or th > 3 or cnt > 256 or p + 17 + cnt > len(seg):
                    raise Corrupt("DHT")
                ht[(tc, th)] = (bits, np.frombuffer(seg[p + 17:p + 17 + cnt], np.uint8).astype(np.int64))
                p += 17 + cnt
        elif m == 0xDD:
            if len(seg) != 2:
                raise Corrupt("DRI")
            h.restart_interval = (seg[0] << 8) | seg[1]
        elif m == 0xE0:
            if len(seg) >= 5 and seg[:5] == b"JFIF\0":
                jfif = True
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise Corrupt("scan before frame")
            ns = seg[0] if seg else 0
            if len(seg) != 4 + 2 * ns:
                raise Corrupt("SOS")
            if ns != h.components:
                raise Unsupported("multiscan")
            if h.components == 3:
                ids = bytes(f[0] for f in frame)
                if not jfif and (adobe == 0 or (adobe is None and ids == b"RGB")):
                    raise Unsupported("rgb")
                (_, h0, v0, _), (_, h1, v1, _), (_, h2, v2, _) = frame
                if (h1, v1, h2, v2) != (1, 1, 1, 1) or (h0, v0) not in ((1, 1), (2, 1), (2, 2)):
                    raise Unsupported("sampling")
                h.h_samp, h.v_samp = h0, v0
            for i in range(ns):
                cid, tabs = seg[1 + 2 * i], seg[2 + 2 * i]
                if cid != frame[i][0]:
                    raise Unsupported("multiscan")
                td, ta = tabs >> 4, tabs & 15
                if frame[i][3] not in qt or (0, td) not in ht or (1, ta) not in ht:
                    raise Corrupt("missing table")
                h.quant.append(qt[frame[i][3]])
                h.dc.append(ht[(0, td)])
                h.ac.append(ht[(1, ta)])
            h.scan_offset = pos
            return h
        # every other segment (APPn, COM, DNL, ...) is skipped


def _derive(bits: np.ndarray, vals: np.ndarray):
    """code length -> (first code, last code, index of the first value); ITU T.81 Annex C / F.2.2.3"""
    out, code, p = {}, 0, 0
    for l in range(1, 17):
        nb = int(bits[l])
        if nb:
            out[l] = (code, code + nb - 1, p)
            code += nb
            p += nb
        if code > (1 << l):
            raise Corrupt("DHT")
        code <<= 1
    return out


class _Bits:
    """The entropy-coded segment as a bit source: FF 00 unstuffed, zeros fed at a marker or the end of the file."""

    def __init__(self, data: bytes, pos: int):
        self.d, self.pos, self.acc, self.n, self.fake = data, pos, 0, 0, 0

    def _fill(self):
        d = self.d
        b = 0
        if self.fake == 0 and self.pos < len(d):
            b = d[self.pos]
            if b == 0xFF:
                if self.pos + 1 < len(d) and d[self.pos + 1] == 0:
                    self.pos += 2
                else:
                    b, self.fake = 0, 8
            else:
                self.pos += 1
        else:
            self.fake += 8
        self.acc = (self.acc << 8) | b
        self.n += 8

    def get(self, k: int) -> int:
        while self.n < k:
            self._fill()
        self.n -= k
        v = (self.acc >> self.n) & ((1 << k) - 1)
        self.acc &= (1 << self.n) - 1
        return v

    def overrun(self) -> bool:
        return self.fake > self.n

    def restart(self):
        """Drops the bits left of the interval and steps over the RSTn marker."""
        self.acc = self.n = self.fake = 0
        d = self.d
        while self.pos + 1 < len(d) and not (d[self.pos] == 0xFF and 0xD0 <= d[self.pos + 1] <= 0xD7):
            self.pos += 1
        if self.pos + 1 >= len(d):
            raise Corrupt("restart marker missing")
        self.pos += 2


def _huff(br: _Bits, tab) -> int:
    code = 0
    for l in range(1, 17):
        code = (code << 1) | br.get(1)
        e = tab[0].get(l)
        if e is not None and e[0] <= code <= e[1]:
            return int(tab[1][e[2] + code - e[0]])
    raise Corrupt("bad Huffman code")


def _extend(v: int, s: int) -> int:
    return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def decode_coefficients(data: bytes, h: Header) -> List[np.ndarray]:
    """Quantised coefficients per component: int64 [blocks_y, blocks_x, 64] in natural order, padded to whole MCUs."""
    nc = h.components
    samp = [(h.h_samp, h.v_samp)] + [(1, 1)] * (nc - 1) if nc == 3 else [(1, 1)]
    planes = [np.zeros((h.mcus_y * v, h.mcus_x * hh, 64), np.int64) for hh, v in samp]
    dct = [(_derive(*t), t[1]) for t in h.dc]
    act = [(_derive(*t), t[1]) for t in h.ac]
    br = _Bits(data, h.scan_offset)
    pred = [0] * nc
    total = h.mcus_x * h.mcus_y
    for mcu in range(total):
        if h.restart_interval and mcu and mcu % h.restart_interval == 0:
            br.restart()
            pred = [0] * nc
        my, mx = divmod(mcu, h.mcus_x)
        for c in range(nc):
            hh, v = samp[c]
            for j in range(hh * v):
                blk = planes[c][my * v + j // hh, mx * hh + j % hh]
                s = _huff(br, dct[c])
                if s > 11:
                    raise Corrupt("DC size")
                if s:
                    pred[c] += _extend(br.get(s), s)
                blk[0] = _wrap(pred[c], 16)                 # a coefficient is an int16: the predictor's low 16 bits
                k = 1
                while k < 64:
                    rs = _huff(br, act[c])
                    r, s = rs >> 4, rs & 15
                    if s:
                        k += r
                        if k > 63:
                            raise Corrupt("coefficient index")
                        blk[ZIGZAG[k]] = _extend(br.get(s), s)
                        k += 1
                    elif r == 15:
                        k += 16
                    else:
                        break
        if br.overrun():
            raise Corrupt("truncated scan")
    return planes


def _wrap(v, bits: int):
    """v as a two's-complement number of `bits` bits"""
    half = 1 << (bits - 1)
    return ((v + half) & ((1 << bits) - 1)) - half


def _idct_pass(d: np.ndarray, shift: int) -> np.ndarray:
    """One 1-D pass of the "islow" IDCT (13-bit constants) along axis -2 of d[..., 8, n]; descale by `shift`.
    The definition (the device's, rpo_amd/csrc/jpeg.hip idct_1d): sums and products modulo 2^32, the sum plus the rounding
    constant read as a signed 32-bit number, arithmetic shift.  + and * commute with the reduction, so the sums are formed
    exactly here (|input| < 2^23.1 and constants < 2^15: far inside int64) and reduced once.  For every block an encoder
    makes from 8-bit samples nothing exceeds 31 bits and the reduction does nothing."""
    in0, in1, in2, in3, in4, in5, in6, in7 = (d[..., i, :] for i in range(8))
    z1 = (in2 + in6) * 4433
    tmp2 = z1 + in6 * -15137
    tmp3 = z1 + in2 * 6270
    tmp0 = (in0 + in4) << 13
    tmp1 = (in0 - in4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = in7, in5, in3, in1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    rnd = 1 << (shift - 1)
    out = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return np.stack([_wrap(o + rnd, 32) >> shift for o in out], axis=-2)


def idct(coef: np.ndarray, quant: np.ndarray) -> np.ndarray:
    """[by, bx, 64] quantised coefficients -> uint8 sample plane [by*8, bx*8]: dequantise, columns (descale 11), rows
    (descale 18), +128, clamp."""
    by, bx, _ = coef.shape
    d = (coef * quant).reshape(by, bx, 8, 8)                     # [.., row, col]
    ws = _idct_pass(d, 11)                                        # along rows index = column transform
    out = _idct_pass(ws.swapaxes(-1, -2), 18).swapaxes(-1, -2)    # row transform
    out = np.clip(out + 128, 0, 255).astype(np.uint8)
    return out.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def _upsample_h(p: np.ndarray) -> np.ndarray:
    """h2v1 triangle filter on rows of int64 [rows, cw] -> [rows, 2*cw]; the edges copy the edge sample."""
    cw = p.shape[1]
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    even = (3 * p + left + 1) >> 2
    odd = (3 * p + right + 2) >> 2
    even[:, 0] = p[:, 0]
    odd[:, -1] = p[:, -1]
    out = np.empty((p.shape[0], 2 * cw), np.int64)
    out[:, 0::2], out[:, 1::2] = even, odd
    return out


def _upsample_hv(p: np.ndarray) -> np.ndarray:
    """h2v2 triangle filter: column sums 3*near + far, then (3*this + neighbour + 8 | 7) >> 4."""
    ch, cw = p.shape
    up = np.concatenate([p[:1], p[:-1]], 0)
    down = np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    for r, far in ((0, up), (1, down)):
        t = 3 * p + far
        left = np.concatenate([t[:, :1], t[:, :-1]], 1)
        right = np.concatenate([t[:, 1:], t[:, -1:]], 1)
        out[r::2, 0::2] = (3 * t + left + 8) >> 4
        out[r::2, 1::2] = (3 * t + right + 7) >> 4
    return out


def upsample(plane: np.ndarray, cw: int, ch: int, hs: int, vs: int) -> np.ndarray:
    """Chroma plane (real samples [ch, cw]) to luma resolution.  A plane at most 2 samples wide is replicated."""
    p = plane[:ch, :cw].astype(np.int64)
    if hs == 1 and vs == 1:
        return p
    if cw <= 2:
        return np.repeat(np.repeat(p, vs, 0), hs, 1)
    return _upsample_h(p) if vs == 1 else _upsample_hv(p)


def ycc_to_rgb(y: np.ndarray, cb: np.ndarray, cr: np.ndarray) -> np.ndarray:
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data: bytes) -> np.ndarray:
    h = parse(data)
    coefs = decode_coefficients(data, h)
    planes = [idct(c, q) for c, q in zip(coefs, h.quant)]
    H, W = h.height, h.width
    if h.components == 1:
        g = planes[0][:H, :W]
        return np.stack([g, g, g], -1)
    cw, ch = -(-W // h.h_samp), -(-H // h.v_samp)
    cb = upsample(planes[1], cw, ch, h.h_samp, h.v_samp)[:H, :W]
    cr = upsample(planes[2], cw, ch, h.h_samp, h.v_samp)[:H, :W]
    return ycc_to_rgb(planes[0][:H, :W], cb, cr)
