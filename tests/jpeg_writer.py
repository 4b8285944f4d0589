"""A baseline JPEG stream WRITER for tests (numpy; scipy only for the forward DCT).  It is never imported by the product.

Pillow's encoder (libjpeg-turbo's writer) has habits -- table ids 0 and 1, one table per DQT / DHT segment, component ids
1 2 3, a JFIF header, no fill bytes, nothing behind EOI -- so streams written by it leave most of what a decoder's parser
and table handling can get wrong untested.  This writer takes explicit quantised coefficient blocks and every such choice
as a parameter:

    data = write_jpeg(width, height, blocks, comps=[Comp(1, 2, 2, tq=3, td=2, ta=0), ...],
                      dqt=[[(3, q_luma), (0, q_cb)], [(2, q_cr)]],          # segments, each a list of (id, natural-order table)
                      dht=[[(0, 2, bits, vals), (1, 0, bits, vals)], ...],  # segments, each a list of (class, id, bits, vals)
                      restart_interval=3, dri=[7, 3], fill=2, sof=0xC1, jfif=False, adobe=1,
                      segments=[(0xE1, payload), (0xFE, b"comment")], tail=b"...")

`blocks[c]` is an integer array [blocks_y, blocks_x, 64] in natural order, padded to whole MCUs (the layout of
`jpeg_oracle.decode_coefficients`).  A table id written twice is allowed: the last definition in file order is the one
the scan is coded with.  The entropy-coded data gets `FF 00` stuffing and 1-bit padding of the last byte of every
interval; `RSTn` cycles n = 0..7.

    blocks = forward(pixels_rgb_or_gray, h_samp, v_samp, [q_y, q_cb, q_cr])   # "in-gamut" content: float64 DCT of real
                                                                               # 8-bit samples, divided, rounded
    bits, vals = long_table(symbols, n16)          # a valid Huffman table with n16 codes of 16 bits
    bits, vals = table_from_lengths({symbol: length})

Corrupt streams for the status tests come from `hook(c, index, tokens) -> tokens` (tokens of one block: ("dc", size, value),
("ac", run, size, value), ("zrl",), ("eob",), ("raw", value, nbits), ("stop",) = end the scan here) and from
`block_offsets` (the byte offset inside the entropy-coded data at which each block starts).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


@dataclass
class Comp:
    id: int
    h: int = 1
    v: int = 1
    tq: int = 0
    td: int = 0
    ta: int = 0


# ---- Huffman tables ---------------------------------------------------------------------------------------------------

def table_from_lengths(lengths: Dict[int, int]) -> Tuple[np.ndarray, np.ndarray]:
    """{symbol: code length 1..16} -> (bits[17], vals) in the DHT's form.  The lengths must leave the all-ones code of
    every length unused (ITU T.81 Annex C; libjpeg refuses a table that uses it)."""
    order = sorted(lengths, key=lambda s: (lengths[s], s))
    bits = np.zeros(17, np.int64)
    for s in order:
        assert 1 <= lengths[s] <= 16 and 0 <= s <= 255
        bits[lengths[s]] += 1
    code = 0
    for l in range(1, 17):
        code += int(bits[l])
        assert code < (1 << l), f"lengths {sorted(lengths.values())} use the all-ones code of length {l} or more"
        code <<= 1
    return bits, np.array(order, np.int64)


def long_table(symbols: Sequence[int], n16: int, long_first: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """A valid table over `symbols` in which `n16` symbols carry 16-bit codes (the decoder's `maxcode` path; codes of at
    most 9 bits take its look-ahead table).  The 16-bit codes go to the LAST symbols, or to the first with `long_first`;
    the others all get the shortest common length that leaves half the code space free."""
    symbols = list(symbols)
    assert 0 <= n16 <= len(symbols) and n16 <= 16384
    short = symbols[n16:] if long_first else symbols[:len(symbols) - n16]
    long_ = symbols[:n16] if long_first else symbols[len(symbols) - n16:]
    L = 1
    while (1 << L) < 2 * len(short) + 1:
        L += 1
    lengths = {s: L for s in short}
    lengths.update({s: 16 for s in long_})
    return table_from_lengths(lengths)


def spread_table(symbols: Sequence[int], lo: int, hi: int, filler: Sequence[int] = ()) -> Tuple[np.ndarray, np.ndarray]:
    """`symbols` get code lengths cycling through lo..hi (e.g. 10..16: every symbol used is on the long-code path);
    `filler` symbols take one short code each (length 2, 3, ...) so the long codes start behind a non-trivial prefix."""
    lengths = {s: 2 + i for i, s in enumerate(filler)}
    for i, s in enumerate(symbols):
        lengths[s] = lo + i % (hi - lo + 1)
    return table_from_lengths(lengths)


def _codes(bits, vals) -> Dict[int, Tuple[int, int]]:
    out, code, p = {}, 0, 0
    for l in range(1, 17):
        for _ in range(int(bits[l])):
            out[int(vals[p])] = (code, l)
            code += 1
            p += 1
        code <<= 1
    return out


AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for s in range(1, 11) for r in range(16)]        # the 162 of baseline coding
DC_SYMBOLS = list(range(12))


def flat_table(symbols: Sequence[int], length: Optional[int] = None):
    """All symbols at one length (default: the shortest that fits)."""
    L = length or max(1, int(np.ceil(np.log2(len(symbols) + 1))))
    return table_from_lengths({s: L for s in symbols})


# ---- bit writer -------------------------------------------------------------------------------------------------------

class _BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value: int, nbits: int):
        assert 0 <= value < (1 << nbits)
        self.acc = (self.acc << nbits) | value
        self.n += nbits
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 255
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _size(v: int) -> int:
    return int(abs(int(v))).bit_length()


def _bits_of(v: int, s: int) -> int:
    return v if v >= 0 else v + (1 << s) - 1


def block_tokens(blk: np.ndarray, pred: int) -> List[tuple]:
    """One block (natural order) -> its tokens; runs of 16 zeros are ZRL, trailing zeros one EOB."""
    zz = [int(x) for x in np.asarray(blk)[ZIGZAG]]
    d = zz[0] - pred
    toks: List[tuple] = [("dc", _size(d), d)]
    run = 0
    last = max((k for k in range(1, 64) if zz[k]), default=0)
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            toks.append(("zrl",))
            run -= 16
        toks.append(("ac", run, _size(zz[k]), zz[k]))
        run = 0
    if last < 63:
        toks.append(("eob",))
    return toks


class _Stop(Exception):
    pass


def _emit(bw: _BitWriter, toks, dc, ac):
    for t in toks:
        if t[0] == "dc":
            code, l = dc[t[1]]
            bw.put(code, l)
            if t[1]:
                bw.put(_bits_of(t[2], t[1]), t[1])
        elif t[0] == "ac":
            code, l = ac[(t[1] << 4) | t[2]]
            bw.put(code, l)
            bw.put(_bits_of(t[3], t[2]), t[2])
        elif t[0] == "zrl":
            bw.put(*ac[0xF0])
        elif t[0] == "eob":
            bw.put(*ac[0x00])
        elif t[0] == "raw":
            bw.put(t[1], t[2])
        elif t[0] == "stop":
            raise _Stop()
        else:
            raise ValueError(t)


# ---- the file ---------------------------------------------------------------------------------------------------------

def _segment(marker: int, payload: bytes) -> bytes:
    assert len(payload) + 2 <= 65535
    return bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)


def jfif_segment() -> Tuple[int, bytes]:
    return 0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"


def adobe_segment(transform: int) -> Tuple[int, bytes]:
    return 0xEE, b"Adobe\0\x64\x00\x00\x00\x00" + bytes([transform])


def write_jpeg(width: int, height: int, blocks: Sequence[np.ndarray], comps: Sequence[Comp], dqt, dht, *,
               restart_interval: int = 0, dri: Optional[Sequence[int]] = None, fill: int = 0, header_fill: int = 0,
               sof: int = 0xC0, jfif: bool = True, adobe: Optional[int] = None, segments: Sequence[Tuple[int, bytes]] = (),
               tail: bytes = b"", eoi: bool = True, hook: Optional[Callable] = None,
               block_offsets: Optional[list] = None) -> bytes:
    """See the module docstring.  `dri`: the DRI segments written, in order (default: one with `restart_interval`, none
    for 0); the scan is coded with `restart_interval` whatever they say, so the last one should equal it.  `fill`: FF
    bytes in front of every RSTn marker; `header_fill`: in front of every header marker behind SOI."""
    nc = len(comps)
    assert nc in (1, 3) and len(blocks) == nc and sof in (0xC0, 0xC1)
    hs, vs = (comps[0].h, comps[0].v) if nc == 3 else (1, 1)
    mx, my = -(-width // (8 * hs)), -(-height // (8 * vs))
    for c, b in enumerate(blocks):
        want = (my * (vs if c == 0 and nc == 3 else 1), mx * (hs if c == 0 and nc == 3 else 1), 64)
        assert tuple(b.shape) == want, (c, b.shape, want)
    fillb = b"\xff" * header_fill
    out = bytearray(b"\xff\xd8")
    head: List[Tuple[int, bytes]] = []
    if jfif:
        head.append(jfif_segment())
    if adobe is not None:
        head.append(adobe_segment(adobe))
    head += list(segments)
    qlast: Dict[int, np.ndarray] = {}
    for seg in dqt:
        payload = b""
        for tid, tab in seg:
            tab = np.asarray(tab).reshape(64)
            assert 0 <= tid <= 3 and tab.min() >= 1 and tab.max() <= 255
            payload += bytes([tid]) + bytes(int(x) for x in tab[ZIGZAG])
            qlast[tid] = tab
        head.append((0xDB, payload))
    head.append((sof, bytes([8, height >> 8, height & 255, width >> 8, width & 255, nc]) +
                 b"".join(bytes([c.id, (c.h << 4) | c.v, c.tq]) for c in comps)))   # gray: the factors are ignored
    hlast: Dict[Tuple[int, int], Dict[int, Tuple[int, int]]] = {}
    for seg in dht:
        payload = b""
        for tc, th, bits, vals in seg:
            assert tc in (0, 1) and 0 <= th <= 3 and int(np.sum(bits[1:])) == len(vals)
            payload += bytes([(tc << 4) | th]) + bytes(int(x) for x in bits[1:17]) + bytes(int(x) for x in vals)
            hlast[(tc, th)] = _codes(bits, vals)
        head.append((0xC4, payload))
    for v in ([restart_interval] if restart_interval else []) if dri is None else dri:
        head.append((0xDD, bytes([v >> 8, v & 255])))
    head.append((0xDA, bytes([nc]) + b"".join(bytes([c.id, (c.td << 4) | c.ta]) for c in comps) + b"\x00\x3f\x00"))
    for marker, payload in head:
        out += fillb + _segment(marker, payload)
    # ---- the scan
    bw = _BitWriter()
    pred = [0] * nc
    total = mx * my
    rst = 0
    scan = bytearray()
    counters = [0] * nc
    try:
        for mcu in range(total):
            if restart_interval and mcu and mcu % restart_interval == 0:
                bw.flush()
                scan += bw.out + b"\xff" * fill + bytes([0xFF, 0xD0 + rst])
                rst = (rst + 1) & 7
                bw = _BitWriter()
                pred = [0] * nc
            yy, xx = divmod(mcu, mx)
            for c, comp in enumerate(comps):
                ch, cv = (hs, vs) if (c == 0 and nc == 3) else (1, 1)
                for j in range(ch * cv):
                    blk = blocks[c][yy * cv + j // ch, xx * ch + j % ch]
                    toks = block_tokens(blk, pred[c])
                    pred[c] = int(blk[0])
                    if hook is not None:
                        toks = hook(c, counters[c], toks)
                    counters[c] += 1
                    if block_offsets is not None:
                        block_offsets.append(len(scan) + len(bw.out))
                    _emit(bw, toks, hlast[(0, comp.td)], hlast[(1, comp.ta)])
    except _Stop:
        pass
    bw.flush()
    scan += bw.out
    out += scan
    if eoi:
        out += b"\xff" * fill + b"\xff\xd9"
    return bytes(out + tail)


# ---- pixels -> blocks -------------------------------------------------------------------------------------------------

def rgb_to_ycc(rgb: np.ndarray) -> np.ndarray:
    rgb = rgb.astype(np.float64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    cb = -0.168735892 * r - 0.331264108 * g + 0.5 * b + 128.0
    cr = 0.5 * r - 0.418687589 * g - 0.081312411 * b + 128.0
    return np.clip(np.round(np.stack([y, cb, cr], -1)), 0, 255)


def plane_to_blocks(plane: np.ndarray, by: int, bx: int, quant: np.ndarray) -> np.ndarray:
    """8-bit sample plane (any size <= by*8 x bx*8, edge-replicated to it) -> quantised coefficients [by, bx, 64]: level
    shift, float64 orthonormal DCT-II per 8x8 block, divide by the table (natural order), round half away from zero."""
    from scipy.fft import dctn
    p = np.asarray(plane, np.float64)
    assert p.min() >= 0 and p.max() <= 255
    p = np.pad(p, ((0, by * 8 - p.shape[0]), (0, bx * 8 - p.shape[1])), mode="edge") - 128.0
    b = p.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3)
    co = dctn(b, axes=(-2, -1), norm="ortho").reshape(by, bx, 64) / np.asarray(quant, np.float64).reshape(64)
    return (np.sign(co) * np.floor(np.abs(co) + 0.5)).astype(np.int64)


def forward(pixels: np.ndarray, h_samp: int, v_samp: int, quants: Sequence[np.ndarray], ycc: bool = False):
    """uint8 [H, W] (gray) or [H, W, 3] (RGB, or YCbCr samples with `ycc`) -> blocks per component for `write_jpeg`.
    Chroma is box-averaged to the subsampled size (rounded to 8-bit samples again)."""
    pixels = np.asarray(pixels)
    H, W = pixels.shape[:2]
    if pixels.ndim == 2:
        return [plane_to_blocks(pixels, -(-H // 8), -(-W // 8), quants[0])]
    planes = pixels.astype(np.float64) if ycc else rgb_to_ycc(pixels)
    mx, my = -(-W // (8 * h_samp)), -(-H // (8 * v_samp))
    out = [plane_to_blocks(planes[..., 0], my * v_samp, mx * h_samp, quants[0])]
    for c in (1, 2):
        p = np.pad(planes[..., c], ((0, my * v_samp * 8 - H), (0, mx * h_samp * 8 - W)), mode="edge")
        p = p.reshape(my * 8, v_samp, mx * 8, h_samp).mean((1, 3))
        out.append(plane_to_blocks(np.clip(np.round(p), 0, 255), my, mx, quants[c]))
    return out


def blocks_shape(width: int, height: int, nc: int, hs: int, vs: int) -> List[Tuple[int, int, int]]:
    if nc == 1:
        return [(-(-height // 8), -(-width // 8), 64)]
    mx, my = -(-width // (8 * hs)), -(-height // (8 * vs))
    return [(my * vs, mx * hs, 64), (my, mx, 64), (my, mx, 64)]


# ---- fixtures written by tools/make_jpeg_streams.py --------------------------------------------------------------------

def load_streams(path: str) -> List[dict]:
    """tests/golden/jpeg_streams.npz -> [{file, rgb, meta, tag, gamut, refused, differ}].  The named cases are stored as
    jpeg_small.npz stores its own (`file{i}`, `rgb{i}`, `meta{i}`, plus `tag{i}`, `gamut{i}` and the arrays `refused`,
    `differ`); the geometry sweep's
    thousands of tiny streams are packed into `sweep_*` arrays, because a zip entry costs more than such a stream."""
    g = np.load(path)
    out = []
    for i in range(int(g["n"])):
        out.append({"file": g[f"file{i}"].tobytes(), "rgb": g[f"rgb{i}"], "meta": tuple(int(v) for v in g[f"meta{i}"]),
                    "tag": str(g[f"tag{i}"]), "gamut": int(g[f"gamut{i}"]), "refused": str(g["refused"][i]),
                    "differ": int(g["differ"][i])})
    files, rgbs, meta = g["sweep_files"], g["sweep_rgb"], g["sweep_meta"].astype(np.int64)
    fo = np.concatenate([[0], np.cumsum(g["sweep_file_len"].astype(np.int64))])
    ro = np.concatenate([[0], np.cumsum(3 * meta[:, 4] * meta[:, 5])])
    for k in range(len(meta)):
        nc, hs, vs, ri, W, H, kind = (int(v) for v in meta[k])
        out.append({"file": files[fo[k]:fo[k + 1]].tobytes(), "rgb": rgbs[ro[k]:ro[k + 1]].reshape(H, W, 3),
                    "meta": (nc, hs, vs, ri), "tag": f"sweep {W}x{H} {'gray' if nc == 1 else f'{hs}x{vs}'} "
                    f"{'flat' if kind == 0 else 'gradient'}", "gamut": 1, "refused": "", "differ": 0})
    return out


# ---- corrupt streams, built live ---------------------------------------------------------------------------------------

STATUS = {"TRUNCATED": 1, "BAD_CODE": 2, "BAD_INDEX": 3, "NO_RESTART": 4}          # include/rpo_amd.h RPO_JPEG_*


def corrupt_streams() -> List[Tuple[str, bytes, int]]:
    """[(what, file, the status word the device must leave)]: gray 32x32 (16 blocks), header-valid, each wrong in one known
    place of the entropy-coded data.  All of them go through tests/host/jpeg_host_decode.cpp (tests/test_jpeg_streams_host.py)
    before a GPU test decodes them."""
    rng = np.random.default_rng(77)
    px = np.clip(np.kron(rng.integers(0, 256, (8, 8)), np.ones((4, 4))) + rng.normal(0, 10, (32, 32)), 0, 255).astype(np.uint8)
    i, j = np.mgrid[0:8, 0:8]
    q = (2 + i + j).reshape(64)
    blocks = forward(px, 1, 1, (q,))
    dc, dc13, ac = flat_table(DC_SYMBOLS), flat_table(list(range(13))), flat_table(AC_SYMBOLS)   # 8-bit AC codes: 94 unused

    def write(hook=None, dct=dc, ri=0, offsets=None):
        return write_jpeg(32, 32, blocks, [Comp(1)], [[(0, q)]], [[(0, 0) + tuple(dct), (1, 0) + tuple(ac)]],
                          restart_interval=ri, hook=hook, block_offsets=offsets)

    def at(n, fn):
        return lambda c, idx, toks: fn(toks) if idx == n else toks
    out = [("an AC symbol outside the table", write(at(5, lambda t: t[:2] + [("raw", 0xFFFF, 16)] + t[2:])), STATUS["BAD_CODE"]),
           ("a DC symbol of category 12", write(at(5, lambda t: [("dc", 12, 2500)] + t[1:]), dct=dc13), STATUS["BAD_CODE"]),
           ("a run that lands past index 63", write(at(5, lambda t: t[:1] + [("ac", 15, 1, 1)] * 4 + [("eob",)])), STATUS["BAD_INDEX"])]
    offs: List[int] = []
    good = write(offsets=offs)
    scan = good.index(b"\xff\xda") + 10                                     # SOS of one component: 2 + 8 bytes
    assert offs[4] - offs[3] >= 4
    out.append(("the scan cut inside block 3", good[:scan + offs[3] + (offs[4] - offs[3]) // 2], STATUS["TRUNCATED"]))
    rst = write(ri=1)
    marks = [k for k in range(scan, len(rst) - 1) if rst[k] == 0xFF and 0xD0 <= rst[k + 1] <= 0xD7]
    assert len(marks) == 15
    out.append(("one RSTn removed from the middle", rst[:marks[7]] + rst[marks[7] + 2:], STATUS["NO_RESTART"]))
    return out
