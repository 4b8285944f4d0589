#!/usr/bin/env python3
"""Generates tests/golden/jpeg_progressive.npz: progressive (SOF2) JPEG streams -- Pillow-written ones over the sizes,
samplings, qualities and restart intervals at which a progressive decoder can go wrong, and streams under scan scripts
Pillow never writes, made with tests/jpeg_prog_writer.py -- each with the pixels PILLOW decodes it to
(`Image.open(...).convert("RGB")`, the reference loader's decode), plus headers that `rpo_jpeg_prog_probe` must refuse with
the code expected.  Run where Pillow and scipy are installed (written with Pillow 12.2.0 / libjpeg-turbo):

    python tools/make_jpeg_progressive.py

Everything is packed into a few arrays (`jpeg_prog_writer.load_progressive` reads them).  The script asserts what the tags
claim (from the writer's token streams) and that tests/jpeg_prog_oracle.py equals Pillow on every stream of at most 10 000
pixels; writer-made streams carry the baseline file of the same coefficient blocks (`twins`), which Pillow must decode to
the same pixels.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_prog_oracle as PO    # noqa: E402
import jpeg_prog_writer as PW    # noqa: E402
import jpeg_writer as JW         # noqa: E402
from jpeg_prog_writer import Scan   # noqa: E402
from jpeg_writer import Comp     # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MODES = {"gray": (1, 1, 1), "444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)}
SUB = {"444": 0, "422": 1, "420": 2}
E_COMPONENTS, E_ARITHMETIC, E_SCRIPT, E_SEQUENTIAL = -25, -22, -29, -30       # include/rpo_amd.h
STREAMS, REFUSED = [], []


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy()


def content(rng, H, W, block=4, noise=6.0):
    base = rng.integers(0, 256, (-(-H // block), -(-W // block), 3))
    img = np.kron(base, np.ones((block, block, 1)))[:H, :W] + rng.normal(0, noise, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(img, mode, **kw):
    b = io.BytesIO()
    if mode == "gray":
        Image.fromarray(img[..., 0] if img.ndim == 3 else img).save(b, "JPEG", progressive=True, **kw)
    else:
        Image.fromarray(img).save(b, "JPEG", progressive=True, subsampling=SUB[mode], **kw)
    return b.getvalue()


def add(tag, data, twin=None):
    rgb = pillow_rgb(data)
    if rgb.shape[0] * rgb.shape[1] <= 10000:
        assert np.array_equal(PO.decode(data), rgb), tag + ": the oracle differs from Pillow"
    if twin is not None:
        assert np.array_equal(pillow_rgb(twin), rgb), tag + ": Pillow decodes the baseline twin to other pixels"
    STREAMS.append(dict(tag=tag, file=data, rgb=rgb, twin=twin or b""))
    print(f"{len(STREAMS) - 1:4d} {tag:90s} {len(data):7d} B {rgb.shape[1]}x{rgb.shape[0]}")


def refuse(tag, data, code):
    REFUSED.append(dict(tag=tag, file=data, code=code))


def ramp_q(base, step):
    i, j = np.mgrid[0:8, 0:8]
    return np.clip(base + step * (i + j), 1, 255).reshape(64)


QA, QB = ramp_q(2, 1), ramp_q(4, 2)


def comps_of(mode, **kw):
    nc, hs, vs = MODES[mode]
    return [Comp(1, hs, vs, 0, **kw)] + ([Comp(2, 1, 1, 1, **kw), Comp(3, 1, 1, 1, **kw)] if nc == 3 else [])


def written(tag, pixels, mode, scans, blocks=None, **kw):
    """one writer-made stream + its baseline twin"""
    nc, hs, vs = MODES[mode]
    H, W = pixels.shape[:2]
    if blocks is None:
        blocks = JW.forward(pixels[..., 0] if nc == 1 else pixels, hs, vs, [QA, QB, QB])
    comps = comps_of(mode)
    dqt = [[(0, QA)]] + ([[(1, QB)]] if nc == 3 else [])
    data = PW.write_progressive(W, H, blocks, comps, dqt, scans, **kw)
    add(tag, data, PW.write_baseline(W, H, blocks, comps, dqt))
    return data, blocks, comps, dqt


def chain(comps, ss, se, al):
    """first scan at `al`, then the refinements down to 0"""
    return [Scan(comps, ss, se, 0, al)] + [Scan(comps, ss, se, a + 1, a) for a in range(al - 1, -1, -1)]


def units_of(W, H, blocks, comps, scans):
    out, ri = [], 0
    for sc in scans:
        ri = ri if sc.dri is None else sc.dri
        out.append(PW.scan_units(W, H, blocks, comps, sc, ri))
    return out


def main():
    rng = np.random.default_rng(20261018)
    # ---- Pillow-written ---------------------------------------------------------------------------------------------
    sizes = (1, 7, 8, 9, 16, 17, 24, 33)
    k = 0
    for mode in MODES:
        for H in sizes:
            for W in sizes:
                q = (30, 95)[(k + k // 8) % 2]
                k += 1
                add(f"pillow {W}x{H} {mode} q{q}", encode(content(rng, H, W), mode, quality=q))
    for mode in MODES:
        for (W, H) in ((17, 33), (33, 17), (24, 9)):
            img = content(rng, H, W)
            add(f"pillow {W}x{H} {mode} q95 optimize", encode(img, mode, quality=95, optimize=True))
            for rmb in (1, 3, 2 if W == 17 else 4):               # 17 and 33 wide: 3 / 5 blocks a row, neither divides
                add(f"pillow {W}x{H} {mode} q30 restart_marker_blocks {rmb}" + (" (does not divide the row)" if rmb in (2, 4) else ""),
                    encode(img, mode, quality=30, restart_marker_blocks=rmb))
    tile = content(rng, 16, 96, block=6, noise=8.0)
    photo = np.tile(tile, (24, 6, 1))[:375, :500]                 # photo-like statistics; periodic so that the record packs
    add("pillow 500x375 420 q90 photo-like", encode(photo, "420", quality=90))
    flat = encode(np.full((1024, 2048), 128, np.uint8), "gray", quality=75)
    add("pillow 2048x1024 gray flat: 32768 blocks, EOBRUN 32767 then 1", flat)
    # the r = 14 symbol (EOB run of 16384..32767) must occur: the first AC scan's data is that symbol + 14 bits, then EOB0
    g = PO.parse(flat)
    br = PO.J._Bits(flat, g.scans[1].starts[0])
    rs = PO.J._huff(br, g.scans[1].ac)
    assert rs == 0xE0 and br.get(14) == 16383 and PO.J._huff(br, g.scans[1].ac) == 0x00, hex(rs)

    # ---- writer-made ------------------------------------------------------------------------------------------------
    img = content(rng, 17, 24)
    for mode in MODES:
        c = list(range(MODES[mode][0]))
        written(f"writer {mode}: spectral selection only, every Al = 0", img, mode,
                [Scan(c, 0, 0, 0, 0)] + [s for i in c for s in (Scan([i], 1, 9, 0, 0), Scan([i], 10, 63, 0, 0))])
        written(f"writer {mode}: successive approximation from Al = 3 (DC and AC)", img, mode,
                chain(c, 0, 0, 3) + [s for i in c for s in chain([i], 1, 63, 3)])
        written(f"writer {mode}: non-interleaved DC, one scan per component", img, mode,
                [Scan([i], 0, 0, 0, 0) for i in c] + [Scan([i], 1, 63, 0, 0) for i in c])
    written("writer 420: successive approximation from Al = 13 on DC (14 levels)", img, "420",
            chain([0, 1, 2], 0, 0, 13) + [Scan([i], 1, 63, 0, 0) for i in range(3)])
    written("writer 422: DC of two components interleaved, the third alone", img, "422",
            [Scan([0, 2], 0, 0, 0, 1), Scan([1], 0, 0, 0, 0), Scan([0, 2], 0, 0, 1, 0)] + [Scan([i], 1, 63, 0, 0) for i in range(3)])
    written("writer gray: AC bands of one coefficient (Ss = Se), 63 of them", content(rng, 9, 16), "gray",
            [Scan([0], 0, 0, 0, 0)] + [Scan([0], k, k, 0, 0) for k in range(1, 64)])
    one = content(rng, 8, 8, block=2, noise=20.0)
    for s in range(1, 63):
        written(f"writer gray 8x8: bands split at {s}", one, "gray",
                [Scan([0], 0, 0, 0, 0), Scan([0], 1, s, 0, 1), Scan([0], s + 1, 63, 0, 0), Scan([0], 1, s, 1, 0)])
    written("writer 420: chroma before luma", img, "420",
            [Scan([0, 1, 2], 0, 0, 0, 0), Scan([1], 1, 63, 0, 0), Scan([2], 1, 63, 0, 0), Scan([0], 1, 63, 0, 0)])
    written("writer 420: an AC scan of component 2 between component 0's first and refinement scans", img, "420",
            [Scan([0, 1, 2], 0, 0, 0, 0), Scan([0], 1, 63, 0, 1), Scan([2], 1, 63, 0, 0), Scan([0], 1, 63, 1, 0), Scan([1], 1, 63, 0, 0)])
    # a table id redefined between two scans that both use it
    t1 = JW.table_from_lengths({s: 8 if s < 128 else 9 for s in range(256)})
    t2 = JW.table_from_lengths({s: 9 if s < 128 else 8 for s in range(256)})
    assert not np.array_equal(t1[1], t2[1])
    written("writer 444: AC table id 0 redefined with other contents between two scans that use it", img, "444",
            [Scan([0, 1, 2], 0, 0, 0, 0), Scan([0], 1, 63, 0, 0), Scan([1], 1, 63, 0, 0, dht=[[(1, 0) + tuple(t2)]]),
             Scan([2], 1, 63, 0, 0, dht=[[(1, 0) + tuple(t1)], [(0, 0) + tuple(JW.flat_table(JW.DC_SYMBOLS, 5))]])])
    # only 10..16-bit codes: every symbol takes the maxcode path
    nc, hs, vs = MODES["420"]
    blocks = JW.forward(img, hs, vs, [QA, QB, QB])
    scans = PW.pillow_script(3)
    sy = PW.symbols(24, 17, blocks, comps_of("420"), scans)
    dcs, acs = sorted(set().union(*(d for d, _ in sy))), sorted(set().union(*(a for _, a in sy)))
    long_dht = [[(0, 0) + tuple(JW.spread_table(dcs, 10, 16))], [(1, 0) + tuple(JW.spread_table(acs, 10, 16))]]
    written("writer 420: tables with only 10..16-bit codes", img, "420", scans, blocks=blocks, dht=long_dht)
    # EOB runs and refinement corner cases, on hand-made sparse blocks: gray 64x24 = 8 x 3 blocks
    B = np.zeros((3, 8, 64), np.int64)
    B[..., 0] = rng.integers(-60, 60, (3, 8))
    B[0, 0, [1, 8]] = (5, -3)
    B[0, 3, 1] = 4                                                # nonzero history, nothing new in the refinement scan
    B[0, 5, [1, 16]] = (-6, 7)
    B[1, 2, 8] = 6                                                # (the run 0,6 .. 1,1 holds blocks with history)
    B[1, 2, 58] = -1                                              # 40+ zero-history coefficients before it: ZRL, passing index 2
    B[1, 4, [1, 9, 2]] = (-1, -1, 9)
    B[2, 6, 1] = -1
    px = np.zeros((24, 64), np.uint8)
    sparse = [Scan([0], 0, 0, 0, 0), Scan([0], 1, 63, 0, 1), Scan([0], 1, 63, 1, 0, dri=5)]
    written("writer gray: EOBRUNs end mid-row, are cut at a restart boundary and cover blocks with nonzero history in a "
            "refinement scan; ZRL in a refinement scan passes nonzero-history coefficients; every new coefficient negative",
            px, "gray", sparse, blocks=[B])
    u = units_of(64, 24, [B], comps_of("gray"), sparse)
    runs1 = PW.eob_runs(u[1][0])
    assert any(r > 1 for r in runs1) and runs1[0] % 8 != 0, runs1             # the first run ends mid-row
    assert len(u[2]) == 5 and sum(len(PW.eob_runs(t)) > 0 and max(PW.eob_runs(t)) > 1 for t in u[2]) >= 2   # cut at restarts
    ref = [t for unit in u[2] for t in unit]
    assert any(t[0] == "sym" and t[2] == 0xF0 for t in ref), "no ZRL in the refinement scan"
    signs = [ref[i + 1][1] for i, t in enumerate(ref) if t[0] == "sym" and (t[2] & 15) == 1]
    assert len(signs) == 4 and not any(signs)
    scans = PW.pillow_script(3)
    scans[0].dri, scans[3].dri, scans[6].dri, scans[8].dri = 2, 5, 0, 1
    written("writer 420: DRI changed between scans (2, 5, 0, 1), including to 0", img, "420", scans)
    written("writer 422: fill bytes before markers", img, "422", PW.pillow_script(3), fill=2)
    scans = PW.pillow_script(3)
    scans[0].dri = 2
    written("writer 420: fill bytes before markers and RSTn", img, "420", scans, fill=3)
    written("writer 444: data behind EOI", img, "444", PW.pillow_script(3), tail=b"\xff\xda\x00\x08trailing bytes \xff\xd0\xff\xd9")

    # ---- refused ----------------------------------------------------------------------------------------------------
    blocks = JW.forward(img, 2, 2, [QA, QB, QB])
    comps, dqt = comps_of("420"), [[(0, QA)], [(1, QB)]]

    def script(scans):
        return PW.write_progressive(24, 17, blocks, comps, dqt, scans)
    full = [Scan([0, 1, 2], 0, 0, 0, 0), Scan([0], 1, 63, 0, 1), Scan([1], 1, 63, 0, 0), Scan([2], 1, 63, 0, 0)]
    refuse("incomplete script: luma coefficient 63 left at Al = 1", script(full + [Scan([0], 1, 62, 1, 0)]), E_SCRIPT)
    refuse("Ah != previous Al", script(full + [Scan([0], 1, 63, 2, 1), Scan([0], 1, 63, 1, 0)]), E_SCRIPT)
    refuse("AC before DC", script([Scan([0], 1, 63, 0, 0), Scan([0, 1, 2], 0, 0, 0, 0), Scan([1], 1, 63, 0, 0), Scan([2], 1, 63, 0, 0)]), E_SCRIPT)
    refuse("AC scan with two components", script([Scan([0, 1, 2], 0, 0, 0, 0), Scan([0], 1, 63, 0, 0), Scan([1, 2], 1, 63, 0, 0)]), E_SCRIPT)
    late = full + [Scan([0], 1, 63, 1, 0)]
    late[2].segments = [(0xDB, bytes([1]) + bytes(int(x) for x in QB[JW.ZIGZAG]))]
    refuse("DQT after the first SOS", script(late), E_SCRIPT)
    refuse("Al = 14", script(chain([0, 1, 2], 0, 0, 14) + full[1:] + [Scan([0], 1, 63, 1, 0)]), E_SCRIPT)
    b = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(b, "JPEG", progressive=True)
    refuse("progressive CMYK", b.getvalue(), E_COMPONENTS)
    good = script(full + [Scan([0], 1, 63, 1, 0)])
    assert np.array_equal(PO.decode(good), pillow_rgb(good))
    sof = good.index(b"\xff\xc2")
    refuse("SOF10 (arithmetic progressive)", good[:sof + 1] + b"\xca" + good[sof + 2:], E_ARITHMETIC)
    refuse("a baseline file given to rpo_jpeg_prog_probe", PW.write_baseline(24, 17, blocks, comps, dqt), E_SEQUENTIAL)
    for r in REFUSED:                                             # a record of what libjpeg itself does with them
        try:
            Image.open(io.BytesIO(r["file"])).load()
            print("refused", r["code"], r["tag"], "-- Pillow reads it")
        except OSError as e:
            print("refused", r["code"], r["tag"], "-- Pillow:", e)

    out = {"files": np.frombuffer(b"".join(s["file"] for s in STREAMS), np.uint8),
           "file_len": np.array([len(s["file"]) for s in STREAMS], np.int64),
           "twins": np.frombuffer(b"".join(s["twin"] for s in STREAMS), np.uint8),
           "twin_len": np.array([len(s["twin"]) for s in STREAMS], np.int64),
           "rgb": np.concatenate([s["rgb"].reshape(-1) for s in STREAMS]),
           "shape": np.array([s["rgb"].shape[:2] for s in STREAMS], np.int64),
           "tags": np.array([s["tag"] for s in STREAMS]),
           "refused_files": np.frombuffer(b"".join(r["file"] for r in REFUSED), np.uint8),
           "refused_len": np.array([len(r["file"]) for r in REFUSED], np.int64),
           "refused_code": np.array([r["code"] for r in REFUSED], np.int64),
           "refused_tags": np.array([r["tag"] for r in REFUSED])}
    path = os.path.join(GOLD, "jpeg_progressive.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes;", len(STREAMS), "streams,", len(REFUSED), "refused; Pillow", Image.__version__)
    assert size < 500 * 1024


if __name__ == "__main__":
    main()
