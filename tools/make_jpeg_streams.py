#!/usr/bin/env python3
"""Generates tests/golden/jpeg_streams.npz: baseline JPEG streams that Pillow's own encoder never writes, made with
tests/jpeg_writer.py, and the pixels PILLOW decodes them to (`Image.open(...).convert("RGB")`, the reference loader's
decode).  Run where Pillow and scipy are installed (written with Pillow 12.2.0 / libjpeg-turbo):

    python tools/make_jpeg_streams.py

Named cases i < n: `file{i}`, `rgb{i}` (Pillow's pixels), `meta{i}` = (components, h_samp, v_samp, restart interval),
`tag{i}`, `gamut{i}`; `refused[i]` (the reason a header-only stream must be refused with, else "") and `differ[i]` (pixels
in which tests/jpeg_oracle.py differs from Pillow).  `gamut` = 1: the coefficient blocks come from a forward DCT of 8-bit
samples (`jpeg_writer.forward`), any quantiser -- the oracle must equal Pillow there, and this script asserts it (oracle
on images of <= 10 000 pixels; the larger ones are compared by tests/test_jpeg_streams_host.py through the decoder's own
code).  `gamut` = 0: header-valid streams no encoder produces; `rgb` is Pillow's output as a record, `differ` is written
into DESIGN.md 9f.  The geometry sweep (every size 1..18 squared x gray / 4:4:4 / 4:2:2 / 4:2:0 x flat / gradient) is
packed into `sweep_*` arrays (jpeg_writer.load_streams reads both).
"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_oracle as J          # noqa: E402
import jpeg_writer as JW         # noqa: E402
from jpeg_writer import AC_SYMBOLS, DC_SYMBOLS, Comp   # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MODES = {"gray": (1, 1, 1), "444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)}


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy()


def ramp_q(base, step):
    i, j = np.mgrid[0:8, 0:8]
    return np.clip(base + step * (i + j), 1, 255).reshape(64)


Q1, Q255 = np.full(64, 1), np.full(64, 255)
QA, QB, QC = ramp_q(2, 1), ramp_q(5, 3), ramp_q(17, 2)                       # three clearly different tables
DC_FLAT, AC_FLAT = JW.flat_table(DC_SYMBOLS), JW.flat_table(AC_SYMBOLS)      # 4-bit / 8-bit codes: look-ahead path only
DC_LONG, AC_LONG = JW.long_table(DC_SYMBOLS, 3), JW.long_table(AC_SYMBOLS, 20)
DC_REV, AC_REV = JW.long_table(DC_SYMBOLS[::-1], 5), JW.long_table(AC_SYMBOLS[::-1], 40)
DC_1016, AC_1016 = JW.spread_table(DC_SYMBOLS, 10, 16), JW.spread_table(AC_SYMBOLS, 10, 16)   # every code 10..16 bits


def noise_img(rng, H, W, block=5, noise=12.0):
    base = rng.integers(0, 256, (-(-H // block), -(-W // block), 3))
    img = np.kron(base, np.ones((block, block, 1)))[:H, :W] + rng.normal(0, noise, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def simple(pixels, mode, quants=(QA, QB, QC), dct=(DC_FLAT, DC_FLAT, DC_FLAT), act=(AC_FLAT, AC_FLAT, AC_FLAT),
           ids=(1, 2, 3), tq=(0, 1, 2), td=(0, 1, 2), ta=(0, 1, 2), one_segment=False, blocks=None, **kw):
    """One stream of `pixels` with per-component tables; equal tables under equal ids are written once."""
    nc, hs, vs = MODES[mode]
    if blocks is None:
        blocks = JW.forward(pixels[..., 0] if nc == 1 and pixels.ndim == 3 else pixels, hs, vs, quants)
    H, W = pixels.shape[:2]
    comps = [Comp(ids[c], hs if c == 0 else 1, vs if c == 0 else 1, tq[c], td[c], ta[c]) for c in range(nc)]
    dq, dh, seen = [], [], set()
    for c in range(nc):
        if ("q", tq[c]) not in seen:
            dq.append((tq[c], quants[c]))
        if ("d", td[c]) not in seen:
            dh.append((0, td[c]) + tuple(dct[c]))
        if ("a", ta[c]) not in seen:
            dh.append((1, ta[c]) + tuple(act[c]))
        seen |= {("q", tq[c]), ("d", td[c]), ("a", ta[c])}
    dqt = [dq] if one_segment else [[t] for t in dq]
    dht = [dh] if one_segment else [[t] for t in dh]
    return JW.write_jpeg(W, H, blocks, comps, kw.pop("dqt", dqt), kw.pop("dht", dht), **kw)


CASES = []


def case(tag, data, mode, ri, gamut=1, refused=""):
    nc, hs, vs = MODES[mode]
    if refused:
        i = data.index(b"\xff\xda")
        data = data[:i + 2 + ((data[i + 2] << 8) | data[i + 3])]
        try:
            J.parse(data)
            raise AssertionError(tag + ": the oracle accepts it")
        except J.Unsupported as e:
            assert e.reason == refused, (tag, e.reason)
        CASES.append(dict(tag=tag, file=data, rgb=np.zeros((0, 0, 3), np.uint8), meta=(nc, hs, vs, ri), gamut=gamut,
                          refused=refused, differ=0))
        return
    rgb = pillow_rgb(data)
    differ = -1
    if rgb.shape[0] * rgb.shape[1] <= 10000:
        got = J.decode(data)
        differ = int((got != rgb).any(-1).sum())
    if gamut:
        assert differ <= 0, f"{tag}: the oracle differs from Pillow in {differ} pixels of an in-gamut stream"
        differ = 0
    h = J.parse(data)
    assert (h.components, h.h_samp, h.v_samp, h.restart_interval) == (nc, hs, vs, ri), tag
    CASES.append(dict(tag=tag, file=data, rgb=rgb, meta=(nc, hs, vs, ri), gamut=gamut, refused="", differ=differ))
    print(f"{len(CASES) - 1:3d} {tag:72s} {len(data):6d} B {rgb.shape[1]}x{rgb.shape[0]} differ={differ}")


def small_jpeg(rng, W, H, ri):
    """a complete gray file with restart markers: the payload of APP1 and the stream appended behind EOI"""
    return simple(rng.integers(0, 256, (H, W), dtype=np.uint8), "gray", quants=(QB,), restart_interval=ri)


def main():
    rng = np.random.default_rng(20261018)

    # ---- third table slots: quantisation ids 3, 0, 2; three DC and three AC tables under ids that are not 0 1 2 in order.
    # Cb / Cr get very different tables and differently ordered codes, so a decoder that swaps components 1 and 2 (or
    # reads slot 1 for component 2) changes pixels.
    for mode in ("444", "422", "420"):
        img = noise_img(rng, 24, 24)
        case(f"third slots {mode}: DQT ids 3 0 2, DC ids 2 0 3, AC ids 1 3 0", simple(
            img, mode, quants=(QA, QC, QB), dct=(DC_LONG, DC_FLAT, DC_REV), act=(AC_REV, AC_LONG, AC_FLAT),
            tq=(3, 0, 2), td=(2, 0, 3), ta=(1, 3, 0)), mode, 0)
        a = pillow_rgb(CASES[-1]["file"])
        swapped = simple(img, mode, quants=(QA, QB, QC), dct=(DC_LONG, DC_FLAT, DC_REV), act=(AC_REV, AC_LONG, AC_FLAT),
                         tq=(3, 0, 2), td=(2, 0, 3), ta=(1, 3, 0),
                         blocks=JW.forward(img, *MODES[mode][1:], (QA, QC, QB)))
        assert (pillow_rgb(swapped) != a).any(), "swapping the chroma quantisation tables must change pixels"

    # ---- tables
    img = noise_img(rng, 32, 32)
    case("all tables in one DQT and one DHT segment, 4:2:0", simple(img, "420", one_segment=True, act=(AC_FLAT, AC_LONG, AC_REV)),
         "420", 0)
    junk_q = ramp_q(90, 20)
    case("tables redefined before SOS: DQT 0 and DHT AC 0 / DC 1 written twice, the last wins", simple(
        img, "420", dqt=[[(0, junk_q), (1, QB)], [(2, QC), (0, QA)]],
        dht=[[(1, 0) + tuple(AC_REV), (0, 1) + tuple(DC_REV)], [(0, 0) + tuple(DC_FLAT)], [(0, 1) + tuple(DC_FLAT), (0, 2) + tuple(DC_LONG)],
             [(1, 0) + tuple(AC_FLAT), (1, 1) + tuple(AC_LONG), (1, 2) + tuple(AC_FLAT)]],
        dct=(DC_FLAT, DC_FLAT, DC_LONG), act=(AC_FLAT, AC_LONG, AC_FLAT)), "420", 0)
    case("every code used is 10..16 bits long (maxcode path), 4:2:2", simple(
        img, "422", dct=(DC_1016,) * 3, act=(AC_1016,) * 3, td=(0, 0, 0), ta=(0, 0, 0)), "422", 0)
    case("no code longer than 9 bits (look-ahead path), 4:4:4", simple(img, "444"), "444", 0)
    case("16-bit codes for the rare symbols, gray", simple(img, "gray", quants=(QA,), dct=(DC_LONG,), act=(AC_LONG,)), "gray", 0)

    # ---- blocks
    img = noise_img(rng, 16, 16, noise=40.0)
    for name, q in (("1", Q1), ("255", Q255)):
        case(f"quantisers all {name}, 4:2:0 noise", simple(img, "420", quants=(q, q, q), tq=(0, 0, 0)), "420", 0)
        case(f"quantisers all {name}, gray noise, long codes", simple(img, "gray", quants=(q,), dct=(DC_LONG,), act=(AC_LONG,)), "gray", 0)
    binary = (rng.integers(0, 2, (16, 16)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:16, 0:16]
    checker = (((yy + xx) & 1) * 255).astype(np.uint8)
    uniform = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    for name, px in (("binary +-128", binary), ("checkerboard", checker), ("uniform noise", uniform)):
        for qv in (1, 2, 100, 255):
            for dc_t, ac_t, tname in ((DC_FLAT, AC_FLAT, "short codes"), (DC_1016, AC_1016, "10..16-bit codes")):
                case(f"{name} q={qv} gray, {tname}", simple(px, "gray", quants=(np.full(64, qv),), dct=(dc_t,), act=(ac_t,)), "gray", 0)
    b = JW.forward(checker, 1, 1, (Q1,))[0]
    assert (b[..., 63] != 0).all(), "checkerboard at q = 1: the last zig-zag coefficient is coded, no EOB"
    assert all(JW.block_tokens(blk, 0)[-1][0] == "ac" for blk in b.reshape(-1, 64))
    # run 62 = three ZRL + (14, s): a block that is DC plus the (7, 7) basis function only
    k = np.arange(8)
    basis = np.outer(np.cos((2 * k + 1) * 7 * np.pi / 16), np.cos((2 * k + 1) * 7 * np.pi / 16))
    px = np.clip(np.round(128 + 100 * np.tile(basis, (1, 2)) * np.array([1] * 8 + [-1] * 8)), 0, 255).astype(np.uint8)
    q = np.full(64, 16)
    q[63] = 1
    b = JW.forward(px, 1, 1, (q,))[0]
    toks = JW.block_tokens(b[0, 0], 0)
    assert [t[0] for t in toks] == ["dc", "zrl", "zrl", "zrl", "ac"] and toks[-1][1] == 14, toks
    case("run 62 as three ZRL + (14, s), gray 16x8", simple(px, "gray", quants=(q,)), "gray", 0)
    # DC differences of category 11: flat blocks 0 / 255 alternating at q = 1
    px = np.kron((np.indices((2, 4)).sum(0) & 1) * 255, np.ones((8, 8))).astype(np.uint8)
    b = JW.forward(px, 1, 1, (Q1,))[0]
    assert int(np.abs(np.diff(b.reshape(-1, 64)[:, 0])).max()).bit_length() == 11
    case("DC differences of category 11: flat 0 / 255 blocks at q = 1, gray 32x16", simple(px, "gray", quants=(Q1,)), "gray", 0)
    case("DC differences of category 11, 4:4:4 with 16-bit codes",
         simple(np.stack([px, px[::-1], px[:, ::-1]], -1), "444", quants=(Q1, Q1, Q1), tq=(0, 0, 0),
                dct=(DC_1016, DC_LONG, DC_REV)), "444", 0)
    # AC of category 10: a full-swing step inside the block at q = 1
    px = np.zeros((8, 16), np.uint8)
    px[:, 4:8] = 255
    px[4:, 8:] = 255
    b = JW.forward(px, 1, 1, (Q1,))[0]
    assert max(t[2] for blk in b.reshape(-1, 64) for t in JW.block_tokens(blk, 0) if t[0] == "ac") == 10
    case("AC of category 10: full-swing steps at q = 1, gray 16x8", simple(px, "gray", quants=(Q1,)), "gray", 0)

    # ---- geometry: the strips (the sweep is packed below)
    # libjpeg's JPEG_MAX_DIMENSION is 65500: Pillow refuses anything longer ("broken data stream"), so the strips that
    # have Pillow's pixels stop there.  ceil(65500 / 8) = 8188 restart intervals are still > 4096 units in one file.
    x = np.arange(65500)
    strip = np.stack([128 + 100 * np.sin(x / 4000.0), 128 + 90 * np.cos(x / 7000.0), (x // 257)], -1)[None].astype(np.uint8)
    case("strip 65500x1 4:2:0 (the longest libjpeg decodes)", simple(strip, "420", quants=(QC, QC, QC), tq=(0, 0, 0)), "420", 0)
    case("strip 1x4099 4:2:0", simple(strip[0, :4099, None, :], "420", quants=(QB, QC, QC), tq=(0, 1, 1)), "420", 0)
    case("strip 1x65500 gray, DRI = 1: 8188 units in one file",
         simple(strip[0, :, None, 0], "gray", quants=(QC,), restart_interval=1), "gray", 1)

    # ---- restart intervals: 40x24 at 4:4:4 is 5 x 3 = 15 MCUs, 48x32 at 4:2:0 is 3 x 2 = 6
    img = noise_img(rng, 24, 40)
    for ri, kw, why in ((2, {}, "does not divide the MCU row"), (14, {}, "total - 1"), (15, {}, "equal to the total"),
                        (65535, {}, "65535, no marker in the scan"), (1, {}, "15 intervals: the RSTn counter wraps"),
                        (2, {"dri": [7, 2]}, "DRI twice (7, then 2): the second wins"),
                        (0, {"dri": [3, 0]}, "DRI twice (3, then 0): no restart markers"),
                        (1, {"fill": 3}, "three fill bytes before every RSTn"),
                        (4, {"fill": 1, "header_fill": 2}, "fill bytes before every marker")):
        case(f"restart 4:4:4 40x24: {why}", simple(img, "444", restart_interval=ri, **kw), "444", ri)
    img420 = noise_img(rng, 32, 48)
    case("restart 4:2:0 48x32: interval 2 on rows of 3 MCUs", simple(img420, "420", restart_interval=2), "420", 2)
    case("restart 4:2:2 48x32: interval 5 on rows of 3 MCUs, long codes",
         simple(img420, "422", restart_interval=5, dct=(DC_LONG,) * 3, act=(AC_1016,) * 3, td=(3, 3, 3), ta=(3, 3, 3)), "422", 5)

    # ---- markers: one 4:2:0 32x32 stream with restart markers, headers varied
    img = noise_img(rng, 32, 32)
    inner, second = small_jpeg(rng, 24, 16, 1), small_jpeg(rng, 40, 8, 2)
    garbage = rng.integers(0, 256, 1024, dtype=np.uint8).tobytes()
    base = dict(restart_interval=1)
    ref = pillow_rgb(simple(img, "420", **base))
    variants = [
        ("APP1 holding a complete JPEG (own SOF 24x16, restart markers) + COM", dict(segments=[(0xE1, b"Exif\0\0" + inner), (0xFE, b"made by a test")])),
        ("fill bytes FF FF FF before every RSTn", dict(fill=3)),
        ("a second JPEG with restart markers and 1 KB of garbage behind EOI", dict(tail=second + garbage)),
        ("SOF1", dict(sof=0xC1)),
        ("component ids 0 1 2", dict(ids=(0, 1, 2))),
        ("component ids 10 20 30", dict(ids=(10, 20, 30))),
        ("component ids R G B with JFIF", dict(ids=(82, 71, 66))),
        ("no JFIF", dict(jfif=False)),
        ("Adobe transform 1 without JFIF", dict(jfif=False, adobe=1)),
        ("Adobe transform 2 without JFIF", dict(jfif=False, adobe=2)),
        ("Adobe transform 0 with JFIF", dict(adobe=0)),
        ("DRI equal to the MCU count", dict(restart_interval=4)),
        ("DRI = 65535 on a scan without markers", dict(restart_interval=65535)),
    ]
    for tag, kw in variants:
        args = dict(base)
        args.update(kw)
        case("markers: " + tag, simple(img, "420", **args), "420", args["restart_interval"])
        assert np.array_equal(CASES[-1]["rgb"], ref), tag + ": Pillow decodes other pixels than for the plain stream"
    g = img[..., 1]
    gref = pillow_rgb(simple(g, "gray", quants=(QA,)))
    for byte in (0x22, 0x41):
        data = JW.write_jpeg(32, 32, JW.forward(g, 1, 1, (QA,)), [Comp(1, byte >> 4, byte & 15, 0, 0, 0)], [[(0, QA)]],
                             [[(0, 0) + tuple(DC_FLAT)], [(1, 0) + tuple(AC_FLAT)]])
        case(f"markers: gray with sampling byte 0x{byte:02x}", data, "gray", 0)
        assert np.array_equal(CASES[-1]["rgb"], gref)
    case("refused: component ids R G B without JFIF", simple(img, "420", ids=(82, 71, 66), jfif=False), "420", 0, refused="rgb")
    case("refused: Adobe transform 0 without JFIF", simple(img, "420", jfif=False, adobe=0), "420", 0, refused="rgb")

    # ---- out of gamut: header-valid streams no encoder produces.  Pillow's pixels are a record only.
    wide_ac = JW.flat_table([0x00, 0xF0] + [(r << 4) | s for s in range(1, 16) for r in range(6)])    # sizes up to 15
    shape = JW.blocks_shape(32, 32, 1, 1, 1)[0]
    for amp, qv, lim in ((765, 255, 3), (765, 1, 765), (1020, 255, 4), (1020, 1, 1020), (4080, 255, 16), (4080, 16, 255)):
        blk = rng.integers(-lim, lim + 1, shape)
        case(f"out of gamut: dense random coefficients, dequantised amplitude {amp} (q = {qv}, |c| <= {lim}), gray 32x32",
             simple(np.zeros((32, 32), np.uint8), "gray", quants=(np.full(64, qv),), blocks=[blk]), "gray", 0, gamut=0)
    blk = rng.integers(-1023, 1024, shape)
    case("out of gamut: q = 255, dense |c| <= 1023 (the IDCT's 32-bit sums wrap), gray 32x32",
         simple(np.zeros((32, 32), np.uint8), "gray", quants=(Q255,), blocks=[blk]), "gray", 0, gamut=0)
    blk3 = [rng.integers(-1023, 1024, s) for s in JW.blocks_shape(32, 32, 3, 2, 2)]
    case("out of gamut: q = 255, dense |c| <= 1023, 4:2:0 32x32",
         simple(np.zeros((32, 32, 3), np.uint8), "420", quants=(Q255,) * 3, tq=(1, 1, 1), blocks=blk3), "420", 0, gamut=0)
    for qv in (1, 255):
        blk = np.zeros(shape, np.int64)
        flat = blk.reshape(-1, 64)
        for n, s in enumerate(range(11, 16)):
            for j, sign in enumerate((1, -1)):
                b = flat[(2 * n + j) % len(flat)]
                b[JW.ZIGZAG[1 + n]] = sign * ((1 << s) - 1)
                b[JW.ZIGZAG[7 + n]] = -sign * (1 << (s - 1))
        case(f"out of gamut: AC magnitudes of category 11..15 at q = {qv}, gray 32x32",
             simple(np.zeros((32, 32), np.uint8), "gray", quants=(np.full(64, qv),), act=(wide_ac,), blocks=[blk]), "gray", 0, gamut=0)
    for sign in (1, -1):
        blk = np.zeros(JW.blocks_shape(8 * 40, 8, 1, 1, 1)[0], np.int64)
        blk[0, :, 0] = sign * 2047 * np.arange(1, 41)
        case(f"out of gamut: DC predictor driven to {sign * 2047 * 40}, gray 320x8",
             simple(np.zeros((8, 320), np.uint8), "gray", quants=(Q1,), blocks=[blk]), "gray", 0, gamut=0)

    # ---- the geometry sweep: every width and height in 1..18, four modes, one flat colour and one gradient each
    files, rgbs, meta = [], [], []
    sweep_ac = {}
    for mode, (nc, hs, vs) in MODES.items():
        for H in range(1, 19):
            for W in range(1, 19):
                yy, xx = np.mgrid[0:H, 0:W]
                flat = np.broadcast_to(np.array([(37 * W) % 256, (91 * H) % 256, (53 * (W + H)) % 256], np.uint8), (H, W, 3))
                grad = np.stack([20 + 12 * xx, 230 - 11 * yy, 40 + 6 * xx + 5 * yy], -1).astype(np.uint8)
                for kind, px in enumerate((flat, grad)):
                    blocks = JW.forward(px[..., 0] if nc == 1 else px, hs, vs, (QA, QB, QB))
                    used = sorted({(t[1] << 4) | t[2] for b in blocks for blk in b.reshape(-1, 64)
                                   for t in JW.block_tokens(blk, 0) if t[0] == "ac"} | {0x00, 0xF0})
                    ac = sweep_ac.setdefault(tuple(used), JW.flat_table(used))
                    comps = [Comp(c + 1, hs if c == 0 else 1, vs if c == 0 else 1, min(c, 1), 0, 0) for c in range(nc)]
                    data = JW.write_jpeg(W, H, blocks, comps, [[(0, QA), (1, QB)][:max(1, nc - 1)]],
                                         [[(0, 0) + tuple(DC_FLAT), (1, 0) + tuple(ac)]])
                    rgb = pillow_rgb(data)
                    assert rgb.shape == (H, W, 3) and np.array_equal(J.decode(data), rgb), (mode, W, H, kind)
                    files.append(data)
                    rgbs.append(rgb.reshape(-1))
                    meta.append((nc, hs, vs, 0, W, H, kind))
        print("sweep", mode, len(files), "streams,", sum(map(len, files)), "bytes")

    out = {"n": np.int64(len(CASES)), "pillow": np.array(Image.__version__)}
    for i, c in enumerate(CASES):
        out[f"file{i}"] = np.frombuffer(c["file"], np.uint8)
        out[f"rgb{i}"] = c["rgb"]
        out[f"meta{i}"] = np.array(c["meta"], np.int64)
        out[f"tag{i}"] = np.array(c["tag"])
        out[f"gamut{i}"] = np.int64(c["gamut"])
    out["refused"] = np.array([c["refused"] for c in CASES])
    out["differ"] = np.array([c["differ"] for c in CASES], np.int64)
    out["sweep_files"] = np.frombuffer(b"".join(files), np.uint8)
    out["sweep_file_len"] = np.array([len(f) for f in files], np.uint16)
    out["sweep_rgb"] = np.concatenate(rgbs)
    out["sweep_meta"] = np.array(meta, np.int16)
    path = os.path.join(GOLD, "jpeg_streams.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes;", len(CASES), "named +", len(files), "sweep streams; Pillow", Image.__version__)
    assert size < 512 * 1024
    print("out-of-gamut streams, pixels in which the oracle differs from Pillow:")
    for c in CASES:
        if not c["gamut"]:
            print(f"  {c['differ']:5d} of {c['rgb'].shape[0] * c['rgb'].shape[1]:5d}  {c['tag']}")


if __name__ == "__main__":
    main()
