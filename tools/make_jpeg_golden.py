#!/usr/bin/env python3
"""Generates tests/golden/jpeg_small.npz, jpeg_photo.npz and jpeg_refused.npz with Pillow -- the library the reference's
dataset loader ends in (Dassl `read_image` -> `PIL.Image.open(path).convert("RGB")`).  Run where Pillow is installed
(written with Pillow 12.2.0 / libjpeg-turbo):

    python tools/make_jpeg_golden.py

jpeg_small / jpeg_photo: per case i the file bytes `file{i}`, Pillow's decoded pixels `rgb{i}` (uint8 [H, W, 3]) and
`meta{i}` = (components, h_samp, v_samp, restart interval in MCUs).  The content is blocky colour plus noise, so AC
coefficients and chroma edges are exercised.  jpeg_refused: files of the kinds the device decoder refuses, cut behind the
first scan header (the header is all `rpo_jpeg_probe` reads), with the reason expected.
"""
import io
import os

import numpy as np
from PIL import Image, ImageFile

ImageFile.MAXBLOCK = 1 << 22
GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
SAMP = {"444": (0, 1, 1), "422": (1, 2, 1), "420": (2, 2, 2)}


def content(rng, H, W, block=5, noise=12.0):
    base = rng.integers(0, 256, (-(-H // block), -(-W // block), 3))
    img = np.kron(base, np.ones((block, block, 1)))[:H, :W] + rng.normal(0, noise, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(img, mode, **kw):
    b = io.BytesIO()
    if mode == "L":
        Image.fromarray(img[..., 0]).save(b, "JPEG", **kw)
    else:
        Image.fromarray(img).save(b, "JPEG", subsampling=SAMP[mode][0], **kw)
    return b.getvalue()


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy()


def header_only(data):
    i = data.index(b"\xff\xda")
    return data[:i + 2 + ((data[i + 2] << 8) | data[i + 3])]


def write(name, cases):
    out = {"n": np.int64(len(cases))}
    for i, (data, meta) in enumerate(cases):
        out[f"file{i}"] = np.frombuffer(data, np.uint8)
        out[f"rgb{i}"] = pillow_rgb(data)
        out[f"meta{i}"] = np.array(meta, np.int64)
    path = os.path.join(GOLD, name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def main():
    rng = np.random.default_rng(20261017)
    small = [  # W, H, mode, quality, extra
        (1, 1, "444", 75, {}), (1, 1, "L", 75, {}), (8, 8, "420", 95, {}),
        (2, 3, "420", 75, {}), (3, 2, "422", 75, {}), (4, 4, "420", 95, {}), (5, 5, "420", 75, {}),    # replication rule
        (17, 9, "422", 30, {}), (17, 9, "L", 75, {}), (33, 16, "420", 75, {"optimize": True}),
        (33, 16, "444", 95, {"optimize": True, "restart_marker_blocks": 1}),
        (16, 16, "444", 30, {}), (64, 48, "422", 95, {"optimize": True}),
        (100, 75, "444", 95, {}), (100, 75, "420", 75, {"restart_marker_blocks": 1}),
        (100, 75, "422", 75, {"restart_marker_blocks": 3}), (100, 75, "L", 100, {"restart_marker_blocks": 3}),
        (100, 75, "420", 100, {}), (100, 75, "420", 30, {"optimize": True}), (100, 75, "422", 100, {}),
        (75, 100, "420", 95, {"restart_marker_blocks": 3}),
    ]
    cases = []
    for (W, H, mode, q, kw) in small:
        data = encode(content(rng, H, W), mode, quality=q, **kw)
        nc, hs, vs = (1, 1, 1) if mode == "L" else (3, SAMP[mode][1], SAMP[mode][2])
        cases.append((data, (nc, hs, vs, kw.get("restart_marker_blocks", 0))))
    write("jpeg_small.npz", cases)
    photo = encode(content(rng, 375, 500, block=25, noise=5.0), "420", quality=90)
    write("jpeg_photo.npz", [(photo, (3, 2, 2, 0))])

    img = content(rng, 24, 32)
    refused = {
        "progressive": encode(img, "420", quality=75, progressive=True),
        "components": (lambda b: (Image.fromarray(img).convert("CMYK").save(b, "JPEG"), b.getvalue())[1])(io.BytesIO()),
        "rgb": (lambda b: (Image.fromarray(img).save(b, "JPEG", keep_rgb=True), b.getvalue())[1])(io.BytesIO()),
    }
    out = {}
    for k, data in refused.items():
        Image.open(io.BytesIO(data)).load()                      # Pillow itself reads the whole file
        out[k] = np.frombuffer(header_only(data), np.uint8)
    # 4:1:1 (luma 4x1): Pillow's encoder does not write it (its "4:1:1" is 4:2:0), so the luma sampling byte of a 4:2:0
    # header is rewritten
    h = bytearray(header_only(encode(img, "420", quality=75)))
    sof = h.index(b"\xff\xc0")
    assert h[sof + 11] == 0x22
    h[sof + 11] = 0x41
    out["sampling"] = np.frombuffer(bytes(h), np.uint8)
    out["reasons"] = np.array(sorted(out))
    path = os.path.join(GOLD, "jpeg_refused.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; Pillow", Image.__version__)


if __name__ == "__main__":
    main()
