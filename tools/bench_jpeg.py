#!/usr/bin/env python3
"""Throughput of the on-device JPEG decode against the host decode it replaces; prints ONE JSON line.

Input: synthetic photo-like 375 x 500 JPEGs (smooth gradients, soft blobs, hard-edged blocks, sensor-like noise), quality
90, 4:2:0, written with Pillow: `--distinct` different files, cycled up to the largest size.  `--files x.npz` reads them
from a file written by `--write-files x.npz` instead (for a box without Pillow).

Per size n in --sizes (default 32 304 1024 4096), each timed end to end with host clocks around a device sync:
  device_decode   JpegDecoder(chunk_images=n).decode(files[:n])      probe + pack + upload of the compressed bytes + the four
                                                                     kernels + the status read-back
  device_set      DeviceImageSet.from_jpeg(files[:n], chunk_images=n)
  host_decode     Pillow `Image.open(...).convert("RGB")` of the same files on 16 host threads (the comparator's first half)
  host_set        host_decode + DeviceImageSet(decoded)               the comparator: what a user does without this decoder
The arms alternate repeat by repeat.  Required (the JSON's `device_set_beats_host_set_at_largest`): at the largest size the
device path's MEDIAN time is below the comparator's BEST repeat.  `n_fallback == 0` is asserted for every set built.

--trace N: only device_decode at size N, a few times (run under `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def photo_like(rng, H=375, W=500):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.zeros((H, W, 3), np.float32)
    for c in range(3):
        a, b = rng.uniform(-0.3, 0.3, 2)
        img[..., c] = rng.uniform(60, 190) + a * xx + b * yy
    for _ in range(12):                                            # soft blobs
        cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(15, 90)
        img += rng.uniform(-90, 90, 3) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))[..., None]
    for _ in range(8):                                             # hard edges
        y0, x0 = int(rng.integers(0, H - 20)), int(rng.integers(0, W - 20))
        img[y0:y0 + int(rng.integers(10, 120)), x0:x0 + int(rng.integers(10, 160))] += rng.uniform(-70, 70, 3)
    img += rng.normal(0, 6, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def make_files(distinct, seed=2024):
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(distinct):
        b = io.BytesIO()
        Image.fromarray(photo_like(rng)).save(b, "JPEG", quality=90, subsampling=2)
        out.append(b.getvalue())
    return out


def _timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 304, 1024, 4096])
    ap.add_argument("--distinct", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--files")
    ap.add_argument("--write-files")
    ap.add_argument("--trace", type=int)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.write_files:
        files = make_files(a.distinct)
        np.savez(a.write_files, **{f"f{i}": np.frombuffer(f, np.uint8) for i, f in enumerate(files)})
        print("wrote", a.write_files, sum(map(len, files)), "bytes of JPEG")
        return
    if a.files:
        g = np.load(a.files)
        base = [g[f"f{i}"].tobytes() for i in range(len(g.files))]
    else:
        base = make_files(a.distinct)
    import torch
    from rpo_amd.input_pipeline import DeviceImageSet
    from rpo_amd.jpeg import JpegDecoder
    assert torch.cuda.is_available(), "bench_jpeg needs cuda:0"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    if a.trace:
        files = [base[i % len(base)] for i in range(a.trace)]
        dec = JpegDecoder(dev, chunk_images=a.trace)
        for _ in range(3):
            dec.decode(files)
        torch.cuda.synchronize()
        return
    try:
        from PIL import Image
        pool = ThreadPoolExecutor(a.threads)

        def host_decode(files):
            return list(pool.map(lambda f: np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), files))
    except ImportError:
        host_decode = None
    rows = {}
    for n in a.sizes:
        files = [base[i % len(base)] for i in range(n)]
        labels = [i % 19 for i in range(n)]
        dec = JpegDecoder(dev, chunk_images=n)

        def device_set():
            ds = DeviceImageSet.from_jpeg(files, labels, dev, chunk_images=n)
            assert ds.n_fallback == 0 and ds.n_device == n
            return ds

        arms = {"device_decode": lambda: dec.decode(files), "device_set": device_set}
        if host_decode is not None:
            arms["host_decode"] = lambda: host_decode(files)
            arms["host_set"] = lambda: DeviceImageSet(host_decode(files), labels, dev)
        times = {k: [] for k in arms}
        for r in range(a.warmup + a.repeats):
            for k, fn in arms.items():
                t, res = _timed(fn, torch)
                del res
                if r >= a.warmup:
                    times[k].append(t)
        row = {"jpeg_bytes_mean": round(sum(map(len, files)) / n)}
        for k, v in times.items():
            med = statistics.median(v)
            row[k] = {"median_ms": round(1e3 * med, 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3),
                      "images_s_median": round(n / med, 1), "images_s_best": round(n / min(v), 1)}
        if "host_set" in row:
            row["device_set_median_over_host_set_best"] = round(row["host_set"]["min_ms"] / row["device_set"]["median_ms"], 3)
        rows[str(n)] = row
    big = rows[str(max(a.sizes))]
    out = {"metric": "jpeg_bench", "device": torch.cuda.get_device_name(0), "image": "375x500 q90 4:2:0 synthetic photo-like",
           "distinct_files": len(base), "host_threads": a.threads, "repeats": a.repeats, "sizes": rows,
           "comparator": "Pillow on this box" if host_decode is not None else "absent (Pillow not importable)",
           "test_rate_images_s_9e": 14200}
    if "host_set" in big:
        out["device_set_beats_host_set_at_largest"] = bool(big["device_set"]["median_ms"] < big["host_set"]["min_ms"])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
