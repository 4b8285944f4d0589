#!/usr/bin/env python3
"""Throughput of the on-device decode of PROGRESSIVE JPEG files against the route they take without it;
prints ONE JSON line.  The protocol is tools/bench_jpeg.py's, and so are the images: its synthetic photo-like 375 x 500
pictures at quality 90, 4:2:0, written with Pillow -- here with `progressive=True`, and once more as baseline files.

Per size n in --sizes (default 32 304 1024 4096), each timed end to end with host clocks around a device sync:
  device_set        DeviceImageSet.from_jpeg(progressive files[:n], chunk_images=n, progressive=True)
  host_set          Pillow `Image.open(...).convert("RGB")` of the same files on 16 host threads, then DeviceImageSet(decoded):
                    the comparator -- today's route for these files
  baseline_set      DeviceImageSet.from_jpeg(baseline encodes of the same images): the existing device path, for scale
The arms alternate repeat by repeat.  Required (the JSON's `device_set_beats_host_set_at_largest`): at the largest size the
device path's MEDIAN time is below the comparator's BEST repeat.  `n_fallback == 0` is asserted for every device set.

--trace N: only JpegDecoder(progressive=True).decode at size N, a few times (run under `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import io
import json
import os
import statistics
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_jpeg import _timed, photo_like   # noqa: E402


def make_files(distinct, seed=2024):
    """-> (progressive, baseline) encodes of the images tools/bench_jpeg.py encodes"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    prog, base = [], []
    for _ in range(distinct):
        im = Image.fromarray(photo_like(rng))
        for out, kw in ((prog, {"progressive": True}), (base, {})):
            b = io.BytesIO()
            im.save(b, "JPEG", quality=90, subsampling=2, **kw)
            out.append(b.getvalue())
    return prog, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 304, 1024, 4096])
    ap.add_argument("--distinct", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--trace", type=int)
    ap.add_argument("--out")
    a = ap.parse_args()
    from PIL import Image
    prog, base = make_files(a.distinct)
    import torch
    from rpo_amd.input_pipeline import DeviceImageSet
    from rpo_amd.jpeg import JpegDecoder, probe
    assert torch.cuda.is_available(), "bench_jpeg_progressive needs cuda:0"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    info = probe(prog[0], progressive=True)
    if a.trace:
        files = [prog[i % len(prog)] for i in range(a.trace)]
        dec = JpegDecoder(dev, chunk_images=a.trace, progressive=True)
        for _ in range(3):
            dec.decode(files)
        torch.cuda.synchronize()
        return
    pool = ThreadPoolExecutor(a.threads)

    def host_decode(files):
        return list(pool.map(lambda f: np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), files))
    rows = {}
    for n in a.sizes:
        files, twins = [prog[i % len(prog)] for i in range(n)], [base[i % len(base)] for i in range(n)]
        labels = [i % 19 for i in range(n)]

        def device_set(fs, flag):
            ds = DeviceImageSet.from_jpeg(fs, labels, dev, chunk_images=n, progressive=flag)
            assert ds.n_fallback == 0 and ds.n_device == n
            return ds
        arms = {"device_set": lambda: device_set(files, True),
                "host_set": lambda: DeviceImageSet(host_decode(files), labels, dev),
                "baseline_set": lambda: device_set(twins, False)}
        times = {k: [] for k in arms}
        for r in range(a.warmup + a.repeats):
            for k, fn in arms.items():
                t, res = _timed(fn, torch)
                del res
                if r >= a.warmup:
                    times[k].append(t)
        row = {"jpeg_bytes_mean": round(sum(map(len, files)) / n), "baseline_jpeg_bytes_mean": round(sum(map(len, twins)) / n)}
        for k, v in times.items():
            med = statistics.median(v)
            row[k] = {"median_ms": round(1e3 * med, 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3),
                      "images_s_median": round(n / med, 1), "images_s_best": round(n / min(v), 1)}
        row["device_set_median_over_host_set_best"] = round(row["host_set"]["min_ms"] / row["device_set"]["median_ms"], 3)
        rows[str(n)] = row
    big = rows[str(max(a.sizes))]
    out = {"metric": "jpeg_progressive_bench", "device": torch.cuda.get_device_name(0),
           "image": "375x500 q90 4:2:0 synthetic photo-like, progressive=True (Pillow's 10-scan script)",
           "units_per_file": int(info.units), "levels": int(info.reserved), "distinct_files": len(prog),
           "host_threads": a.threads, "repeats": a.repeats, "sizes": rows, "comparator": "Pillow on this box",
           "device_set_beats_host_set_at_largest": bool(big["device_set"]["median_ms"] < big["host_set"]["min_ms"])}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
