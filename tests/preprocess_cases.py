"""Geometries and inputs shared by tests/test_preprocess_host.py (the oracle against Pillow, on the host) and
tests/test_gpu_preprocess_sizes.py (the kernels against the oracle): both files check exactly the same cases, so a size
the kernels are held to is a size at which the oracle itself is pinned."""
import numpy as np

from oracle import resample_oracle as R

TRAIN_SIZES = (256, 257, 336, 513)     # one full pass of the 256 threads, 1st element of a 2nd, the shipped size, 1st of a 3rd
EVAL_SIZES = (257, 336, 513)
SATURATION_SIZES = (224, 336)


def train_cases(S):
    """[(name, (H, W) of the image, (top, left, h, w) of the crop)], every crop resized to S x S."""
    return [
        ("downscale both axes", (375, 500), (20, 30, 300, 400)),
        ("upscale both axes", (60, 40), (0, 0, 60, 40)),
        ("horizontal identity only", (S + 50, S + 9), (5, 3, S + 37, S)),
        ("vertical identity only", (S + 4, S + 3), (2, 1, S, S - 19)),
        ("both identity", (S + 2, S + 5), (1, 4, S, S)),
        ("8 rows x 1500 columns", (12, 1510), (3, 7, 8, 1500)),
        ("1 x 1 crop", (9, 11), (4, 6, 1, 1)),
        ("crop ends at the last row and column", (200, 300), (50, 100, 150, 200)),
    ]


def eval_sizes(S):
    return [(375, 500), (500, 375), (S, S), (S + 1, S + 6), (40, 60), (517, 1023)]


def random_image(rng, hw):
    return rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)


def saturation_images(rng):
    """[(name, image)]: 0/255 inputs, where the bicubic lobes overshoot on both sides and Pillow clips to uint8 after
    the horizontal pass and again after the vertical pass."""
    def noise(h, w):
        return np.where(rng.random((h, w, 3)) < 0.5, 0, 255).astype(np.uint8)
    y, x = np.mgrid[0:90, 0:120]
    stripes = np.stack([(x // 3) % 2, (y // 3) % 2, (x // 3 + y // 3) % 2], axis=2).astype(np.uint8) * 255
    return [("noise 90x120 (upscale)", noise(90, 120)), ("noise 500x700 (downscale)", noise(500, 700)),
            ("3-pixel stripes 90x120", stripes)]


def clip_fractions(img, S):
    """Fractions of the oracle's PRE-clip values below 0 / above 255 in the horizontal pass of img -> S x S and in the
    vertical pass over its (clipped) result: (h_lo, h_hi, v_lo, v_hi).  Restates R.resample_axis without the clip."""
    def preclip(src, axis, n_out):
        n_in = src.shape[axis]
        _, bounds, kk = R.precompute_coeffs(n_in, 0.0, float(n_in), n_out)
        s = np.moveaxis(src, axis, 0).astype(np.int64)
        acc = np.stack([(1 << (R.PRECISION_BITS - 1)) + np.tensordot(kk[o, :n].astype(np.int64), s[lo:lo + n], axes=(0, 0))
                        for o, (lo, n) in enumerate(bounds)])
        return np.moveaxis(acc >> R.PRECISION_BITS, 0, axis)
    h = preclip(img, 1, S)
    v = preclip(np.clip(h, 0, 255).astype(np.uint8), 0, S)
    return float((h < 0).mean()), float((h > 255).mean()), float((v < 0).mean()), float((v > 255).mean())
