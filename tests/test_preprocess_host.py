"""Host side of the on-device input transforms, no device needed: the descriptor validation (`rpo_preprocess_check`, pure
host code that launches nothing, so descriptors with wild offsets are safe to try anywhere), the tap count, the geometry
functions against the oracle's, the int32 range check of `DeviceTransform`, and the oracle itself against Pillow at the
output sizes and geometries tests/test_gpu_preprocess_sizes.py holds the kernels to."""
import numpy as np
import pytest

import preprocess_cases as PC
from oracle import resample_oracle as R

I32_MAX, I64_MAX = 2 ** 31 - 1, 2 ** 63 - 1
SIZE = 224


@pytest.fixture(scope="module")
def lib():
    from rpo_amd import _lib
    from rpo_amd.build import build_library
    build_library()
    return _lib.load()


def desc(**kw):
    """A valid descriptor of a 100 x 100 image at offset 0 (whole-image crop -> 224 x 224), with fields replaced."""
    from rpo_amd._lib import ImageDesc
    base = dict(src_offset=0, width=100, height=100, crop_x=0, crop_y=0, crop_w=100, crop_h=100, resize_w=SIZE,
                resize_h=SIZE, win_x=0, win_y=0, flip=0)
    base.update(kw)
    return ImageDesc(**base)


def run_check(lib, descs, size=SIZE, max_rows=100, kmax=5, src_bytes=30000):
    arr = (type(descs[0]) * len(descs))(*descs)
    return lib.rpo_preprocess_check(arr, len(descs), size, max_rows, kmax, src_bytes)


OVERFLOW = {                                                     # fields whose sums wrap in 32 / 64-bit arithmetic
    "crop_x INT32_MAX + crop_w 1": dict(crop_x=I32_MAX, crop_w=1),
    "crop_y INT32_MAX - 10 + crop_h 100": dict(crop_y=I32_MAX - 10, crop_h=100),
    "crop_x INT32_MAX - 10 + crop_w 100": dict(crop_x=I32_MAX - 10, crop_w=100),
    "crop_y INT32_MAX + crop_h 1": dict(crop_y=I32_MAX, crop_h=1),
    "crop_w INT32_MAX": dict(crop_x=1, crop_w=I32_MAX),
    "crop_h INT32_MAX": dict(crop_y=1, crop_h=I32_MAX),
    "win_x INT32_MAX": dict(win_x=I32_MAX),
    "win_y INT32_MAX": dict(win_y=I32_MAX),
    "win_x INT32_MAX - 100, resize_w INT32_MAX": dict(win_x=I32_MAX - 100, resize_w=I32_MAX),
    "win_y INT32_MAX - 100, resize_h INT32_MAX": dict(win_y=I32_MAX - 100, resize_h=I32_MAX),
    "src_offset INT64_MAX": dict(src_offset=I64_MAX),
    "src_offset INT64_MAX - 29999": dict(src_offset=I64_MAX - 29999),
    "width = height = INT32_MAX": dict(width=I32_MAX, height=I32_MAX),
    "width INT32_MAX": dict(width=I32_MAX),
    "height INT32_MAX": dict(height=I32_MAX),
}


@pytest.mark.parametrize("name", sorted(OVERFLOW))
def test_check_refuses_descriptors_whose_sums_overflow(lib, name):
    from rpo_amd._lib import E_SHAPE
    assert run_check(lib, [desc(**OVERFLOW[name])]) == E_SHAPE
    # the same descriptor behind two valid ones, and with a src_bytes that no image size can exceed by overflow alone
    assert run_check(lib, [desc(), desc(), desc(**OVERFLOW[name])]) == E_SHAPE
    if "src_offset" not in name and "width" not in name and "height" not in name:
        assert run_check(lib, [desc(**OVERFLOW[name])], src_bytes=I64_MAX) == E_SHAPE


def test_check_refuses_an_image_outside_a_huge_buffer(lib):
    """src_bytes near INT64_MAX: width * height * 3 and src_offset + bytes must be bounded without being formed."""
    from rpo_amd._lib import E_SHAPE, E_WORKSPACE
    big = dict(width=I32_MAX, height=I32_MAX, crop_w=100, crop_h=100)
    assert 3 * I32_MAX * I32_MAX > I64_MAX                       # the product itself does not fit
    assert run_check(lib, [desc(**big)], src_bytes=I64_MAX) == E_SHAPE
    assert run_check(lib, [desc(src_offset=I64_MAX - 29999)], src_bytes=I64_MAX) == E_SHAPE
    assert run_check(lib, [desc(src_offset=I64_MAX - 30000)], src_bytes=I64_MAX) == 0
    # an INT32_MAX-wide crop that does lie inside its image needs more taps than any kmax: refused, not wrapped
    wide = dict(width=I32_MAX, height=1, crop_w=I32_MAX, crop_h=1, resize_w=1, resize_h=1)
    assert run_check(lib, [desc(**wide)], size=1, src_bytes=I64_MAX, kmax=I32_MAX - 1) == E_WORKSPACE
    assert lib.rpo_preprocess_ksize(I32_MAX, 1) == I32_MAX


def test_check_keeps_the_existing_refusals(lib):
    from rpo_amd._lib import E_BADARG, E_SHAPE, E_WORKSPACE
    shape = [dict(crop_x=50, crop_w=80), dict(crop_y=50, crop_h=80), dict(crop_x=1), dict(crop_y=1),      # crop leaves the image
             dict(crop_x=-1, crop_w=50), dict(crop_y=-1, crop_h=50),
             dict(win_x=8), dict(win_y=8), dict(resize_w=300, win_x=77), dict(resize_h=300, win_y=77),    # window leaves the resize
             dict(win_x=-1, resize_w=300), dict(win_y=-1, resize_h=300),
             dict(resize_w=SIZE - 1), dict(resize_h=SIZE - 1), dict(resize_w=0), dict(resize_h=-5),       # resize < size
             dict(width=0), dict(height=0), dict(width=-100), dict(height=-100), dict(crop_w=0), dict(crop_h=0),
             dict(crop_w=-3), dict(crop_h=-3),
             dict(src_offset=-1), dict(src_offset=1), dict(src_offset=16)]                                # leaves src
    for kw in shape:
        assert run_check(lib, [desc(**kw)]) == E_SHAPE, kw
        assert run_check(lib, [desc(), desc(**kw)]) == E_SHAPE, kw
    assert run_check(lib, [desc()], src_bytes=29999) == E_SHAPE
    assert run_check(lib, [desc()], src_bytes=0) == E_SHAPE
    assert run_check(lib, [desc()], src_bytes=-1) == E_SHAPE
    # workspace: more taps than kmax on either axis, more crop rows than max_rows
    assert lib.rpo_preprocess_ksize(100, SIZE) == 5
    assert run_check(lib, [desc()], kmax=4) == E_WORKSPACE
    tall = dict(width=10, height=1000, crop_w=10, crop_h=1000)   # the vertical 1000 -> 224 alone sets the tap count
    k = lib.rpo_preprocess_ksize(1000, SIZE)
    assert k == R.precompute_coeffs(1000, 0.0, 1000.0, SIZE)[0] > 5 and lib.rpo_preprocess_ksize(10, SIZE) == 5
    assert run_check(lib, [desc(**tall)], max_rows=1000, kmax=k - 1) == E_WORKSPACE
    assert run_check(lib, [desc(**tall)], max_rows=1000, kmax=k) == 0
    assert run_check(lib, [desc(**tall)], max_rows=999, kmax=k) == E_WORKSPACE
    wide = dict(width=1000, height=10, crop_w=1000, crop_h=10)
    assert run_check(lib, [desc(**wide)], kmax=k - 1) == E_WORKSPACE
    assert run_check(lib, [desc()], max_rows=99) == E_WORKSPACE
    assert run_check(lib, [desc(), desc(crop_h=50), desc()], max_rows=99) == E_WORKSPACE
    # arguments
    for kw in (dict(size=0), dict(size=-224), dict(max_rows=0), dict(max_rows=-1), dict(kmax=0), dict(kmax=-7)):
        assert run_check(lib, [desc()], **kw) == E_BADARG, kw
    arr = (type(desc()) * 1)(desc())
    assert lib.rpo_preprocess_check(arr, 0, SIZE, 100, 5, 30000) == E_BADARG
    assert lib.rpo_preprocess_check(arr, -1, SIZE, 100, 5, 30000) == E_BADARG
    assert lib.rpo_preprocess_check(None, 1, SIZE, 100, 5, 30000) == E_BADARG


def test_check_accepts_the_boundaries(lib):
    assert run_check(lib, [desc()]) == 0
    # a crop that touches the right and the bottom edge exactly
    assert run_check(lib, [desc(crop_x=20, crop_w=80, crop_y=35, crop_h=65)]) == 0
    assert run_check(lib, [desc(crop_x=99, crop_w=1, crop_y=99, crop_h=1)], kmax=5) == 0
    # a window that touches the edge of the resized image exactly
    assert run_check(lib, [desc(resize_w=300, win_x=76, resize_h=298, win_y=74)]) == 0
    assert run_check(lib, [desc(resize_w=I32_MAX, win_x=I32_MAX - SIZE, resize_h=I32_MAX, win_y=I32_MAX - SIZE)]) == 0
    # src_offset + bytes == src_bytes
    assert run_check(lib, [desc(src_offset=16)], src_bytes=30016) == 0
    assert run_check(lib, [desc(), desc(src_offset=30000)], src_bytes=60000) == 0
    assert run_check(lib, [desc(src_offset=I64_MAX - 30000)], src_bytes=I64_MAX) == 0
    # kmax exactly what rpo_preprocess_ksize says, max_rows exactly crop_h
    photo = dict(width=500, height=375, crop_x=30, crop_y=20, crop_w=400, crop_h=300)
    kmax = max(lib.rpo_preprocess_ksize(400, SIZE), lib.rpo_preprocess_ksize(300, SIZE))
    assert run_check(lib, [desc(**photo)], max_rows=300, kmax=kmax, src_bytes=500 * 375 * 3) == 0
    assert run_check(lib, [desc(**photo)], max_rows=300, kmax=kmax - 1, src_bytes=500 * 375 * 3) != 0
    assert run_check(lib, [desc(**photo)], max_rows=299, kmax=kmax, src_bytes=500 * 375 * 3) != 0
    # both passes skipped: one tap
    assert run_check(lib, [desc(width=SIZE, height=SIZE, crop_w=SIZE, crop_h=SIZE)], max_rows=SIZE, kmax=1,
                     src_bytes=SIZE * SIZE * 3) == 0
    # size == 1 and the flip / reserved fields are not looked at
    assert run_check(lib, [desc(resize_w=1, resize_h=1, flip=-7)], size=1, kmax=lib.rpo_preprocess_ksize(100, 1)) == 0


KSIZE_IN = (1, 2, 3, 7, 97, 224, 257, 336, 500, 1500, 4000)
KSIZE_OUT = (224, 256, 257, 336, 513)


def test_ksize_equals_the_oracles_tap_count(lib):
    for n_in in KSIZE_IN:
        for n_out in KSIZE_OUT:
            if n_in == n_out:
                continue                                         # Pillow skips the pass: no coefficients exist
            ksize, bounds, _ = R.precompute_coeffs(n_in, 0.0, float(n_in), n_out)
            assert lib.rpo_preprocess_ksize(n_in, n_out) == ksize, (n_in, n_out)
            assert bounds[:, 1].max() <= ksize
    for n in sorted(set(KSIZE_IN) | set(KSIZE_OUT)):
        assert lib.rpo_preprocess_ksize(n, n) == 1
    from rpo_amd._lib import E_BADARG
    assert lib.rpo_preprocess_ksize(0, 224) == E_BADARG and lib.rpo_preprocess_ksize(224, 0) == E_BADARG


def test_center_crop_window_equals_the_oracles():
    from rpo_amd.input_pipeline import center_crop_window
    dims = set(range(1, 601, 7))
    for c in (224, 336, 513):
        dims |= set(range(c - 2, c + 3))
    dims = sorted(dims)
    for size in (224, 257, 336, 513):
        for H in dims:
            for W in dims:
                assert center_crop_window(H, W, size) == R.eval_window(H, W, size), (H, W, size)


class Seq:
    """The scripted generator of tests/test_resample_oracle.py: draws are read off two lists."""
    def __init__(self, u, r): self.u, self.r = list(u), list(r)
    def uniform(self, a, b): return a + (b - a) * self.u.pop(0)
    def randint(self, lo, hi): return lo + int(self.r.pop(0) * (hi - lo))


def test_random_resized_crop_params_equal_the_oracles():
    from rpo_amd.input_pipeline import random_resized_crop_params
    rng = np.random.default_rng(17)
    shapes = [(375, 500), (500, 375), (224, 224), (336, 336), (1, 1), (2, 3), (97, 1024), (1024, 97), (100, 1000),
              (1000, 100)]
    outcomes = set()
    for n in range(200):
        H, W = shapes[n % len(shapes)]
        u, r = rng.random(20), rng.random(2)
        if n % 4 == 3:
            u[0::2] = 1.0 - u[0::2] * 1e-3                        # area fractions at the top of the range
        a, b = Seq(u, r), Seq(u, r)
        got = random_resized_crop_params(H, W, a)
        assert got == R.random_resized_crop_params(H, W, b), (n, H, W)
        assert (a.u, a.r) == (b.u, b.r), "both consume the same draws"
        i, j, h, w = got
        assert 0 < h <= H and 0 < w <= W and 0 <= i <= H - h and 0 <= j <= W - w
        outcomes.add("fallback" if len(a.u) == 0 else ("first try" if len(a.u) == 18 else "retry"))
    assert outcomes == {"fallback", "first try", "retry"}, outcomes


class RecordingLib:
    """Stands in for the loaded library: forwards the pure host entry points, records every call."""
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            assert name in ("rpo_preprocess_ksize", "rpo_preprocess_workspace_bytes"), f"{name} must not be reached"
            return getattr(self.real, name)(*args)
        return call


WRAPS = [("crop_y", dict(crop=(2 ** 32 + 5, 0, 10, 10))), ("crop_x", dict(crop=(0, 2 ** 32 + 5, 10, 10))),
         ("crop_h", dict(crop=(0, 0, 2 ** 32 + 10, 10))), ("crop_w", dict(crop=(0, 0, 10, 2 ** 32 + 10))),
         ("resize_w", dict(resize=(2 ** 32 + SIZE, SIZE))), ("resize_h", dict(resize=(SIZE, 2 ** 31))),
         ("win_x", dict(window=(2 ** 32, 0))), ("win_y", dict(window=(0, -2 ** 31 - 1)))]


@pytest.mark.parametrize("field,kw", WRAPS, ids=[w[0] for w in WRAPS])
def test_plan_numbers_that_do_not_fit_int32_raise_instead_of_wrapping(lib, field, kw):
    """ctypes stores 2**32 + 5 into a c_int32 field as 5: the wrapped plan is a VALID crop of another place.  Both
    entry points refuse it by name before a staging slot, a device buffer or the library is touched."""
    from rpo_amd.input_pipeline import DeviceTransform, InputConfig, SamplePlan
    tf = DeviceTransform(InputConfig(), True, "cpu", max_batch=2, max_image_bytes=1 << 16)
    tf.lib = rec = RecordingLib(lib)
    slots = tf.slots
    tf.slots = None                                              # any use of a staging slot fails loudly
    img = np.zeros((100, 100, 3), np.uint8)
    good = SamplePlan((0, 0, 100, 100), (SIZE, SIZE), (0, 0), False)
    plan = dict(crop=(0, 0, 10, 10), resize=(SIZE, SIZE), window=(0, 0), flip=False)
    plan.update(kw)
    with pytest.raises(ValueError, match=rf"image 1: {field} = "):
        tf([img, img], [good, SamplePlan(**plan)])
    assert "rpo_preprocess_batch" not in rec.calls and tf.turn == 0

    class Set:                                                   # a DeviceImageSet as far as from_set looks before it plans
        dev = tf.dev
        sizes = [(100, 100), (100, 100)]

        def stage_spilled(self, *a):
            raise AssertionError("the set's buffer must not be touched")
    with pytest.raises(ValueError, match=rf"image 1: {field} = "):
        tf.from_set(Set(), [0, 1], [good, SamplePlan(**plan)])
    assert "rpo_preprocess_batch" not in rec.calls and getattr(tf, "dslots", None) is None
    tf.slots = slots


def test_an_image_size_that_does_not_fit_int32_raises(lib):
    from rpo_amd.input_pipeline import DeviceTransform, InputConfig, SamplePlan
    tf = DeviceTransform(InputConfig(), True, "cpu", max_batch=1, max_image_bytes=1 << 16)
    tf.lib = rec = RecordingLib(lib)

    class Set:
        dev = tf.dev
        sizes = [(3, 2 ** 32 + 100)]

        def stage_spilled(self, *a):
            raise AssertionError("the set's buffer must not be touched")
    with pytest.raises(ValueError, match="image 0: width = "):
        tf.from_set(Set(), [0], [SamplePlan((0, 0, 3, 100), (SIZE, SIZE), (0, 0), False)])
    Set.sizes = [(2 ** 31, 100)]
    with pytest.raises(ValueError, match="image 0: height = "):
        tf.from_set(Set(), [0], [SamplePlan((0, 0, 3, 100), (SIZE, SIZE), (0, 0), False)])
    assert rec.calls == []


# ---- the oracle against Pillow at the sizes and geometries of tests/test_gpu_preprocess_sizes.py ----------------------

def pil_resize(Image, img, ow, oh):
    return Image.fromarray(img).resize((ow, oh), Image.BICUBIC)


@pytest.mark.parametrize("S", PC.TRAIN_SIZES)
def test_oracle_matches_pillow_on_the_train_geometries(S):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(100 + S)
    for name, hw, (top, left, h, w) in PC.train_cases(S):
        img = PC.random_image(rng, hw)
        ref = np.asarray(Image.fromarray(img).crop((left, top, left + w, top + h)).resize((S, S), Image.BICUBIC))
        got = R.resize_bicubic(np.ascontiguousarray(img[top:top + h, left:left + w]), S, S)
        assert np.array_equal(got, ref), (S, name)


@pytest.mark.parametrize("S", PC.EVAL_SIZES)
def test_oracle_matches_pillow_on_the_eval_geometries(S):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(200 + S)
    for hw in PC.eval_sizes(S):
        img = PC.random_image(rng, hw)
        ow, oh, left, top = R.eval_window(hw[0], hw[1], S)
        ref = np.asarray(pil_resize(Image, img, ow, oh).crop((left, top, left + S, top + S)))
        assert np.array_equal(R.resize_bicubic(img, ow, oh, (left, top, S, S)), ref), (S, hw)
        assert np.array_equal(R.eval_transform(img, S), R.to_tensor_normalize(ref)), (S, hw)


@pytest.mark.parametrize("S", PC.SATURATION_SIZES + (513,))
def test_oracle_matches_pillow_on_saturated_inputs(S):
    Image = pytest.importorskip("PIL.Image")
    for name, img in PC.saturation_images(np.random.default_rng(300)):
        ref = np.asarray(pil_resize(Image, img, S, S))
        assert np.array_equal(R.resize_bicubic(img, S, S), ref), (S, name)


@pytest.mark.parametrize("S", PC.SATURATION_SIZES)
def test_saturated_noise_clips_in_both_passes(S):
    """What makes the 0/255 inputs a check of the saturating arithmetic: on the reference alone, at least 1 % of the
    pre-clip values of each pass fall below 0 and at least 1 % above 255."""
    name, img = PC.saturation_images(np.random.default_rng(300))[0]
    fr = PC.clip_fractions(img, S)
    print(f"S = {S}, {name}: pre-clip < 0 / > 255: horizontal {fr[0]:.3f} / {fr[1]:.3f}, vertical {fr[2]:.3f} / {fr[3]:.3f}")
    assert min(fr) >= 0.01, fr
