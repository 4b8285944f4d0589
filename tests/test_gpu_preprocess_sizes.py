"""The on-device input transforms at output sizes beyond one pass of a block's 256 threads (256, 257, 336, 513), against
the Pillow-pinned oracle, bit for bit: every loop `for (o = threadIdx.x; o < S; o += 256)` of preprocess.hip takes a second
and a third pass, and the `size`-strided workspace offsets are no longer those of S = 224.  The oracle is pinned against
Pillow at exactly these sizes and geometries by tests/test_preprocess_host.py."""
import ctypes

import numpy as np
import pytest
import torch

import preprocess_cases as PC
from oracle import resample_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make(S, is_train=True, max_batch=8, **cfg):
    from rpo_amd.input_pipeline import InputConfig, build_transform
    return build_transform(InputConfig(SIZE=(S, S), **cfg), is_train, DEV, max_batch)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def train_plan(box, flip, S):
    from rpo_amd.input_pipeline import SamplePlan
    return SamplePlan(tuple(box), (S, S), (0, 0), bool(flip))


@pytest.mark.parametrize("S", PC.TRAIN_SIZES)
def test_train_plans_bit_exact(S):
    rng = np.random.default_rng(100 + S)
    cases = PC.train_cases(S)
    imgs = [PC.random_image(rng, hw) for _, hw, _ in cases]
    flips = [b % 2 == 1 for b in range(len(cases))]
    got = make(S)(imgs, [train_plan(box, f, S) for (_, _, box), f in zip(cases, flips)]).cpu().numpy()
    assert got.shape == (len(cases), 3, S, S)
    for b, (name, _, box) in enumerate(cases):
        assert same(got[b], R.train_transform(imgs[b], box, flips[b], S)), (S, name)


@pytest.mark.parametrize("S", PC.EVAL_SIZES)
def test_eval_transform_bit_exact(S):
    rng = np.random.default_rng(200 + S)
    sizes = PC.eval_sizes(S)
    imgs = [PC.random_image(rng, hw) for hw in sizes]
    got = make(S, is_train=False)(imgs).cpu().numpy()
    for b, im in enumerate(imgs):
        assert same(got[b], R.eval_transform(im, S)), (S, sizes[b])


@pytest.mark.parametrize("S", PC.SATURATION_SIZES)
def test_saturated_inputs_bit_exact(S):
    """0/255 inputs: the bicubic lobes overshoot, and Pillow clips to uint8 after the horizontal pass and again after the
    vertical pass.  That the inputs do saturate both passes is asserted on the reference alone."""
    cases = PC.saturation_images(np.random.default_rng(300))
    fr = PC.clip_fractions(cases[0][1], S)
    print(f"S = {S}: pre-clip < 0 / > 255: horizontal {fr[0]:.3f} / {fr[1]:.3f}, vertical {fr[2]:.3f} / {fr[3]:.3f}")
    assert min(fr) >= 0.01, fr
    imgs = [im for _, im in cases]
    got = make(S)(imgs, [train_plan((0, 0, im.shape[0], im.shape[1]), False, S) for im in imgs]).cpu().numpy()
    for b, (name, im) in enumerate(cases):
        assert same(got[b], R.train_transform(im, (0, 0, im.shape[0], im.shape[1]), False, S)), (S, name)


def test_workspace_layout_exact_size_between_guards():
    """The C ABI directly at S = 257, B = 3: image 0 alone sets kmax, image 1 alone sets max_rows, the workspace is exactly
    what rpo_preprocess_workspace_bytes says, inside guard bytes, and `out` lies between NaN slabs.  A second call on the
    uncleared workspace with another layout (reverse order, fewer taps) must not see the first call's coefficients."""
    from rpo_amd import _lib
    lib = _lib.load()
    S, B, GUARD = 257, 3, 4096
    rng = np.random.default_rng(41)
    imgs = [PC.random_image(rng, hw) for hw in ((10, 1506), (903, 33), (5, 5))]
    mean, std = (ctypes.c_float * 3)(*R.CLIP_MEAN), (ctypes.c_float * 3)(*R.CLIP_STD)
    offs = np.cumsum([0] + [(im.size + 15) // 16 * 16 for im in imgs])
    packed = np.zeros(int(offs[-1]), np.uint8)
    for im, o in zip(imgs, offs):
        packed[o:o + im.size] = im.reshape(-1)
    src = torch.from_numpy(packed).to(DEV)

    def run(order, boxes, flips, ws, ws_bytes, max_rows, kmax):
        descs = (_lib.ImageDesc * B)()
        for d, i, (top, left, h, w), f in zip(descs, order, boxes, flips):
            d.src_offset, d.height, d.width = int(offs[i]), imgs[i].shape[0], imgs[i].shape[1]
            d.crop_x, d.crop_y, d.crop_w, d.crop_h = left, top, w, h
            d.resize_w = d.resize_h = S
            d.flip = int(f)
        assert lib.rpo_preprocess_check(descs, B, S, max_rows, kmax, src.numel()) == 0
        desc_dev = torch.from_numpy(np.frombuffer(bytes(descs), np.uint8).copy()).to(DEV)
        full = torch.full((B + 2, 3, S, S), float("nan"), device=DEV)
        _lib.check(lib.rpo_preprocess_batch(src.data_ptr(), src.numel(), ctypes.addressof(descs), desc_dev.data_ptr(), B, S,
                                            max_rows, kmax, ctypes.addressof(mean), ctypes.addressof(std),
                                            full[1].data_ptr(), ws, ws_bytes,
                                            torch.cuda.current_stream().cuda_stream), "rpo_preprocess_batch")
        torch.cuda.synchronize()
        assert torch.isnan(full[0]).all() and torch.isnan(full[-1]).all(), "an out guard slab was written"
        got = full[1:-1].cpu().numpy()
        for b, (i, box, f) in enumerate(zip(order, boxes, flips)):
            assert same(got[b], R.train_transform(imgs[i], box, f, S)), (order, b)

    boxes = [(1, 3, 8, 1500), (2, 1, 900, 30), (0, 0, 5, 5)]
    ksz = [[lib.rpo_preprocess_ksize(w, S), lib.rpo_preprocess_ksize(h, S)] for (_, _, h, w) in boxes]
    kmax, max_rows = max(max(k) for k in ksz), max(h for (_, _, h, _) in boxes)
    assert max(ksz[0]) == kmax > max(max(k) for k in ksz[1:]), "image 0 alone sets kmax"
    assert boxes[1][2] == max_rows > max(boxes[0][2], boxes[2][2]), "image 1 alone sets max_rows"
    need = lib.rpo_preprocess_workspace_bytes(B, S, max_rows, kmax)
    buf = torch.full((need + 2 * GUARD + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    lo = GUARD + (-(buf.data_ptr() + GUARD)) % 16
    assert (buf.data_ptr() + lo) % 16 == 0 and lo >= GUARD and buf.numel() - (lo + need) >= GUARD

    def guards_intact():
        return bool((buf[:lo] == 0xA5).all()) and bool((buf[lo + need:] == 0xA5).all())

    run([0, 1, 2], boxes, [False, True, False], buf.data_ptr() + lo, need, max_rows, kmax)
    assert guards_intact(), "a workspace guard was written"
    assert bool((buf[lo:lo + need] != 0xA5).any())
    # the same workspace, uncleared: reverse order, image 0 cropped to 600 columns so that image 1's rows set kmax
    boxes2 = [boxes[2], boxes[1], (1, 3, 8, 600)]
    kmax2 = max(lib.rpo_preprocess_ksize(s, S) for (_, _, h, w) in boxes2 for s in (h, w))
    assert kmax2 < kmax and lib.rpo_preprocess_workspace_bytes(B, S, max_rows, kmax2) < need
    run([2, 1, 0], boxes2, [True, False, True], buf.data_ptr() + lo, need, max_rows, kmax2)
    assert guards_intact(), "a workspace guard was written"


def test_resident_set_against_the_oracle_at_336():
    """`from_set` at the shipped 336 px against the oracle (not against the staging transform, which runs the same
    kernels): 5 ragged images, a budget that spills two of them."""
    from rpo_amd.input_pipeline import DeviceImageSet
    S = 336
    rng = np.random.default_rng(51)
    sizes = [(375, 500), (60, 40), (S, S + 7), (500, 333), (341, 337)]
    imgs = [PC.random_image(rng, hw) for hw in sizes]
    budget = sum((im.size + 15) // 16 * 16 for im in (imgs[0], imgs[1], imgs[2])) + 64
    ds = DeviceImageSet(imgs, list(range(5)), DEV, budget_bytes=budget, max_batch=8)
    assert ds.plan.spilled == [3, 4]
    boxes = [(20, 30, 300, 400), (0, 0, 60, 40), (0, 3, S, S), (100, 33, 400, 300), (5, 1, S, S - 19)]
    order = [4, 0, 3, 1, 2]
    tf = make(S)
    plans = [train_plan(boxes[i], b % 2 == 0, S) for b, i in enumerate(order)]
    got = tf.from_set(ds, order, plans).cpu().numpy()
    for b, i in enumerate(order):
        assert same(got[b], R.train_transform(imgs[i], boxes[i], b % 2 == 0, S)), ("train", i)
    got = make(S, is_train=False).from_set(ds, order).cpu().numpy()
    for b, i in enumerate(order):
        assert same(got[b], R.eval_transform(imgs[i], S)), ("eval", i)


def test_other_normalisation_constants_bit_exact():
    """ImageNet's mean / std instead of CLIP's, S = 257: a channel or constant mix-up that CLIP's nearly equal values
    could mask."""
    S = 257
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    rng = np.random.default_rng(61)
    cases = PC.train_cases(S)[:3]
    imgs = [PC.random_image(rng, hw) for _, hw, _ in cases]
    imgs[1][..., 0], imgs[1][..., 2] = 255, 0                    # channels that differ by far more than the constants do
    tf = make(S, PIXEL_MEAN=mean, PIXEL_STD=std)
    got = tf(imgs, [train_plan(box, b == 2, S) for b, (_, _, box) in enumerate(cases)]).cpu().numpy()
    for b, (name, _, (top, left, h, w)) in enumerate(cases):
        px = R.resize_bicubic(np.ascontiguousarray(imgs[b][top:top + h, left:left + w]), S, S)
        want = R.to_tensor_normalize(px[:, ::-1] if b == 2 else px, mean, std)
        assert same(got[b], want), name
        assert not same(got[b], R.to_tensor_normalize(px[:, ::-1] if b == 2 else px)), "CLIP's constants differ"
