"""Progressive JPEG files decoded on the device (rpo_jpeg_prog_decode_batch through rpo_amd/jpeg.py with progressive=True)
against tests/golden/jpeg_progressive.npz: Pillow's recorded pixels bit for bit, in any batch and order, mixed with baseline
files, guard bytes around every destination; corrupt streams end in their exact status; `DeviceImageSet.from_jpeg(...,
progressive=True)` builds the set `DeviceImageSet(decoded)` builds.  Every stream here ran through the decoder's own code on
the CPU first (tests/test_jpeg_progressive_host.py; with the host sanitizers)."""
import functools
import os

import numpy as np
import pytest
import torch

import jpeg_prog_writer as PW
from test_gpu_jpeg import _set_equal, guarded_decode
from test_gpu_loop import DEV, _make

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def fixtures():
    return PW.load_progressive(os.path.join(GOLD, "jpeg_progressive.npz"))


def streams():
    return fixtures()[0]


def small():
    return [s for s in streams() if s["rgb"].shape[0] * s["rgb"].shape[1] <= 2048]


def decoder(chunk_images=4096):
    from rpo_amd.jpeg import JpegDecoder
    return JpegDecoder(DEV, chunk_images=chunk_images, progressive=True)


def test_every_stream_in_one_call_equals_pillow_and_again_in_chunks_of_7():
    cs = streams()
    assert len(cs) >= 390
    files, shapes = [c["file"] for c in cs], [c["rgb"].shape[:2] for c in cs]
    st, first = guarded_decode(decoder(), files, shapes)
    assert st.shape == (len(cs),) and not st.any(), [cs[k]["tag"] for k in np.flatnonzero(st)][:5]
    for c, im in zip(cs, first):
        assert np.array_equal(im, c["rgb"]), (c["tag"], int((im != c["rgb"]).any(-1).sum()))
    order = list(np.random.default_rng(3).permutation(len(cs)))
    st, second = guarded_decode(decoder(7), [files[j] for j in order], [shapes[j] for j in order], guard=5)
    assert not st.any()
    for j, im in zip(order, second):
        assert np.array_equal(im, first[j]), cs[j]["tag"]


def test_each_progressive_file_equals_its_baseline_twin_in_one_mixed_batch():
    """the twin goes through rpo_jpeg_decode_batch, the existing path, in the same chunk"""
    from rpo_amd.jpeg import probe
    cs = [c for c in streams() if c["twin"] is not None]
    assert len(cs) >= 80
    files, shapes = [], []
    for c in cs:
        files += [c["file"], c["twin"]]
        shapes += [c["rgb"].shape[:2]] * 2
        assert probe(c["twin"], progressive=True).reserved == 0 and probe(c["file"], progressive=True).reserved > 0
    st, imgs = guarded_decode(decoder(), files, shapes)
    assert not st.any()
    for k, c in enumerate(cs):
        assert np.array_equal(imgs[2 * k], imgs[2 * k + 1]) and np.array_equal(imgs[2 * k], c["rgb"]), c["tag"]


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_mixed_batches_alternating_baseline_and_progressive(n):
    """n files in one chunk, baseline and progressive alternating (so both library calls write into the same buffer, between
    each other's destinations, at odd offsets); the same bits when decoded again and in another composition"""
    tw = [c for c in streams() if c["twin"] is not None]
    sm = small()
    rng = np.random.default_rng(n)
    files, want = [], []
    for k in range(n):
        if k % 2 == 0:
            c = sm[int(rng.integers(0, len(sm)))]
            files.append(c["file"])
        else:
            c = tw[int(rng.integers(0, len(tw)))]
            files.append(c["twin"])
        want.append(c["rgb"])
    shapes = [w.shape[:2] for w in want]
    dec = decoder()
    st, first = guarded_decode(dec, files, shapes)
    assert st.shape == (n,) and not st.any()
    for k, (im, w) in enumerate(zip(first, want)):
        assert np.array_equal(im, w), k
    st, second = guarded_decode(dec, files, shapes)
    assert not st.any() and all(np.array_equal(a, b) for a, b in zip(first, second))
    order = list(rng.permutation(n))[:max(1, n // 2)]
    st, third = guarded_decode(decoder(7), [files[j] for j in order], [shapes[j] for j in order], guard=5)
    assert not st.any() and all(np.array_equal(first[j], im) for j, im in zip(order, third))


def test_the_32768_block_file_alone_and_among_299_small_ones():
    """An EOB run of 32767 blocks and then one of 1 inside a single unit; alone the call has 6 units."""
    from rpo_amd.jpeg import probe
    flat = next(c for c in streams() if "EOBRUN 32767" in c["tag"])
    info = probe(flat["file"], progressive=True)
    assert info.coef_bytes == 32768 * 128 and info.units == 6 and info.reserved == 3
    dec = decoder()
    st, (alone,) = guarded_decode(dec, [flat["file"]], [flat["rgb"].shape[:2]])
    assert not st.any() and np.array_equal(alone, flat["rgb"])
    sm = small()
    pick = [sm[j] for j in np.random.default_rng(4).integers(0, len(sm), 299)]
    mixed = pick[:150] + [flat] + pick[150:]
    st, imgs = guarded_decode(dec, [c["file"] for c in mixed], [c["rgb"].shape[:2] for c in mixed])
    assert not st.any() and np.array_equal(imgs[150], alone)
    for c, im in zip(mixed, imgs):
        assert np.array_equal(im, c["rgb"]), c["tag"]


def test_more_than_4096_units_take_the_lanes_per_wave_path():
    """Files with restart intervals of one block: > 4096 units in one call, several units per wave, tables read from global
    memory; the same bits."""
    from rpo_amd.jpeg import probe
    rst = [c for c in streams() if "restart_marker_blocks 1" in c["tag"] or "DRI changed" in c["tag"]]
    assert len(rst) >= 12
    pick = [rst[j % len(rst)] for j in range(400)] + small()[:40]
    assert sum(probe(c["file"], progressive=True).units for c in pick) > 2 * 4096
    st, imgs = guarded_decode(decoder(), [c["file"] for c in pick], [c["rgb"].shape[:2] for c in pick])
    assert not st.any()
    for c, im in zip(pick, imgs):
        assert np.array_equal(im, c["rgb"]), c["tag"]


def test_corrupt_streams_end_in_their_exact_status_between_exact_neighbours():
    """Only streams the sanitized host program ran clean; the kernels' bounds come from the header and the
    plan, so these are ordinary work for them."""
    from rpo_amd.jpeg import JpegCorrupt
    good = [c for c in streams() if c["rgb"].shape[0] == 33 and c["tag"].startswith("pillow")][:6]
    assert len(good) == 6
    corrupt = PW.corrupt_streams()
    assert [s for _, _, s in corrupt][:4] == [1, 2, 3, 4] and len(corrupt) == 5
    files, want, shapes = [good[0]["file"]], [0], [good[0]["rgb"].shape[:2]]
    for k, (_, data, status) in enumerate(corrupt):
        files += [data, good[k + 1]["file"]]
        want += [status, 0]
        shapes += [(32, 32), good[k + 1]["rgb"].shape[:2]]
    dec = decoder()
    st, imgs = guarded_decode(dec, files, shapes)
    print("device status:", st.tolist())
    assert st.tolist() == want
    for k, c in enumerate(good):
        assert np.array_equal(imgs[2 * k], c["rgb"]), c["tag"]
    st2, imgs2 = guarded_decode(dec, files, shapes)
    assert np.array_equal(st, st2) and all(np.array_equal(a, b) for a, b in zip(imgs, imgs2))
    with pytest.raises(JpegCorrupt) as e:
        dec.decode(files)
    assert e.value.index == 1 and e.value.status == want[1]


def test_from_jpeg_progressive_builds_the_set_the_decoded_images_build():
    from rpo_amd import _lib
    from rpo_amd.input_pipeline import DeviceImageSet
    cs, refused = fixtures()
    stand_in = np.random.default_rng(2).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    files, images = [], []
    for k, c in enumerate(cs):
        files.append(c["file"])
        images.append(c["rgb"])
        if k % 40 == 0 and k // 40 < len(refused):
            files.append(refused[k // 40]["file"])
            images.append(stand_in)
    # a baseline file is "refused" only by rpo_jpeg_prog_probe itself: from_jpeg decodes it through the existing path
    sequential = [r for r in refused if r["code"] == _lib.E_JPEG_SEQUENTIAL]
    assert len(sequential) == 1 and len(files) == len(cs) + len(refused)
    images[files.index(sequential[0]["file"])] = next(c["rgb"] for c in cs if c["tag"] == "writer 420: chroma before luma")
    n_refused = len(refused) - 1
    seen = []

    def fallback(data):
        seen.append(data)
        return stand_in
    labels = [i % 19 for i in range(len(files))]
    ds = DeviceImageSet.from_jpeg(files, labels, DEV, fallback=fallback, progressive=True)
    assert (ds.n_device, ds.n_fallback) == (len(files) - n_refused, n_refused)
    assert seen == [r["file"] for r in refused if r["code"] != _lib.E_JPEG_SEQUENTIAL]
    ref = DeviceImageSet(images, labels, DEV)
    _set_equal(ref, ds, images)
    budget = sum((im.size + 15) // 16 * 16 for im in images[:200])
    part = DeviceImageSet.from_jpeg(files, labels, DEV, budget_bytes=budget, max_batch=8, chunk_images=50, fallback=fallback,
                                    progressive=True)
    assert part.plan.spilled and part.n_fallback == n_refused
    _set_equal(DeviceImageSet(images, labels, DEV, budget_bytes=budget, max_batch=8), part, images)
    # one evaluation pass over either set
    tr = _make("coop", "f16", True, 32, 2)
    a, b = tr.test(ref, batch_size=32), tr.test(ds, batch_size=32)
    assert (a["total"], a["correct"], a["accuracy"]) == (b["total"], b["correct"], b["accuracy"]) and a["total"] == len(files)
    assert np.array_equal(a["confusion_matrix"], b["confusion_matrix"])


def test_from_jpeg_default_and_one_pillow_file_under_the_flag():
    """The flag decides: off (the default) a progressive file is the fallback's, on it is the device's."""
    from rpo_amd.input_pipeline import DeviceImageSet
    c = next(s for s in streams() if s["tag"].startswith("pillow 33x24 420"))
    seen = []

    def fallback(data):
        seen.append(data)
        return c["rgb"]
    off = DeviceImageSet.from_jpeg([c["file"]] * 3, [0, 1, 2], DEV, fallback=fallback)
    assert (off.n_device, off.n_fallback) == (0, 3) and len(seen) == 3
    on = DeviceImageSet.from_jpeg([c["file"]] * 3, [0, 1, 2], DEV, fallback=fallback, progressive=True)
    assert on.n_fallback == 0 and on.n_device == 3 and len(seen) == 3
    _set_equal(off, on, [c["rgb"]] * 3)
