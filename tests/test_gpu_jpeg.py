"""On-device JPEG decode (rpo_jpeg_decode_batch through rpo_amd/jpeg.py) against the Pillow fixtures and the numpy oracle
(tests/jpeg_oracle.py): bit for bit, in any batch, with guard bytes around every destination; corrupt streams end in a
per-image status; `DeviceImageSet.from_jpeg` builds the set `DeviceImageSet(decoded)` builds."""
import functools
import os

import numpy as np
import pytest
import torch

import jpeg_oracle as J
import jpeg_writer as JW
from test_gpu_loop import DEV, _make, _staging, _state, bits

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 0xA5


@functools.lru_cache(maxsize=None)
def fixtures():
    out = []
    for name in ("jpeg_small.npz", "jpeg_photo.npz"):
        g = np.load(os.path.join(GOLD, name))
        out += [(g[f"file{i}"].tobytes(), g[f"rgb{i}"]) for i in range(int(g["n"]))]
    return out


@functools.lru_cache(maxsize=None)
def metas():
    """(components, h_samp, v_samp, restart interval) per fixture, in the order of fixtures()"""
    out = []
    for name in ("jpeg_small.npz", "jpeg_photo.npz"):
        g = np.load(os.path.join(GOLD, name))
        out += [tuple(int(v) for v in g[f"meta{i}"]) for i in range(int(g["n"]))]
    return out


@functools.lru_cache(maxsize=None)
def streams():
    """tests/golden/jpeg_streams.npz: streams Pillow's encoder never writes (tests/jpeg_writer.py), `rgb` = Pillow's decode"""
    return JW.load_streams(os.path.join(GOLD, "jpeg_streams.npz"))


def in_gamut():
    return [c for c in streams() if c["gamut"] and not c["refused"]]


def refused_file(kind):
    return np.load(os.path.join(GOLD, "jpeg_refused.npz"))[kind].tobytes()


def guarded_decode(dec, files, shapes, guard=48):
    """Decodes into a sentinel-filled buffer with `guard` bytes before, between and behind the destinations (odd offsets:
    nothing in the decoder may rely on an aligned destination); -> (status, images), after checking every guard byte."""
    offsets, off = [], guard + 1
    for (H, W) in shapes:
        offsets.append(off)
        off += H * W * 3 + guard
    buf = torch.full((off,), SENTINEL, dtype=torch.uint8, device=DEV)
    st = dec.decode_into(files, buf, offsets, raise_corrupt=False)
    flat = buf.cpu().numpy()
    mask = np.ones(off, bool)
    imgs = []
    for o, (H, W) in zip(offsets, shapes):
        mask[o:o + H * W * 3] = False
        imgs.append(flat[o:o + H * W * 3].reshape(H, W, 3))
    assert (flat[mask] == SENTINEL).all(), "a byte outside the images' own H*W*3 was written"
    return st, imgs


def test_every_fixture_equals_pillow_and_the_oracle():
    from rpo_amd.jpeg import JpegDecoder
    dec = JpegDecoder(DEV)
    for i, (data, rgb) in enumerate(fixtures()):
        buf, offs, sizes = dec.decode([data])
        assert sizes == [rgb.shape[:2]] and offs == [0]
        got = buf.cpu().numpy()[:rgb.size].reshape(rgb.shape)
        assert np.array_equal(got, rgb), (i, rgb.shape, int(np.abs(got.astype(int) - rgb).max()))
        if rgb.shape[0] <= 100:                                   # the pure-Python oracle: small images only
            assert np.array_equal(got, J.decode(data)), i
    # all of them in one call, every destination guarded
    files = [f for f, _ in fixtures()]
    st, imgs = guarded_decode(dec, files, [r.shape[:2] for _, r in fixtures()])
    assert not st.any()
    for i, (im, (_, rgb)) in enumerate(zip(imgs, fixtures())):
        assert np.array_equal(im, rgb), i


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_mixed_batches_one_call_deterministic_and_composition_independent(n):
    """n images of mixed modes and sizes in ONE rpo_jpeg_decode_batch call; the same bits on a second run, and the same
    bits when the images sit in another batch (other order, other neighbours, other unit-per-lane geometry)."""
    from rpo_amd.jpeg import JpegDecoder
    fx = fixtures()
    small = [k for k, (_, r) in enumerate(fx) if r.shape[0] <= 100]
    rng = np.random.default_rng(n)
    pick = [len(fx) - 1] + [small[j] for j in rng.integers(0, len(small), n - 1)] if n > 1 else [small[14]]
    pick = list(rng.permutation(pick))
    dec = JpegDecoder(DEV, chunk_images=4096)
    files, shapes = [fx[k][0] for k in pick], [fx[k][1].shape[:2] for k in pick]
    st, first = guarded_decode(dec, files, shapes)
    assert st.shape == (n,) and not st.any()
    for k, im in zip(pick, first):
        assert np.array_equal(im, fx[k][1]), k
    st, second = guarded_decode(dec, files, shapes)
    assert not st.any() and all(np.array_equal(a, b) for a, b in zip(first, second))
    order = list(rng.permutation(n))[:max(1, n // 2)]               # another composition: half of them, shuffled
    st, third = guarded_decode(JpegDecoder(DEV, chunk_images=7), [files[j] for j in order], [shapes[j] for j in order], guard=5)
    assert not st.any() and all(np.array_equal(first[j], im) for j, im in zip(order, third))


def test_many_restart_intervals_take_the_units_per_wave_path():
    """Up to 4096 units run one per wave with the tables in LDS; beyond that several units share a wave and read the tables
    from global memory.  300 files with short restart intervals are > 4096 units in one call: same bits."""
    from rpo_amd.jpeg import JpegDecoder, probe
    fx = fixtures()
    rst = [k for k in range(len(fx)) if metas()[k][3] > 0 and fx[k][1].shape[0] >= 75]
    pick = [rst[j % len(rst)] for j in range(296)] + [len(fx) - 1, 0, 3, 8]
    files, shapes = [fx[k][0] for k in pick], [fx[k][1].shape[:2] for k in pick]
    assert sum(probe(f).units for f in files) > 2 * 4096
    st, imgs = guarded_decode(JpegDecoder(DEV, chunk_images=4096), files, shapes)
    assert not st.any()
    for k, im in zip(pick, imgs):
        assert np.array_equal(im, fx[k][1]), k


def test_corrupt_streams_end_in_a_status_and_leave_the_others_exact():
    """Error reporting only: the kernels' bounds come from the header, so these inputs are ordinary work for them."""
    from rpo_amd.jpeg import JpegCorrupt, JpegDecoder
    fx = fixtures()
    good = [k for k, (_, r) in enumerate(fx) if r.shape[:2] == (75, 100)]
    victim = fx[next(k for k in good if metas()[k] == (3, 2, 2, 0))][0]   # 4:2:0 without restart markers
    victim_rst = fx[next(k for k in good if metas()[k] == (3, 2, 2, 1))][0]
    hdr, hdr_rst = J.parse(victim).scan_offset, J.parse(victim_rst).scan_offset
    assert J.parse(victim_rst).restart_interval == 1
    truncated = victim[:hdr + (len(victim) - hdr) // 2]
    noise = victim[:hdr] + np.random.default_rng(9).integers(0, 256, len(victim) - hdr, dtype=np.uint8).tobytes()
    no_rst = victim_rst[:hdr_rst + (len(victim_rst) - hdr_rst) // 2]    # the later restart intervals are gone
    files = [fx[good[0]][0], truncated, fx[good[2]][0], noise, no_rst, fx[-1][0]]
    shapes = [(75, 100)] * 5 + [fx[-1][1].shape[:2]]
    dec = JpegDecoder(DEV)
    st, imgs = guarded_decode(dec, files, shapes)
    print("device status:", st.tolist())
    assert st[0] == 0 and st[2] == 0 and st[5] == 0
    assert st[1] != 0 and st[3] != 0 and st[4] != 0
    assert np.array_equal(imgs[0], fx[good[0]][1]) and np.array_equal(imgs[2], fx[good[2]][1]) and np.array_equal(imgs[5], fx[-1][1])
    st2, imgs2 = guarded_decode(dec, files, shapes)                       # deterministic, corrupt ones included
    assert np.array_equal(st, st2) and all(np.array_equal(a, b) for a, b in zip(imgs, imgs2))
    with pytest.raises(JpegCorrupt) as e:
        dec.decode(files)
    assert e.value.index == 1 and e.value.status == st[1]


def _set_equal(a, b, images):
    assert a.sizes == b.sizes and a.labels == b.labels and a.plan == b.plan
    assert a.buffer.numel() == b.buffer.numel() and torch.equal(a.labels_dev, b.labels_dev)
    fa, fb = a.buffer.cpu().numpy(), b.buffer.cpu().numpy()
    for i, (off, im) in enumerate(zip(a.plan.offsets, images)):
        if off >= 0:
            assert np.array_equal(fa[off:off + im.size], im.reshape(-1)), i
            assert np.array_equal(fb[off:off + im.size], im.reshape(-1)), i
        else:
            assert np.array_equal(a.host_images[i], im) and np.array_equal(b.host_images[i], im), i
            assert b.host_images[i].flags.c_contiguous and b.host_images[i].dtype == np.uint8
    assert sorted(a.host_images) == sorted(b.host_images) == a.plan.spilled


def test_from_jpeg_builds_the_set_the_decoded_images_build(tmp_path):
    from rpo_amd.input_pipeline import DeviceImageSet
    fx = fixtures()
    files, images = [f for f, _ in fx], [r for _, r in fx]
    labels = list(range(len(fx)))
    full = DeviceImageSet.from_jpeg(files, labels, DEV)
    assert (full.n_device, full.n_fallback) == (len(fx), 0), "a decoder that refuses the supported fixtures passes nothing"
    _set_equal(DeviceImageSet(images, labels, DEV), full, images)
    budget = sum((im.size + 15) // 16 * 16 for im in images[:14]) + 5000
    part = DeviceImageSet.from_jpeg(files, labels, DEV, budget_bytes=budget, max_batch=8, chunk_images=3)
    assert part.plan.spilled and len(part.plan.spilled) < len(fx) and part.n_fallback == 0
    _set_equal(DeviceImageSet(images, labels, DEV, budget_bytes=budget, max_batch=8), part, images)
    none = DeviceImageSet.from_jpeg(files, labels, DEV, budget_bytes=0)
    _set_equal(DeviceImageSet(images, labels, DEV, budget_bytes=0), none, images)
    # paths instead of bytes
    paths = []
    for i, f in enumerate(files[:5]):
        paths.append(str(tmp_path / f"{i}.jpg"))
        open(paths[-1], "wb").write(f)
    _set_equal(DeviceImageSet(images[:5], labels[:5], DEV), DeviceImageSet.from_jpeg(paths, labels[:5], DEV), images[:5])
    # a refused file goes through `fallback`, resident or spilled
    stand_in = np.random.default_rng(1).integers(0, 256, (24, 32, 3), dtype=np.uint8)
    seen = []

    def fallback(data):
        seen.append(data)
        return stand_in
    prog = refused_file("progressive")
    mixed_files, mixed_images = files[:6] + [prog] + files[6:9], images[:6] + [stand_in] + images[6:9]
    for bud in (None, 0):
        seen.clear()
        ds = DeviceImageSet.from_jpeg(mixed_files, list(range(10)), DEV, budget_bytes=bud, fallback=fallback)
        assert seen == [prog] and (ds.n_device, ds.n_fallback) == (9, 1)
        _set_equal(DeviceImageSet(mixed_images, list(range(10)), DEV, budget_bytes=bud), ds, mixed_images)
    with pytest.raises(IndexError):
        DeviceImageSet.from_jpeg(files[:4], [0, 1, 2, 30], DEV, n_cls=10)
    with pytest.raises(ValueError, match="fallback must return"):
        DeviceImageSet.from_jpeg([prog], [0], DEV, fallback=lambda data: stand_in.astype(np.float32))


def _training_files(n):
    fx = fixtures()
    big = [k for k, (_, r) in enumerate(fx) if min(r.shape[:2]) >= 48]
    pick = [big[j % len(big)] for j in range(n)]
    return [fx[k][0] for k in pick], [fx[k][1] for k in pick]


@pytest.mark.parametrize("kind,mode", [("rpo", "f32"), ("coop", "f16")])
def test_run_epoch_on_a_from_jpeg_set_is_bit_identical(kind, mode):
    from rpo_amd.input_pipeline import DeviceImageSet
    from rpo_amd.loop import epoch_indices
    B, nb = 4, 3
    n = B * nb + 1
    files, images = _training_files(n)
    labels = np.random.default_rng(32).integers(0, 19, n).tolist()
    budget = sum(im.size for im in images) * 2 // 3
    sets = [DeviceImageSet(images, labels, DEV, budget_bytes=budget), DeviceImageSet.from_jpeg(files, labels, DEV, budget_bytes=budget)]
    assert sets[0].plan.spilled and sets[1].n_fallback == 0
    stage = _staging(True, B)
    torch.manual_seed(5)
    order = epoch_indices(n, B, torch.Generator().manual_seed(40))
    plans = [[stage.plan(*images[i].shape[:2]) for i in batch] for batch in order]
    results = []
    for ds in sets:
        tr = _make(kind, mode, True, B, nb)
        out = tr.run_epoch(ds, torch.Generator().manual_seed(40), plans)
        assert out["indices"] == order
        p, m = _state(tr, kind)
        results.append((out["loss"].cpu(), p, m, out["counts"].tolist() if "counts" in out else None))
    (l0, p0, m0, c0), (l1, p1, m1, c1) = results
    assert torch.equal(bits(l0), bits(l1)) and torch.equal(bits(p0), bits(p1)) and torch.equal(bits(m0), bits(m1)) and c0 == c1


def test_test_on_a_from_jpeg_set_is_bit_identical():
    from rpo_amd.input_pipeline import DeviceImageSet
    n, bs = 23, 10
    files, images = _training_files(n)
    labels = np.random.default_rng(52).integers(0, 19, n).tolist()
    budget = sum(im.size for im in images) * 3 // 4
    tr = _make("coop", "f16", True, bs, 2)
    a = tr.test(DeviceImageSet(images, labels, DEV, budget_bytes=budget), batch_size=bs)
    ds = DeviceImageSet.from_jpeg(files, labels, DEV, budget_bytes=budget)
    assert ds.n_fallback == 0
    b = tr.test(ds, batch_size=bs)
    assert (a["total"], a["correct"], a["accuracy"]) == (b["total"], b["correct"], b["accuracy"]) and a["total"] == n
    assert np.array_equal(a["confusion_matrix"], b["confusion_matrix"])


# ---- streams Pillow's encoder never writes (tools/make_jpeg_streams.py) ---------------------------------------------------

def test_every_in_gamut_stream_in_one_call_equals_pillow():
    """2600+ streams -- third table slots, packed / redefined tables, 16-bit codes, every size 1..18 squared in four modes,
    restart and marker variants, the 8188-unit strip next to 1x1 images -- in ONE launch: each equals Pillow's pixels; the
    same bits in chunks of 7 in another order."""
    from rpo_amd.jpeg import JpegDecoder
    cs = in_gamut()
    assert len(cs) > 2592 + 60
    files, shapes = [c["file"] for c in cs], [c["rgb"].shape[:2] for c in cs]
    st, first = guarded_decode(JpegDecoder(DEV, chunk_images=4096), files, shapes)
    assert st.shape == (len(cs),) and not st.any(), [cs[k]["tag"] for k in np.flatnonzero(st)][:5]
    for c, im in zip(cs, first):
        assert np.array_equal(im, c["rgb"]), (c["tag"], int((im != c["rgb"]).any(-1).sum()))
    order = list(np.random.default_rng(3).permutation(len(cs)))
    st, second = guarded_decode(JpegDecoder(DEV, chunk_images=7), [files[j] for j in order], [shapes[j] for j in order], guard=5)
    assert not st.any()
    for j, im in zip(order, second):
        assert np.array_equal(im, first[j]), cs[j]["tag"]


def test_the_8188_unit_strip_alone_and_among_299_small_streams():
    """One file of 8188 restart intervals is > 4096 units with a single descriptor: several units per wave, every lane's
    binary search ends on image 0.  Then the same file behind and in front of 299 small ones."""
    from rpo_amd.jpeg import JpegDecoder, probe
    cs = in_gamut()
    strip = next(c for c in cs if "8188 units" in c["tag"])
    assert probe(strip["file"]).units == 8188
    dec = JpegDecoder(DEV, chunk_images=4096)
    st, (alone,) = guarded_decode(dec, [strip["file"]], [strip["rgb"].shape[:2]])
    assert not st.any() and np.array_equal(alone, strip["rgb"])
    small = [c for c in cs if c["rgb"].shape[0] * c["rgb"].shape[1] <= 2048]
    pick = [small[j] for j in np.random.default_rng(4).integers(0, len(small), 299)]
    mixed = pick[:150] + [strip] + pick[150:]
    st, imgs = guarded_decode(dec, [c["file"] for c in mixed], [c["rgb"].shape[:2] for c in mixed])
    assert not st.any() and np.array_equal(imgs[150], alone)
    for c, im in zip(mixed, imgs):
        assert np.array_equal(im, c["rgb"]), c["tag"]


def test_out_of_gamut_streams_are_defined_and_equal_the_oracle():
    """Header-valid streams no encoder produces (dense coefficients at dequantised amplitudes up to 32767 x 255, AC
    categories 11..15, a DC predictor past int16): status 0, the oracle's bits (sums modulo 2^32), the same
    bits again.  Pillow clamps narrower intermediates there; equality with it is required only where the generator saw it."""
    from rpo_amd.jpeg import JpegDecoder
    cs = [c for c in streams() if not c["gamut"]]
    assert len(cs) >= 12
    dec = JpegDecoder(DEV)
    files, shapes = [c["file"] for c in cs], [c["rgb"].shape[:2] for c in cs]
    st, first = guarded_decode(dec, files, shapes)
    assert not st.any()
    for c, im in zip(cs, first):
        assert np.array_equal(im, J.decode(c["file"])), c["tag"]
        differ = int((im != c["rgb"]).any(-1).sum())
        print(f"{differ:5d} of {im.shape[0] * im.shape[1]} pixels differ from Pillow: {c['tag']}")
        if c["differ"] == 0:
            assert differ == 0, c["tag"]
    st, second = guarded_decode(dec, files, shapes)
    assert not st.any() and all(np.array_equal(a, b) for a, b in zip(first, second))


def test_constructed_corrupt_streams_end_in_their_exact_status():
    """Each stream is wrong in one known place (tests/jpeg_writer.py corrupt_streams; all of them ran through the decoder's
    code on the CPU first, tests/test_jpeg_streams_host.py); good streams sit between them and stay exact."""
    from rpo_amd.jpeg import JpegDecoder
    good = [c for c in in_gamut() if c["rgb"].shape[:2] == (32, 32)][:6]
    corrupt = JW.corrupt_streams()
    assert [s for _, _, s in corrupt] == [2, 2, 3, 1, 4]            # BAD_CODE, BAD_CODE, BAD_INDEX, TRUNCATED, NO_RESTART
    files, want = [good[0]["file"]], [0]
    for k, (_, data, status) in enumerate(corrupt):
        files += [data, good[k + 1]["file"]]
        want += [status, 0]
    dec = JpegDecoder(DEV)
    st, imgs = guarded_decode(dec, files, [(32, 32)] * len(files))
    print("device status:", st.tolist())
    assert st.tolist() == want
    for k, c in enumerate(good):
        assert np.array_equal(imgs[2 * k], c["rgb"]), c["tag"]
    st2, imgs2 = guarded_decode(dec, files, [(32, 32)] * len(files))
    assert np.array_equal(st, st2) and all(np.array_equal(a, b) for a, b in zip(imgs, imgs2))


def test_from_jpeg_on_a_folder_of_the_streams_and_the_refused_ones(tmp_path):
    from rpo_amd.input_pipeline import DeviceImageSet
    cs = [c for c in streams() if c["gamut"]]
    stand_in = np.random.default_rng(2).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    paths, images = [], []
    for i, c in enumerate(cs):
        paths.append(str(tmp_path / f"{i:04d}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(c["file"])
        images.append(stand_in if c["refused"] else c["rgb"])
    n_refused = sum(bool(c["refused"]) for c in cs)
    assert n_refused == 2
    seen = []

    def fallback(data):
        seen.append(data)
        return stand_in
    labels = [i % 19 for i in range(len(cs))]
    ds = DeviceImageSet.from_jpeg(paths, labels, DEV, fallback=fallback)
    assert (ds.n_device, ds.n_fallback) == (len(cs) - n_refused, n_refused)
    assert seen == [c["file"] for c in cs if c["refused"]]
    _set_equal(DeviceImageSet(images, labels, DEV), ds, images)
