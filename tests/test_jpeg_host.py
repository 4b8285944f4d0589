"""Host side of the on-device JPEG decode: the numpy oracle (tests/jpeg_oracle.py, the checker of rpo_amd/csrc/jpeg.hip) is
pinned bit for bit to the committed Pillow fixtures and to Pillow itself, and `rpo_jpeg_probe` (host C++ inside the
library, no GPU) reports what Pillow reports, refuses what the device does not decode, and never reads past nbytes."""
import ctypes
import io
import mmap
import os

import numpy as np
import pytest

import jpeg_oracle as J

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixtures(*names):
    for name in names or ("jpeg_small.npz", "jpeg_photo.npz"):
        g = np.load(os.path.join(GOLD, name))
        for i in range(int(g["n"])):
            yield f"{name}:{i}", g[f"file{i}"].tobytes(), g[f"rgb{i}"], tuple(int(v) for v in g[f"meta{i}"])


def refused():
    g = np.load(os.path.join(GOLD, "jpeg_refused.npz"))
    return {str(k): g[str(k)].tobytes() for k in g["reasons"]}


def test_fixture_set_covers_the_issue_list():
    cases = list(fixtures())
    assert len(cases) >= 20
    sizes = {(rgb.shape[1], rgb.shape[0]) for _, _, rgb, _ in cases}
    assert {(1, 1), (8, 8), (2, 3), (17, 9), (33, 16), (100, 75), (500, 375)} <= sizes
    metas = {m for _, _, _, m in cases}
    assert {(3, 1, 1), (3, 2, 1), (3, 2, 2), (1, 1, 1)} == {m[:3] for m in metas}
    assert {0, 1, 3} == {m[3] for m in metas}
    assert sorted(refused()) == ["components", "progressive", "rgb", "sampling"]
    total = sum(os.path.getsize(os.path.join(GOLD, f)) for f in ("jpeg_small.npz", "jpeg_photo.npz", "jpeg_refused.npz"))
    assert total < 1_000_000                 # jpeg_streams.npz has a cap of its own (tests/test_jpeg_streams_host.py)


def test_oracle_equals_every_fixture():
    for name, data, rgb, meta in fixtures():
        h = J.parse(data)
        assert (h.components, h.h_samp, h.v_samp, h.restart_interval) == meta, name
        got = J.decode(data)
        assert got.dtype == np.uint8 and np.array_equal(got, rgb), name


def test_oracle_refuses_and_flags_corruption():
    reasons = {"components": "components", "progressive": "progressive", "rgb": "rgb", "sampling": "sampling"}
    for k, data in refused().items():
        with pytest.raises(J.Unsupported) as e:
            J.parse(data)
        assert e.value.reason == reasons[k]
    name, data, _, _ = next(f for f in fixtures("jpeg_small.npz") if f[3] == (3, 2, 2, 0) and f[2].shape[0] == 75)
    with pytest.raises(J.Corrupt):
        J.decode(data[:len(data) * 2 // 3])


def _content(rng, H, W):
    base = rng.integers(0, 256, (-(-H // 5), -(-W // 5), 3))
    img = np.kron(base, np.ones((5, 5, 1)))[:H, :W] + rng.normal(0, 12, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def test_oracle_equals_pillow_on_fresh_files():
    """The sweep behind the feasibility claim: sizes 1x1 .. 100x75 (odd, non-MCU-multiple, the <= 2 wide chroma planes),
    qualities 30 / 75 / 95 / 100, 4:4:4 / 4:2:2 / 4:2:0 / gray, plain / optimised tables / restart intervals 1 and 3."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(0)
    n = 0
    for (H, W) in [(1, 1), (8, 8), (3, 2), (2, 3), (9, 17), (16, 33), (75, 100), (5, 4), (7, 3)]:
        img = _content(rng, H, W)
        for q in (30, 75, 95, 100):
            for ss in (0, 1, 2, "L"):
                for kw in ({}, {"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 3}):
                    if (H, W) == (75, 100) and (q, kw) not in ((75, {}), (95, {"optimize": True}), (30, {"restart_marker_blocks": 3})):
                        continue                                   # the pure-Python entropy decode is slow at this size
                    b = io.BytesIO()
                    if ss == "L":
                        Image.fromarray(img[..., 0]).save(b, "JPEG", quality=q, **kw)
                    else:
                        Image.fromarray(img).save(b, "JPEG", quality=q, subsampling=ss, **kw)
                    data = b.getvalue()
                    want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
                    assert np.array_equal(J.decode(data), want), (H, W, q, ss, kw)
                    n += 1
    assert n >= 216


# ---- rpo_jpeg_probe -----------------------------------------------------------------------------------------------------

def test_probe_reports_size_mode_sampling():
    from rpo_amd import _lib, jpeg
    for name, data, rgb, meta in fixtures():
        info = jpeg.probe(data)
        h = J.parse(data)
        assert (info.height, info.width) == rgb.shape[:2], name
        assert (info.components, info.h_samp, info.v_samp, info.restart_interval) == meta, name
        assert (info.mcus_x, info.mcus_y, info.scan_offset) == (h.mcus_x, h.mcus_y, h.scan_offset), name
        assert info.scan_offset + info.scan_bytes == len(data), name
        mcus = h.mcus_x * h.mcus_y
        assert info.units == (-(-mcus // meta[3]) if meta[3] else 1), name
        assert info.coef_bytes == mcus * (1 if meta[0] == 1 else meta[1] * meta[2] + 2) * 128, name
        assert info.table_bytes > 0 and info.table_bytes % 16 == 0
    assert ctypes.sizeof(_lib.JpegInfo) == 72 and ctypes.sizeof(_lib.JpegDesc) == 120


def test_probe_agrees_with_pillow():
    Image = pytest.importorskip("PIL.Image")
    from rpo_amd import jpeg
    for name, data, _, meta in fixtures():
        im = Image.open(io.BytesIO(data))
        info = jpeg.probe(data)
        assert im.size == (info.width, info.height), name
        assert im.mode == ("L" if info.components == 1 else "RGB"), name
        if info.components == 3:
            assert im.layer[0][1:3] == (info.h_samp, info.v_samp) and im.layer[1][1:3] == (1, 1), name


def test_probe_refuses_each_unsupported_kind_with_its_own_reason():
    from rpo_amd import _lib, jpeg
    want = {"progressive": (_lib.E_JPEG_PROGRESSIVE, "progressive"), "components": (_lib.E_JPEG_COMPONENTS, "components"),
            "rgb": (_lib.E_JPEG_RGB, "RGB"), "sampling": (_lib.E_JPEG_SAMPLING, "sampling")}
    codes = set()
    for k, data in refused().items():
        with pytest.raises(jpeg.JpegRefused) as e:
            jpeg.probe(data)
        assert e.value.code == want[k][0] and want[k][1] in e.value.reason, (k, e.value.code, e.value.reason)
        codes.add(e.value.code)
    assert len(codes) == 4
    with pytest.raises(jpeg.JpegRefused) as e:
        jpeg.probe(b"not a jpeg at all")
    assert e.value.code == _lib.E_JPEG_CORRUPT
    # the frame types / precisions the fixtures do not carry: patch the SOF marker / precision byte of a good header
    _, good, _, _ = next(fixtures("jpeg_small.npz"))
    sof = good.index(b"\xff\xc0")
    for patch, code in (((sof + 1, 0xC9), _lib.E_JPEG_ARITHMETIC), ((sof + 1, 0xC3), _lib.E_JPEG_LOSSLESS),
                        ((sof + 4, 12), _lib.E_JPEG_PRECISION)):
        bad = bytearray(good)
        bad[patch[0]] = patch[1]
        with pytest.raises(jpeg.JpegRefused) as e:
            jpeg.probe(bytes(bad))
        assert e.value.code == code


def test_probe_rejects_truncated_headers_without_reading_past_nbytes():
    """Every prefix of a header is placed so that it ENDS at the last byte of a mapped page followed by an unmapped-for-read
    page: a parser that looked one byte past nbytes would fault instead of returning."""
    from rpo_amd import _lib
    lib = _lib.load()
    _, data, _, _ = next(f for f in fixtures("jpeg_small.npz") if f[3][3] == 3)           # has DQT, DHT, DRI, SOF, SOS
    hdr = J.parse(data).scan_offset
    page = mmap.PAGESIZE
    span = (hdr + page - 1) // page * page
    m = mmap.mmap(-1, span + page)
    libc = ctypes.CDLL(None, use_errno=True)
    base = ctypes.addressof(ctypes.c_char.from_buffer(m))
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert libc.mprotect(base + span, page, 0) == 0                                        # PROT_NONE guard page
    info = _lib.JpegInfo()
    try:
        for n in range(1, hdr + 1):
            m[span - n:span] = data[:n]
            rc = lib.rpo_jpeg_probe(base + span - n, n, ctypes.byref(info))
            assert rc == (0 if n == hdr else _lib.E_JPEG_CORRUPT), (n, rc)
        assert (info.width, info.height) == (100, 75) and info.scan_bytes == 0
        assert lib.rpo_jpeg_probe(None, 10, ctypes.byref(info)) == _lib.E_BADARG
        assert lib.rpo_jpeg_probe(base, 0, ctypes.byref(info)) == _lib.E_BADARG
    finally:
        libc.mprotect(base + span, page, 3)
        del base
    # rpo_jpeg_tables: the same parse, a blob of table_bytes; too small a blob is refused
    blob = (ctypes.c_char * info.table_bytes)()
    assert lib.rpo_jpeg_tables(data, len(data), ctypes.addressof(blob), info.table_bytes) == 0
    assert lib.rpo_jpeg_tables(data, len(data), ctypes.addressof(blob), info.table_bytes - 1) == _lib.E_WORKSPACE
    q = np.frombuffer(blob, np.uint16, 64)
    assert np.array_equal(q, J.parse(data).quant[0])


def test_workspace_layout_and_descriptor_validation():
    """rpo_jpeg_workspace_bytes lays a batch out; rpo_jpeg_decode_batch validates the host descriptors before any launch, so
    these calls return argument errors without a GPU."""
    from rpo_amd import _lib, jpeg
    lib = _lib.load()
    files = [f[1] for f in fixtures("jpeg_small.npz")][:6]
    descs = (_lib.JpegDesc * len(files))()
    off = out = 0
    for d, data in zip(descs, files):
        d.info = jpeg.probe(data)
        d.file_offset, d.file_bytes = off, len(data)
        off += (len(data) + 15) // 16 * 16
        d.table_offset = off
        off += d.info.table_bytes
        d.out_offset = out
        out += d.info.width * d.info.height * 3
    need = lib.rpo_jpeg_workspace_bytes(descs, len(files))
    units = sum(d.info.units for d in descs)
    assert need >= sum(d.info.coef_bytes for d in descs) + 4 * units
    assert [d.unit_base for d in descs] == list(np.cumsum([0] + [d.info.units for d in descs])[:-1])
    assert all(d.coef_offset % 128 == 0 for d in descs)
    assert lib.rpo_jpeg_workspace_bytes(descs, 0) == 0
    fake = 1 << 20                                                       # never dereferenced: validation comes first

    def call(n=len(files), files_bytes=off, out_bytes=out, ws_bytes=need, ptr=fake):
        return lib.rpo_jpeg_decode_batch(ptr, files_bytes, ctypes.addressof(descs), fake, n, fake, out_bytes, fake, ws_bytes,
                                         fake, None)
    assert call(n=0) == _lib.E_BADARG
    assert call(files_bytes=off - 1) == _lib.E_SHAPE
    assert call(out_bytes=out - 1) == _lib.E_SHAPE
    assert call(ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert call(ptr=fake + 8) == _lib.E_ALIGN
    descs[2].info.mcus_x += 1
    assert call() == _lib.E_SHAPE
    descs[2].info.mcus_x -= 1
    descs[3].coef_offset += 128
    assert call() == _lib.E_WORKSPACE
