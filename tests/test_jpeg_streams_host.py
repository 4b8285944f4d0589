"""The JPEG decoder's own C++ on the CPU (tests/host/jpeg_host_decode.cpp includes rpo_amd/csrc/jpeg.hip and runs parse_header,
rpo_jpeg_tables, the restart offsets, decode_unit, idct_block and pixel_rgb without the HIP runtime) against streams Pillow's
encoder never writes (tests/golden/jpeg_streams.npz, written by tools/make_jpeg_streams.py with tests/jpeg_writer.py; `rgb`
there is PILLOW's decode).  Three judges: Pillow (recorded, and live where importable), the numpy oracle, the host program.
In gamut -- coefficient blocks an encoder can make from 8-bit samples -- all three agree bit for bit; out of gamut the host
program equals the oracle and Pillow's pixels are a record.  No GPU is needed."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_oracle as J
import jpeg_writer as JW

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)
ORACLE_PIXELS = 10_000                                             # the oracle's entropy decode is pure Python


def streams():
    return JW.load_streams(os.path.join(GOLD, "jpeg_streams.npz"))


def small_fixtures():
    g = np.load(os.path.join(GOLD, "jpeg_small.npz"))
    return [{"file": g[f"file{i}"].tobytes(), "rgb": g[f"rgb{i}"], "meta": tuple(int(v) for v in g[f"meta{i}"]),
             "tag": f"jpeg_small:{i}"} for i in range(int(g["n"]))]


def build_host_program(out_dir, extra_flags=()):
    from rpo_amd.build import _hipcc
    exe = os.path.join(str(out_dir), "jpeg_host_decode")
    cmd = [_hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", *extra_flags,
           os.path.join(HERE, "host", "jpeg_host_decode.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_host_program(exe, files, work_dir):
    """-> [(record of 12 int32, rgb [H, W, 3] or None)] per file"""
    src, dst = os.path.join(str(work_dir), "in.bin"), os.path.join(str(work_dir), "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(files)))
        for data in files:
            f.write(struct.pack("<q", len(data)) + data)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    raw = open(dst, "rb").read()
    out, pos = [], 0
    for _ in files:
        rec = struct.unpack_from("<12i", raw, pos)
        pos += 48
        rgb = None
        if rec[0] == 0:
            n = rec[2] * rec[3] * 3
            rgb = np.frombuffer(raw, np.uint8, n, pos).reshape(rec[3], rec[2], 3)
            pos += n
        out.append((rec, rgb))
    assert pos == len(raw)
    return out


@pytest.fixture(scope="module")
def decoded(tmp_path_factory):
    """every stream of jpeg_streams.npz and jpeg_small.npz, and the corrupt ones, through the host program: ONE child process"""
    d = tmp_path_factory.mktemp("jpeg_host")
    exe = build_host_program(d)
    cases = streams() + small_fixtures()
    corrupt = JW.corrupt_streams()
    res = run_host_program(exe, [c["file"] for c in cases] + [f for _, f, _ in corrupt], d)
    return cases, res[:len(cases)], corrupt, res[len(cases):]


def test_the_stream_set_covers_what_it_claims():
    cases = streams()
    tags = " | ".join(c["tag"] for c in cases)
    for word in ("third slots 444", "third slots 422", "third slots 420", "one DQT and one DHT", "redefined", "10..16 bits",
                 "no code longer than 9", "quantisers all 1,", "quantisers all 255,", "binary", "checkerboard", "run 62",
                 "category 11", "category 10", "65500x1", "1x4099", "1x65500", "does not divide", "total - 1",
                 "equal to the total", "65535", "DRI twice (7, then 2)", "DRI twice (3, then 0)", "counter wraps",
                 "fill bytes", "APP1", "behind EOI", "SOF1", "ids 0 1 2", "ids 10 20 30", "R G B with JFIF", "no JFIF",
                 "Adobe transform 1", "Adobe transform 2", "Adobe transform 0 with JFIF", "0x22", "0x41",
                 "refused: component ids R G B", "refused: Adobe transform 0", "amplitude 765", "amplitude 1020",
                 "amplitude 4080", "32-bit sums wrap", "category 11..15", "DC predictor"):
        assert word in tags, word
    sweep = {(c["meta"][:3], c["rgb"].shape[:2]) for c in cases if c["tag"].startswith("sweep")}
    assert len(sweep) == 4 * 18 * 18 and sum(c["tag"].startswith("sweep") for c in cases) == 2 * len(sweep)
    assert all(c["differ"] == 0 for c in cases if c["gamut"]), "the in-gamut set has zero pixels differing from Pillow"
    assert any(c["differ"] > 0 for c in cases if not c["gamut"])
    assert os.path.getsize(os.path.join(GOLD, "jpeg_streams.npz")) < 512 * 1024
    # the writer's table helper: n16 codes of 16 bits, the rest within the look-ahead; never the all-ones code
    bits, vals = JW.long_table(JW.AC_SYMBOLS, 20)
    assert bits[16] == 20 and bits[10:16].sum() == 0 and bits.sum() == len(vals) == 162
    bits, _ = JW.spread_table(JW.AC_SYMBOLS, 10, 16)
    assert bits[:10].sum() == 0 and (bits[10:] > 0).all()


def test_host_program_equals_pillow_and_the_oracle_in_gamut(decoded):
    cases, res, _, _ = decoded
    n_oracle = 0
    for c, (rec, rgb) in zip(cases, res):
        if c.get("refused") or not c.get("gamut", 1):
            continue
        assert rec[0] == 0 and rec[1] == 0, (c["tag"], rec)
        assert rgb.shape == c["rgb"].shape and np.array_equal(rgb, c["rgb"]), (c["tag"], int((rgb != c["rgb"]).any(-1).sum()))
        if rgb.shape[0] * rgb.shape[1] <= ORACLE_PIXELS:
            assert np.array_equal(J.decode(c["file"]), rgb), c["tag"]
            n_oracle += 1
    assert n_oracle >= 2592 + 60


def test_live_pillow_agrees_with_the_recorded_pixels():
    Image = pytest.importorskip("PIL.Image")
    for c in streams():
        if c["refused"]:
            continue
        want = np.asarray(Image.open(io.BytesIO(c["file"])).convert("RGB"))
        if c["gamut"]:
            assert np.array_equal(want, c["rgb"]), c["tag"]
        else:                                                      # another libjpeg build may treat these differently
            print(c["tag"], "live Pillow differs from the record in", int((want != c["rgb"]).any(-1).sum()), "pixels")


def test_probe_reports_the_writers_parameters_and_refuses_the_refused(decoded):
    from rpo_amd import _lib, jpeg
    cases, res, _, _ = decoded
    n_refused = 0
    for c, (rec, _) in zip(cases, res):
        if c.get("refused"):
            assert c["refused"] == "rgb"
            with pytest.raises(jpeg.JpegRefused) as e:
                jpeg.probe(c["file"])
            assert e.value.code == _lib.E_JPEG_RGB and rec[0] == _lib.E_JPEG_RGB, c["tag"]
            n_refused += 1
            continue
        info = jpeg.probe(c["file"])
        H, W = c["rgb"].shape[:2]
        nc, hs, vs, ri = c["meta"]
        h = J.parse(c["file"])
        mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
        got = (info.width, info.height, info.components, info.h_samp, info.v_samp, info.restart_interval, info.units,
               info.scan_offset, info.mcus_x, info.mcus_y)
        assert got == (W, H, nc, hs, vs, ri, -(-mcus // ri) if ri else 1, h.scan_offset, -(-W // (8 * hs)), -(-H // (8 * vs))), c["tag"]
        assert tuple(rec[2:12]) == got, c["tag"]                   # the program's own parse_header says the same
        assert info.scan_offset + info.scan_bytes == len(c["file"])
    assert n_refused == 2


def test_host_program_equals_the_oracle_out_of_gamut(decoded):
    cases, res, _, _ = decoded
    n = 0
    for c, (rec, rgb) in zip(cases, res):
        if c.get("gamut", 1):
            continue
        assert rec[0] == 0 and rec[1] == 0, (c["tag"], rec)
        assert np.array_equal(rgb, J.decode(c["file"])), c["tag"]
        differ = int((rgb != c["rgb"]).any(-1).sum())
        print(f"{differ:5d} pixels differ from Pillow: {c['tag']}")
        n += 1
    assert n >= 12


def test_corrupt_streams_end_in_their_exact_status_on_the_host(decoded):
    _, _, corrupt, res = decoded
    for (what, data, status), (rec, rgb) in zip(corrupt, res):
        assert rec[0] == 0 and rec[1] == status, (what, rec[:2])
        assert rgb.shape == (32, 32, 3)
        with pytest.raises(J.Corrupt):
            J.decode(data)


def test_an_image_of_more_than_2_31_pixels_is_refused_before_any_launch():
    """The colour kernel counts pixels in an int: 65535 x 65535 passes the header checks, so the batch call must refuse it
    (validation comes before any pointer is used, as in tests/test_jpeg_host.py)."""
    import ctypes
    from rpo_amd import _lib, jpeg
    lib = _lib.load()
    data = bytearray(next(c for c in streams() if c["tag"].startswith("sweep 8x8 gray"))["file"])
    sof = data.index(b"\xff\xc0")
    descs = (_lib.JpegDesc * 1)()

    def call(h, w):
        data[sof + 5:sof + 9] = bytes([h >> 8, h & 255, w >> 8, w & 255])
        d = descs[0]
        d.info = jpeg.probe(bytes(data))
        d.file_offset, d.file_bytes, d.table_offset, d.out_offset = 0, len(data), 1024, 0
        need = lib.rpo_jpeg_workspace_bytes(descs, 1)
        assert need > d.info.coef_bytes
        fake = 1 << 20
        # a workspace one byte short: were the size check missing, the call would still end before any launch
        return lib.rpo_jpeg_decode_batch(fake, 1 << 20, ctypes.addressof(descs), fake, 1, fake, 3 * h * w, fake, need - 1, fake, None)
    assert call(65535, 65535) == _lib.E_SHAPE and call(46341, 46341) == _lib.E_SHAPE
