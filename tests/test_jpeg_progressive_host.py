"""The progressive JPEG decoder's own C++ on the CPU (tests/host/jpeg_prog_host_decode.cpp includes rpo_amd/csrc/jpeg.hip and
runs rpo_jpeg_prog_probe, rpo_jpeg_prog_plan, every unit in level order, idct_block and pixel_rgb without the HIP runtime)
against tests/golden/jpeg_progressive.npz (tools/make_jpeg_progressive.py: Pillow-written progressive files and streams
under scan scripts Pillow never writes, from tests/jpeg_prog_writer.py; `rgb` there is PILLOW's decode).  Judges: Pillow
(recorded, and live where importable), the pure-Python oracle tests/jpeg_prog_oracle.py (streams of at most ORACLE_PIXELS),
the host program's own baseline decode of the writer's twin file.  No GPU is needed."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_prog_oracle as PO
import jpeg_prog_writer as PW
from test_jpeg_streams_host import ORACLE_PIXELS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def fixtures():
    return PW.load_progressive(os.path.join(GOLD, "jpeg_progressive.npz"))


def build_host_program(out_dir, extra_flags=()):
    """as test_jpeg_streams_host.build_host_program builds tests/host/jpeg_host_decode.cpp"""
    from rpo_amd.build import _hipcc
    exe = os.path.join(str(out_dir), "jpeg_prog_host_decode")
    cmd = [_hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", *extra_flags,
           os.path.join(HERE, "host", "jpeg_prog_host_decode.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_host_program(exe, files, work_dir, probe_only=False):
    """-> [(record of 12 int32, rgb [H, W, 3] or None)] per file"""
    src, dst = os.path.join(str(work_dir), "in.bin"), os.path.join(str(work_dir), "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(files)))
        for data in files:
            f.write(struct.pack("<q", len(data)) + data)
    r = subprocess.run([exe, src, dst] + (["probe"] if probe_only else []), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    raw = open(dst, "rb").read()
    out, pos = [], 0
    for _ in files:
        rec = struct.unpack_from("<12i", raw, pos)
        pos += 48
        rgb = None
        if (rec[0] == 0 or rec[11] == 0) and not probe_only:
            n = rec[2] * rec[3] * 3
            rgb = np.frombuffer(raw, np.uint8, n, pos).reshape(rec[3], rec[2], 3)
            pos += n
        out.append((rec, rgb))
    assert pos == len(raw)
    return out


def header_prefixes(streams):
    """every prefix, up to the first entropy-coded byte of the LAST scan, of three progressive files"""
    out = []
    for word in ("pillow 17x33 420 q95 optimize", "redefined", "DRI changed"):
        data = next(s for s in streams if word in s["tag"])["file"]
        last_sos = data.rindex(b"\xff\xda")
        out += [data[:k] for k in range(1, last_sos + 14)]
    return out


@pytest.fixture(scope="module")
def decoded(tmp_path_factory):
    """every stream, its baseline twin, the corrupt streams and the refused files through the host program: ONE child process"""
    d = tmp_path_factory.mktemp("jpeg_prog_host")
    exe = build_host_program(d)
    streams, refused = fixtures()
    twins = [s["twin"] for s in streams if s["twin"]]
    corrupt = PW.corrupt_streams()
    files = [s["file"] for s in streams] + twins + [f for _, f, _ in corrupt] + [r["file"] for r in refused]
    res = run_host_program(exe, files, d)
    a, b, c = len(streams), len(streams) + len(twins), len(streams) + len(twins) + len(corrupt)
    return {"streams": streams, "res": res[:a], "twins": res[a:b], "corrupt": corrupt, "corrupt_res": res[b:c],
            "refused": refused, "refused_res": res[c:], "exe": exe, "dir": d}


def test_the_library_exports_the_progressive_entry_points():
    from rpo_amd import _lib
    lib = _lib.load()
    for name in ("rpo_jpeg_prog_probe", "rpo_jpeg_prog_plan", "rpo_jpeg_prog_workspace_bytes", "rpo_jpeg_prog_decode_batch"):
        assert getattr(lib, name) is not None, name
    assert (_lib.E_JPEG_SCRIPT, _lib.E_JPEG_SEQUENTIAL) == (-29, -30)
    assert b"script" in lib.rpo_error_string(-29) and b"sequential" in lib.rpo_error_string(-30)


def test_the_stream_set_covers_what_it_claims():
    streams, refused = fixtures()
    tags = " | ".join(s["tag"] for s in streams)
    for word in ("spectral selection only", "from Al = 3", "from Al = 13 on DC", "non-interleaved DC", "Ss = Se",
                 "bands split at 1", "bands split at 62", "chroma before luma", "component 2 between component 0's first and refinement",
                 "redefined", "only 10..16-bit codes", "end mid-row", "cut at a restart boundary", "nonzero history",
                 "ZRL in a refinement scan", "every new coefficient negative", "DRI changed between scans", "including to 0",
                 "fill bytes before markers", "data behind EOI", "does not divide the row", "optimize", "photo-like",
                 "EOBRUN 32767 then 1", "restart_marker_blocks 1", "restart_marker_blocks 3"):
        assert word in tags, word
    assert sum("bands split at" in s["tag"] for s in streams) == 62
    sweep = {(s["tag"].split()[1], s["tag"].split()[2]) for s in streams if s["tag"].startswith("pillow") and len(s["tag"].split()) == 4}
    sizes = (1, 7, 8, 9, 16, 17, 24, 33)
    assert sweep == {(f"{w}x{h}", m) for w in sizes for h in sizes for m in ("gray", "444", "422", "420")}
    for m in ("gray", "444", "422", "420"):
        assert {s["tag"].split()[3] for s in streams if s["tag"].startswith("pillow") and s["tag"].split()[2] == m} >= {"q30", "q95"}
    assert all((s["twin"] is not None) == s["tag"].startswith("writer") for s in streams)
    rtags = " | ".join(r["tag"] for r in refused)
    for word in ("incomplete script", "Ah != previous Al", "AC before DC", "two components", "DQT after the first SOS",
                 "Al = 14", "CMYK", "SOF10", "baseline file"):
        assert word in rtags, word
    assert os.path.getsize(os.path.join(GOLD, "jpeg_progressive.npz")) < 500 * 1024
    # the flat 2048 x 1024 file: its first AC scan is the r = 14 symbol (an EOB run of 32767) and then a run of one
    flat = next(s for s in streams if "EOBRUN 32767" in s["tag"])["file"]
    g = PO.parse(flat)
    assert (g.width, g.height) == (2048, 1024) and (g.scans[1].ss, g.scans[1].ah) == (1, 0)
    br = PO.J._Bits(flat, g.scans[1].starts[0])
    assert PO.J._huff(br, g.scans[1].ac) == 0xE0 and br.get(14) == 16383 and PO.J._huff(br, g.scans[1].ac) == 0x00
    # Pillow's own script has three levels and all four scan kinds
    g = PO.parse(next(s for s in streams if s["tag"].startswith("pillow 33x33 420 q"))["file"])
    assert [(len(s.comps), s.ss, s.se, s.ah, s.al) for s in g.scans] == [
        (3, 0, 0, 0, 1), (1, 1, 5, 0, 2), (1, 1, 63, 0, 1), (1, 1, 63, 0, 1), (1, 6, 63, 0, 2), (1, 1, 63, 2, 1),
        (3, 0, 0, 1, 0), (1, 1, 63, 1, 0), (1, 1, 63, 1, 0), (1, 1, 63, 1, 0)]


def test_host_program_equals_pillow_and_the_oracle(decoded):
    n_oracle = 0
    for s, (rec, rgb) in zip(decoded["streams"], decoded["res"]):
        assert rec[0] == 0 and rec[1] == 0, (s["tag"], rec)
        assert rgb.shape == s["rgb"].shape and np.array_equal(rgb, s["rgb"]), (s["tag"], int((rgb != s["rgb"]).any(-1).sum()))
        if rgb.shape[0] * rgb.shape[1] <= ORACLE_PIXELS:
            assert np.array_equal(PO.decode(s["file"]), rgb), s["tag"]
            n_oracle += 1
    assert n_oracle == len(decoded["streams"]) - 2                   # all but the photo-sized and the 2048 x 1024 file


def test_live_pillow_agrees_with_the_recorded_pixels():
    Image = pytest.importorskip("PIL.Image")
    for s in fixtures()[0]:
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(s["file"])).convert("RGB")), s["rgb"]), s["tag"]


def test_progressive_equals_the_baseline_twin_bit_for_bit(decoded):
    twins = iter(decoded["twins"])
    n = 0
    for s, (rec, rgb) in zip(decoded["streams"], decoded["res"]):
        if s["twin"] is None:
            continue
        trec, trgb = next(twins)
        assert trec[0] == -30 and trec[11] == 0 and trec[1] == 0, (s["tag"], trec)   # RPO_E_JPEG_SEQUENTIAL, then the old probe
        assert np.array_equal(trgb, rgb), s["tag"]
        n += 1
    assert n == sum(s["tag"].startswith("writer") for s in decoded["streams"]) and n >= 80


def test_probe_reports_levels_units_and_a_plan_size(decoded):
    from rpo_amd import _lib, jpeg
    for s, (rec, _) in zip(decoded["streams"], decoded["res"]):
        with pytest.raises(jpeg.JpegRefused) as e:
            jpeg.probe(s["file"])
        assert e.value.code == _lib.E_JPEG_PROGRESSIVE, s["tag"]     # the old probe keeps refusing them
        info = jpeg.probe(s["file"], progressive=True)
        g = PO.parse(s["file"])
        H, W = s["rgb"].shape[:2]
        units = 0
        for sc in g.scans:
            c = sc.comps[0]
            h, v = (g.h_samp, g.v_samp) if (c == 0 and g.components == 3) else (1, 1)
            total = g.mcus_x * g.mcus_y if len(sc.comps) > 1 else -(-(-(-W * h // g.h_samp)) // 8) * -(-(-(-H * v // g.v_samp)) // 8)
            units += -(-total // sc.ri) if sc.ri else 1
        assert (info.width, info.height, info.components, info.h_samp, info.v_samp, info.units, info.scan_offset) == \
            (W, H, g.components, g.h_samp, g.v_samp, units, g.scans[0].starts[0]), s["tag"]
        assert tuple(rec[2:11]) == (W, H, g.components, g.h_samp, g.v_samp, info.reserved, units, info.scan_offset, info.table_bytes)
        assert 1 <= info.reserved <= 14 and info.table_bytes % 16 == 0 and info.restart_interval == 0
        if s["tag"].startswith("pillow"):
            assert info.reserved == 3, s["tag"]
        if "Al = 13" in s["tag"]:
            assert info.reserved == 14
        if "spectral selection only" in s["tag"]:
            assert info.reserved == 1


def test_every_refusal_has_its_code(decoded):
    from rpo_amd import _lib, jpeg
    codes = set()
    for r, (rec, _) in zip(decoded["refused"], decoded["refused_res"]):
        assert rec[0] == r["code"], (r["tag"], rec[0])
        codes.add(r["code"])
        if r["code"] == _lib.E_JPEG_SEQUENTIAL:                       # probe(progressive=True) asks the old probe first,
            assert jpeg.probe(r["file"], progressive=True).reserved == 0   # which simply accepts a baseline file
            continue
        with pytest.raises(jpeg.JpegRefused) as e:
            jpeg.probe(r["file"], progressive=True)
        assert e.value.code == r["code"] and e.value.reason, r["tag"]
    assert codes == {_lib.E_JPEG_SCRIPT, _lib.E_JPEG_COMPONENTS, _lib.E_JPEG_ARITHMETIC, _lib.E_JPEG_SEQUENTIAL}


def test_corrupt_streams_end_in_their_exact_status_on_the_host(decoded):
    assert [s for _, _, s in decoded["corrupt"]][:4] == [1, 2, 3, 4]   # TRUNCATED, BAD_CODE, BAD_INDEX, NO_RESTART
    for (what, data, status), (rec, rgb) in zip(decoded["corrupt"], decoded["corrupt_res"]):
        assert rec[0] == 0 and rec[1] == status, (what, rec[:2])
        assert rgb.shape == (32, 32, 3)
        assert PO.decode_coefficients(data)[2] == status, what
        with pytest.raises(PO.Corrupt):
            PO.decode(data)


def test_every_header_prefix_is_probed_inside_its_own_bytes(decoded):
    """Each prefix sits in a heap buffer of exactly its size; the probe must answer (a code, no crash) from those bytes
    alone, and the same as the library's probe given the same bytes."""
    import ctypes
    from rpo_amd import _lib
    prefixes = header_prefixes(decoded["streams"])
    assert len(prefixes) > 1500
    res = run_host_program(decoded["exe"], prefixes, decoded["dir"], probe_only=True)
    lib = _lib.load()
    info = _lib.JpegInfo()
    accepted = 0
    for data, (rec, _) in zip(prefixes, res):
        assert rec[0] == lib.rpo_jpeg_prog_probe(data, len(data), ctypes.byref(info)), len(data)
        assert rec[0] in (0, _lib.E_JPEG_CORRUPT, _lib.E_JPEG_SCRIPT), (len(data), rec[0])
        accepted += rec[0] == 0
    assert accepted <= 3 * 14                                       # only prefixes that reach into the last scan are complete
