"""JPEG files decoded on the device (include/rpo_amd.h `rpo_jpeg_*`, rpo_amd/csrc/jpeg.hip).

The reference reads its datasets through Dassl's `read_image`, i.e. Pillow's `Image.open(path).convert("RGB")`, one file at
a time on CPU workers.  Here the header of each file is parsed on the host (C++ inside the library), the compressed bytes
and the derived tables travel to the device, and entropy decode, IDCT, chroma upsampling and colour conversion run there
for whole chunks of files of mixed sizes and modes.  `probe` accepts baseline, 8-bit, gray or YCbCr at 4:4:4 / 4:2:2 /
4:2:0, any restart interval, any table ids and segment packing.  Files it refuses raise `JpegRefused` with the library's
reason; `DeviceImageSet.from_jpeg` routes those through a host decoder.

Progressive files (SOF2, Huffman coded, 8-bit, the same components / sampling / colour rules) are decoded on the device too
when `progressive=True` is given to `probe`, `JpegDecoder` and `DeviceImageSet.from_jpeg`; the default is off, and then they
are refused as before.  The host walks all scans of such a file, checks that the scan script is consistent and complete
(DESIGN.md 9f lists the rules; incomplete or inconsistent scripts, which libjpeg smooths or only warns about, stay with the
host decoder, as do arithmetic-coded files) and uploads a per-file plan; the device zeroes the coefficient blocks, runs one
entropy kernel per dependency level of the script (Pillow's ten-scan script has three) and then the same IDCT and colour
kernels, so the pixels are those of the baseline file of the same coefficients.  A chunk's baseline and progressive files
go through their two library calls into the same output buffer.  How large a share of the reference's datasets is
progressive has not been measured by this project.

What is tested (tests/golden/jpeg_streams.npz): the pixels are bit-identical to Pillow's for coefficient
blocks an encoder can produce from 8-bit samples, at any quantiser (1..255) and with any valid Huffman tables.  Outside
that domain -- header-valid streams no encoder writes: dense coefficients at dequantised amplitudes of 1020 and more, AC
magnitudes of category 11..15, a DC predictor run past int16 -- the decode is still defined and deterministic and equals
the numpy oracle (32-bit sums wrap), but may differ from Pillow, which clamps narrower intermediates: 0-7 of 1024 pixels at
amplitude 1020, about a third at 4080, half and more beyond (the table in 9f).  Pillow itself refuses files wider or
higher than 65500; the device decodes up to 65535.

    dec = JpegDecoder("cuda:0")
    info = dec.probe(data)                        # width / height / components / sampling ... or JpegRefused
    buffer, offsets, sizes = dec.decode(files)    # uint8 device buffer; image i = buffer[offsets[i]:][:H*W*3] as [H, W, 3]

The HIP library is required; there is no CPU fallback for the supported files.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import JpegDesc, JpegInfo, check

STATUS_NAMES = {0: "ok", 1: "scan truncated", 2: "invalid Huffman code", 3: "coefficient run leaves the block",
                4: "restart marker missing"}                       # include/rpo_amd.h RPO_JPEG_*


class JpegRefused(ValueError):
    """`rpo_jpeg_probe` does not accept the file; `code` is the RPO_E_JPEG_* value, `reason` its text."""

    def __init__(self, code: int, reason: str):
        super().__init__(f"{reason} (code {code})")
        self.code, self.reason = code, reason


class JpegCorrupt(RuntimeError):
    """The header was fine, the entropy-coded data was not: `index` in the decoded sequence, `status` from the device."""

    def __init__(self, index: int, status: int):
        super().__init__(f"JPEG {index}: corrupt entropy-coded data, device status {status} "
                         f"({STATUS_NAMES.get(status, 'unknown')})")
        self.index, self.status = index, status


def _align16(n: int) -> int:
    return (n + 15) // 16 * 16


def probe(data: bytes, progressive: bool = False) -> JpegInfo:
    """Host only (no GPU): the header of one file, or `JpegRefused`.  With `progressive`, a file refused as progressive is
    walked by `rpo_jpeg_prog_probe`; what that accepts has `info.reserved` (its number of dependency levels) > 0, what it
    refuses raises with its reason."""
    lib = _lib.load()
    info = JpegInfo()
    data = bytes(data)
    rc = lib.rpo_jpeg_probe(data, len(data), ctypes.byref(info))
    if rc == _lib.E_JPEG_PROGRESSIVE and progressive:
        rc = lib.rpo_jpeg_prog_probe(data, len(data), ctypes.byref(info))
    if rc != 0:
        msg = lib.rpo_error_string(int(rc))
        raise JpegRefused(int(rc), msg.decode() if msg else str(rc))
    return info


class JpegDecoder:
    """Chunked batch decode.  Two pinned staging slots alternate, as in `DeviceTransform`: chunk t+1 is packed on the host
    while chunk t is in flight; a slot is reused only after the event recorded behind its kernels has completed."""

    def __init__(self, device, chunk_images: int = 1024, chunk_bytes: int = 256 << 20, progressive: bool = False):
        if not 0 < chunk_images <= 65535:
            raise ValueError("chunk_images must be in 1..65535")
        self.dev = torch.device(device)
        if self.dev.type == "cuda" and self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.chunk_images, self.chunk_bytes, self.progressive = int(chunk_images), int(chunk_bytes), bool(progressive)
        self.lib = _lib.load()
        self.slots = [{"host": None, "dev": None, "done": None} for _ in range(2)]
        self.turn = 0
        self.ws = None

    def probe(self, data: bytes) -> JpegInfo:
        return probe(data, self.progressive)

    # ---- one chunk ---------------------------------------------------------------------------------------------
    def _slot(self, need: int):
        slot = self.slots[self.turn]
        self.turn ^= 1
        if slot["done"] is not None:
            slot["done"].synchronize()              # the device side of this slot is free again
        if slot["host"] is None or slot["host"].numel() < need:
            cap = int(need * 1.25) + 4096
            slot["host"] = torch.empty(cap, dtype=torch.uint8).pin_memory()
            slot["dev"] = torch.empty(cap, dtype=torch.uint8, device=self.dev)
        return slot

    def _chunk(self, files, infos, out: torch.Tensor, offsets) -> torch.Tensor:
        """Enqueues the decode of `files` into out[offsets[i]:]; returns the chunk's int32 status tensor (device), in file
        order.  Baseline files (info.reserved == 0) and progressive ones go through their own library call, one behind the
        other on the stream, out of the same staging slot and workspace."""
        n = len(files)
        groups = [[i for i in range(n) if infos[i].reserved == 0], [i for i in range(n) if infos[i].reserved != 0]]
        calls = [(self.lib.rpo_jpeg_tables, self.lib.rpo_jpeg_workspace_bytes, self.lib.rpo_jpeg_decode_batch, "rpo_jpeg"),
                 (self.lib.rpo_jpeg_prog_plan, self.lib.rpo_jpeg_prog_workspace_bytes, self.lib.rpo_jpeg_prog_decode_batch,
                  "rpo_jpeg_prog")]
        descs = [(JpegDesc * max(len(g), 1))() for g in groups]
        desc_bytes = _align16(n * ctypes.sizeof(JpegDesc))
        off, need_ws = desc_bytes, 0
        for g, ds, (_, ws_bytes, _, name) in zip(groups, descs, calls):
            for k, i in enumerate(g):
                d = ds[k]
                d.info = infos[i]
                d.file_offset, d.file_bytes = off - desc_bytes, len(files[i])
                off += _align16(len(files[i]))
                d.table_offset = off - desc_bytes
                off += _align16(int(infos[i].table_bytes))
                d.out_offset = int(offsets[i])
            if g:
                need = ws_bytes(ds, len(g))
                if need == 0:
                    raise ValueError("inconsistent JPEG descriptors (were the infos produced by probe()?)")
                need_ws = max(need_ws, need)
        slot = self._slot(off)
        host, dev = slot["host"], slot["dev"]
        hv, base = host.numpy(), host.data_ptr() + desc_bytes
        at = 0
        for g, ds, (tables, _, _, name) in zip(groups, descs, calls):
            for k, i in enumerate(g):
                d = ds[k]
                fo = desc_bytes + d.file_offset
                hv[fo:fo + len(files[i])] = np.frombuffer(files[i], np.uint8)
                check(tables(base + d.file_offset, len(files[i]), base + d.table_offset, int(d.info.table_bytes)), name + "_tables")
            ctypes.memmove(host.data_ptr() + at, ds, len(g) * ctypes.sizeof(JpegDesc))
            at += len(g) * ctypes.sizeof(JpegDesc)
        if self.ws is None or self.ws.numel() < need_ws:
            self.ws = torch.empty(int(need_ws) + 4096, dtype=torch.uint8, device=self.dev)
        status = torch.empty(n, dtype=torch.int32, device=self.dev)
        stream = torch.cuda.current_stream(self.dev)
        dev[:off].copy_(host[:off], non_blocking=True)
        at = 0
        for g, ds, (_, _, decode, name) in zip(groups, descs, calls):
            if g:
                check(decode(dev.data_ptr() + desc_bytes, off - desc_bytes, ctypes.addressof(ds),
                             dev.data_ptr() + at * ctypes.sizeof(JpegDesc), len(g), out.data_ptr(), out.numel(),
                             self.ws.data_ptr(), self.ws.numel(), status.data_ptr() + 4 * at, stream.cuda_stream),
                      name + "_decode_batch")
            at += len(g)
        if groups[0] and groups[1]:                     # grouped order -> file order
            ordered = torch.empty_like(status)
            ordered[torch.tensor(groups[0] + groups[1], device=self.dev)] = status
            status = ordered
        slot["done"] = torch.cuda.Event()
        slot["done"].record(stream)
        return status

    # ---- public ------------------------------------------------------------------------------------------------
    def decode_into(self, files: Sequence[bytes], out: torch.Tensor, offsets: Sequence[int],
                    infos: Optional[Sequence[JpegInfo]] = None, raise_corrupt: bool = True) -> np.ndarray:
        """Decodes files[i] to packed RGB uint8 [H, W, 3] at out[offsets[i]:], in chunks of at most `chunk_images` files /
        `chunk_bytes` compressed bytes.  Returns, after the device has finished, the per-file device status (int32, 0 =
        decoded); raises `JpegCorrupt` for the first file whose entropy-coded data was bad unless `raise_corrupt` is off
        (the other files are decoded all the same)."""
        if out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.dev:
            raise ValueError(f"out must be a contiguous uint8 tensor on {self.dev}")
        if infos is None:
            infos = [probe(f, self.progressive) for f in files]
        if not (len(files) == len(offsets) == len(infos)):
            raise ValueError("files, offsets and infos differ in length")
        statuses, lo = [], 0
        with torch.cuda.device(self.dev):
            while lo < len(files):
                hi, nbytes = lo, 0
                while hi < len(files) and hi - lo < self.chunk_images and (hi == lo or nbytes + len(files[hi]) <= self.chunk_bytes):
                    nbytes += len(files[hi])
                    hi += 1
                statuses.append(self._chunk(files[lo:hi], infos[lo:hi], out, offsets[lo:hi]))
                lo = hi
            if not statuses:
                return np.zeros(0, np.int32)
            st = torch.cat(statuses).cpu().numpy()          # synchronises the stream
        bad = np.flatnonzero(st)
        if bad.size and raise_corrupt:
            raise JpegCorrupt(int(bad[0]), int(st[bad[0]]))
        return st

    def decode(self, files: Sequence[bytes]) -> Tuple[torch.Tensor, List[int], List[Tuple[int, int]]]:
        """-> (buffer, offsets, sizes): one packed device buffer, 16-byte aligned offsets, (H, W) per file."""
        infos = [probe(f, self.progressive) for f in files]
        sizes = [(int(i.height), int(i.width)) for i in infos]
        offsets, off = [], 0
        for (H, W) in sizes:
            offsets.append(off)
            off += _align16(H * W * 3)
        buffer = torch.empty(max(off, 16), dtype=torch.uint8, device=self.dev)
        self.decode_into(files, buffer, offsets, infos)
        return buffer, offsets, sizes
