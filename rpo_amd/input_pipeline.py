"""On-device input transforms with the reference's configuration surface.

The reference names its transforms in `configs/trainers/RPO/main_K24.yaml:8-13`:

    INPUT.SIZE (224, 224) · INTERPOLATION "bicubic" · PIXEL_MEAN / PIXEL_STD (CLIP)
    TRANSFORMS ["random_resized_crop", "random_flip", "normalize"]

and Dassl (un-vendored) turns them into torchvision's `RandomResizedCrop`, `RandomHorizontalFlip`,
`ToTensor`, `Normalize` for training and `Resize(max(SIZE))`, `CenterCrop(SIZE)`, `ToTensor`, `Normalize` for
testing, each applied per sample on CPU workers (`DATALOADER.NUM_WORKERS: 16`, `:6`).  At MI355X step rates
(> 8 k images/s per GPU) that CPU path cannot keep up, so here the random decisions are drawn on the host and the
pixel work -- Pillow's 8-bit bicubic resample, flip, /255, normalise -- runs in `rpo_preprocess_batch`
(`rpo_amd/csrc/preprocess.hip`) on whole batches of decoded uint8 images, bit-identical to the CPU path.

    tf = build_transform(InputConfig(), is_train=True, device="cuda:0", max_batch=32)
    x = tf(list_of_uint8_HWC_arrays)            # -> float32 [B, 3, 224, 224] on the device

The HIP library is required; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
import random
from collections import defaultdict
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .ops import check

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)      # main_K24.yaml:11
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)      # main_K24.yaml:12


@dataclass
class InputConfig:
    """The `INPUT` node of the reference's yacs config (main_K24.yaml:8-13; RRCROP_SCALE is Dassl's default)."""
    SIZE: Tuple[int, int] = (224, 224)
    INTERPOLATION: str = "bicubic"
    PIXEL_MEAN: Tuple[float, float, float] = CLIP_MEAN
    PIXEL_STD: Tuple[float, float, float] = CLIP_STD
    TRANSFORMS: Tuple[str, ...] = ("random_resized_crop", "random_flip", "normalize")
    RRCROP_SCALE: Tuple[float, float] = (0.08, 1.0)


class TorchRng:
    """Draws from torch's global generator the way torchvision's transforms do (`torch.empty(1).uniform_`,
    `torch.randint`, `torch.rand(1)`), so seeding with `torch.manual_seed` gives torchvision's crop sequence."""

    def uniform(self, a: float, b: float) -> float:
        return torch.empty(1).uniform_(a, b).item()

    def randint(self, lo: int, hi: int) -> int:
        return int(torch.randint(lo, hi, size=(1,)).item())

    def rand(self) -> float:
        return torch.rand(1).item()


def random_resized_crop_params(height: int, width: int, rng, scale=(0.08, 1.0),
                               ratio=(3.0 / 4.0, 4.0 / 3.0)) -> Tuple[int, int, int, int]:
    """torchvision `RandomResizedCrop.get_params` -> (top, left, h, w): ten attempts at an area fraction in
    `scale` with a log-uniform aspect ratio, then the central-crop fallback."""
    area = height * width
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = area * rng.uniform(scale[0], scale[1])
        aspect = math.exp(rng.uniform(lo, hi))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= width and 0 < h <= height:
            i = rng.randint(0, height - h + 1)
            j = rng.randint(0, width - w + 1)
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def center_crop_window(height: int, width: int, size: int) -> Tuple[int, int, int, int]:
    """torchvision `Resize(size)` (shorter side -> size, `int()` truncation of the longer) followed by
    `CenterCrop(size)` -> (resize_w, resize_h, left, top)."""
    if width <= height:
        rw, rh = size, int(size * height / width)
    else:
        rh, rw = size, int(size * width / height)
    return rw, rh, int(round((rw - size) / 2.0)), int(round((rh - size) / 2.0))


@dataclass
class SamplePlan:
    """Everything random about one sample, decided on the host."""
    crop: Tuple[int, int, int, int]          # top, left, h, w
    resize: Tuple[int, int]                  # w, h
    window: Tuple[int, int]                  # left, top
    flip: bool


_I32_MIN, _I32_MAX = -2 ** 31, 2 ** 31 - 1
_DESC_I32_FIELDS = ("width", "height", "crop_x", "crop_y", "crop_w", "crop_h", "resize_w", "resize_h", "win_x", "win_y")


def _fill_desc(d, b: int, src_offset: int, height: int, width: int, pl: SamplePlan) -> None:
    """One `rpo_image_desc` from a plan.  ctypes stores a Python int into a `c_int32` field modulo 2^32 without a word,
    and a wrapped crop can pass the library's validation as another, valid crop: a number that does not fit its field
    is refused here, by name."""
    top, left, ch, cw = pl.crop
    vals = (width, height, left, top, cw, ch, pl.resize[0], pl.resize[1], pl.window[0], pl.window[1])
    if max(vals) > _I32_MAX or min(vals) < _I32_MIN:
        name, v = next((n, v) for n, v in zip(_DESC_I32_FIELDS, vals) if not _I32_MIN <= v <= _I32_MAX)
        raise ValueError(f"image {b}: {name} = {v} does not fit the int32 field of rpo_image_desc")
    if not 0 <= src_offset < 2 ** 63:
        raise ValueError(f"image {b}: src_offset = {src_offset} does not fit the int64 field of rpo_image_desc")
    d.src_offset = src_offset
    (d.width, d.height, d.crop_x, d.crop_y, d.crop_w, d.crop_h, d.resize_w, d.resize_h, d.win_x, d.win_y) = vals
    d.flip = int(pl.flip)


class DeviceTransform:
    """Batch transform: host plans + one packed H2D copy + `rpo_preprocess_batch`.

    Two pinned staging slots alternate so the copy of batch t+1 can be filled while batch t is in flight; the
    device buffers of a slot are reused only after the event recorded behind its kernels has completed."""

    def __init__(self, cfg: InputConfig, is_train: bool, device, max_batch: int = 32,
                 max_image_bytes: int = 3 * 1024 * 1024, rng=None):
        if cfg.INTERPOLATION != "bicubic":
            raise NotImplementedError("only INPUT.INTERPOLATION == 'bicubic' (main_K24.yaml:10) is implemented")
        unknown = set(cfg.TRANSFORMS) - {"random_resized_crop", "random_flip", "normalize"}
        if unknown:
            raise NotImplementedError(f"transforms not used by the RPO configs: {sorted(unknown)}")
        if cfg.SIZE[0] != cfg.SIZE[1]:
            raise NotImplementedError("square INPUT.SIZE only")
        if "normalize" not in cfg.TRANSFORMS:
            raise NotImplementedError("the RPO configs always normalise")
        self.cfg, self.is_train = cfg, is_train
        self.size = int(cfg.SIZE[0])
        self.dev = torch.device(device)
        self.max_batch = max_batch
        self.rng = rng if rng is not None else TorchRng()
        self.lib = _lib.load()
        self.mean = (ctypes.c_float * 3)(*cfg.PIXEL_MEAN)
        self.std = (ctypes.c_float * 3)(*cfg.PIXEL_STD)
        self.desc_bytes = (ctypes.sizeof(_lib.ImageDesc) * max_batch + 15) // 16 * 16
        self.cap = self.desc_bytes + max_batch * max_image_bytes
        self.slots = []
        for _ in range(2):
            self.slots.append({
                "host": torch.empty(self.cap, dtype=torch.uint8).pin_memory() if self.dev.type == "cuda"
                else torch.empty(self.cap, dtype=torch.uint8),
                "dev": torch.empty(self.cap, dtype=torch.uint8, device=self.dev),
                "ws": None, "done": None})
        self.turn = 0

    # ---- host-side decisions -----------------------------------------------------------------------------
    def plan(self, height: int, width: int) -> SamplePlan:
        S = self.size
        if self.is_train and "random_resized_crop" in self.cfg.TRANSFORMS:
            crop = random_resized_crop_params(height, width, self.rng, self.cfg.RRCROP_SCALE)
            resize, window = (S, S), (0, 0)
        else:                                   # test: Resize(max(SIZE)) + CenterCrop(SIZE)
            rw, rh, left, top = center_crop_window(height, width, S)
            crop, resize, window = (0, 0, height, width), (rw, rh), (left, top)
        flip = bool(self.is_train and "random_flip" in self.cfg.TRANSFORMS and self.rng.rand() < 0.5)
        return SamplePlan(crop, resize, window, flip)

    # ---- device work -------------------------------------------------------------------------------------
    def __call__(self, images: Sequence[np.ndarray], plans: Optional[Sequence[SamplePlan]] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        B, S = len(images), self.size
        if not 0 < B <= self.max_batch:
            raise ValueError(f"batch of {B} images, transform built for 1..{self.max_batch}")
        if plans is None:
            plans = [self.plan(im.shape[0], im.shape[1]) for im in images]
        descs = (_lib.ImageDesc * B)()          # the descriptors first: a bad image or plan raises with no slot touched
        off = self.desc_bytes
        offs = []
        max_rows, kmax = 1, 1
        for b, (im, pl) in enumerate(zip(images, plans)):
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("images must be uint8 arrays of shape [H, W, 3] (decoded RGB)")
            H, W = im.shape[:2]
            n = H * W * 3
            if off + n > self.cap:
                raise ValueError("staging buffer too small: raise max_image_bytes")
            _fill_desc(descs[b], b, off - self.desc_bytes, H, W, pl)
            ch, cw = pl.crop[2], pl.crop[3]
            max_rows = max(max_rows, ch)
            kmax = max(kmax, self.lib.rpo_preprocess_ksize(cw, pl.resize[0]),
                       self.lib.rpo_preprocess_ksize(ch, pl.resize[1]))
            offs.append(off)
            off += (n + 15) // 16 * 16
        slot = self.slots[self.turn]
        self.turn ^= 1
        if slot["done"] is not None:
            slot["done"].synchronize()          # the device side of this slot is free again
        host = slot["host"]
        hv = host.numpy()
        for im, o in zip(images, offs):
            hv[o:o + im.size] = np.ascontiguousarray(im).reshape(-1)
        ctypes.memmove(host.data_ptr(), descs, ctypes.sizeof(descs))
        need = self.lib.rpo_preprocess_workspace_bytes(B, S, max_rows, kmax)
        if slot["ws"] is None or slot["ws"].numel() < need:
            slot["ws"] = torch.empty(int(need * 1.25) + 1024, dtype=torch.uint8, device=self.dev)
        if out is None:
            out = torch.empty(B, 3, S, S, dtype=torch.float32, device=self.dev)
        assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (B, 3, S, S)
        dev = slot["dev"]
        dev[:off].copy_(host[:off], non_blocking=True)
        stream = torch.cuda.current_stream(self.dev)
        check(self.lib.rpo_preprocess_batch(dev.data_ptr() + self.desc_bytes, off - self.desc_bytes,
                                            ctypes.addressof(descs), dev.data_ptr(), B, S, max_rows, kmax,
                                            ctypes.addressof(self.mean), ctypes.addressof(self.std),
                                            out.data_ptr(), slot["ws"].data_ptr(), slot["ws"].numel(),
                                            stream.cuda_stream), "rpo_preprocess_batch")
        slot["done"] = torch.cuda.Event()
        slot["done"].record(stream)
        return out

    def _ksize(self, in_size: int, out_size: int) -> int:
        key = (in_size, out_size)
        k = self._ksize_cache.get(key)
        if k is None:
            k = self._ksize_cache[key] = self.lib.rpo_preprocess_ksize(in_size, out_size)
        return k

    def from_set(self, image_set: "DeviceImageSet", indices: Sequence[int],
                 plans: Optional[Sequence[SamplePlan]] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The same transform for images of a `DeviceImageSet`: the pixels are already on the device, so only the
        descriptors travel (a pinned slot pair of `desc_bytes` each).  `plan()` is called per image in batch order, as
        `__call__` does, so a seeded run draws the same crops.  Spilled images of the batch are staged into the set's
        tail behind the resident pixels and the whole batch is one `rpo_preprocess_batch` launch."""
        B, S = len(indices), self.size
        if not 0 < B <= self.max_batch:
            raise ValueError(f"batch of {B} images, transform built for 1..{self.max_batch}")
        if image_set.dev != self.dev:
            raise ValueError(f"the image set lives on {image_set.dev}, the transform on {self.dev}")
        indices = [int(i) for i in indices]
        if plans is None:
            plans = [self.plan(*image_set.sizes[i]) for i in indices]
        descs = (_lib.ImageDesc * B)()          # everything but src_offset: a bad plan raises with no buffer touched
        for b, (i, pl) in enumerate(zip(indices, plans)):
            _fill_desc(descs[b], b, 0, *image_set.sizes[i], pl)
        if getattr(self, "dslots", None) is None:
            self.dslots = [{"host": torch.empty(self.desc_bytes, dtype=torch.uint8).pin_memory(),
                            "dev": torch.empty(self.desc_bytes, dtype=torch.uint8, device=self.dev),
                            "ws": None, "done": None} for _ in range(2)]
            self.dturn = 0
            self._ksize_cache = {}
        slot = self.dslots[self.dturn]
        if slot["done"] is not None:
            slot["done"].synchronize()          # the descriptors of two calls ago have been read
        stream = torch.cuda.current_stream(self.dev)
        turn = self.dturn
        self.dturn ^= 1
        offsets = image_set.stage_spilled(indices, turn, stream)
        max_rows, kmax = 1, 1
        for b, pl in enumerate(plans):
            descs[b].src_offset = offsets[b]    # inside the set's buffer
            ch, cw = pl.crop[2], pl.crop[3]
            max_rows = max(max_rows, ch)
            kmax = max(kmax, self._ksize(cw, pl.resize[0]), self._ksize(ch, pl.resize[1]))
        nbytes = ctypes.sizeof(descs)
        ctypes.memmove(slot["host"].data_ptr(), descs, nbytes)
        need = self.lib.rpo_preprocess_workspace_bytes(B, S, max_rows, kmax)
        if slot["ws"] is None or slot["ws"].numel() < need:
            slot["ws"] = torch.empty(int(need * 1.25) + 1024, dtype=torch.uint8, device=self.dev)
        if out is None:
            out = torch.empty(B, 3, S, S, dtype=torch.float32, device=self.dev)
        assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (B, 3, S, S)
        slot["dev"][:nbytes].copy_(slot["host"][:nbytes], non_blocking=True)
        check(self.lib.rpo_preprocess_batch(image_set.buffer.data_ptr(), image_set.buffer.numel(),
                                            ctypes.addressof(descs), slot["dev"].data_ptr(), B, S, max_rows, kmax,
                                            ctypes.addressof(self.mean), ctypes.addressof(self.std),
                                            out.data_ptr(), slot["ws"].data_ptr(), slot["ws"].numel(),
                                            stream.cuda_stream), "rpo_preprocess_batch")
        slot["done"] = torch.cuda.Event()
        slot["done"].record(stream)
        image_set.tail_read(turn, slot["done"])
        return out


# ---- a few-shot set that lives on the device ------------------------------------------------------------------

def _align16(n: int) -> int:
    return (n + 15) // 16 * 16


@dataclass
class PackingPlan:
    """Where every image of a set goes: `offsets[i]` = byte offset in the packed buffer, or -1 for an image that
    stays on the host ("spilled"); `resident_bytes` = the packed pixels; `tail_bytes` = one of the two staging areas
    behind them, large enough for the spilled images of any batch of up to `max_batch` images."""
    offsets: List[int]
    resident_bytes: int
    tail_bytes: int

    @property
    def spilled(self) -> List[int]:
        return [i for i, o in enumerate(self.offsets) if o < 0]


def plan_packing(sizes: Sequence[Tuple[int, int]], budget_bytes: Optional[int] = None,
                 max_batch: int = 128) -> PackingPlan:
    """Pure host function.  Images are packed in order at 16-byte aligned offsets (as the staging path packs a batch);
    an image that would take the resident pixels beyond `budget_bytes` is spilled, later smaller ones may still fit.
    Offsets are Python ints: a set beyond 4 GiB is addressed through `rpo_image_desc.src_offset` (64 bit)."""
    offsets, off, spilled = [], 0, []
    for (H, W) in sizes:
        if H <= 0 or W <= 0:
            raise ValueError("empty image")
        n = _align16(int(H) * int(W) * 3)
        if budget_bytes is not None and off + n > budget_bytes:
            offsets.append(-1)
            spilled.append(n)
        else:
            offsets.append(off)
            off += n
    tail = sum(sorted(spilled, reverse=True)[:max_batch])
    return PackingPlan(offsets, off, tail)


class DeviceImageSet:
    """Decoded uint8 [H, W, 3] images of arbitrary sizes, uploaded once into one packed device buffer, and their
    labels (host list + one int64 device tensor).  `DeviceTransform.from_set(set, indices)` then reads the pixels where
    they are.  Images beyond `budget_bytes` stay on the host and are staged per batch into the buffer's tail:

        buffer = [ resident pixels | tail slot 0 | tail slot 1 ]

    The two tail slots alternate like the staging slots of `DeviceTransform`; a slot is refilled only after the event
    recorded behind the kernels that read it (`tail_read`) has completed."""

    CHUNK = 64 << 20                               # pinned upload chunk

    def __init__(self, images: Sequence[np.ndarray], labels: Sequence[int], device, budget_bytes: Optional[int] = None,
                 n_cls: Optional[int] = None, max_batch: int = 128):
        if len(images) != len(labels):
            raise ValueError(f"{len(images)} images, {len(labels)} labels")
        for im in images:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("images must be uint8 arrays of shape [H, W, 3] (decoded RGB)")
        self.dev = torch.device(device)
        if self.dev.type == "cuda" and self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        self.labels = [int(y) for y in labels]
        self.plan = plan_packing(self.sizes, budget_bytes, max_batch)
        if n_cls is not None:
            self.check_labels(n_cls)
        p = self.plan
        self.host_images = {i: np.ascontiguousarray(images[i]) for i in p.spilled}
        self.buffer = torch.empty(max(16, p.resident_bytes + 2 * p.tail_bytes), dtype=torch.uint8, device=self.dev)
        self.labels_dev = torch.tensor(self.labels, dtype=torch.int64, device=self.dev)
        self._tail = None                          # pinned host mirrors of the two tail slots + their events
        self._upload(images)

    def __len__(self) -> int:
        return len(self.sizes)

    @property
    def resident_bytes(self) -> int:
        return self.plan.resident_bytes

    def check_labels(self, n_cls: int) -> None:
        """F.cross_entropy raises on an out-of-range target; the head kernels cannot: checked once per set, where
        `parse_batch_train` checks once per batch."""
        if not self.labels:
            return
        lo, hi = min(self.labels), max(self.labels)
        if lo < 0 or hi >= n_cls:
            raise IndexError(f"Target {hi if hi >= n_cls else lo} is out of bounds "
                             f"(n_cls = {n_cls}; labels must be renumbered after the base/new split)")

    def _upload(self, images) -> None:
        p = self.plan
        if p.resident_bytes == 0:
            return
        cap = min(self.CHUNK, p.resident_bytes)
        cap = max(cap, max((_align16(h * w * 3) for (h, w), o in zip(self.sizes, p.offsets) if o >= 0), default=16))
        pinned = torch.empty(cap, dtype=torch.uint8).pin_memory()
        hv = pinned.numpy()
        start = fill = 0                           # the chunk holds buffer[start : start + fill]

        def flush():
            nonlocal start, fill
            if fill:
                self.buffer[start:start + fill].copy_(pinned[:fill], non_blocking=True)
                torch.cuda.current_stream(self.dev).synchronize()     # the chunk is reused
            start, fill = start + fill, 0

        with torch.cuda.device(self.dev):
            for im, off in zip(images, p.offsets):
                if off < 0:
                    continue
                n = im.size
                assert off == start + fill
                if fill + _align16(n) > cap:
                    flush()
                hv[fill:fill + n] = np.ascontiguousarray(im).reshape(-1)
                fill += _align16(n)
            flush()

    def stage_spilled(self, indices: Sequence[int], turn: int, stream) -> List[int]:
        """Byte offsets in `buffer` of the images `indices`, after copying the spilled ones among them into tail slot
        `turn` on `stream`."""
        p = self.plan
        offs = [p.offsets[i] for i in indices]
        if all(o >= 0 for o in offs):
            return offs
        if self._tail is None:
            self._tail = [{"host": torch.empty(p.tail_bytes, dtype=torch.uint8).pin_memory(), "done": None}
                          for _ in range(2)]
        slot = self._tail[turn]
        if slot["done"] is not None:
            slot["done"].synchronize()
        base = p.resident_bytes + turn * p.tail_bytes
        hv, fill = slot["host"].numpy(), 0
        for b, i in enumerate(indices):
            if offs[b] >= 0:
                continue
            flat = self.host_images[i].reshape(-1)
            if fill + flat.size > p.tail_bytes:
                raise ValueError("the batch's spilled images exceed the set's staging tail: raise max_batch")
            hv[fill:fill + flat.size] = flat
            offs[b] = base + fill
            fill += _align16(flat.size)
        with torch.cuda.stream(stream):
            self.buffer[base:base + fill].copy_(slot["host"][:fill], non_blocking=True)
        slot["busy"] = True
        return offs

    def tail_read(self, turn: int, event) -> None:
        """`event` completes behind the kernels that read what `stage_spilled` put into tail slot `turn`."""
        if self._tail is not None and self._tail[turn].pop("busy", False):
            self._tail[turn]["done"] = event

    @classmethod
    def from_jpeg(cls, files: Sequence, labels: Sequence[int], device, budget_bytes: Optional[int] = None,
                  n_cls: Optional[int] = None, max_batch: int = 128, fallback: Optional[Callable] = None,
                  chunk_images: int = 1024, progressive: bool = False) -> "DeviceImageSet":
        """The same set from JPEG files (`bytes`, or paths that are read here) without a host decode: Dassl's `read_image`
        (Pillow's `Image.open(path).convert("RGB")`) runs on the device (rpo_amd/jpeg.py), bit-identical to it.  Sizes
        come from the headers, so the packing plan is the one `DeviceImageSet(decoded)` computes.  Resident images are
        uploaded compressed and decoded straight into their offsets of `buffer`; spilled ones are decoded on the device
        in chunks and read back into `host_images`.  A file the device decoder refuses (progressive, CMYK, ...) goes
        through `fallback(bytes) -> uint8 [H, W, 3]` (default: Pillow, if importable) and is uploaded as pixels.
        `n_device` / `n_fallback` count the two routes; the set is otherwise indistinguishable from one built from
        decoded arrays.  `progressive=True` also decodes progressive files on the device (rpo_amd/jpeg.py: complete,
        consistent Huffman scan scripts); what its probe refuses too takes the fallback with that probe's reason."""
        from .jpeg import JpegCorrupt, JpegDecoder, JpegRefused, probe
        if len(files) != len(labels):
            raise ValueError(f"{len(files)} files, {len(labels)} labels")
        datas, names = [], []
        for i, f in enumerate(files):
            if isinstance(f, (bytes, bytearray, memoryview)):
                datas.append(bytes(f))
                names.append(f"file {i}")
            else:
                with open(f, "rb") as fh:
                    datas.append(fh.read())
                names.append(str(f))
        infos, decoded = [], {}
        for i, data in enumerate(datas):
            try:
                infos.append(probe(data, progressive))
            except JpegRefused as e:
                infos.append(None)
                if fallback is None:
                    try:
                        import io
                        from PIL import Image
                    except ImportError:
                        raise JpegRefused(e.code, f"{names[i]}: {e.reason}; no fallback decoder was given and Pillow is "
                                                  "not importable") from e
                    fallback = lambda b: np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))   # noqa: E731
                im = np.ascontiguousarray(fallback(data))
                if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                    raise ValueError(f"{names[i]}: fallback must return a uint8 array of shape [H, W, 3]")
                decoded[i] = im
        self = cls.__new__(cls)
        self.dev = torch.device(device)
        if self.dev.type == "cuda" and self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.sizes = [(int(decoded[i].shape[0]), int(decoded[i].shape[1])) if info is None
                      else (int(info.height), int(info.width)) for i, info in enumerate(infos)]
        self.labels = [int(y) for y in labels]
        self.plan = plan_packing(self.sizes, budget_bytes, max_batch)
        if n_cls is not None:
            self.check_labels(n_cls)
        p = self.plan
        self.n_fallback = len(decoded)
        self.n_device = len(datas) - self.n_fallback
        self.buffer = torch.empty(max(16, p.resident_bytes + 2 * p.tail_bytes), dtype=torch.uint8, device=self.dev)
        self.labels_dev = torch.tensor(self.labels, dtype=torch.int64, device=self.dev)
        self._tail = None
        self.host_images = {i: decoded[i] for i in p.spilled if i in decoded}
        dec = JpegDecoder(self.dev, chunk_images, progressive=progressive)
        with torch.cuda.device(self.dev):
            for i, im in decoded.items():           # refused files that are resident: uploaded as pixels, as in _upload
                if p.offsets[i] >= 0:
                    self.buffer[p.offsets[i]:p.offsets[i] + im.size].copy_(torch.from_numpy(im.reshape(-1)))
            res = [i for i, info in enumerate(infos) if info is not None and p.offsets[i] >= 0]
            st = dec.decode_into([datas[i] for i in res], self.buffer, [p.offsets[i] for i in res], [infos[i] for i in res],
                                 raise_corrupt=False)
            for k in np.flatnonzero(st):
                raise JpegCorrupt(res[k], int(st[k]))          # the index in `files`, not in the resident subset
            spill = [i for i, info in enumerate(infos) if info is not None and p.offsets[i] < 0]
            for lo in range(0, len(spill), chunk_images):
                part = spill[lo:lo + chunk_images]
                try:
                    buf, offs, _ = dec.decode([datas[i] for i in part])
                except JpegCorrupt as e:
                    raise JpegCorrupt(part[e.index], e.status) from None
                flat = buf.cpu().numpy()            # one read-back per chunk
                for i, o in zip(part, offs):
                    H, W = self.sizes[i]
                    self.host_images[i] = flat[o:o + H * W * 3].reshape(H, W, 3).copy()
        return self


def build_transform(cfg: InputConfig, is_train: bool, device, max_batch: int = 32, **kw) -> DeviceTransform:
    """Counterpart of Dassl's `build_transform(cfg, is_train)` for the choices the RPO configs make."""
    return DeviceTransform(cfg, is_train, device, max_batch, **kw)


# ---- few-shot sampling and the base / new class split ---------------------------------------------------------

@dataclass
class Datum:
    """Dassl's `Datum` as the reference uses it (datasets/oxford_pets.py:65-72, :176-180)."""
    impath: str
    label: int
    classname: str = ""


def subsample_classes(*datasets: Sequence[Datum], subsample: str = "all") -> List[List[Datum]]:
    """`OxfordPets.subsample_classes` (datasets/oxford_pets.py:140-186): sorted label set split at ceil(n/2);
    "base" keeps the first half, "new" the second, labels renumbered from 0."""
    if subsample not in ("all", "base", "new"):
        raise ValueError(subsample)
    if subsample == "all":
        return [list(d) for d in datasets]
    labels = sorted({item.label for item in datasets[0]})
    m = math.ceil(len(labels) / 2)
    selected = labels[:m] if subsample == "base" else labels[m:]
    relabel = {y: i for i, y in enumerate(selected)}
    return [[Datum(it.impath, relabel[it.label], it.classname) for it in d if it.label in relabel]
            for d in datasets]


def generate_fewshot_dataset(data: Sequence[Datum], num_shots: int, repeat: bool = False,
                             rng: Optional[random.Random] = None) -> List[Datum]:
    """Dassl `DatasetBase.generate_fewshot_dataset` as called at datasets/oxford_pets.py:44-45: group by label in
    first-seen order, `random.sample` num_shots per class (all of them, or sampling with replacement when
    `repeat`, if a class has fewer).  Dassl is un-vendored: restated from its published source, unpinned."""
    if num_shots < 1:
        return list(data)
    rng = rng if rng is not None else random
    tracker: Dict[int, List[Datum]] = defaultdict(list)
    for it in data:
        tracker[it.label].append(it)
    out: List[Datum] = []
    for _, items in tracker.items():
        if len(items) >= num_shots:
            out.extend(rng.sample(items, num_shots))
        elif repeat:
            out.extend(rng.choices(items, k=num_shots))
        else:
            out.extend(items)
    return out
