"""The image tower's attention (rpo_amd/csrc/attn_image.hip) keeps the bits of the commit before its forward kernels were
folded onto one V^T staging, one key walk and one output store, and their build-time A/B arms removed.  `bits(case)` runs
one case on seeded CPU-generated inputs (test_gpu_attn_long.make_qkv: queries x 1.5, NaN in the K / V columns of the prompt
rows; every buffer inside a NaN-filled allocation; outputs pre-filled with NaN, so a hash also pins which rows are NOT
written) and returns sha256 hashes.  tools/capture_attn_bits.py --image recorded them with a library built from the parent
commit on the device type the suite runs on (tests/golden/image_attn_parent_bits.json), twice in separate processes with
equal results.  Every later tree is held to those hashes: kernel selection by shape and every output bit stay as they were.
The backward cases beyond the first six were added, and recorded the same way, with the library of the commit before the
backward kernels were put on one pass-2 tile step and one launcher; the 77 earlier hashes came out unchanged."""
import functools
import hashlib
import json
import os

import pytest
import torch

import test_gpu_attn_long as TL
import test_gpu_ops as TO
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

PARENT_BITS = os.path.join(GOLDEN, "image_attn_parent_bits.json")
MODES = TL.MODES
HALF = ["bf16", "f16"]

# rpo_attn_readonly_fwd_rows, (N, B, H, Kp, q_first).  One-barrier kernel (attn_fwd_kernel): base shape; the last block's
# form (whole query tiles skipped, leading queries of the first tile computed and not stored); no full key tile; one full
# key tile and a partial one; rem == 0 with tiles past N skipped; nfull == NT and S = 264 (a wave takes a second query
# tile); NT = 9; NT = 9 with full tiles only; NT = 9 with q_first inside a tile
FWD = [(197, 2, 3, 24, 0), (197, 2, 2, 24, 197), (5, 1, 1, 0, 0), (50, 1, 2, 7, 0), (192, 1, 2, 4, 0), (224, 1, 2, 40, 0),
       (257, 1, 2, 33, 0), (288, 1, 2, 1, 0), (225, 1, 2, 24, 225)]
# Two-phase kernel (attn_fwd16_kernel: 16-bit, N <= 224, more (image, head) units than CUs), (N, Kp, q_first) at H = 12 and
# B = CUs // 12 + 1: base shape; last block's form; second query tile after barrier B; three full tiles (phase B holds only
# the partial tile); no full tile in either phase
FWD_2PHASE = [(197, 24, 0), (197, 24, 197), (224, 40, 0), (100, 3, 0), (5, 0, 0)]
# Long kernel: just over the chunk limit; one key in the last chunk; ViT-L/14 at 336 px, last block's form
FWD_LONG = [(289, 1, 2, 24, 0), (513, 1, 1, 1, 0), (577, 1, 2, 24, 577)]
# rpo_attn_prompt_fwd / rpo_attn_prompt_bwd, (N, B, H, Kp, sets, first): first None = no pointer, "dev1" = device scalar 1
# over 3 cached images ([3 N, 2 d] K | V), 0 = device scalar 0
PFWD = [(197, 2, 2, 24, 1, None), (197, 2, 2, 5, 3, "dev1"), (257, 1, 2, 33, 2, 0), (5, 1, 1, 1, 1, None),
        (224, 1, 2, 24, 12, None)]                                  # the last: Q = 288, nine query tiles
# the added three: smallest problem; Q = 288 (a wave takes a second query tile and reloads qf / df); NT = 9 full
PBWD = [(197, 2, 2, 5, 3, "dev1"), (257, 1, 2, 33, 2, 0), (5, 1, 1, 1, 1, None), (224, 1, 2, 24, 12, None),
        (288, 1, 1, 1, 1, None)]
# rpo_attn_readonly_bwd, (N, B, H, Kp).  Base shape, NT = 9, the long backward; then: only tile 0 holds keys (waves 1 to 3
# keep (-inf, 0)); one full tile plus a one-key tile; four full tiles, one per wave; NT = 7 full with two query tiles through
# the in-kernel loop; four query tiles (the entry point's maximum); NT = 9 smallest and full; long kernel: two full chunks
# and two workgroups per head, one key in the last chunk (three waves skip it), ViT-L/14 at 336 px, the limit
BWD = [(197, 2, 3, 24), (257, 1, 2, 33), (289, 1, 2, 24),
       (5, 1, 1, 1), (33, 1, 2, 7), (128, 1, 2, 32), (224, 1, 2, 40), (50, 1, 1, 128), (225, 1, 2, 24), (288, 1, 2, 1),
       (512, 1, 1, 33), (513, 1, 1, 1), (577, 1, 2, 24), (1025, 1, 1, 1)]
# rpo_attn_readonly_bwd_proj, bf16 and f16 (the folded out-proj, NCW = H / 4).  Base shape (NCW = 3); NCW = 2 and 4 at
# NT = 7; NT = 9 with each NCW (the middle one has Kp > 32: two workgroups per (image, head)); the Kp limit; only tile 0
# holds keys; NT = 9 full
BWD_PROJ = [(197, 2, 12, 24), (197, 1, 8, 24), (197, 1, 16, 24), (257, 1, 8, 5), (257, 1, 12, 33), (257, 1, 16, 24),
            (224, 1, 12, 64), (5, 1, 12, 1), (288, 1, 8, 32)]


def _id(kind, mode, p):
    return f"{kind}_{mode}_" + "_".join(str(x) for x in p)


SPECS = {}
for _m in MODES:
    SPECS.update({_id("fwd", _m, p): ("fwd", _m, p) for p in FWD + FWD_LONG})
    SPECS.update({_id("pfwd", _m, p): ("pfwd", _m, p) for p in PFWD})
    SPECS.update({_id("pbwd", _m, p): ("pbwd", _m, p) for p in PBWD})
    SPECS.update({_id("bwd", _m, p): ("bwd", _m, p) for p in BWD})
for _m in HALF:
    SPECS.update({_id("fwd2phase", _m, p): ("fwd2phase", _m, p) for p in FWD_2PHASE})
    SPECS.update({_id("bwdproj", _m, p): ("bwdproj", _m, p) for p in BWD_PROJ})
CASES = list(SPECS)


def sha(t) -> str:
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _prompt_inputs(mode, N, B, H, Kp, sets, first, seed):
    """(q rows, k, v, first_image) of one multi-set launch: K / V in the packed in-proj layout, or in a 3-image cache"""
    d = 64 * H
    q, _ = TL.put(TO.rnd((sets * B * Kp, d), seed) * 1.5, mode)
    if first == "dev1":
        kv, _ = TL.put(TO.rnd((3 * N, 2 * d), seed + 1), mode)
        return q, kv[:, :d], kv[:, d:], torch.tensor([1], dtype=torch.int32, device=TL.dev())
    t, _ = TL.put(TL.make_qkv(B, H, N, Kp, seed + 1), mode)
    fi = None if first is None else torch.tensor([first], dtype=torch.int32, device=TL.dev())
    return q, t[:, d:2 * d], t[:, 2 * d:], fi


def bits(case: str) -> dict:
    kind, mode, p = SPECS[case]
    o, dt = TO.ops(), TL.DT[mode]
    if kind in ("fwd", "fwd2phase"):
        if kind == "fwd2phase":
            (N, Kp, q_first), H = p, 12
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            B = cus // H + 1
            assert B * H > cus and N <= 224, "this case must take the two-phase kernel"
        else:
            N, B, H, Kp, q_first = p
        t, _ = TL.put(TL.make_qkv(B, H, N, Kp, 51), mode)
        out, whole = TL.run_fwd(t, B, H, N, Kp, mode, q_first=q_first)
        got = dict(out=sha(out))
    elif kind in ("pfwd", "pbwd"):
        N, B, H, Kp, sets, first = p
        q, k, v, fi = _prompt_inputs(mode, N, B, H, Kp, sets, first, 53)
        out, whole = TL.guarded(sets * B * Kp, 64 * H, dt)
        if kind == "pfwd":
            o.attn_prompt_fwd(q, k, v, out, B, H, N, Kp, sets, first_image=fi)
        else:
            da, _ = TL.put(TO.rnd((sets * B * Kp, 64 * H), 55), mode)
            o.attn_prompt_bwd(q, k, v, da, out, B, H, N, Kp, sets, first_image=fi)
        got = dict(out=sha(out))
    else:
        N, B, H, Kp = p
        d, Rf = 64 * H, B * N
        t, _ = TL.put(TL.make_qkv(B, H, N, Kp, 57, sharp=1.0), mode)
        da, _ = TL.put(TO.rnd((B * Kp, d), 58), mode)
        if kind == "bwd":
            out, whole = TL.run_bwd(t, da, B, H, N, Kp, mode)
        else:
            w_t, _ = TL.put(TO.rnd((d, d), 59, d ** -0.5), mode)
            out, whole = TL.guarded(B * Kp, d, dt)
            o.attn_readonly_bwd_proj(t[Rf:, :d], t[:Rf, d:2 * d], t[:Rf, 2 * d:], da, w_t, out, B, H, N, Kp)
        got = dict(out=sha(out))
    torch.cuda.synchronize()
    assert TL.guards_intact(whole), "a guard element was overwritten"
    return got


@functools.lru_cache(maxsize=None)
def _recorded():
    return json.load(open(PARENT_BITS))


@pytest.mark.parametrize("case", CASES)
def test_image_attention_keeps_the_parents_bits(case):
    rec = _recorded()
    assert case in rec["bits"], f"{case} has no recorded hashes (tools/capture_attn_bits.py --image)"
    got = bits(case)
    assert got == rec["bits"][case], f"{case}: differs from the parent commit's bits"
