"""The plain text tower keeps the bits of the commit before its block loop, backward chain and attention row body were
folded into one each (rpo_amd/engine_text.py, rpo_amd/csrc/attn_text.hip).  `bits(case)` runs one case on seeded
CPU-generated inputs and returns sha256 hashes of its outputs; tools/capture_text_tower_bits.py recorded them with the
parent's Python and library on the device type the suite runs on (tests/golden/text_tower_parent_bits.json), twice in
separate processes with equal results.  Every later tree is held to those hashes: the kernels launched, their order, their
arguments and every output bit stay as they were."""
import functools
import hashlib
import json
import os
import struct

import numpy as np
import pytest
import torch

import test_gpu_class_sets as TC
import test_gpu_coop_prefix as TP
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

DEV = TP.DEV
DT = TP.DT
PARENT_BITS = os.path.join(GOLDEN, "text_tower_parent_bits.json")
H = 2                                           # op level: two heads
LENS = [5, 80, 66, 64, 20]                      # keys on both sides of lane 64, one class far short of Lmax
PREFIX_CASES = ["smallest", "L80", "three_images", "max_prefix"]

OP_KINDS = ["fwd_causal", "fwd_bwd_rows", "fwd_bwd_rows_shared", "bwd_dense"] + [f"prefix_{n}" for n in PREFIX_CASES]
CASES = [f"op_{k}_{m}" for k in OP_KINDS for m in TP.MODES] + \
        [f"step_{k}_{m}" for k in ("coop_dense", "coop_shared", "cocoop_dense", "cocoop_shared", "coop_middle", "coop_csc")
         for m in ("bf16", "f32")] + \
        [f"fwd_{k}_{m}" for k in ("encode_text", "class_set_rpo", "class_set_coop", "conditional_class_set", "cache_text_kv")
         for m in ("bf16", "f32")]


def sha(t) -> str:
    if not isinstance(t, torch.Tensor):
        return hashlib.sha256(struct.pack("<d", float(t))).hexdigest()
    t = t.detach().contiguous()
    raw = t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def _packed(rows, d, mode, seed):
    qkv = TP.rnd((rows, 3 * d), seed)
    qkv[:, :d] *= 1.5                           # sharper softmax rows
    return qkv.to(DEV, DT[mode])


def _lens(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def _op_bits(kind, mode):
    from rpo_amd import ops
    d = 64 * H
    dt = DT[mode]
    zeros = lambda r, c=d: torch.zeros(r, c, dtype=dt, device=DEV)
    if kind == "fwd_causal":
        L, n = 80, len(LENS)
        t, out = _packed(n * L, d, mode, 301), zeros(n * L)
        ops.text_attn_fwd(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], out, _lens(LENS), n, L, L, H, causal=True, scale=0.125)
        return dict(out=sha(out))
    if kind in ("fwd_bwd_rows", "fwd_bwd_rows_shared"):
        # 16-bit: Lmax 100 is past what the MFMA kernel of csrc/attn_image.hip takes (96), so the VALU kernel runs
        L, rows = (80 if mode == "f32" else 100), 3
        lens = [5, L, 66, 64, 20]
        n_kv = 2 if kind.endswith("shared") else len(lens)
        n = 4 if kind.endswith("shared") else len(lens)
        cache = _packed(n_kv * L, d, mode, 302)
        q, da = _packed(n * rows, d, mode, 303), TP.rnd((n * rows, d), 304).to(DEV, dt)
        out, dq = zeros(n * rows), zeros(n * rows)
        kc, vc, ln = cache[:, d:2 * d], cache[:, 2 * d:], _lens(lens[:n_kv])
        if kind.endswith("shared"):
            ops.text_attn_fwd_shared(q[:, :d], kc, vc, out, ln, n, n_kv, rows, L, H, 0.125)
            ops.text_attn_bwd_shared(q[:, :d], kc, vc, da, dq, ln, n, n_kv, rows, L, H, 0.125)
        else:
            ops.text_attn_fwd(q[:, :d], kc, vc, out, ln, n, rows, L, H, causal=False, scale=0.125)
            ops.text_attn_bwd(q[:, :d], kc, vc, da, dq, ln, n, rows, L, H, 0.125)
        return dict(out=sha(out), dq=sha(dq))
    if kind == "bwd_dense":
        L, n = 80, len(LENS)
        t, g = _packed(n * L, d, mode, 305), zeros(n * L, 3 * d)
        dout = torch.zeros(n * L, d + 96)       # d_out: [:, 32:32 + d] of a wider buffer
        dout[:, 32:32 + d] = TP.rnd((n * L, d), 306)
        dout = dout.to(DEV, dt)
        ops.text_attn_bwd_dense(t[:, :d], t[:, d:2 * d], t[:, 2 * d:], dout[:, 32:32 + d], g[:, :d], g[:, d:2 * d],
                                g[:, 2 * d:], _lens(LENS), n, L, H, 0.125)
        return dict(g=sha(g))
    Hc, n_img, P, S, lens = TP.OP_CASES[kind[len("prefix_"):]]
    dc = 64 * Hc
    qkv, dout = TP._op_inputs(kind[len("prefix_"):])
    t, do_w = qkv.to(DEV, dt), dout.to(DEV, dt)
    out, g = zeros(t.shape[0], dc), zeros(t.shape[0], 3 * dc)
    ops.text_attn_fwd_prefix(t[:, :dc], t[:, dc:2 * dc], t[:, 2 * dc:], out, _lens(lens), n_img, len(lens), P, S, Hc, 0.125)
    ops.text_attn_bwd_prefix(t[:, :dc], t[:, dc:2 * dc], t[:, 2 * dc:], do_w[:, 32:32 + dc], g[:, :dc], g[:, dc:2 * dc],
                             g[:, 2 * dc:], _lens(lens), n_img, len(lens), P, S, Hc, 0.125)
    return dict(out=sha(out), g=sha(g))


def _csc_trainer(mode, B):
    """`TP._trainer("coop", ...)` with class-specific contexts: a seeded context per class (the helper's is generic)."""
    from rpo_amd.coop import CoOp
    _, sd = TP._d2()
    toks = TP._gold("coop_d2_b3_ctx4")["tokenized_prompts"]
    ctx = TP.rnd((toks.shape[0], 4, sd["positional_embedding"].shape[1]), 307, 0.02).numpy()
    return CoOp(sd, toks, 4, TP._optim(), DEV, DT[mode], batch_size=B, num_batches=10 ** 9, ctx=ctx, csc=True)


def _step_bits(kind, mode):
    B = 2 if kind.startswith("cocoop") else 3
    if kind == "coop_csc":
        tr = _csc_trainer(mode, B)
    elif kind == "coop_middle":
        tr = TP._trainer("coop", mode, False, B, class_token_position="middle")
    else:
        tr = TP._trainer(kind.split("_")[0], mode, kind.endswith("shared"), B)
    out = {}
    for step in range(2):
        loss = tr.forward_backward(TP._batch(B, step))["loss"]
        out.update({f"loss{step}": sha(loss), f"logits{step}": sha(tr.engine.logits[:B]),
                    f"params{step}": sha(tr.engine.coop_params)})
    return out


@functools.lru_cache(maxsize=None)
def _new_tokens():
    return dict(np.load(os.path.join(GOLDEN, "ref_classset_coop_end.npz")))["tokens"]


def _forward_bits(kind, mode):
    image = TP._batch(3, 5)["img"].to(DEV)
    if kind == "encode_text":
        eng = TC._engine(mode)
        toks = TC.synth.synthetic_tokens(eng.cfg, [9, 31, 3, 69, 12], seed=308)
        return dict(features=sha(eng.encode_text(toks, chunk=2)))
    if kind == "class_set_rpo":
        tr = TC._rpo(mode)
        return dict(logits=sha(tr.model_inference(TC._image(), classes=tr.class_set(TC.gold("rpo")["tokens"]))))
    if kind == "cache_text_kv":
        eng = TC._rpo(mode).engine
        eng.cache_text_kv()
        return dict(kv=sha(eng.kv_t[-1]))
    if kind == "class_set_coop":
        tr = TP._trainer("coop", mode, False, 3)
        return dict(logits=sha(tr.model_inference(image, classes=tr.class_set(_new_tokens()))))
    tr = TP._trainer("cocoop", mode, False, 2)
    tr.model.prompt_learner.eval()
    P, Lmax = 1 + 4, int((_new_tokens().argmax(-1) + 1).max())
    # a row budget that holds 2 images x 4 of the 18 classes per pass: the last class chunk is a short one
    ccs = tr.conditional_class_set(_new_tokens(), images_per_pass=2, row_budget=2 * (P + 4 * (Lmax - P)))
    assert ccs.classes_per_pass == 4 < ccs.n
    return dict(logits=sha(tr.model_inference(image, classes=ccs)))


def bits(case: str) -> dict:
    level, rest = case.split("_", 1)
    kind, mode = rest.rsplit("_", 1)
    got = {"op": _op_bits, "step": _step_bits, "fwd": _forward_bits}[level](kind, mode)
    torch.cuda.synchronize()
    return got


@functools.lru_cache(maxsize=None)
def _recorded():
    return json.load(open(PARENT_BITS))


@pytest.mark.parametrize("case", CASES)
def test_text_tower_keeps_the_parents_bits(case):
    rec = _recorded()
    assert case in rec["bits"], f"{case} has no recorded hashes (tools/capture_text_tower_bits.py)"
    got = bits(case)
    diff = [k for k in rec["bits"][case] if got.get(k) != rec["bits"][case][k]]
    assert set(got) == set(rec["bits"][case]) and not diff, f"{case}: {diff} differ from the parent commit's bits"
