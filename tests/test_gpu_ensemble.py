"""Prompt ensembling on the GPU (rpo_amd/csrc/ensemble.hip, Engine.encode_text, rpo_amd.zeroshot.ZeroshotCLIP2): the two
kernels against float64 numpy, their bit-level contracts (split accumulation, aliasing, repeatability), `encode_text`
against the reference's per-template text features, and ZeroshotCLIP2 against the reference's own trainer
(tests/golden/ref_zsclip2_*.npz, tools/make_golden_zsclip2.py).  Depth-2 models, a few seconds in total."""
import functools
import os

import numpy as np
import pytest
import torch

from rpo_amd import ops, synth
from rpo_amd.config import rn_clip, vit_b16

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
TAGS = ("d2_b3", "d2_b3_imagenet", "rn_mini_b3")
# logits bounds: the project's plain-CLIP bounds (tests/test_gpu_model.py, plain CLIP against CLIP.forward) for the ViT
# cases, PLAIN_TOL["mini"] of tests/test_gpu_rn.py for the reduced ResNet
LOGIT_TOL = {"d2_b3": {"f32": 1e-3, "f16": 1e-2, "bf16": 0.12}, "d2_b3_imagenet": {"f32": 1e-3, "f16": 1e-2, "bf16": 0.12},
             "rn_mini_b3": {"f32": 1e-4, "f16": 8e-3, "bf16": 0.11}}
# rows whose reference top-1 / top-2 gap is within twice the bound are left out of the argmax check -- no more than these
# (gaps: d2_b3 0.73 0.20 0.39, d2_b3_imagenet 0.59 0.23 0.38, rn_mini_b3 0.30 0.30 0.29)
MAX_SKIPPED = {"d2_b3": {"f32": 0, "f16": 0, "bf16": 1}, "d2_b3_imagenet": {"f32": 0, "f16": 0, "bf16": 1},
               "rn_mini_b3": {"f32": 0, "f16": 0, "bf16": 0}}
GUARD = 32


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _gold(tag):
    return dict(np.load(os.path.join(GOLD, f"ref_zsclip2_{tag}.npz")))


@functools.lru_cache(maxsize=None)
def _workload(tag):
    """(cfg, state dict) of a fixture: the synthetic weights it was made with; of the token table only the rows any
    template uses."""
    rows = sorted(set(np.unique(np.concatenate([_gold(t)["tokens"].ravel() for t in TAGS])).tolist() + [49407]))
    if tag.startswith("rn"):
        cfg = rn_clip((1, 1, 1, 1), 64, 1024, layers_t=2)
        return cfg, synth.rn_clip_state_dict(cfg, seed=0, token_rows=rows, logit_scale=float(np.log(100.0)), check=False)
    cfg = vit_b16(layers_v=2, layers_t=2, K=1)
    return cfg, synth.clip_state_dict(cfg, seed=0, token_rows=rows, logit_scale=float(np.log(100.0)))


@functools.lru_cache(maxsize=None)
def _single(tag, mode):
    """Plain zero-shot CLIP on the LAST template of a fixture (OxfordPets: the dataset's own): what exists without ensembling."""
    from rpo_amd.zeroshot import ZeroshotCLIP
    return ZeroshotCLIP(_workload(tag)[1], _gold(tag)["tokens"][-1], DEV, DT[mode], max_batch=4)


@functools.lru_cache(maxsize=None)
def _ensemble(tag, mode):
    from rpo_amd.zeroshot import ZeroshotCLIP2
    return ZeroshotCLIP2(_workload(tag)[1], _gold(tag)["tokens"], DEV, DT[mode], max_batch=4)


def _images(tag, B=3):
    return torch.from_numpy(synth.images(_workload(tag)[0], B))


# ---- 1. the kernels against float64 ---------------------------------------------------------------------------------------

def _guarded(rows, e):
    whole = torch.full((rows * e + 2 * GUARD,), -7.0, dtype=torch.float32, device=DEV)
    return whole, whole[GUARD:GUARD + rows * e].view(rows, e)


def _guards_intact(whole, n):
    w = whole.cpu()
    return bool((w[:GUARD] == -7.0).all() and (w[GUARD + n:] == -7.0).all())


def _features(n, e, T, ld, stride, seed):
    """(device buffer [T * stride, ld] with NaN in every float the kernel must not read, its valid part as float64
    [T, n, e]): N(0, 1) times per-row scales log-uniform over 1e-3 .. 1e3."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((T, n, e)) * 10.0 ** rng.uniform(-3.0, 3.0, (T, n, 1))
    f = f.astype(np.float32)
    host = np.full((T, stride, ld), np.nan, dtype=np.float32)
    host[:, :n, :e] = f
    return torch.from_numpy(host.reshape(T * stride, ld)).to(DEV), f.astype(np.float64)


def _ensemble64(f):
    mean = (f / np.linalg.norm(f, axis=-1, keepdims=True)).sum(0) / f.shape[0]
    return mean / np.linalg.norm(mean, axis=-1, keepdims=True)


# (n_cls, e, T, ld - e, template_stride_rows - n_cls).  e % 4 != 0, an unaligned ld: the one-float-per-load element map.
KERNEL_CASES = [(1, 512, 1, 0, 0), (3, 72, 2, 0, 0), (19, 512, 8, 0, 0), (257, 1024, 3, 0, 0), (130, 640, 80, 0, 0),
                (19, 512, 8, 8, 3), (5, 77, 3, 0, 0), (3, 72, 2, 3, 1), (9, 1023, 2, 1, 0)]


@pytest.mark.parametrize("n,e,T,pad,gap", KERNEL_CASES)
def test_ensemble_kernels_against_float64(n, e, T, pad, gap):
    """Bound 1e-4 absolute on unit-norm outputs: the worst-case fp32 error of two norms over e <= 1024 terms and T <= 80
    sequential adds is about 2 (e / 2 + T + 4) 2^-24 ~ 7e-5."""
    ld, stride = e + pad, n + gap
    feat, f64 = _features(n, e, T, ld, stride, seed=1000 * n + e + T)
    before = bits(feat).clone()
    acc_w, acc = _guarded(n, e)
    out_w, out = _guarded(n, e)
    ops.text_ensemble_accumulate(feat[:, :e], n, acc, first=True, template_stride_rows=stride)
    ops.text_ensemble_finish(acc, T, out)
    got = out.cpu().numpy().astype(np.float64)
    err = np.abs(got - _ensemble64(f64)).max()
    print(f"[ensemble n={n} e={e} T={T} ld={ld} stride={stride}] max abs error {err:.3e}")
    assert err <= 1e-4
    s_err = np.abs(acc.cpu().numpy() - (f64 / np.linalg.norm(f64, axis=-1, keepdims=True)).sum(0)).max()
    # the running sum itself: T terms of magnitude <= 1, each off by at most (e / 2 + 2) 2^-24 relative (norm + division),
    # and T adds of partial sums <= T: T (e / 2 + T + 4) 2^-24 in the worst case
    assert s_err <= T * (e / 2 + T + 4) * 2.0 ** -24, s_err
    assert _guards_intact(acc_w, n * e) and _guards_intact(out_w, n * e)
    assert torch.equal(bits(feat), before), "the features (their padding included) are read-only"


# ---- 2. the bit-level contracts ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,e,pad", [(19, 512, 0), (19, 77, 0), (6, 1024, 4), (5, 72, 2)])
def test_split_accumulation_repeat_and_alias_give_the_same_bits(n, e, pad):
    T, T1 = 8, 3
    feat, _ = _features(n, e, T, e + pad, n, seed=77 + e)
    feat = feat[:, :e]
    one = ops.text_ensemble_accumulate(feat, n, torch.empty(n, e, device=DEV), first=True)
    again = ops.text_ensemble_accumulate(feat, n, torch.full((n, e), 3.0, device=DEV), first=True)
    assert torch.equal(bits(one), bits(again)), "two identical calls"
    split = ops.text_ensemble_accumulate(feat[:T1 * n], n, torch.empty(n, e, device=DEV), first=True)
    ops.text_ensemble_accumulate(feat[T1 * n:], n, split, first=False)
    assert torch.equal(bits(one), bits(split)), "3 templates, then the other 5"
    sep = ops.text_ensemble_finish(one, T, torch.empty(n, e, device=DEV))
    alias = ops.text_ensemble_finish(split, T)
    assert alias.data_ptr() == split.data_ptr()
    assert torch.equal(bits(sep), bits(alias)), "out aliasing acc"
    assert torch.equal(bits(sep), bits(ops.text_ensemble_finish(one, T, torch.empty(n, e, device=DEV))))


# ---- 3. encode_text against the reference -------------------------------------------------------------------------------------

def test_encode_text_matches_the_reference_per_template():
    """f32: every template's features within 1e-4 max(1, max |gold|) of the reference's `encode_text` (the bound of the
    plain-CLIP text features in tests/test_gpu_model.py), for the default chunk, a ragged chunking (152 prompts in
    chunks of 5) and chunks of one prompt; chunkings against each other under the same bound (the GEMM's tile choice
    may depend on the row count); the same call twice: the same bits."""
    g = _gold("d2_b3")
    m = _single("d2_b3", "f32")
    T, n, _ = g["tokens"].shape
    flat = g["tokens"].reshape(T * n, 77)
    ref = g["per_template_features"]
    bound = 1e-4 * max(1.0, float(np.abs(ref).max()))
    full = m.encode_text(flat)
    assert full.shape == (T * n, 512) and full.dtype == torch.float32 and full.is_cuda
    got = full.cpu().numpy().reshape(T, n, -1)
    for t in range(T):
        err = np.abs(got[t] - ref[t]).max()
        print(f"[encode_text f32] template {t}: max abs error {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (t, err)
    assert torch.equal(bits(full), bits(m.encode_text(flat))), "the same call twice"
    by5 = m.encode_text(flat, chunk=5)
    e5 = np.abs(by5.cpu().numpy().reshape(T, n, -1) - ref).max()
    by1 = m.encode_text(flat[:3], chunk=1)
    e1 = np.abs(by1.cpu().numpy() - ref[0, :3]).max()
    x5, x1 = (by5 - full).abs().max().item(), (by1 - full[:3]).abs().max().item()
    print(f"[encode_text f32] chunk 5: {e5:.3e}, chunk 1: {e1:.3e}; against the default chunk: {x5:.3e} / {x1:.3e}")
    assert e5 <= bound and e1 <= bound and x5 <= bound and x1 <= bound
    assert tuple(m.encode_text(flat[7:8]).shape) == (1, 512)


# ---- 4. encode_text leaves the engine alone -----------------------------------------------------------------------------------

def test_encode_text_leaves_zeroshot_and_rpo_state_alone():
    g = _gold("d2_b3")
    other = g["tokens"][:3].reshape(-1, 77)
    m = _single("d2_b3", "f16")
    image = _images("d2_b3")
    eng = m.engine
    before = m.model_inference(image)
    state = (eng.text_cache_ready, eng.text_f_version, eng.text_x_final.data_ptr(), eng.plain_text_f.data_ptr())
    kv = [bits(t).clone() for t in eng.kv_t]
    frozen, final, plain = bits(eng.text_x_frozen).clone(), bits(eng.text_x_final).clone(), bits(eng.plain_text_f).clone()
    m.encode_text(other, chunk=7)
    assert state == (eng.text_cache_ready, eng.text_f_version, eng.text_x_final.data_ptr(), eng.plain_text_f.data_ptr())
    assert all(torch.equal(a, bits(b)) for a, b in zip(kv, eng.kv_t))
    assert torch.equal(frozen, bits(eng.text_x_frozen)) and torch.equal(final, bits(eng.text_x_final))
    assert torch.equal(plain, bits(eng.plain_text_f))
    assert torch.equal(bits(before), bits(m.model_inference(image)))

    from rpo_amd.trainer import RPO
    cfg = vit_b16(layers_v=2, layers_t=2, K=8)
    sd = _workload("d2_b3")[1]
    tr = RPO(cfg, sd, g["tokens"][-1], device=DEV, act_dtype=torch.bfloat16, batch_size=4, prompts=synth.prompts(cfg, sd, seed=7))
    img = image.to(DEV)
    eval_before = tr.model_inference(img).clone()
    version = tr.engine.text_f_version
    feats = tr.engine.encode_text(other)
    ref = g["per_template_features"][:3].reshape(-1, 512)
    assert np.abs(feats.cpu().numpy() - ref).max() <= 0.05 * np.abs(ref).max()      # (bf16 towers: a sanity bound only)
    assert tr.engine.text_f_version == version
    assert torch.equal(bits(eval_before), bits(tr.model_inference(img)))


# ---- 5. ZeroshotCLIP2 against the reference's trainer ------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_zeroshotclip2_matches_the_reference_trainer(tag, mode):
    """Logits of ZeroshotCLIP2 against trainers/zsclip.py's ZeroshotCLIP2 (build_model + model_inference) under the plain-CLIP
    bounds; the single-template model on the same images is NOT the answer (the reference's ensemble differs from its
    last template alone by 4.07 / 3.28 / 3.61 in the three fixtures)."""
    g = _gold(tag)
    tol = LOGIT_TOL[tag][mode]
    image = _images(tag)
    m = _ensemble(tag, mode)
    assert m.n_templates == g["tokens"].shape[0] == {"d2_b3": 8, "rn_mini_b3": 8, "d2_b3_imagenet": 7}[tag]
    logits = m.model_inference(image).cpu().numpy()
    err = np.abs(logits - g["logits"]).max()
    print(f"[zsclip2 {tag} {mode}] logits err {err:.3e} (bound {tol})")
    assert err <= tol, f"{tag} {mode}: logits differ from the reference by {err:.3e} (bound {tol})"
    srt = np.sort(g["logits"], axis=1)
    decided = (srt[:, -1] - srt[:, -2]) > 2 * tol
    assert (~decided).sum() <= MAX_SKIPPED[tag][mode], (~decided).sum()
    assert (logits.argmax(1)[decided] == g["logits"].argmax(1)[decided]).all()
    single = _single(tag, mode).model_inference(image).cpu().numpy()
    away = np.abs(single - g["logits"]).max()
    print(f"[zsclip2 {tag} {mode}] one template alone is {away:.3f} away")
    assert away > min(10 * tol, 0.5)
    assert tuple(m.text_features.shape) == g["text_features"].shape and m.text_features.is_cuda
    ferr = np.abs(m.text_features.cpu().numpy() - g["text_features"]).max()
    print(f"[zsclip2 {tag} {mode}] text_features err {ferr:.3e}")
    if mode == "f32":
        assert ferr <= 1e-4
    assert np.array_equal(m.model_inference(image).cpu().numpy(), logits)


# ---- 6. the override's life cycle ---------------------------------------------------------------------------------------------

def test_text_feature_override_life_cycle():
    g = _gold("d2_b3")
    m = _single("d2_b3", "f16")
    image = _images("d2_b3")
    m.set_text_features(None)
    base = m.model_inference(image)
    m.set_text_features(g["text_features"])
    over = m.model_inference(image)
    assert np.abs(over.cpu().numpy() - g["logits"]).max() <= 1e-2            # the reference's classifier: its logits
    assert (over - base).abs().max().item() > 0.5
    with torch.cuda.device(m.engine.dev):
        m.engine.cache_text_kv()                                             # forced: the override stays
    assert torch.equal(bits(over), bits(m.model_inference(image)))
    m.set_text_features(None)
    assert torch.equal(bits(base), bits(m.model_inference(image)))
    with pytest.raises(AssertionError, match="features"):
        m.set_text_features(g["text_features"][:5])
    with pytest.raises(NotImplementedError, match="template"):
        _ensemble("d2_b3", "f16").set_context(np.zeros((4, 512), np.float32))


# ---- 7. test() ------------------------------------------------------------------------------------------------------------------

def test_zeroshotclip2_test_reports_model_inference_accuracy(capsys):
    from rpo_amd.input_pipeline import DeviceImageSet, InputConfig, build_transform
    m = _ensemble("d2_b3", "f16")
    n, bs, C = 7, 4, 19
    rng = np.random.default_rng(61)
    sizes = [(260, 300), (224, 224), (97, 260), (301, 97), (60, 40), (230, 231), (256, 192)]
    imgs = [rng.integers(0, 256, (*sizes[i], 3), dtype=np.uint8) for i in range(n)]
    stage = build_transform(InputConfig(SIZE=(224, 224)), False, DEV, bs)
    pred = np.concatenate([torch.max(m.model_inference(stage(imgs[b0:b0 + bs])).float().cpu(), 1)[1].numpy()
                           for b0 in range(0, n, bs)])
    labels = [int(p) if i % 2 == 0 else int((p + 1) % C) for i, p in enumerate(pred)]   # 4 of 7 right by construction
    res = m.test(DeviceImageSet(imgs, labels, DEV), batch_size=bs)
    assert res["total"] == n and res["correct"] == 4 and res["accuracy"] == 100.0 * 4 / n
    assert f"* accuracy: {100.0 * 4 / n:.1f}%" in capsys.readouterr().out
