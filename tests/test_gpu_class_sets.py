"""Class sets on the GPU (rpo_amd/class_set.py, rpo_text_embed): the embedding kernel bit for bit
against the host expression, `encode_text` with the device and the host gather, a class set of the engine's own tokens
against the built-in path bit for bit, the 18 Oxford-Pets new classes against the reference's fixtures
(tests/golden/ref_classset_*.npz) for RPO / CoOp / zero-shot / LP, edge sets against the oracles, what class-set
evaluation leaves untouched, the evaluators, and the refusals.  Depth 2, ViT-B/16 widths, K = 8, B <= 3."""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import BF16_LOGIT_ATOL, F16_LOGIT_ATOL, GOLDEN, TOL_F32, workload
from rpo_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MODES = ["f32", "bf16", "f16"]
BOUND = {"f32": TOL_F32, "bf16": BF16_LOGIT_ATOL, "f16": F16_LOGIT_ATOL}
TAG = "d2_k8_b3"
GUARD = 64


def bound(mode, tokens=0):
    """The mode's logit bound; the 16-bit bounds doubled above 64 tokens, as tests/test_gpu_model.py does at 71."""
    return BOUND[mode] * (2.0 if (tokens > 64 and mode != "f32") else 1.0)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def gold(name):
    return dict(np.load(os.path.join(GOLDEN, f"ref_classset_{name}.npz")))


def _image():
    return torch.from_numpy(workload(TAG)[5]).to(DEV)


def _set_prompts(eng, tp, ip):
    eng.text_prompt.copy_(torch.from_numpy(tp))
    eng.img_prompt.copy_(torch.from_numpy(ip))
    eng.params_version += 1


@functools.lru_cache(maxsize=None)
def _engine(mode):
    """An RPO engine on the 19 base classes with the workload's prompts, max_batch 3."""
    from rpo_amd.engine import Engine
    cfg, sd, toks, tp, ip, _, _ = workload(TAG)
    eng = Engine(cfg, sd, toks, torch.device(DEV), DT[mode], max_batch=3)
    _set_prompts(eng, tp, ip)
    return eng


@functools.lru_cache(maxsize=None)
def _oracle_rpo(key):
    """OracleRPO eval logits [3, n'] on the edge set `key` with the workload's prompts (mode independent: computed once)."""
    from oracle.rpo_oracle import OracleRPO
    cfg, sd, _, tp, ip, image, _ = workload(TAG)
    m = OracleRPO(sd, EDGE_TOKENS(key), cfg.K, cfg.patch)
    m.set_prompts(tp, ip)
    with torch.no_grad():
        return m.forward(image).logits.numpy()


@functools.lru_cache(maxsize=None)
def _oracle_plain(key):
    from oracle.rpo_oracle import plain_clip_forward
    cfg, sd, _, _, _, image, _ = workload(TAG)
    with torch.no_grad():
        return plain_clip_forward(sd, image, EDGE_TOKENS(key), cfg.patch)[0].numpy()


# edge sets (synth.synthetic_tokens): name -> (lengths, chunk).  K = 8: the longest RPO prompt has 77 - 8 = 69 tokens; the
# engine's own Lmax is that of the 19 base prompts (14 at most)
EDGES = {
    "one": ([10], None),                                            # n' = 1
    "ragged9": ([5, 9, 12, 7, 20, 6, 11, 8, 15], 4),                # chunks 4, 4, 1; Lmax' above the engine's
    "short_long": ([3, 69], None),                                  # the shortest and the longest that fits, in one set
    "below": ([5, 4, 5, 3], None),                                  # Lmax' below the engine's
    "forty": ([4 + (7 * c) % 13 for c in range(40)], 16),           # larger than cfg.n_cls (40 against 19); chunks 16, 16, 8
}


def EDGE_TOKENS(key):
    cfg = workload(TAG)[0]
    return synth.synthetic_tokens(cfg, EDGES[key][0], seed=500 + len(EDGES[key][0]))


# ============================================================================================ 1. rpo_text_embed

def _host_embed(ids, table, pos, ctx, L):
    """The host expression: table[id] + pos[p] (ctx[-1 - id] + pos[p] for an id < 0), torch on the CPU, fp32."""
    idl = ids[:, :L].long()
    rows = table[idl.clamp(min=0)]
    if ctx is not None:
        rows = torch.where((idl < 0).unsqueeze(-1), ctx[(-1 - idl).clamp(min=0)], rows)
    return (rows + pos[None, :L]).reshape(-1, table.shape[1])


def _guarded(n):
    whole = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _guards_nan(whole):
    w = whole.cpu()
    return bool(torch.isnan(w[:GUARD]).all() and torch.isnan(w[-GUARD:]).all())


@pytest.mark.parametrize("n,L,d", [(1, 1, 512), (19, 20, 512), (257, 77, 512), (3, 77, 768)])
def test_text_embed_equals_the_host_expression_bit_for_bit(n, L, d):
    """ld_ids = 77 whatever L; ids 0 and vocab - 1 occur; the ids at positions >= L are far outside the vocabulary and must
    not be read (nor anything written for them: the guards around `out` stay NaN); a second launch gives the same bits."""
    from rpo_amd import ops
    vocab = 1000
    g = torch.Generator().manual_seed(1000 * n + L + d)
    table = torch.randn(vocab, d, generator=g) * 0.02
    pos = torch.randn(77, d, generator=g) * 0.01
    ids = torch.randint(0, vocab, (n, 77), generator=g, dtype=torch.int32)
    ids[0, 0] = vocab - 1
    ids[-1, L - 1] = 0
    if n > 1:
        ids[1, 0] = 0
        ids[n // 2, L - 1] = vocab - 1
    ids[:, L:] = 2 ** 30
    whole, flat = _guarded(n * L * d)
    out = flat.view(n * L, d)
    ops.text_embed(ids.to(DEV), table.to(DEV), pos.to(DEV), out, L)
    torch.cuda.synchronize()
    want = _host_embed(ids, table, pos, None, L)
    assert same(out, want), f"max diff {float((out.cpu() - want).abs().max()):.3e}"
    assert _guards_nan(whole)
    whole2, flat2 = _guarded(n * L * d)
    ops.text_embed(ids.to(DEV), table.to(DEV), pos.to(DEV), flat2.view(n * L, d), L)
    assert same(flat2, flat) and _guards_nan(whole2)


@pytest.mark.parametrize("n_ctx", [4, 16])
@pytest.mark.parametrize("position", ["end", "middle", "front"])
def test_text_embed_context_slots(position, n_ctx):
    """Negative ids: slot -1 - id of `ctx`, placed by the layout rule for every class-token position; names of 1 token and
    of the longest that fits."""
    from rpo_amd import ops
    from rpo_amd.engine_coop import coop_layout_of
    d, vocab = 512, 1000
    lens = np.array([n_ctx + 4, 77, n_ctx + 9, 40])
    L = 77
    g = torch.Generator().manual_seed(77 + n_ctx)
    table, pos, ctx = torch.randn(vocab, d, generator=g), torch.randn(77, d, generator=g), torch.randn(n_ctx, d, generator=g)
    toks = torch.randint(0, vocab, (4, L), generator=g, dtype=torch.int32).numpy()
    src, cp = coop_layout_of(lens, n_ctx, position, L)
    ids = np.take_along_axis(toks, np.maximum(src, 0), 1).astype(np.int32)
    np.put_along_axis(ids, cp, (-1 - np.arange(n_ctx, dtype=np.int32))[None, :], 1)
    assert (ids < 0).sum() == 4 * n_ctx
    ids = torch.from_numpy(ids)
    whole, flat = _guarded(4 * L * d)
    out = flat.view(4 * L, d)
    ops.text_embed(ids.to(DEV), table.to(DEV), pos.to(DEV), out, L, ctx=ctx.to(DEV))
    torch.cuda.synchronize()
    assert same(out, _host_embed(ids, table, pos, ctx, L)) and _guards_nan(whole)
    # context vector j sits where the layout says, for every class
    o = out.cpu().view(4, L, d)
    for c in range(4):
        for j in range(n_ctx):
            assert torch.equal(o[c, cp[c, j]], ctx[j] + pos[cp[c, j]])


def test_text_embed_refuses_bad_arguments_and_launches_nothing():
    from rpo_amd import _lib
    lib = _lib.load()
    n, L, d, vocab = 3, 20, 512, 100
    table = torch.zeros(vocab, d, device=DEV)
    pos = torch.zeros(77, d, device=DEV)
    ids = torch.zeros(n, 77, dtype=torch.int32, device=DEV)
    whole, flat = _guarded(n * L * d + 4)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda out, L_, d_, ld=77: lib.rpo_text_embed(ids.data_ptr(), ld, table.data_ptr(), vocab, pos.data_ptr(), None, 0,
                                                         out, n, L_, d_, s)
    assert call(flat.data_ptr(), L, 510) == _lib.E_SHAPE
    assert call(flat.data_ptr() + 4, L, d) == _lib.E_ALIGN                      # misaligned `out`
    assert call(flat.data_ptr(), 21, d, ld=20) == _lib.E_SHAPE                  # L > ld_ids
    torch.cuda.synchronize()
    assert bool(torch.isnan(whole).all()), "a refused call wrote something"
    assert call(flat.data_ptr(), L, d) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(flat[:n * L * d]).any()) and bool(torch.isnan(flat[n * L * d:]).all())


# ============================================================================================ 2. encode_text

@pytest.mark.parametrize("mode", MODES)
def test_encode_text_device_gather_equals_host_gather(mode, monkeypatch):
    """300 prompts of mixed length, chunks of 256 and of 7: the same bits with and without RPO_TEXT_EMBED_HOST=1."""
    eng = _engine(mode)
    cfg = eng.cfg
    lens = [3 + (11 * i) % 40 for i in range(300)]
    lens[5], lens[299] = 77 - cfg.K, 3
    toks = synth.synthetic_tokens(cfg, lens, seed=321)
    for chunk in (256, 7):
        monkeypatch.delenv("RPO_TEXT_EMBED_HOST", raising=False)
        dev = eng.encode_text(toks, chunk).clone()
        monkeypatch.setenv("RPO_TEXT_EMBED_HOST", "1")
        host = eng.encode_text(toks, chunk).clone()
        assert tuple(dev.shape) == (300, cfg.embed) and bool(torch.isfinite(dev).all())
        assert same(dev, host), f"chunk {chunk}: max diff {float((dev - host).abs().max()):.3e}"
    assert eng.hbm_bytes() >= eng._tok_emb_dev.numel() * 4              # (the table is counted)


# ============================================================================================ 3. identity

@pytest.mark.parametrize("mode", MODES)
def test_class_set_of_the_engines_own_tokens_is_the_built_in_path_bit_for_bit(mode):
    eng = _engine(mode)
    cfg, _, toks, *_ = workload(TAG)
    image = _image()
    cs = eng.class_set(toks)
    assert (cs.n, cs.Lmax) == (cfg.n_cls, eng.Lmax)
    ref = eng.forward_eval(image).clone()
    ref_eager = eng.forward_eval(image, use_graph=False).clone()
    got = eng.forward_eval(image, classes=cs).clone()
    assert same(cs.x_frozen, eng.text_x_frozen), "rpo_text_embed != the host's make_prompts rows"
    for l in range(cfg.layers_t):
        assert torch.equal(cs.kv_t[l].view(torch.int16) if mode != "f32" else cs.kv_t[l].view(torch.int32),
                           eng.kv_t[l].view(torch.int16) if mode != "f32" else eng.kv_t[l].view(torch.int32)), f"K / V of block {l}"
    assert same(cs.text_f, eng.text_f), "the prompt-row pass under the buffer swap != engine.text_f"
    assert same(got, ref) and same(ref, ref_eager)
    eager = eng.forward_eval(image, use_graph=False, classes=cs).clone()
    replay = eng.forward_eval(image, classes=cs).clone()
    assert same(eager, ref) and same(replay, ref), "graph replay != eager launches"
    plain = eng.forward_plain(image).clone()
    assert same(eng.forward_plain(image, classes=cs), plain)
    assert got.data_ptr() != ref.data_ptr() and cs.logits.data_ptr() != eng.logits.data_ptr()


# ============================================================================================ 4. the reference fixtures

def _report(what, mode, got, ref, lim):
    err = float(np.abs(got - ref).max())
    print(f"\n[class set {what} {mode}] worst logits err vs the reference {err:.3e} (bound {lim})")
    assert np.isfinite(got).all() and err <= lim, f"{what} {mode}: {err:.3e} > {lim}"


@pytest.mark.parametrize("mode", MODES)
def test_new_classes_rpo_against_the_reference(mode):
    eng, g = _engine(mode), gold("rpo")
    cs = eng.class_set(g["tokens"])
    got = eng.forward_eval(_image(), classes=cs)
    assert tuple(got.shape) == (3, 18)
    _report("RPO", mode, got.cpu().numpy(), g["logits"], bound(mode))


@pytest.mark.parametrize("mode", MODES)
def test_new_classes_zeroshot_against_the_reference(mode):
    from rpo_amd.zeroshot import ZeroshotCLIP
    cfg, sd, toks, *_ = workload(TAG)
    g = gold("zeroshot")
    zs = ZeroshotCLIP(sd, toks, DEV, DT[mode], max_batch=3)
    cs = zs.class_set(g["tokens"])
    _report("zero-shot", mode, zs.model_inference(_image(), classes=cs).cpu().numpy(), g["logits"], bound(mode))
    # ... and through the evaluator-facing path of an RPO engine (forward_plain on any ViT engine)
    eng = _engine(mode)
    _report("zero-shot (RPO engine)", mode, eng.forward_plain(_image(), classes=eng.class_set(g["tokens"])).cpu().numpy(),
            g["logits"], bound(mode))


@pytest.mark.parametrize("position", ["end", "middle"])
@pytest.mark.parametrize("mode", MODES)
def test_new_classes_coop_against_the_reference(mode, position):
    """A CoOp trainer built on the 19 base classes ("X X X X name." ids), the reference's context, evaluated on the 18 new
    classes' ids: the context goes where the layout rule puts it for THEIR name lengths."""
    from rpo_amd.coop import CoOp
    cfg, sd, toks, *_ = workload(TAG)
    g = gold(f"coop_{position}")
    tr = CoOp(sd, synth.coop_tokens(toks, 4), n_ctx=4, device=DEV, act_dtype=DT[mode], batch_size=3, ctx=g["ctx"],
              class_token_position=position)
    cs = tr.class_set(g["tokens"])
    got = tr.model_inference(_image(), classes=cs)
    _report(f"CoOp {position}", mode, got.cpu().numpy(), g["logits"], bound(mode))
    base = tr.model_inference(_image())
    assert tuple(base.shape) == (3, 19) and tuple(got.shape) == (3, 18)


@pytest.mark.parametrize("mode", MODES)
def test_new_classes_lp_against_the_reference(mode):
    from lp_fixtures import c1_init
    from rpo_amd.lp import LP
    cfg, sd, toks, *_ = workload(TAG)
    g = gold("lp")
    base = dict(np.load(os.path.join(GOLDEN, "ref_lp_d2_b3.npz")))["tokenized_prompts"]
    w, b = c1_init(cfg.embed)
    tr = LP(sd, base, device=DEV, act_dtype=DT[mode], batch_size=3, weight=w, bias=b, max_batch=3)
    cs = tr.class_set(g["tokens"])
    got = tr.model_inference(_image(), classes=cs)
    _report("LP", mode, got.cpu().numpy(), g["logits"], bound(mode))
    assert tuple(got.shape) == (3, 18) and tuple(tr.model_inference(_image()).shape) == (3, 19)


# ============================================================================================ 5. edge sets

@pytest.mark.parametrize("key", list(EDGES))
@pytest.mark.parametrize("mode", MODES)
def test_edge_sets_against_the_oracle(mode, key):
    eng = _engine(mode)
    lens, chunk = EDGES[key]
    toks = EDGE_TOKENS(key)
    cs = eng.class_set(toks, chunk=chunk)
    assert (cs.n, cs.Lmax) == (len(lens), max(lens))
    lim = bound(mode, max(lens) + eng.cfg.K)
    got = eng.forward_eval(_image(), classes=cs).clone()
    ref = _oracle_rpo(key)
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print(f"\n[edge set {key} {mode}] n' {cs.n} Lmax' {cs.Lmax} (engine {eng.Lmax}): RPO logits err {err:.3e} (bound {lim})")
    assert tuple(got.shape) == (3, len(lens)) and err <= lim
    if key in ("ragged9", "short_long"):
        errp = float(np.abs(eng.forward_plain(_image(), classes=cs).cpu().numpy() - _oracle_plain(key)).max())
        print(f"[edge set {key} {mode}] plain logits err {errp:.3e}")
        assert errp <= lim


@pytest.mark.parametrize("mode", MODES)
def test_permuting_the_classes_permutes_the_columns(mode):
    eng = _engine(mode)
    toks = EDGE_TOKENS("ragged9")
    perm = np.array([4, 0, 8, 2, 6, 1, 7, 3, 5])
    a = eng.forward_eval(_image(), classes=eng.class_set(toks, chunk=4)).clone()
    b = eng.forward_eval(_image(), classes=eng.class_set(toks[perm], chunk=4)).clone()
    err = float((a[:, perm] - b).abs().max())
    print(f"\n[permutation {mode}] worst difference {err:.3e}")
    assert err <= bound(mode) and not same(a, b)


# ============================================================================================ 6. state

def _rpo(mode):
    from rpo_amd.trainer import RPO
    cfg, sd, toks, tp, ip, _, _ = workload(TAG)
    return RPO(cfg, sd, toks, None, DEV, DT[mode], batch_size=3, num_batches=10 ** 9, prompts=(tp, ip))


@pytest.mark.parametrize("mode", MODES)
def test_class_set_evaluation_leaves_the_engine_and_the_training_untouched(mode):
    from oracle.rpo_oracle import OracleRPO
    cfg, sd, toks, tp, ip, image_np, label_np = workload(TAG)
    image, label = _image(), torch.from_numpy(label_np).to(DEV)
    tr, twin = _rpo(mode), _rpo(mode)
    eng = tr.engine
    for t in (tr, twin):
        t.step_async(image, label)                                   # (step 0 captures the graphs)
    torch.cuda.synchronize()
    before = tr.model_inference(image)
    twin.model_inference(image)
    new_t, edge_t = gold("rpo")["tokens"], EDGE_TOKENS("ragged9")
    cs_a, cs_b = tr.class_set(new_t), tr.class_set(edge_t, chunk=4)
    a1 = tr.model_inference(image, classes=cs_a)
    b1 = tr.model_inference(image, classes=cs_b)
    a2 = tr.model_inference(image, classes=cs_a)
    b2 = tr.model_inference(image, classes=cs_b)
    assert same(a1, a2) and same(b1, b2) and tuple(a1.shape) == (3, 18) and tuple(b1.shape) == (3, 9)
    assert same(eng.logits[:3], before), "a class-set head wrote the built-in logits buffer"
    assert same(tr.model_inference(image), before), "the built-in classes' logits moved"
    text_f_before = cs_a.text_f.clone()
    # the next train step: a twin that never saw a class set
    la, lb = tr.step_async(image, label).clone(), twin.step_async(image, label).clone()
    torch.cuda.synchronize()
    assert same(la, lb) and same(eng.grads, twin.engine.grads) and same(eng.params, twin.engine.params)
    # ... after which the class sets follow the new prompts
    a3 = tr.model_inference(image, classes=cs_a)
    m = OracleRPO(sd, new_t, cfg.K, cfg.patch)
    m.set_prompts(eng.text_prompt.cpu().numpy(), eng.img_prompt.cpu().numpy())
    with torch.no_grad():
        ref = m.forward(image_np).logits.numpy()
    err = float(np.abs(a3.cpu().numpy() - ref).max())
    print(f"\n[after a step {mode}] class-set logits err vs the oracle on the stepped prompts {err:.3e} (bound {bound(mode)}); "
          f"moved by {float((a3 - a1).abs().max()):.3e}")
    assert err <= bound(mode) and not same(a3, a1)
    assert not same(cs_a.text_f, text_f_before), "stale text_f after a step"
    assert same(tr.model_inference(image, classes=cs_b), tr.model_inference(image, classes=cs_b)) and not same(
        tr.model_inference(image, classes=cs_b), b1)


@pytest.mark.parametrize("mode", MODES)
def test_class_set_follows_set_context(mode):
    """ZeroshotCLIP.set_context (generic context, class token at the end): a class set made BEFORE the call follows it."""
    from rpo_amd.zeroshot import ZeroshotCLIP
    cfg, sd, toks, *_ = workload(TAG)
    g = gold("coop_end")
    zs = ZeroshotCLIP(sd, synth.coop_tokens(toks, 4), DEV, DT[mode], max_batch=3)
    cs = zs.class_set(g["tokens"])
    plain = zs.model_inference(_image(), classes=cs)
    zs.set_context(g["ctx"])
    got = zs.model_inference(_image(), classes=cs)
    _report("set_context", mode, got.cpu().numpy(), g["logits"], bound(mode))
    assert not same(got, plain)
    zs.set_context(2.0 * g["ctx"])
    assert not same(zs.model_inference(_image(), classes=cs), got)


# ============================================================================================ 7. evaluators

def _image_set(n, seed, C):
    from rpo_amd.input_pipeline import DeviceImageSet
    from test_gpu_loop import _decoded
    imgs = _decoded(n, seed)
    labels = np.random.default_rng(seed + 1).integers(0, C, n).tolist()
    labels[0] = C - 1
    return DeviceImageSet(imgs, labels, DEV), imgs, labels


@pytest.mark.parametrize("mode", MODES)
def test_test_on_a_class_set_equals_the_host_evaluator(mode):
    from rpo_amd.evaluator import Classification, base_to_new, harmonic_mean
    from rpo_amd.frozen_kv import FrozenImageKV
    from test_gpu_loop import _staging
    tr = _rpo(mode)
    cs = tr.class_set(gold("rpo")["tokens"])
    n = 7
    ds, imgs, labels = _image_set(n, 91, cs.n)
    res = tr.test(ds, verbose=False, classes=cs)
    stage = _staging(False, 3)
    logits = torch.cat([tr.model_inference(stage(imgs[b0:b0 + 3]), classes=cs) for b0 in range(0, n, 3)])
    ev = Classification(cs.n)
    ev.process(logits.cpu().argmax(1).tolist(), labels)
    want = ev.evaluate(verbose=False)
    for k in want:
        assert res[k] == want[k], k
    assert res["confusion_matrix"].shape == (18, 18) and np.array_equal(res["confusion_matrix"], ev.cmat) and res["total"] == n
    # a label outside the class set
    bad, _, _ = _image_set(4, 92, cs.n + 1)
    with pytest.raises(IndexError, match="out of bounds"):
        tr.test(bad, verbose=False, classes=cs)
    # the frozen cache does not depend on the classes: the same cache, the new classes
    cache = FrozenImageKV.build(tr.engine, ds)
    got = {}
    fr = tr.test(ds, verbose=False, frozen=cache, classes=cs, hook=lambda b0, lg: got.__setitem__(b0, lg.detach().clone()))
    fl = torch.cat([got[b0] for b0 in sorted(got)], dim=1)[0]
    err = float((fl - logits).abs().max())
    print(f"\n[test(frozen, classes) {mode}] worst logits diff vs the live class-set path {err:.3e} (bound {bound(mode)})")
    assert tuple(fl.shape) == (n, 18) and err <= bound(mode) and fr["total"] == n and set(fr) == set(res)
    base_ds, _, _ = _image_set(5, 93, tr.cfg.n_cls)
    # base-to-new: two tests and the harmonic mean of their accuracies
    b2n = base_to_new(tr, base_ds, ds, cs, verbose=False)
    assert b2n["base"] == tr.test(base_ds, verbose=False)["accuracy"] and b2n["new"] == res["accuracy"]
    assert b2n["H"] == harmonic_mean(b2n["base"], b2n["new"])


@pytest.mark.parametrize("mode", MODES)
def test_multi_test_all_on_a_class_set_agrees_with_each_member(mode):
    """`test_all(classes=)` member s against `model_inference(member=s, classes=)`: f32 within TOL_F32 / 100, the 16-bit
    modes within the mode bound (the pair's bounds in tests/test_gpu_shared_eval.py)."""
    from rpo_amd.multi import RPOMulti
    from test_gpu_loop import _staging
    cfg, sd, toks, *_ = workload(TAG)
    S, B, n = 2, 2, 5
    prompts = [synth.prompts(cfg, sd, seed=7 + 13 * s) for s in range(S)]
    tr = RPOMulti(cfg, sd, toks, n_runs=S, batch_size=B, prompts=prompts, device=DEV, act_dtype=DT[mode], num_batches=10 ** 9)
    cs = tr.class_set(gold("rpo")["tokens"])
    ds, imgs, labels = _image_set(n, 95, cs.n)
    got = {}
    res = tr.test_all(ds, verbose=False, classes=cs, hook=lambda b0, lg: got.__setitem__(b0, lg.detach().clone()))
    allm = torch.cat([got[b0] for b0 in sorted(got)], dim=1)
    assert tuple(allm.shape) == (S, n, 18) and not same(allm[0], allm[1])
    stage = _staging(False, S * B)
    lim = TOL_F32 / 100 if mode == "f32" else bound(mode)
    for s in range(S):
        one = torch.cat([tr.model_inference(stage(imgs[b0:b0 + S * B]), member=s, classes=cs) for b0 in range(0, n, S * B)])
        err = float((allm[s] - one).abs().max())
        print(f"\n[test_all(classes) {mode}] member {s}: worst logits diff vs model_inference(member, classes) {err:.3e} (bound {lim})")
        assert err <= lim
        single = tr.test(ds, member=s, verbose=False, classes=cs)
        assert single["total"] == res[s]["total"] == n and single["confusion_matrix"].shape == (18, 18)
    # the built-in classes still evaluate as before through both paths
    base_ds, _, _ = _image_set(4, 96, cfg.n_cls)
    assert tr.test_all(base_ds, verbose=False)[1]["total"] == tr.test(base_ds, member=1, verbose=False)["total"] == 4


# ============================================================================================ 8. refusals

def test_refusals():
    from rpo_amd.coop import CoCoOp, CoOp
    from rpo_amd.engine import Engine
    from rpo_amd.sweep import RPOSweep
    cfg, sd, toks, tp, ip, _, _ = workload(TAG)
    eng = _engine("bf16")
    image = _image()
    new = gold("rpo")["tokens"]
    with pytest.raises(ValueError, match="tokens must be"):
        eng.class_set(new[:, :76])
    with pytest.raises(ValueError, match="tokens must be"):
        eng.class_set(new[None])
    with pytest.raises(ValueError, match="tokens must be"):
        eng.class_set(new[:0])
    with pytest.raises(TypeError, match="integer"):
        eng.class_set(new.astype(np.float32))
    for bad in (-1, cfg.vocab):
        t = new.copy()
        t[3, 2] = bad
        with pytest.raises(ValueError, match="outside the vocabulary"):
            eng.class_set(t)
    with pytest.raises(ValueError, match="chunk"):
        eng.class_set(new, chunk=0)
    # len' + K > 77: refused when RPO features are first asked for (the plain towers take the set)
    long_t = new.copy()
    long_t[0] = 0
    long_t[0, 0], long_t[0, 1:69], long_t[0, 69] = 49406, 1234, 49407          # 70 tokens, K = 8
    cs = eng.class_set(long_t)
    with pytest.raises(ValueError, match="must fit the context"):
        eng.forward_eval(image, classes=cs)
    assert tuple(eng.forward_plain(image, classes=cs).shape) == (3, 18)
    # a class set of another engine
    other = Engine(cfg, sd, toks, torch.device(DEV), torch.bfloat16, max_batch=3)
    foreign = other.class_set(new)
    with pytest.raises(ValueError, match="another engine"):
        eng.forward_eval(image, classes=foreign)
    with pytest.raises(ValueError, match="another engine"):
        eng.forward_plain(image, classes=foreign)
    with pytest.raises(TypeError, match="ClassSet"):
        eng.forward_eval(image, classes=new)
    # the built-in row count is still pinned
    with pytest.raises(AssertionError):
        eng.set_plain_text_features(torch.zeros(18, cfg.embed))
    # CSC and CoCoOp, by name
    ctoks = synth.coop_tokens(toks, 4)
    csc = CoOp(sd, ctoks, n_ctx=4, device=DEV, act_dtype=torch.bfloat16, batch_size=3, csc=True)
    with pytest.raises(NotImplementedError, match="CSC"):
        csc.class_set(gold("coop_end")["tokens"])
    coco = CoCoOp(sd, ctoks, n_ctx=4, device=DEV, act_dtype=torch.bfloat16, batch_size=1)
    with pytest.raises(NotImplementedError, match="CoCoOp"):
        coco.class_set(gold("coop_end")["tokens"])
    # RPOSweep, by name
    sweep = RPOSweep(cfg, sd, toks, members=[dict(seed=1, K=8), dict(seed=2, K=4)], batch_size=1, device=DEV,
                     act_dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="RPOSweep"):
        sweep.class_set(new)
    with pytest.raises(NotImplementedError, match="RPOSweep"):
        sweep.model_inference(image[:1], member=0, classes=cs)
    ds, _, _ = _image_set(2, 97, 18)
    with pytest.raises(NotImplementedError, match="RPOSweep"):
        sweep.test(ds, member=1, verbose=False, classes=cs)
    with pytest.raises(NotImplementedError, match="RPOSweep"):
        sweep.test_all(ds, verbose=False, classes=cs)
