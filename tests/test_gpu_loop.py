"""The epoch loops on the device: `rpo_eval_accumulate` against torch's CPU argmax and numpy's integer counts, the resident
transform against the staging transform (bit for bit), `run_epoch` against sequential `forward_backward` (bit for bit) and
`test()` against `model_inference` + CPU argmax.  Depth-2 models."""
import functools
import os

import numpy as np
import pytest
import torch

from rpo_amd import synth
from rpo_amd.config import vit_b16

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- 5. rpo_eval_accumulate -----------------------------------------------------------------------------------------------

GUARD = 32


def _guarded(n, dtype, sentinel):
    """(whole, inner): `inner` = n elements with GUARD sentinel words on either side."""
    whole = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n, sentinel):
    w = whole.cpu()
    return bool((w[:GUARD] == sentinel).all() and (w[GUARD + n:] == sentinel).all())


def _crafted_rows(C):
    """Rows whose argmax depends on torch's tie / NaN rules (the first four are the rows of the issue, padded)."""
    inf, nan = float("inf"), float("nan")
    rows = [[1, 3, 3, 2], [nan, 5, nan, 1], [2, nan, 9, 9], [inf, inf, 0, 0], [-inf] * 4, [0.0, -0.0, -0.0, 0.0],
            [-0.0, 0.0, -1, -1], [-inf, -inf, -inf, -5], [5, inf, nan, inf], [-1, -1, -1, -1]]
    if C == 1:
        return [[nan], [inf], [-inf], [-0.0]]
    if C < 4:
        return []
    return [r + [-inf] * (C - 4) for r in rows]            # -inf behind the row never beats or precedes its maximum


def _eval_case(B, C, ldl, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, generator=g)
    if C > 2:                                                   # exact ties between random positions
        for b in range(0, B, 3):
            i, j = torch.randint(0, C, (2,), generator=g).tolist()
            logits[b, j] = logits[b, i] = logits[b].max() + (1.0 if b % 2 else 0.0)
    crafted = _crafted_rows(C)
    for k, r in enumerate(crafted[:B]):
        logits[(k * 7) % B] = torch.tensor(r)
    label = torch.randint(0, C, (B,), generator=g)
    bad = [-1, C, C + 5, 2 ** 40, -2 ** 40]
    for k in range(0, B, 5):
        label[k] = bad[(k // 5) % len(bad)]
    for b in range(1, B, 2):                                    # enough correct ones to make `correct` non-trivial
        if 0 <= int(label[b]) < C:
            label[b] = torch.max(logits[b:b + 1], 1)[1][0]
    return logits, label


@pytest.mark.parametrize("C", [1, 19, 37, 1000])
@pytest.mark.parametrize("B", [1, 37, 100, 128])
def test_eval_accumulate(B, C):
    from rpo_amd import ops
    ldl = C + 13
    counts_w, counts = _guarded(2, torch.int64, -7)
    cmat_w, cmat = _guarded(C * C, torch.int32, -7)
    pred_w, pred = _guarded(B, torch.int32, -7)
    counts.zero_()
    cmat.zero_()
    ref_counts, ref_cmat = np.zeros(2, np.int64), np.zeros((C, C), np.int64)
    calls = []
    for call in range(3):                                       # three accumulating calls on different data
        logits, label = _eval_case(B, C, ldl, seed=1000 * B + 10 * C + call)
        dl = torch.full((B, ldl), float("nan"), device=DEV)     # the padding columns are NaN: reading one changes pred
        dl[:, :C] = logits.to(DEV)
        lab_w, lab = _guarded(B, torch.int64, 0)                # (label guards are valid labels: a stray read would count)
        lab.copy_(label)
        ops.eval_accumulate(dl[:, :C], lab, counts, cmat, pred)
        ref_pred = torch.max(logits, 1)[1].numpy()              # torch on the CPU, fp32: the yardstick
        lab_np = label.numpy()
        ok = (lab_np >= 0) & (lab_np < C)
        ref_counts += np.array([int((ok & (ref_pred == lab_np)).sum()), B])
        np.add.at(ref_cmat, (lab_np[ok], ref_pred[ok]), 1)
        assert np.array_equal(pred.cpu().numpy(), ref_pred), f"call {call}: pred"
        assert np.array_equal(counts.cpu().numpy(), ref_counts), f"call {call}: counts"
        assert np.array_equal(cmat.cpu().numpy().reshape(C, C), ref_cmat), f"call {call}: cmat"
        calls.append((dl, lab, ref_pred, lab_np, ok))
    assert ref_counts[0] > 0 or B == 1
    # cmat / pred NULL: only the counts move
    dl, lab, ref_pred, lab_np, ok = calls[0]
    pred.fill_(-3)
    ops.eval_accumulate(dl[:, :C], lab, counts)
    ref_counts += np.array([int((ok & (ref_pred == lab_np)).sum()), B])
    assert np.array_equal(counts.cpu().numpy(), ref_counts)
    assert np.array_equal(cmat.cpu().numpy().reshape(C, C), ref_cmat) and bool((pred == -3).all())
    # the same call replayed from a captured graph, twice
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.eval_accumulate(dl[:, :C], lab, counts, cmat, pred)
    for _ in range(2):
        graph.replay()
        ref_counts += np.array([int((ok & (ref_pred == lab_np)).sum()), B])
        np.add.at(ref_cmat, (lab_np[ok], ref_pred[ok]), 1)
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), ref_counts)
    assert np.array_equal(cmat.cpu().numpy().reshape(C, C), ref_cmat)
    assert np.array_equal(pred.cpu().numpy(), ref_pred)
    assert _guards_intact(counts_w, 2, -7) and _guards_intact(cmat_w, C * C, -7) and _guards_intact(pred_w, B, -7)


def test_eval_accumulate_issue_rows_and_arguments():
    """The five rows the issue lists give 1, 0, 1, 0, 0, as torch gives on the CPU; bad arguments are refused."""
    from rpo_amd import _lib, ops
    inf, nan = float("inf"), float("nan")
    rows = torch.tensor([[1, 3, 3, 2], [nan, 5, nan, 1], [2, nan, 9, 9], [inf, inf, 0, 0], [-inf] * 4])
    assert torch.max(rows, 1)[1].tolist() == [1, 0, 1, 0, 0]
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    pred = torch.zeros(5, dtype=torch.int32, device=DEV)
    label = torch.tensor([1, 0, 0, 0, 3], device=DEV)
    ops.eval_accumulate(rows.to(DEV), label, counts, None, pred)
    assert pred.tolist() == [1, 0, 1, 0, 0] and counts.tolist() == [3, 5]
    lib = _lib.load()
    x = rows.to(DEV)
    args = lambda **kw: [kw.get("logits", x.data_ptr()), kw.get("ldl", 4), label.data_ptr(), kw.get("B", 5), kw.get("C", 4),
                         kw.get("counts", counts.data_ptr()), None, None, None]
    assert lib.rpo_eval_accumulate(*args(logits=None)) == _lib.E_BADARG
    assert lib.rpo_eval_accumulate(*args(counts=None)) == _lib.E_BADARG
    assert lib.rpo_eval_accumulate(*args(ldl=3)) == _lib.E_SHAPE
    assert lib.rpo_eval_accumulate(*args(B=0)) == _lib.E_SHAPE
    assert lib.rpo_eval_accumulate(*args(C=0)) == _lib.E_SHAPE
    torch.cuda.synchronize()
    assert counts.tolist() == [3, 5]


# ---- shared fixtures ------------------------------------------------------------------------------------------------------

def _decoded(n, seed):
    """n decoded uint8 images of ragged sizes (portrait, landscape, smaller and larger than the crop)."""
    rng = np.random.default_rng(seed)
    sizes = [(375, 500), (500, 333), (224, 224), (97, 260), (301, 97), (60, 40), (230, 231), (256, 192)]
    return [rng.integers(0, 256, (*sizes[i % len(sizes)], 3), dtype=np.uint8) for i in range(n)]


def _staging(is_train, max_batch, size=224):
    from rpo_amd.input_pipeline import InputConfig, build_transform
    return build_transform(InputConfig(SIZE=(size, size)), is_train, DEV, max_batch)


# ---- 6. resident transform == staging transform -----------------------------------------------------------------------------

@pytest.mark.parametrize("is_train", [True, False])
def test_resident_transform_bit_identical(is_train):
    from rpo_amd.input_pipeline import DeviceImageSet
    imgs = _decoded(16, seed=5)
    labels = list(range(16))
    nbytes = [im.size for im in imgs]
    full = DeviceImageSet(imgs, labels, DEV)
    assert full.plan.spilled == [] and full.resident_bytes >= sum(nbytes)
    budget = sum((n + 15) // 16 * 16 for n in nbytes[:3]) + 20000          # images 0-2, then only the small ones
    part = DeviceImageSet(imgs, labels, DEV, budget_bytes=budget)
    spilled = set(part.plan.spilled)
    assert spilled and len(spilled) < 16 and part.resident_bytes <= budget
    none = DeviceImageSet(imgs, labels, DEV, budget_bytes=0)
    assert len(none.plan.spilled) == 16
    stage, res = _staging(is_train, 8), _staging(is_train, 8)
    torch.manual_seed(21)
    resident_idx = [i for i in range(16) if i not in spilled]
    spilled_idx = sorted(spilled)
    batches = [[0, 1, 2, 3, 4, 5, 6, 7], [15, 3, 9], [5], resident_idx[:4], spilled_idx[:4],
               [resident_idx[0], spilled_idx[0], resident_idx[1], spilled_idx[1], spilled_idx[2]], [8, 9, 10, 11, 12, 13, 14, 15]]
    for rep in range(2):                                         # twice: both slot pairs are reused
        for idx in batches:
            plans = [stage.plan(*imgs[i].shape[:2]) for i in idx]
            if is_train:
                plans[0].flip, plans[-1].flip = True, False
            want = stage([imgs[i] for i in idx], plans).clone()
            for name, ds in (("resident", full), ("mixed", part), ("spilled", none)):
                got = res.from_set(ds, idx, plans)
                assert torch.equal(bits(got), bits(want)), (name, idx, rep)
    # un-injected plans: the same draws in the same order as today's call
    idx = [3, 0, 7, 12, 5]
    torch.manual_seed(77)
    want = stage([imgs[i] for i in idx]).clone()
    after = torch.rand(1).item()
    torch.manual_seed(77)
    got = res.from_set(part, idx)
    assert torch.equal(bits(got), bits(want)) and torch.rand(1).item() == after
    out = torch.empty(5, 3, 224, 224, device=DEV)
    assert res.from_set(full, idx, [stage.plan(*imgs[i].shape[:2]) for i in idx], out=out).data_ptr() == out.data_ptr()
    with pytest.raises(IndexError):
        DeviceImageSet(imgs, labels, DEV, n_cls=10)
    assert full.labels_dev.tolist() == labels and full.labels_dev.dtype == torch.int64


# ---- 7. run_epoch == sequential forward_backward ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rpo_workload():
    cfg = vit_b16(layers_v=2, layers_t=2, K=8)
    toks = synth.oxford_pets_base_tokens()
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407], logit_scale=float(np.log(100.0)))
    tp, ip = synth.prompts(cfg, sd, seed=7)
    return cfg, sd, toks, tp, ip


@functools.lru_cache(maxsize=None)
def _coop_workload(which):
    gold = dict(np.load(os.path.join(GOLD, {"coop": "ref_coop_d2_b3_ctx4.npz", "cocoop": "ref_cocoop_d2_b3_ctx4.npz"}[which])))
    cfg = vit_b16(layers_v=2, layers_t=2, K=1)
    toks = gold["tokenized_prompts"]
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407], logit_scale=float(np.log(100.0)))
    return cfg, sd, toks, gold


@functools.lru_cache(maxsize=None)
def _lp_workload():
    g = np.load(os.path.join(GOLD, "ref_lp_d2_b3.npz"))
    toks = g["tokenized_prompts"]
    cfg = vit_b16(layers_v=2, layers_t=2, K=1)
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist(), logit_scale=float(np.log(100.0)))
    return cfg, sd, toks


def _make(kind, mode, use_graph, B, nb):
    """A trainer of `kind` with fixed initial parameters; the default schedules (one warm-up epoch, then the cosine)."""
    from rpo_amd.coop import CoCoOp, CoOp
    from rpo_amd.lp import LP
    from rpo_amd.trainer import RPO
    if kind == "rpo":
        cfg, sd, toks, tp, ip = _rpo_workload()
        return RPO(cfg, sd, toks, None, DEV, DT[mode], batch_size=B, num_batches=nb, use_graph=use_graph, prompts=(tp, ip))
    if kind == "coop":
        cfg, sd, toks, gold = _coop_workload("coop")
        return CoOp(sd, toks, 4, None, DEV, DT[mode], batch_size=B, num_batches=nb, ctx=gold["ctx"], use_graph=use_graph)
    if kind == "cocoop":
        cfg, sd, toks, gold = _coop_workload("cocoop")
        meta = {k: gold[k] for k in ("w1", "b1", "w2", "b2")}
        return CoCoOp(sd, toks, 4, None, DEV, DT[mode], batch_size=B, num_batches=nb, ctx=gold["ctx"], meta=meta,
                      use_graph=use_graph)
    cfg, sd, toks = _lp_workload()
    return LP(sd, toks, None, DEV, DT[mode], batch_size=B, num_batches=nb, use_graph=use_graph, cfg=cfg, max_batch=B)


def _state(tr, kind):
    eng = tr.engine
    p, m = {"rpo": lambda: (eng.params, eng.mom), "coop": lambda: (eng.coop_params, eng.coop_moms),
            "cocoop": lambda: (eng.coop_params, eng.coop_moms), "lp": lambda: (eng.lp_params, eng.lp_moms)}[kind]()
    torch.cuda.synchronize()
    return p.detach().clone(), m.detach().clone()


RUN_EPOCH_CASES = [("rpo", m, g) for m in ("f32", "bf16", "f16") for g in (True, False)] + \
                  [("coop", "f16", True), ("cocoop", "f32", False), ("lp", "f32", True)]


@pytest.mark.parametrize("kind,mode,use_graph", RUN_EPOCH_CASES)
def test_run_epoch_equals_sequential_forward_backward(kind, mode, use_graph):
    from rpo_amd.input_pipeline import DeviceImageSet
    from rpo_amd.loop import epoch_indices
    from rpo_amd.trainer import lr_at_epoch
    B, nb, epochs = (2 if kind == "cocoop" else 4), 3, 2
    n = B * nb + 1                                               # the last partial batch is dropped
    imgs = _decoded(n, seed=31)
    labels = np.random.default_rng(32).integers(0, 19, n).tolist()
    ds = DeviceImageSet(imgs, labels, DEV, budget_bytes=sum(im.size for im in imgs) * 2 // 3)      # some images spill
    assert ds.plan.spilled and len(ds.plan.spilled) < n
    stage = _staging(True, B)
    torch.manual_seed(5)
    g_plan = torch.Generator().manual_seed(40)
    order = [epoch_indices(n, B, g_plan) for _ in range(epochs)]
    plans = [[[stage.plan(*imgs[i].shape[:2]) for i in batch] for batch in ep] for ep in order]

    # sequential: today's API, one batch at a time, float tensors from the staging transform
    seq = _make(kind, mode, use_graph, B, nb)
    seq_loss, seq_correct, seq_lrs = [], 0, []
    for ep in range(epochs):
        for t, batch in enumerate(order[ep]):
            seq_lrs.append(seq.lr)
            image = stage([imgs[i] for i in batch], plans[ep][t])
            out = seq.forward_backward({"img": image, "label": torch.tensor([labels[i] for i in batch])})
            seq_loss.append(np.float32(out["loss"]))
            if "acc" in out:
                seq_correct += int(round(out["acc"] * B / 100.0))
    seq_p, seq_m = _state(seq, kind)
    assert seq.epoch == epochs and seq_lrs[0] != seq_lrs[-1], "the run must cross the warm-up -> cosine LR change"

    # the loop
    tr = _make(kind, mode, use_graph, B, nb)
    g_loop = torch.Generator().manual_seed(40)
    losses, correct, total = [], 0, 0
    for ep in range(epochs):
        assert tr.lr == lr_at_epoch(tr.optim_cfg, ep)
        out = tr.run_epoch(ds, g_loop, plans[ep])
        assert out["indices"] == order[ep] and out["loss"].is_cuda and out["loss"].shape == (nb,)
        losses.append(out["loss"])
        if kind in ("coop", "lp"):
            c = out["counts"].tolist()
            correct, total = correct + c[0], total + c[1]
        else:
            assert "counts" not in out
    got_loss = torch.cat(losses).cpu().numpy()
    p, m = _state(tr, kind)
    print(f"\n{kind} {mode} graph={use_graph}: losses seq {[float(v) for v in seq_loss]} loop {got_loss.tolist()}")
    assert np.array_equal(got_loss.view(np.uint32), np.array(seq_loss, np.float32).view(np.uint32)), "per-step losses"
    assert torch.equal(bits(p), bits(seq_p)), f"parameters: max diff {(p - seq_p).abs().max().item():.3e}"
    assert torch.equal(bits(m), bits(seq_m)), f"momentum: max diff {(m - seq_m).abs().max().item():.3e}"
    assert tr.epoch == epochs and tr.batch_idx == 0 and tr.lr == seq.lr and tr._steps == seq._steps
    if kind in ("coop", "lp"):
        assert (correct, total) == (seq_correct, epochs * nb * B)
    if kind == "rpo" and use_graph:
        assert len(tr._g_patch) == 2, "the loop owns two image buffers: two patch-embed graphs"
    with pytest.raises(ValueError, match="num_batches"):
        tr.run_epoch(DeviceImageSet(imgs[:B], labels[:B], DEV))


# ---- 8. test() == model_inference per batch + CPU argmax ----------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rpo", "coop", "cocoop", "lp", "zeroshot"])
def test_test_equals_model_inference(kind, capsys):
    from rpo_amd.input_pipeline import DeviceImageSet
    n, bs, C = 23, 10, 19
    imgs = _decoded(n, seed=51)
    labels = np.random.default_rng(52).integers(0, C, n).tolist()
    ds = DeviceImageSet(imgs, labels, DEV, budget_bytes=sum(im.size for im in imgs) * 3 // 4)
    if kind == "zeroshot":
        from rpo_amd.zeroshot import ZeroshotCLIP
        cfg, sd, toks, _, _ = _rpo_workload()
        tr = ZeroshotCLIP(sd, toks, DEV, torch.float16, max_batch=100)
    else:
        tr = _make(kind, {"rpo": "bf16", "coop": "f16", "cocoop": "f32", "lp": "f32"}[kind], True, bs, 2)
    chunk = min(bs, tr.engine.max_batch)
    assert chunk == bs
    # the yardstick: today's API per batch, torch's argmax on the CPU, numpy's counts
    stage = _staging(False, chunk)
    ref_cm, ref_correct = np.zeros((C, C), np.int64), 0
    for b0 in range(0, n, chunk):
        image = stage(imgs[b0:b0 + chunk])
        logits = tr.model_inference(image).float().cpu()
        assert logits.shape == (min(chunk, n - b0), C)
        pred = torch.max(logits, 1)[1].numpy()
        lab = np.array(labels[b0:b0 + chunk])
        ref_correct += int((pred == lab).sum())
        np.add.at(ref_cm, (lab, pred), 1)
    for rep in range(2):                                         # twice: the accumulators start from zero each time
        res = tr.test(ds, batch_size=bs)
        assert res["total"] == n and res["correct"] == ref_correct, (rep, res["correct"], ref_correct)
        assert np.array_equal(res["confusion_matrix"], ref_cm), rep
        assert res["accuracy"] == 100.0 * ref_correct / n
    out = capsys.readouterr().out
    assert f"* accuracy: {100.0 * ref_correct / n:.1f}%" in out and "* macro_f1: " in out


def test_train_runs_epochs_evaluates_and_keeps_the_best(tmp_path):
    """`train()`: run_epoch per epoch, test(val_set) behind each, model-best through after_epoch_eval."""
    from rpo_amd.input_pipeline import DeviceImageSet
    B, nb = 4, 2
    imgs = _decoded(B * nb, seed=61)
    labels = np.random.default_rng(62).integers(0, 19, B * nb).tolist()
    ds = DeviceImageSet(imgs, labels, DEV)
    tr = _make("coop", "f16", True, B, nb)
    torch.manual_seed(3)
    hist = tr.train(ds, max_epoch=2, val_set=ds, directory=str(tmp_path), generator=torch.Generator().manual_seed(1))
    assert [h["epoch"] for h in hist] == [1, 2] and tr.epoch == 2 and tr._steps == 2 * nb
    assert all(np.isfinite(h["loss"]) and 0.0 <= h["acc"] <= 100.0 and 0.0 <= h["val_acc"] <= 100.0 for h in hist)
    assert tr.best_result == max(h["val_acc"] for h in hist)
    assert os.path.exists(os.path.join(str(tmp_path), "prompt_learner", "model-best.pth.tar"))
