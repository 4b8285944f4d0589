"""Both ends of the ViT patch-grid range on the MI355X, depth 2, every storage mode: ViT-L/14 at 336 px (24 x 24 grid,
577 frozen tokens: the image tower's attention walks the keys in chunks) and ViT-B/32 (7 x 7 grid, patch rows of 3072)
against the reference's own outputs (tools/make_golden_grids.py).  The bounds are the project's model-level ones
(tests/helpers.py, as tests/test_gpu_model.py applies them); the RPOMulti bar is tests/test_gpu_multi.py's.

Every 336-px test fails on a library without the long-sequence kernels (RPO_E_SHAPE in the first image forward); the
ViT-B/32 tests pin a grid that ran unpinned before.
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import BF16_GRAD_REL, BF16_LOGIT_ATOL, F16_GRAD_REL, F16_LOGIT_ATOL, GOLDEN, TOL_F32  # noqa: E402
from rpo_amd import synth  # noqa: E402
from rpo_amd.config import vit_b32, vit_l14_336  # noqa: E402

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MODES = ["f32", "bf16", "f16"]
BOUNDS = {"f32": (TOL_F32, TOL_F32), "bf16": (BF16_LOGIT_ATOL, BF16_GRAD_REL), "f16": (F16_LOGIT_ATOL, F16_GRAD_REL)}
D2 = dict(layers_v=2, layers_t=2)
GRIDS = {"vitl14_336": (vit_l14_336, 2), "vitb32": (vit_b32, 3)}       # tag -> (config, batch of its fixtures)


def gold(name):
    return dict(np.load(os.path.join(GOLDEN, f"ref_{name}.npz")))


def _relmax(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@functools.lru_cache(maxsize=None)
def rpo_workload(tag):
    make, B = GRIDS[tag]
    cfg = make(K=24, **D2)
    toks = synth.oxford_pets_base_tokens()
    sd = synth.clip_state_dict(cfg, seed=0, token_rows=np.unique(toks).tolist() + [49407])
    return cfg, sd, toks, synth.prompts(cfg, sd, seed=7), B


@functools.lru_cache(maxsize=None)
def plain_workload(tag):
    make, B = GRIDS[tag]
    cfg = make(K=1, **D2)
    return cfg, synth.clip_state_dict(cfg, seed=0, logit_scale=float(np.log(100.0))), B


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,name", [("vitl14_336", "vitl14_336_d2_k24_b2"), ("vitb32", "vitb32_d2_k24_b3")])
def test_rpo_matches_the_reference_at_both_grids(tag, name, mode):
    """Eval logits, loss and both prompt gradients of the HIP path against trainers/rpo.py's own CustomCLIP at the grid;
    f32 at 336 px also the prompt rows after every block of both towers."""
    from rpo_amd.custom_clip import CustomCLIP
    g = gold(name)
    cfg, sd, toks, (tp, ip), B = rpo_workload(tag)
    image, label = torch.from_numpy(synth.images(cfg, B)).cuda(), torch.from_numpy(synth.labels(cfg, B)).cuda()
    m = CustomCLIP(cfg, sd, toks, DEV, DT[mode], max_batch=B, prompts=(tp, ip))
    m.prompt_learner.eval()
    logits = m(image).cpu().numpy()
    eng = m.engine
    eng.forward_backward(image, label)
    torch.cuda.synchronize()
    loss = float(eng.loss.item())
    le, ll = np.abs(logits - g["logits"]).max(), abs(loss - float(g["loss"]))
    rt, ri = _relmax(eng.g_text.cpu().numpy(), g["g_text"]), _relmax(eng.g_img.cpu().numpy(), g["g_img"])
    print(f"\n[{tag} {mode}] logits err {le:.3e} loss err {ll:.3e} g_text rel {rt:.3e} g_img rel {ri:.3e}")
    lt, gr = BOUNDS[mode]
    assert np.isfinite(logits).all() and le <= lt and ll <= lt
    assert rt <= gr and ri <= gr
    if mode == "f32" and "img_rows" in g:
        N, K = cfg.n_frozen, cfg.K
        for l in range(cfg.layers_v):
            rows = eng.x[l + 1][B * N:B * (N + K)].view(B, K, cfg.d_v).cpu().numpy()
            assert np.abs(rows - g["img_rows"][l]).max() <= TOL_F32, f"image block {l}"
        nc = g["text_rows"].shape[1]
        for l in range(cfg.layers_t):
            rows = eng.xt[l + 1].view(cfg.n_cls, K, cfg.d_t)[:nc].cpu().numpy()
            assert np.abs(rows - g["text_rows"][l]).max() <= TOL_F32, f"text block {l}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,name", [("vitl14_336", "plainclip_vitl14_336_d2_b2"), ("vitb32", "plainclip_vitb32_d2_b3")])
def test_plain_clip_matches_the_reference_at_both_grids(tag, name, mode):
    """ZeroshotCLIP (the unmasked towers; the configuration comes from the state dict) against CLIP.forward."""
    from rpo_amd.zeroshot import ZeroshotCLIP
    g = gold(name)
    cfg, sd, B = plain_workload(tag)
    m = ZeroshotCLIP(sd, device=DEV, act_dtype=DT[mode], max_batch=4)
    assert (m.cfg.image_size, m.cfg.patch, m.cfg.name) == (cfg.image_size, cfg.patch, cfg.name)
    image = torch.from_numpy(synth.images(cfg, B))
    logits = m.model_inference(image).cpu().numpy()
    err = np.abs(logits - g["logits"]).max()
    print(f"\n[plain {tag} {mode}] logits err {err:.3e}")
    assert err <= BOUNDS[mode][0], f"{mode}: logits differ from the reference by {err:.3e}"
    assert np.array_equal(m.model_inference(image).cpu().numpy(), logits)
    if mode == "f32":
        img_f = m.engine.img_cls_f[:B].cpu().numpy()
        assert np.abs(img_f - g["image_features"]).max() <= 1e-4 * max(1.0, np.abs(g["image_features"]).max())


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("tag,name", [("vitl14_336", "plainclip_vitl14_336_d2_b2"), ("vitb32", "plainclip_vitb32_d2_b3")])
def test_linear_probe_with_its_identity_layer_gives_clip_forward_logits(tag, name, mode):
    """LP's image pass is the plain tower; with the reference's initial lp_layer (eye / zeros, trainers/linear_prob.py:71-72)
    its logits are exp(logit_scale) * image_features @ normalise(text_features).T of the reference's own features (:85-95:
    the image feature is NOT normalised).  That is CLIP.forward's logit times the norm of the image feature, so the plain
    tower's logits bound scales by the largest such norm."""
    from rpo_amd.lp import LPCustomCLIP
    g = gold(name)
    cfg, sd, B = plain_workload(tag)
    m = LPCustomCLIP(sd, synth.oxford_pets_base_tokens(), DEV, DT[mode], max_batch=4)
    logits = m(torch.from_numpy(synth.images(cfg, B))).cpu().numpy()
    img_f, txt_f = g["image_features"].astype(np.float64), g["text_features"].astype(np.float64)
    want = 100.0 * img_f @ (txt_f / np.linalg.norm(txt_f, axis=1, keepdims=True)).T
    norm = np.linalg.norm(img_f, axis=1).max()
    err = np.abs(logits - want).max()
    print(f"\n[lp {tag} {mode}] logits err {err:.3e} (largest |image feature| {norm:.3f})")
    assert err <= BOUNDS[mode][0] * max(1.0, norm)


@pytest.mark.parametrize("mode", MODES)
def test_coop_training_matches_the_reference_at_patch_32(mode):
    from rpo_amd.coop import CoOpCustomCLIP
    g = gold("coop_vitb32_d2_b3_ctx16")
    cfg, sd, B = plain_workload("vitb32")
    m = CoOpCustomCLIP(sd, g["tokenized_prompts"], 16, DEV, DT[mode], max_batch=4, ctx=g["ctx"])
    image, label = torch.from_numpy(synth.images(cfg, B)).cuda(), torch.from_numpy(g["label"]).cuda()
    eng = m.engine
    logits = eng.coop_forward_backward(image, label).cpu().numpy()
    loss, grad = eng.loss.item(), eng.coop_grad.cpu().numpy()
    le, ll, gr = np.abs(logits - g["logits"]).max(), abs(loss - float(g["loss"])), _relmax(grad, g["ctx_grad"])
    print(f"\n[coop vitb32 {mode}] logits err {le:.3e} loss err {ll:.3e} ctx_grad rel {gr:.3e}")
    lt, gt = BOUNDS[mode]
    assert le <= lt and ll <= lt and gr <= gt


@pytest.mark.parametrize("mode", MODES)
def test_multi_step_equals_standalone_steps_at_336px(mode):
    """One RPOMulti step with two members against two standalone RPO steps (tests/test_gpu_multi.py's
    test_three_sgd_steps_equal_standalone_trainers: its bounds on the prompts, the momentum and the loss)."""
    from test_gpu_multi import SGD_TOL
    from rpo_amd.multi import RPOMulti
    from rpo_amd.trainer import OptimConfig, RPO
    cfg, sd, toks, _, _ = rpo_workload("vitl14_336")
    S, B = 2, 1
    oc = OptimConfig(lr=0.01, warmup_epoch=0, lr_scheduler="constant")
    prompts = [synth.prompts(cfg, sd, seed=7 + 13 * s) for s in range(S)]
    tr = RPOMulti(cfg, sd, toks, n_runs=S, batch_size=B, prompts=prompts, optim=oc, device=DEV, act_dtype=DT[mode],
                  num_batches=10 ** 9)
    image = torch.from_numpy(np.concatenate([synth.images(cfg, B, seed=1234 + 100 * s) for s in range(S)])).to(DEV)
    label = torch.from_numpy(np.concatenate([synth.labels(cfg, B, seed=4321 + 100 * s) for s in range(S)])).to(DEV)
    loss = tr.step_async(image, label).clone()
    torch.cuda.synchronize()
    for s in range(S):
        solo = RPO(cfg, sd, toks, oc, DEV, DT[mode], batch_size=B, num_batches=10 ** 9, prompts=prompts[s])
        l1 = solo.step_async(image[s * B:(s + 1) * B].contiguous(), label[s * B:(s + 1) * B].contiguous()).clone()
        solo._join_side()
        torch.cuda.synchronize()
        ep = float((tr.engine.m_params[s] - solo.engine.params).abs().max())
        em = float((tr.engine.m_mom[s] - solo.engine.mom).abs().max())
        el = abs(float(loss[s]) - float(l1))
        print(f"\n[multi 336 {mode}] member {s}: prompts err {ep:.2e} momentum err {em:.2e} loss err {el:.2e}")
        assert ep <= SGD_TOL[mode]
        em_tol = 1e-6 if mode == "f32" else 2.71 * 2 * BOUNDS[mode][1] * float(solo.engine.mom.abs().max())
        assert em <= em_tol and el <= (1e-6 if mode == "f32" else BOUNDS[mode][0])


@pytest.mark.parametrize("mode", MODES)
def test_graph_replay_equals_eager_at_336px(mode):
    from rpo_amd.trainer import RPO
    cfg, sd, toks, prompts, B = rpo_workload("vitl14_336")
    outs = []
    for use_graph in (False, True):
        tr = RPO(cfg, sd, toks, None, DEV, DT[mode], batch_size=B, use_graph=use_graph, prompts=prompts)
        ls = []
        for step in range(2):
            batch = {"img": torch.from_numpy(synth.images(cfg, B, seed=50 + step)),
                     "label": torch.from_numpy(synth.labels(cfg, B, seed=60 + step))}
            ls.append(tr.forward_backward(batch)["loss"])
        outs.append((ls, tr.engine.params.clone()))
    assert outs[0][0] == outs[1][0], "graph replay must be bit-identical to eager launches"
    assert torch.equal(outs[0][1], outs[1][1])


def test_run_epoch_from_a_resident_set_at_size_336():
    """Two batches from a DeviceImageSet through the resident transform at SIZE 336: the losses and the prompts of the
    same batches fed one at a time through the staging transform."""
    from rpo_amd.input_pipeline import DeviceImageSet, InputConfig, build_transform
    from rpo_amd.loop import epoch_indices
    from rpo_amd.trainer import RPO
    cfg, sd, toks, prompts, B = rpo_workload("vitl14_336")
    nb = 2
    rng = np.random.default_rng(31)
    sizes = [(375, 500), (500, 333), (336, 336), (97, 260), (400, 350)]
    imgs = [rng.integers(0, 256, (*sizes[i], 3), dtype=np.uint8) for i in range(B * nb + 1)]
    labels = rng.integers(0, cfg.n_cls, len(imgs)).tolist()
    ds = DeviceImageSet(imgs, labels, DEV)
    stage = build_transform(InputConfig(SIZE=(336, 336)), True, DEV, B)
    torch.manual_seed(5)
    order = epoch_indices(len(imgs), B, torch.Generator().manual_seed(40))
    plans = [[stage.plan(*imgs[i].shape[:2]) for i in batch] for batch in order]
    make = lambda: RPO(cfg, sd, toks, None, DEV, torch.bfloat16, batch_size=B, num_batches=nb, prompts=prompts)
    seq, seq_loss = make(), []
    for t, batch in enumerate(order):
        image = stage([imgs[i] for i in batch], plans[t])
        assert tuple(image.shape[1:]) == (3, 336, 336)
        seq_loss.append(np.float32(seq.forward_backward({"img": image, "label": torch.tensor([labels[i] for i in batch])})["loss"]))
    tr = make()
    out = tr.run_epoch(ds, torch.Generator().manual_seed(40), plans)
    torch.cuda.synchronize()
    assert out["indices"] == order and tr.epoch == 1
    assert np.array_equal(out["loss"].cpu().numpy().view(np.uint32), np.array(seq_loss, np.float32).view(np.uint32))
    assert torch.equal(tr.engine.params, seq.engine.params) and np.isfinite(seq_loss).all()
